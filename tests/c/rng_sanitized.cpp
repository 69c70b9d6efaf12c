// rng_sanitized.cpp -- the lane body of surf_stream_k (gpqhe_amd/csrc/rng_kernels.hpp: surf_chunk, host- and device-callable) on the CPU under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_rng_sanitized.py): every lane of the grid the launcher would start, for
// positions at every phase and near 2^64, 2^127 and 2^128, destinations at every byte offset of a 16-byte line and lengths around a lane's,
// a wave's and a workgroup's bytes.  The bytes must be those of surf_block_at position by position, the guard bytes on both sides must
// stay, and exact-size heap blocks let the sanitizer see any store outside [dst, dst + len).
#include <hip/hip_runtime.h>
#include "rng_kernels.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace gpq;
static const uint32_t kSeed[32] = {3,1,4,1,5,9,2,6,5,3,5,8,9,7,9,3,2,3,8,4,6,2,6,4,3,3,8,3,2,7,9,5};
static void ref_bytes(uint8_t *x, size_t len, const SurfSeed &s, U128 pos) {
  uint64_t w = 0;                                             // one block per 8 bytes
  for (size_t k = 0; k < len; ++k) {
    U128 p = u128_add(pos, k);
    if (k == 0 || (p.lo & 7) == 0) w = surf_block_at(s, U128{(p.lo >> 3) | (p.hi << 61), p.hi >> 3});
    x[k] = (uint8_t)(w >> (8 * (p.lo & 7)));
  }
}
int main() {
  SurfSeed s; memcpy(s.w, kSeed, sizeof kSeed);
  long checked = 0;
  const U128 poss[] = {{0,0},{1,0},{7,0},{8,0},{13,0},{~0ull-20,0},{~0ull-3,~0ull>>1},{~0ull - 5000, ~0ull}};
  for (const U128 &pos0 : poss)
    for (unsigned ph = 0; ph < 8; ++ph)
      for (unsigned off = 0; off < 16; ++off)
        for (size_t len : {1,2,7,8,9,15,16,17,31,32,33,47,48,49,255,256,257,4095,4096,4097}) {
          U128 pos = u128_add(pos0, ph);
          std::vector<uint8_t> backing(len + 32 + 16);
          uint8_t *al = backing.data() + ((16 - ((uintptr_t)backing.data() & 15)) & 15);
          uint8_t *dst = al + 16 + off;   // guards checked by value below
          memset(backing.data(), 0x5A, backing.size());
          SurfStreamArgs a; a.head = (uint32_t)((uintptr_t)dst & 15); a.base = dst - a.head; a.end = (uint64_t)a.head + len;
          a.start = U128{pos.lo - a.head, pos.hi - (pos.lo < a.head)}; a.seed = s;
          const uint64_t blocks = (a.end + 4095) / 4096;
          for (uint64_t t = 0; t < blocks * 256; ++t) surf_chunk(a, t);
          std::vector<uint8_t> want(len); ref_bytes(want.data(), len, s, pos);
          if (memcmp(dst, want.data(), len)) { printf("MISMATCH ph %u off %u len %zu\n", ph, off, len); return 1; }
          for (uint8_t *q = backing.data(); q < dst; ++q) if (*q != 0x5A) { printf("GUARD lo\n"); return 1; }
          for (uint8_t *q = dst + len; q < backing.data() + backing.size(); ++q) if (*q != 0x5A) { printf("GUARD hi\n"); return 1; }
          ++checked;
        }
  // exact-size heap blocks (malloc aligns to 16): a store past dst + len lands in the sanitizer's red zone
  for (size_t len : {1,5,16,17,33,1000}) {
    uint8_t *dst = (uint8_t *)malloc(len);
    SurfStreamArgs a; a.head = (uint32_t)((uintptr_t)dst & 15); a.base = dst - a.head; a.end = (uint64_t)a.head + len; a.start = U128{0 - (uint64_t)a.head, a.head ? ~0ull : 0}; a.seed = s;
    for (uint64_t t = 0; t < ((a.end + 4095) / 4096) * 256; ++t) surf_chunk(a, t);
    free(dst); ++checked;
  }
  printf("ok %ld cases\n", checked);
  return 0;
}
