// csub_model.cpp -- integer model of the two spellings of csub_by (gpqhe_amd/csrc/modarith.hpp) on one 64-lane wave, on the host.
//   select form:  every lane adds (x >= m ? -m : 0)
//   masked form:  take = lanes of the current mask with x >= m;  save = mask;  mask &= take;  lanes of the mask add -m;  mask = save
// Checks, for m = p, 2p, 3p, 4p of a wide-, a split- and a plain-class modulus, x in {0, m-1, m, m+1, 2m-1} spread over the lanes in
// every rotation, and entry masks full / empty / alternating / half (a workgroup of 96) / ragged: both forms give the same word in every
// lane that is on, the masked form leaves the lanes that are off untouched and the mask as it found it, and the word is x - m [x >= m].
// Plain C++17, no device:   c++ -std=c++17 -fsanitize=undefined -fno-sanitize-recover=all tools/csub_model.cpp -o csub_model && ./csub_model
#include <cstdint>
#include <cstdio>

namespace {

struct Wave { uint64_t x[64]; uint64_t exec; };

void csub_select(Wave &w, uint64_t m, uint64_t neg_m) {
  for (int l = 0; l < 64; ++l)
    if (w.exec >> l & 1) w.x[l] = w.x[l] + (w.x[l] >= m ? neg_m : (uint64_t)0);
}

void csub_masked(Wave &w, uint64_t m, uint64_t neg_m) {
  uint64_t take = 0;                                        // v_cmp_le_u64 into an SGPR pair: lanes that are off read as 0
  for (int l = 0; l < 64; ++l)
    if ((w.exec >> l & 1) && w.x[l] >= m) take |= 1ull << l;
  const uint64_t save = w.exec;                             // s_and_saveexec_b64 save, take
  w.exec &= take;
  for (int l = 0; l < 64; ++l)                              // v_lshl_add_u64 x, x, 0, -m
    if (w.exec >> l & 1) w.x[l] += neg_m;
  w.exec = save;                                            // s_mov_b64 exec, save
}

}  // namespace

int main() {
  const uint64_t B59 = 1ull << 59;
  const uint64_t primes[3] = {B59 + 257, B59 + 134217001ull, B59 + 318999999ull};   // c below the wide limit, between wide and split, just under the 7-mad limit
  const uint64_t masks[6] = {~0ull, 0, 0x5555555555555555ull, 0xaaaaaaaaaaaaaaaaull, 0x00000000ffffffffull, 0x0123456789abcdefull};
  const uint64_t FILL = 0xDEADBEEFDEADBEEFull;
  long checked = 0;
  for (uint64_t p : primes)
    for (uint64_t mul = 1; mul <= 4; ++mul) {
      const uint64_t m = mul * p, neg_m = (uint64_t)0 - m;
      const uint64_t edge[5] = {0, m - 1, m, m + 1, 2 * m - 1};
      for (uint64_t mask : masks)
        for (int rot = 0; rot < 5; ++rot)
          for (int stride = 1; stride <= 3; ++stride) {
            Wave a, b;
            for (int l = 0; l < 64; ++l) {
              const uint64_t v = edge[(l / stride + rot) % 5];
              a.x[l] = b.x[l] = (mask >> l & 1) ? v : FILL;
            }
            a.exec = b.exec = mask;
            csub_select(a, m, neg_m);
            csub_masked(b, m, neg_m);
            if (b.exec != mask) { std::printf("mask not restored: m = %llu p, mask %016llx\n", (unsigned long long)mul, (unsigned long long)mask); return 1; }
            for (int l = 0; l < 64; ++l) {
              const uint64_t v = edge[(l / stride + rot) % 5];
              const uint64_t want = (mask >> l & 1) ? (v >= m ? v - m : v) : FILL;
              if (a.x[l] != want || b.x[l] != want) {
                std::printf("lane %d: x = %llu, m = %llu: select %llu, masked %llu, want %llu\n", l, (unsigned long long)v, (unsigned long long)m,
                            (unsigned long long)a.x[l], (unsigned long long)b.x[l], (unsigned long long)want);
                return 1;
              }
              ++checked;
            }
          }
    }
  std::printf("csub_model: %ld lane results, select form == masked form == x - m [x >= m]\n", checked);
  return 0;
}
