"""Numpy model of the reference's deterministic randombytes (src/rng.c:36-77, SUPERCOP's surf generator), addressed by byte position:
what tests/test_surf_model.py holds against the executed reference and its stored stream, and what the host and device generators
(gpq_surf_bytes_host, gpq_surf_bytes, gpq_rng_*) are held against.

  The generator runs in counter mode.  in[0..3] is a 128-bit block counter, little-endian words, incremented BEFORE a block is computed
  (src/rng.c:69); in[4..11] never change from 0.  surf() (:46-63) mixes t = in ^ seed[12..24) for 2 x 16 rounds of 12 steps
      x = t[i] += ((x ^ seed[i]) + sum) ^ rotl(x, b_i),   b = 5, 7, 9, 13 repeating, sum += 0x9e3779b9 per round,
  and out = seed[24..32) ^ t[4..12) after the first 16 rounds ^ t[4..12) after the second.  randombytes hands out out[7], out[6], ..,
  out[0], each truncated to its low byte (`*x = out[--outleft]`, :73).  So byte k of a process's stream is the low byte of out[7 - k % 8]
  of the block whose counter is k // 8 + 1: any slice is computed on its own."""
import numpy as np

SEED = (3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3, 2, 3, 8, 4, 6, 2, 6, 4, 3, 3, 8, 3, 2, 7, 9, 5)     # src/rng.c:36-38
ROT = (5, 7, 9, 13)
GOLDEN = 0x9E3779B9


def blocks(counters, seed=SEED):
    """uint8 [len(counters)][8]: the 8 bytes, in the order they are handed out, of the blocks with these counter values (Python integers
    below 2^128)"""
    seed = [int(v) & 0xFFFFFFFF for v in seed]
    assert len(seed) == 32
    counters = [int(c) for c in counters]
    assert all(0 <= c < 1 << 128 for c in counters)
    u32 = np.uint32
    t = [np.array([(c >> (32 * i)) & 0xFFFFFFFF for c in counters], dtype=u32) ^ u32(seed[12 + i]) for i in range(4)]
    t += [np.full(len(counters), seed[12 + i], dtype=u32) for i in range(4, 12)]
    out = [np.full(len(counters), seed[24 + i], dtype=u32) for i in range(8)]
    x, total = t[11].copy(), 0
    with np.errstate(over="ignore"):
        for _ in range(2):
            for _ in range(16):
                total = (total + GOLDEN) & 0xFFFFFFFF
                for i in range(12):
                    b = ROT[i % 4]
                    t[i] = t[i] + (((x ^ u32(seed[i])) + u32(total)) ^ ((x << u32(b)) | (x >> u32(32 - b))))
                    x = t[i]
            for i in range(8):
                out[i] = out[i] ^ t[i + 4]
    return np.stack([out[7 - j] & u32(0xFF) for j in range(8)], axis=1).astype(np.uint8)


def stream(pos, length, seed=SEED):
    """uint8 [length]: the bytes [pos, pos + length) of the stream of `seed`"""
    assert 0 <= pos and length >= 0 and pos + length <= 1 << 128
    if length == 0:
        return np.zeros(0, dtype=np.uint8)
    first, last = pos // 8, (pos + length - 1) // 8
    whole = blocks(range(first + 1, last + 2), seed).reshape(-1)
    return whole[pos - 8 * first:pos - 8 * first + length].copy()


class Surf:
    """the sequential generator as the reference's process sees it: a position that every draw advances"""

    def __init__(self, seed=SEED, pos=0):
        self.seed, self.pos = tuple(seed), pos

    def take(self, count):
        out = stream(self.pos, count, self.seed)
        self.pos += count
        return out
