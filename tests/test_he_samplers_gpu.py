"""gpq_sample_zo / gpq_sample_error / gpq_sample_uniform / gpq_small_to_big: the device against the model (tests/enc_model.py, which
tests/test_ref_enc.py holds against the executed reference) on seeded bytes and on the recorded stream of the reference's randombytes.

Byte inputs at offset 0 and at an odd offset of an allocation; rings of one byte per polynomial (logn 2), of a single-pass and of a
two-pass size; every one of the 65536 byte pairs through the Gaussian table, the b1 = 0 ones included; uniform samples with a dropped last
byte (nbits 64, 2040), with ragged bit counts, at the reference's default modulus (439 bits) and at W = 32, into a buffer filled with a
pattern beforehand; a ring so small that a staging tile is partial and spans polynomials; and the refusals.

Every alignment: gpq_sample_error's input at each of the 16 byte offsets of a line and gpq_sample_zo's at each of the 4 of a dword, with byte
counts that make one launch do vector lanes AND a tail, into aligned and unaligned outputs between guard bytes; gpq_sample_uniform with
every byte count per coefficient 1..255, with W above the least, and with tiles shorter than the alignment head."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

from gpqhe_amd import ints_to_big, to_device, to_host
from oracle import bigint_ref as ref
from oracle.expect import ints_to_words
from tests import enc_model, enc_record

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A5A5A5A5A


def _bytes_at(data, offset):
    """the bytes on the device, starting `offset` bytes into an allocation"""
    buf = torch.zeros(data.size + offset + 16, dtype=torch.uint8, device="cuda")
    buf[offset:offset + data.size] = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    view = buf[offset:offset + data.size]
    assert view.data_ptr() % 16 == offset % 16
    return view


def _small(count, n):
    return torch.full((count * n,), 0x5A, dtype=torch.int8, device="cuda")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("logn", [2, 7, 13])
def test_zo_and_error_equal_the_model(engine_ctx, logn, offset):
    g, count = engine_ctx(logn, 2), 3
    n, rng = g.n, np.random.default_rng(500 + 10 * logn + offset)
    zb, eb = rng.integers(0, 256, count * n // 4, dtype=np.uint8), rng.integers(0, 256, count * n, dtype=np.uint8)
    eb[1::2][::5] = 0                                                             # b1 = 0 pairs in every polynomial
    zo = g.sample_zo(_small(count, n), _bytes_at(zb, offset))
    er = g.sample_error(_small(count, n), _bytes_at(eb, offset))
    torch.cuda.synchronize()
    want_zo = np.concatenate([enc_model.zo_from_bytes(zb[k * n // 4:(k + 1) * n // 4], n) for k in range(count)])
    want_er = np.concatenate([enc_model.error_from_bytes(eb[k * n:(k + 1) * n], n) for k in range(count)])
    assert np.array_equal(zo.cpu().numpy(), want_zo)
    assert np.array_equal(er.cpu().numpy(), want_er)
    assert set(np.unique(want_zo).tolist()) == {-1, 0, 1}


def test_error_on_every_byte_pair_once(engine_ctx):
    """count 32 at logn 12 = 65536 pairs: every table entry, the 256 undefined ones (b1 = 0 -> (0, 0)) included, in a shuffled order"""
    g, count = engine_ctx(12, 2), 32
    pairs = np.random.default_rng(65536).permutation(65536).astype(np.uint32)
    data = np.empty(2 * 65536, dtype=np.uint8)
    data[0::2], data[1::2] = pairs >> 8, pairs & 255
    assert data.size == count * g.n and (data[1::2] == 0).sum() == 256
    got = g.sample_error(_small(count, g.n), _bytes_at(data, 1)).cpu().numpy()
    T = enc_model.gauss_table()
    assert np.array_equal(got.reshape(-1, 2), T[pairs])
    assert not got.reshape(-1, 2)[(pairs & 255) == 0].any()


def test_unaligned_small_slab_takes_the_byte_path(engine_ctx):
    g = engine_ctx(7, 2)
    rng = np.random.default_rng(77)
    zb, eb = rng.integers(0, 256, g.n // 4, dtype=np.uint8), rng.integers(0, 256, g.n, dtype=np.uint8)
    room = torch.zeros(2 * g.n + 32, dtype=torch.int8, device="cuda")
    zo, er = room[3:3 + g.n], room[g.n + 21:2 * g.n + 21]
    g.sample_zo(zo, _bytes_at(zb, 0))
    g.sample_error(er, _bytes_at(eb, 0))
    assert np.array_equal(zo.cpu().numpy(), enc_model.zo_from_bytes(zb, g.n)) and np.array_equal(er.cpu().numpy(), enc_model.error_from_bytes(eb, g.n))
    assert not room[:3].any() and not room[3 + g.n:g.n + 21].any() and not room[2 * g.n + 21:].any()


GUARD = 32


def _guarded(nbytes, shift):
    """(room, out): an int8 output of `nbytes` bytes, `shift` bytes past a 16-byte boundary, with GUARD patterned bytes on both sides"""
    room = torch.full((2 * GUARD + nbytes,), 0x5A, dtype=torch.int8, device="cuda")
    out = room[GUARD + shift:GUARD + shift + nbytes]
    assert out.data_ptr() % 16 == shift
    return room, out


def _guards_kept(room, out):
    lo = out.data_ptr() - room.data_ptr()
    return bool((room[:lo] == 0x5A).all()) and bool((room[lo + out.numel():] == 0x5A).all())


# gpq_sample_error: (logn, count) -> count n bytes = 16 per vector lane + a tail of pairs IN THE SAME LAUNCH when the output is aligned
ERROR_SHAPES = {(7, 3): (24, 0), (3, 3): (1, 8), (4, 3): (3, 0), (5, 3): (6, 0), (2, 7): (1, 12), (1, 9): (1, 2)}     # -> (vectors, tail bytes)


def test_error_at_every_input_alignment(engine_ctx):
    """load16_any at each of its 16 shifts (p & 15: the a & 8 word move with and without a funnel shift, s == 0 at 0 and 8), with whole
    vectors only, and with one vector plus tails of 1, 4 and 6 pairs in one launch; then the byte path (an output at an odd address) at
    inputs {0, 7, 8, 9, 15}.  Guard bytes on both sides of the output stay"""
    rng = np.random.default_rng(1616)
    assert {t for _, t in ERROR_SHAPES.values()} >= {0, 2, 8, 12}                # whole vectors, and three different tail lengths
    for (logn, count), (nvec, tail) in ERROR_SHAPES.items():
        g = engine_ctx(logn, 2)
        nbytes = count * g.n
        assert (nbytes // 16, nbytes % 16) == (nvec, tail) and nvec >= 1        # tail > 0: nbytes % 16 != 0 and nbytes > 16, both paths in one launch
        data = rng.integers(0, 256, nbytes, dtype=np.uint8)
        data[1::2][::3] = 0                                                      # b1 = 0 pairs, in the tail too
        want = np.concatenate([enc_model.error_from_bytes(data[k * g.n:(k + 1) * g.n], g.n) for k in range(count)])
        runs = [(offset, 0) for offset in range(16)] + [(offset, shift) for offset, shift in ((0, 1), (7, 3), (8, 5), (9, 15), (15, 1))]
        assert sum(1 for offset, shift in runs if not shift and offset & 8) == 8 and sum(1 for offset, shift in runs if not shift and not offset & 7) == 2
        for offset, shift in runs:
            room, out = _guarded(nbytes, shift)
            assert (out.data_ptr() % 16 != 0) == bool(shift)                     # shift != 0: wide is false, everything goes by pairs
            g.sample_error(out, _bytes_at(data, offset))
            assert np.array_equal(out.cpu().numpy(), want), (logn, count, offset, shift)
            assert _guards_kept(room, out), (logn, count, offset, shift)


# gpq_sample_zo: (logn, count) -> count n/4 bytes = 4 per vector lane + a tail of single bytes
ZO_SHAPES = {(3, 3): (1, 2), (4, 3): (3, 0), (5, 3): (6, 0), (7, 3): (24, 0), (2, 7): (1, 3)}                          # -> (vectors, tail bytes)


def test_zo_at_every_input_alignment(engine_ctx):
    """load4_any at each of its four shifts (p & 3) and at {8, 13} of a 16-byte line, with whole vectors only, and with one vector plus a
    tail of 2 and of 3 bytes in one launch; into an aligned output and into an unaligned one (all by bytes), guards on both sides"""
    rng = np.random.default_rng(44)
    assert {t for _, t in ZO_SHAPES.values()} == {0, 2, 3}
    for (logn, count), (nvec, tail) in ZO_SHAPES.items():
        g = engine_ctx(logn, 2)
        nbytes = count * g.n // 4
        assert (nbytes // 4, nbytes % 4) == (nvec, tail) and nvec >= 1           # tail > 0: nbytes % 4 != 0 and nbytes > 4, both paths in one launch
        data = rng.integers(0, 256, nbytes, dtype=np.uint8)
        want = np.concatenate([enc_model.zo_from_bytes(data[k * g.n // 4:(k + 1) * g.n // 4], g.n) for k in range(count)])
        offsets = (0, 1, 2, 3, 8, 13)
        assert {t & 3 for t in offsets} == {0, 1, 2, 3}
        for offset in offsets:
            for shift in (0, 5):
                room, out = _guarded(4 * nbytes, shift)
                g.sample_zo(out, _bytes_at(data, offset))
                assert np.array_equal(out.cpu().numpy(), want), (logn, count, offset, shift)
                assert _guards_kept(room, out), (logn, count, offset, shift)


def _uniform_sweep(g, rng, cases, count=1):
    """[(nbits, W, offset)]: every launch into a patterned buffer against enc_model.uniform_from_bytes; the words above the value are zero"""
    n = g.n
    for nbits, W, offset in cases:
        nb = nbits // 8 + 1
        assert 64 * W > nbits
        data = rng.integers(0, 256, count * n * nb, dtype=np.uint8)
        data[nb - 1::nb] |= 0x80 | (1 << (nbits % 8))                          # set in every coefficient: the first dropped bit and the top bit of the last byte
        got = _uniform(g, data, nbits, W, count, offset)
        want = [enc_model.uniform_from_bytes(data[k * n * nb:(k + 1) * n * nb], n, nbits) for k in range(count)]
        assert np.array_equal(got, np.concatenate([ints_to_words(v, W) for v in want])), (nbits, W, offset)
        assert not got.reshape(count, W, n)[:, (nbits + 63) // 64:, :].any()    # (what ints_to_words put there: zero, not the pattern)


def test_uniform_at_every_byte_count_per_coefficient(engine_ctx):
    """logn 6, count 1 = exactly one full staging tile, W the least: nb = nbits / 8 + 1 takes every value 1..255 (256 is
    test_uniform_equals_the_model's 2040), so __umulhi(o, magic) divides by every nb it can meet and nb == 1 takes its own branch; bit
    counts at a byte and at a word boundary; inputs at offset 0 (head 0) and 5 (head 11, which nb < 11 makes span coefficients)"""
    g = engine_ctx(6, 2)
    assert g.n == 64                                                             # kUniformTile
    widths = [1, 7, 8, 15, 16, 63] + [8 * k + 3 for k in range(255)]
    assert {t // 8 + 1 for t in widths} == set(range(1, 256)) and [t for t in widths if t < 8] == [1, 7, 3]     # nb == 1 three times over
    _uniform_sweep(g, np.random.default_rng(255), [(nbits, nbits // 64 + 1, offset) for nbits in widths for offset in (0, 5)])


def test_uniform_with_words_above_the_least(engine_ctx):
    """W = 32 for values of 1 .. 17 words: the planes above the value are written as zero (64 j >= nbits), not left as the pattern"""
    g = engine_ctx(6, 2)
    widths = [1, 7, 8, 63, 64, 439, 1027]
    assert all(32 > t // 64 + 1 for t in widths)
    _uniform_sweep(g, np.random.default_rng(32), [(nbits, 32, offset) for nbits in widths for offset in (0, 5)])


def test_uniform_with_tiles_shorter_than_the_alignment_head(engine_ctx):
    """logn 2: count 1 at nbits 1 is a launch of 4 bytes at offset 3, fewer than the 13 bytes to the next 16-byte line (head > len, clamped);
    count 5 at nbits 17 is 20 coefficients of 3 bytes at offset 9: one partial tile over five polynomials, head 7 = two coefficients and a byte"""
    g = engine_ctx(2, 2)
    rng = np.random.default_rng(2)
    assert g.n * 1 * (1 // 8 + 1) == 4 < (-3) % 16 and 5 * g.n < 64 and (-9) % 16 == 7 and 7 % (17 // 8 + 1) != 0
    _uniform_sweep(g, rng, [(1, 1, 3)], count=1)
    _uniform_sweep(g, rng, [(17, 1, 9), (17, 2, 9)], count=5)


def _uniform(g, data, nbits, W, count, offset):
    big = torch.full((count * W * g.n,), PATTERN, dtype=torch.int64, device="cuda")
    g.sample_uniform(big, _bytes_at(data, offset), nbits, W)
    torch.cuda.synchronize()
    return to_host(big)


@pytest.mark.parametrize("offset", [0, 3])
@pytest.mark.parametrize("nbits,W", [(64, 2), (101, 2), (121, 2), (439, 7), (2040, 32)])
def test_uniform_equals_the_model(engine_ctx, nbits, W, offset):
    g, count = engine_ctx(7, 2), 2
    n, nb = g.n, nbits // 8 + 1
    data = np.random.default_rng(nbits + offset).integers(0, 256, count * n * nb, dtype=np.uint8)
    data[nb - 1::nb] |= 0x80                                                     # the dropped bits of the last byte are set in every coefficient
    got = _uniform(g, data, nbits, W, count, offset)
    want = [enc_model.uniform_from_bytes(data[k * n * nb:(k + 1) * n * nb], n, nbits) for k in range(count)]
    assert np.array_equal(got, np.concatenate([ints_to_words(v, W) for v in want]))      # every word written: none keeps the pattern by mistake
    assert max(max(v) for v in want).bit_length() == nbits and min(min(v) for v in want) >= 0
    if nbits % 8 == 0:
        assert all(int.from_bytes(data[i * nb:(i + 1) * nb].tobytes(), "little") >> nbits >= 0x80 for i in range(4))   # a whole byte dropped


def test_uniform_with_a_partial_tile_across_polynomials(engine_ctx):
    """logn 2, count 3: twelve coefficients, less than one staging tile, three polynomials in it"""
    g, count, nbits, W = engine_ctx(2, 2), 3, 101, 3
    nb = nbits // 8 + 1
    data = np.random.default_rng(12).integers(0, 256, count * g.n * nb, dtype=np.uint8)
    got = _uniform(g, data, nbits, W, count, 5)
    want = [enc_model.uniform_from_bytes(data[k * g.n * nb:(k + 1) * g.n * nb], g.n, nbits) for k in range(count)]
    assert np.array_equal(got, np.concatenate([ints_to_words(v, W) for v in want]))


@pytest.mark.parametrize("case", enc_record.CASES, ids=enc_record.case_name)
def test_samplers_on_the_recorded_stream(engine_ctx, case):
    """the reference's own bytes: the device's words have the sha256 the executed reference's outputs have"""
    logn, logq = case
    g, stream, rec = engine_ctx(logn, 3), enc_record.stored_stream(), enc_record.enc_golden()["cases"][enc_record.case_name(case)]
    n, W, nbits = g.n, rec["W"], logq + 1
    zo = g.sample_zo(_small(1, n), _bytes_at(stream[:n // 4], 0)).cpu().numpy()
    er = g.sample_error(_small(1, n), _bytes_at(stream[:n], 0)).cpu().numpy()
    un = _uniform(g, stream[:n * (nbits // 8 + 1)], nbits, W, 1, 0)
    assert enc_record.sha(zo.tolist(), W) == rec["sha256"]["sample_zo"]
    assert enc_record.sha(er.tolist(), W) == rec["sha256"]["sample_error"]
    assert hashlib.sha256(un.tobytes()).hexdigest() == rec["sha256"]["sample_uniform"]
    if logn == 7:
        assert (stream[1:n:2] == 0).any()                                        # a b1 = 0 pair of the reference's own run


def test_small_to_big_round_trip(engine_ctx):
    g, count, W = engine_ctx(7, 2), 3, 3
    small = np.random.default_rng(8).integers(-128, 128, count * g.n, dtype=np.int8)
    small[:4] = [-128, 127, 0, -1]
    big = torch.full((count * W * g.n,), PATTERN, dtype=torch.int64, device="cuda")
    g.small_to_big(big, torch.from_numpy(small).cuda(), W)
    got = to_host(big).reshape(count, W, g.n)
    assert np.array_equal(got[:, 0, :].view(np.int64), small.reshape(count, g.n).astype(np.int64))
    for j in range(1, W):
        assert np.array_equal(got[:, j, :].view(np.int64), (small.reshape(count, g.n) < 0).astype(np.int64) * -1)
    assert np.array_equal(got.reshape(-1), np.concatenate([ints_to_words(small[k * g.n:(k + 1) * g.n].tolist(), W) for k in range(count)]))


def test_small_slab_through_he_genswk(engine_ctx, oracle_ctx):
    """gpq_he_genswk's `e` from gpq_sample_error + gpq_small_to_big gives the key the host-converted polynomial gives"""
    logn, logq = 7, 120
    n, q = 1 << logn, 1 << logq
    dimP, dimA, dimB, dimevk = engine_ctx(logn, 20).he_dims(logq, logq)
    g, o = engine_ctx(logn, dimevk), oracle_ctx(logn, dimevk)
    rng = np.random.default_rng(9)
    PqL = ref.RnsBasis(o.p[:dimP]).P * q
    W = PqL.bit_length() // 64 + 1
    s = [int(v) for v in rng.integers(-1, 2, n)]
    p1 = [int.from_bytes(rng.bytes(8 * W), "little") % PqL for _ in range(n)]
    eb = rng.integers(0, 256, n, dtype=np.uint8)
    e = enc_model.error_from_bytes(eb, n)
    small = g.sample_error(_small(1, n), _bytes_at(eb, 1))
    e_dev = g.small_to_big(torch.empty(W * n, dtype=torch.int64, device="cuda"), small, W)
    keys = []
    for e_big in (e_dev, to_device(ints_to_big(e.tolist(), W))):
        dev = [to_device(ints_to_big(p1, W)), to_device(ints_to_big(s, W)), e_big, to_device(ints_to_big(ref.negacyclic_mul(s, s), W))]
        evk0, evk1 = (torch.empty(dimevk * n, dtype=torch.int64, device="cuda") for _ in range(2))
        g.he_genswk(evk0, evk1, *dev, W, dimP, logq, dimevk)
        keys.append((to_host(evk0), to_host(evk1)))
    assert np.array_equal(to_host(e_dev), ints_to_big(e.tolist(), W))
    assert np.array_equal(keys[0][0], keys[1][0]) and np.array_equal(keys[0][1], keys[1][1]) and e.any()


def test_table_is_accounted_with_the_read_only_tables(engine_ctx):
    import gpqhe_amd
    g = gpqhe_amd.PolyContext(7, 2)
    before = g.debug_table_bytes(0)
    g.sample_error(_small(1, g.n), _bytes_at(np.zeros(g.n, dtype=np.uint8), 0))
    assert g.debug_table_bytes(0) - before == 2 * 65536
    g.sample_error(_small(1, g.n), _bytes_at(np.ones(g.n, dtype=np.uint8), 0))
    assert g.debug_table_bytes(0) - before == 2 * 65536                          # built once
    torch.cuda.synchronize()
    g.close()


def test_refusals(engine_ctx):
    g, tiny = engine_ctx(7, 2), engine_ctx(1, 2)
    n = g.n
    data = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    small, big = _small(2, n), torch.zeros(2 * 32 * n, dtype=torch.int64, device="cuda")
    p, s = (lambda t: C.c_void_p(t.data_ptr())), g._stream()
    L = g.lib
    assert L.gpq_sample_zo(g.h, None, p(data), 1, s) == -1 and L.gpq_sample_zo(g.h, p(small), None, 1, s) == -1
    assert L.gpq_sample_zo(g.h, p(small), p(data), 0, s) == -1
    assert L.gpq_sample_zo(tiny.h, p(small), p(data), 1, s) == -1                # logn < 2: no n/4 bytes
    assert L.gpq_sample_zo(None, p(small), p(data), 1, s) == -1
    assert L.gpq_sample_error(g.h, None, p(data), 1, s) == -1 and L.gpq_sample_error(g.h, p(small), None, 1, s) == -1
    assert L.gpq_sample_error(g.h, p(small), p(data), 0, s) == -1
    assert L.gpq_sample_error(g.h, p(small), p(small), 1, s) == -1               # the output overlaps the input
    for nbits, W in ((0, 1), (64, 1), (128, 2), (100, 0), (100, 33)):            # 64 W > nbits, W in 1..32
        assert L.gpq_sample_uniform(g.h, p(big), p(data), nbits, W, 1, s) == -1, (nbits, W)
    assert L.gpq_sample_uniform(g.h, None, p(data), 100, 2, 1, s) == -1 and L.gpq_sample_uniform(g.h, p(big), None, 100, 2, 1, s) == -1
    assert L.gpq_sample_uniform(g.h, p(big), p(data), 100, 2, 0, s) == -1
    assert L.gpq_small_to_big(g.h, p(big), p(small), 0, 1, s) == -1 and L.gpq_small_to_big(g.h, p(big), p(small), 33, 1, s) == -1
    assert L.gpq_small_to_big(g.h, None, p(small), 2, 1, s) == -1 and L.gpq_small_to_big(g.h, p(big), None, 2, 1, s) == -1
    assert L.gpq_small_to_big(g.h, p(big), p(small), 2, 0, s) == -1
    assert L.gpq_sample_error_table(None) == -1
    assert L.gpq_sample_zo(g.h, p(small), p(data), 2, s) == 0 and L.gpq_sample_uniform(g.h, p(big), p(data), 127, 2, 2, s) == 0
    torch.cuda.synchronize()
