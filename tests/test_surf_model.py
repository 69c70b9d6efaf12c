"""The position-addressed model of the reference's deterministic randombytes (tests/surf_model.py) against the stored stream and, where
oracle/_ref/ is built, against the EXECUTED reference; then the library's host generators (gpq_surf_bytes_host, gpq_rng_host_bytes,
gpq_randombytes) against the model.  No GPU: the host calls run wherever the library loads."""
import ctypes as C

import numpy as np
import pytest

import gpqhe_amd
from oracle import ref
from tests import enc_record, surf_model
from tests.ref_jobs import require_reference

LIVE_BYTES = 65536
RANDOM_SEED = tuple(int(v) for v in np.random.default_rng(1701).integers(0, 1 << 32, 32, dtype=np.uint64))
# byte positions whose block counters cross 2^32, 2^64 and 2^96 (counter = pos // 8 + 1), and the last 40 bytes a stream has
EDGES = [8 * ((1 << 32) - 2) + 3, 8 * ((1 << 64) - 2) + 5, 8 * ((1 << 96) - 2) + 1, (1 << 128) - 40]


@pytest.fixture(scope="module")
def first64k():
    """the model's first 64 KiB, once"""
    return surf_model.stream(0, LIVE_BYTES)


def test_model_equals_the_stored_stream(first64k):
    stored = enc_record.stored_stream()
    assert stored.size == enc_record.STREAM_BYTES == 16384
    assert np.array_equal(first64k[:stored.size], stored)


def test_model_equals_the_executed_reference(first64k):
    require_reference()
    live, = ref.run(enc_record.ref_stream, [LIVE_BYTES], workers=1)
    bad = np.flatnonzero(live != first64k)
    assert not bad.size, "%d bytes differ from the executed reference, first at %d" % (bad.size, bad[0])


def test_slices_at_every_phase(first64k):
    for pos in list(range(16)) + [1001, 8191]:
        for length in (0, 1, 7, 8, 9, 31):
            assert np.array_equal(surf_model.stream(pos, length), first64k[pos:pos + length]), (pos, length)


def test_counter_carries_reach_the_next_word():
    """a slice across a carry of the 128-bit counter is the blocks on both sides of it"""
    for k in (32, 64, 96):
        before, after = surf_model.blocks([(1 << k) - 1])[0], surf_model.blocks([1 << k])[0]
        pos = 8 * ((1 << k) - 2)
        assert np.array_equal(surf_model.stream(pos, 16), np.concatenate([before, after]))
        assert not np.array_equal(after, surf_model.blocks([0])[0])                   # the carry is not dropped


def test_host_slices_equal_the_model(first64k):
    for pos in range(8):
        for length in list(range(1, 34)) + [4096 + pos]:
            got = gpqhe_amd.surf_bytes_host(length, pos)
            assert np.array_equal(got, first64k[pos:pos + length]), (pos, length)
    assert np.array_equal(gpqhe_amd.surf_bytes_host(LIVE_BYTES), first64k)
    for pos in EDGES:
        assert np.array_equal(gpqhe_amd.surf_bytes_host(40, pos), surf_model.stream(pos, 40)), hex(pos)
        assert np.array_equal(gpqhe_amd.surf_bytes_host(40, pos, RANDOM_SEED), surf_model.stream(pos, 40, RANDOM_SEED)), hex(pos)
    assert not np.array_equal(gpqhe_amd.surf_bytes_host(64, 0, RANDOM_SEED), first64k[:64])


def test_sequential_draws_of_1_to_17_bytes(first64k):
    """every state of the reference's `outleft` between two draws"""
    r, pos = gpqhe_amd.Rng(), 0
    for rounds in range(3):
        for length in range(1, 18):
            assert np.array_equal(r.host_bytes(length), first64k[pos:pos + length]), (rounds, length)
            pos += length
            assert r.tell() == pos
    r.seek(EDGES[1])
    assert np.array_equal(r.host_bytes(24), surf_model.stream(EDGES[1], 24)) and r.tell() == EDGES[1] + 24
    s = gpqhe_amd.Rng(RANDOM_SEED, pos=5)
    assert np.array_equal(s.host_bytes(19), surf_model.stream(5, 19, RANDOM_SEED))


def test_default_stream_is_the_reference_stream_with_a_position(first64k):
    lib = gpqhe_amd.load()
    pos = (C.c_uint64 * 2)()

    def draw(length):
        buf = np.zeros(length, dtype=np.uint8)
        lib.gpq_randombytes(buf.ctypes.data_as(C.c_void_p), length)
        return buf

    try:
        assert lib.gpq_randombytes_seed(None) == 0
        assert np.array_equal(draw(13), first64k[:13]) and np.array_equal(draw(8), first64k[13:21])
        assert lib.gpq_randombytes_tell(pos) == 0 and (pos[0], pos[1]) == (21, 0)
        assert lib.gpq_randombytes_seek(EDGES[2] & (2 ** 64 - 1), EDGES[2] >> 64) == 0
        assert np.array_equal(draw(20), surf_model.stream(EDGES[2], 20))
        seed = np.array(RANDOM_SEED, dtype=np.uint32)
        assert lib.gpq_randombytes_seed(seed.ctypes.data_as(C.c_void_p)) == 0
        assert lib.gpq_randombytes_tell(pos) == 0 and (pos[0], pos[1]) == (0, 0)
        assert np.array_equal(draw(17), surf_model.stream(0, 17, RANDOM_SEED))
    finally:
        lib.gpq_randombytes_seed(None)


def test_host_calls_refuse_what_the_header_says():
    lib = gpqhe_amd.load()
    buf = np.zeros(16, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    top = 2 ** 64 - 1
    assert lib.gpq_surf_bytes_host(None, 8, None, 0, 0) == -1 and lib.gpq_surf_bytes_host(p, 0, None, 0, 0) == -1
    assert lib.gpq_surf_bytes_host(p, 16, None, top - 14, top) == -1                 # pos + len = 2^128 + 1
    assert lib.gpq_surf_bytes_host(p, 16, None, top - 15, top) == 0                  # pos + len = 2^128: the last 16 bytes
    assert np.array_equal(buf, surf_model.stream((1 << 128) - 16, 16))
    r = gpqhe_amd.Rng(pos=(1 << 128) - 8)
    assert lib.gpq_rng_host_bytes(r.h, p, 9) == -1 and r.tell() == (1 << 128) - 8
    assert lib.gpq_rng_host_bytes(r.h, None, 4) == -1 and lib.gpq_rng_host_bytes(None, p, 4) == -1
    assert lib.gpq_rng_create(None, None) == -1 and lib.gpq_rng_tell(r.h, None) == -1
    assert b"2^128" in lib.gpq_last_error() or b"null" in lib.gpq_last_error()
