"""gpq_surf_bytes / gpq_rng_device_bytes: the device generator of the reference's deterministic randombytes against the model
(tests/surf_model.py, which tests/test_surf_model.py holds against the executed reference and the stored stream).

Every phase of the position (pos % 8) x every length 1..33 x every byte offset 0..15 of the destination, between guard bytes; lengths
around one lane's 16 bytes, a wave's 1 KiB and a workgroup's 4 KiB on the 16-byte-store path and off it; block counters that cross 2^32,
2^64 and 2^96, and the last bytes of a stream; another seed; a slice split into several launches; device and host draws interleaved on
one stream object; a captured launch replayed; the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import gpqhe_amd
from tests import surf_model

pytestmark = pytest.mark.gpu

FILL = 0x5A
SLOT, LEAD = 96, 32                                    # the sweep: one destination per 96-byte slot, 32 + offset bytes into it
RANDOM_SEED = tuple(int(v) for v in np.random.default_rng(1701).integers(0, 1 << 32, 32, dtype=np.uint64))
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def g(engine_ctx):
    return engine_ctx(7, 2)


@pytest.fixture(scope="module")
def first64k():
    return surf_model.stream(0, 65536)


def _room(nbytes):
    room = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    assert room.data_ptr() % 16 == 0
    return room


def _fill(g, room, at, length, pos, seed=None):
    """the raw call on room[at : at + length]"""
    seed_p = None if seed is None else np.array(seed, dtype=np.uint32).ctypes.data_as(C.c_void_p)
    return g.lib.gpq_surf_bytes(g.h, C.c_void_p(room.data_ptr() + at), length, seed_p, pos & M64, pos >> 64, g._stream())


def test_every_phase_length_and_destination_offset(g, first64k):
    cases = [(phase, length, offset) for phase in range(8) for length in range(1, 34) for offset in range(16)]
    room = _room(SLOT * len(cases))
    want = np.full(SLOT * len(cases), FILL, dtype=np.uint8)
    for k, (phase, length, offset) in enumerate(cases):
        pos, at = 8 * (k % 977) + phase, SLOT * k + LEAD + offset
        assert _fill(g, room, at, length, pos) == 0
        want[at:at + length] = first64k[pos:pos + length]
    got = room.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert not bad.size, "%d bytes differ (guards included), first in case (phase, length, offset) = %s" % (bad.size, cases[bad[0] // SLOT])


@pytest.mark.parametrize("offset,phase", [(0, 0), (0, 3), (5, 0), (8, 0), (13, 5)])
def test_lengths_around_a_lane_a_wave_and_a_workgroup(g, first64k, offset, phase):
    """(0, 0) and (8, 0) sit on the 16-byte-store path ((address - pos) % 8 == 0), the rest off it"""
    for unit in (16, 32, 1024, 4096, 8192):
        for length in (unit - 1, unit, unit + 1):
            room = _room(length + 64)
            pos = 8 * 100 + phase
            assert _fill(g, room, 32 + offset, length, pos) == 0
            got = room.cpu().numpy()
            assert np.array_equal(got[32 + offset:32 + offset + length], first64k[pos:pos + length]), (unit, length)
            assert (got[:32 + offset] == FILL).all() and (got[32 + offset + length:] == FILL).all(), (unit, length)


@pytest.mark.parametrize("seed", [None, RANDOM_SEED], ids=["reference_seed", "random_seed"])
def test_counters_across_word_boundaries(g, seed):
    """4 KiB whose block counters run from 2^k - 256 to 2^k + 255, aligned and not; and the last 4 KiB a stream has"""
    model_seed = surf_model.SEED if seed is None else seed
    for k in (32, 64, 96):
        for shift, offset in ((0, 0), (3, 7)):
            pos = 8 * ((1 << k) - 257) + shift
            room = _room(4096 + 64)
            assert _fill(g, room, 16 + offset, 4096, pos, seed) == 0
            got = room.cpu().numpy()
            assert np.array_equal(got[16 + offset:16 + offset + 4096], surf_model.stream(pos, 4096, model_seed)), (k, shift)
            assert (got[:16 + offset] == FILL).all() and (got[16 + offset + 4096:] == FILL).all()
    pos = (1 << 128) - 4096
    room = _room(4096)
    assert _fill(g, room, 0, 4096, pos, seed) == 0
    assert np.array_equal(room.cpu().numpy(), surf_model.stream(pos, 4096, model_seed))


def test_a_slice_split_into_several_launches(g, first64k):
    lib = g.lib
    assert lib.gpq_debug_rng_split(24) == -1                                       # no multiple of 16
    try:
        assert lib.gpq_debug_rng_split(64) == 0
        for offset, pos, length in ((0, 0, 64), (0, 8, 65), (0, 16, 200), (5, 3, 200), (11, 1029, 129)):
            room = _room(length + 64)
            assert _fill(g, room, 32 + offset, length, pos) == 0
            got = room.cpu().numpy()
            assert np.array_equal(got[32 + offset:32 + offset + length], first64k[pos:pos + length]), (offset, pos, length)
            assert (got[:32 + offset] == FILL).all() and (got[32 + offset + length:] == FILL).all()
    finally:
        assert lib.gpq_debug_rng_split(0) == 0


def test_device_and_host_draws_interleave_on_one_stream_object(g):
    for seed, start in ((None, 0), (RANDOM_SEED, 8 * ((1 << 64) - 3) + 6)):
        r = gpqhe_amd.Rng(seed, pos=start)
        model_seed = surf_model.SEED if seed is None else seed
        room, parts, at = _room(4096), [], 0
        for kind, length in (("d", 100), ("h", 5), ("d", 16), ("d", 1), ("h", 64), ("d", 1031), ("h", 3), ("d", 7)):
            if kind == "d":
                r.device_bytes(g, room[at:at + length])
                parts.append(("d", at, length))
                at += length
            else:
                parts.append(("h", r.host_bytes(length), length))
        torch.cuda.synchronize()
        dev = room.cpu().numpy()
        drawn = np.concatenate([dev[p[1]:p[1] + p[2]] if p[0] == "d" else p[1] for p in parts])
        assert r.tell() == start + drawn.size
        assert np.array_equal(drawn, surf_model.stream(start, drawn.size, model_seed))
        assert (dev[at:] == FILL).all()


def test_a_replayed_graph_repeats_its_bytes(g, first64k):
    room = _room(2048 + 32)
    assert _fill(g, room, 16, 2048, 40) == 0                                       # (outside the capture once)
    torch.cuda.synchronize()
    room.fill_(FILL)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert _fill(g, room, 16, 2048, 40) == 0
    for _ in range(2):
        room.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        got = room.cpu().numpy()
        assert np.array_equal(got[16:16 + 2048], first64k[40:40 + 2048]) and (got[:16] == FILL).all() and (got[-16:] == FILL).all()


def test_profile_books_the_generator_apart_from_the_samplers(g, first64k):
    room = _room(4096)
    g.profile(True)
    try:
        assert _fill(g, room, 0, 4096, 0) == 0
        booked = g.profile_collect()
    finally:
        g.profile(False)
    assert "surf_stream" in booked and booked["surf_stream"][1] == 1 and "sample_bytes" not in booked
    assert np.array_equal(room.cpu().numpy(), first64k[:4096])


def test_refusals_launch_nothing(g):
    lib, room = g.lib, _room(64)
    r = gpqhe_amd.Rng(pos=(1 << 128) - 8)
    p = C.c_void_p(room.data_ptr() + 16)
    assert lib.gpq_surf_bytes(g.h, None, 8, None, 0, 0, g._stream()) == -1
    assert lib.gpq_surf_bytes(g.h, p, 0, None, 0, 0, g._stream()) == -1
    assert lib.gpq_surf_bytes(None, p, 8, None, 0, 0, g._stream()) == -1
    assert lib.gpq_surf_bytes(g.h, p, 16, None, M64 - 14, M64, g._stream()) == -1   # pos + len = 2^128 + 1
    assert lib.gpq_rng_device_bytes(g.h, r.h, p, 9, g._stream()) == -1 and r.tell() == (1 << 128) - 8
    assert lib.gpq_rng_device_bytes(g.h, None, p, 8, g._stream()) == -1
    assert lib.gpq_rng_device_bytes(g.h, r.h, None, 8, g._stream()) == -1
    assert lib.gpq_rng_device_bytes(g.h, r.h, p, 0, g._stream()) == -1
    torch.cuda.synchronize()
    assert bool((room == FILL).all())
    assert lib.gpq_rng_device_bytes(g.h, r.h, p, 8, g._stream()) == 0 and r.tell() == 0   # pos + len = 2^128: the last bytes; the position wraps
    assert np.array_equal(room.cpu().numpy()[16:24], surf_model.stream((1 << 128) - 8, 8))
