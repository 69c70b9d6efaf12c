"""A context gives back what it took (engine_internal.hpp: gpq_dev, gpq_table_cache): create -> use -> gpq_ctx_destroy, cycle after cycle, with
every kind of device allocation a context makes on the way -- the transform tables, every bridge constant of the prescaled streaming route and of
the relinearisation front, the peer lane with its stream, events and workspace, wave words, redo flags and zero flags, and the blocks that are
retired when scratch grows -- leaves the device's free memory where it was, and the words of the first cycle are the words of the last."""
import pytest

from tests.test_overlap_gpu import _centred, _run

pytestmark = pytest.mark.gpu

MIB = 1 << 20
# Allowed fall of the device's free memory from the end of cycle 2 to the end of cycle 5 (cycle 1 absorbs the runtime's one-time pools and
# code objects).  PARENT_DRIFT_MIB are the three readings of this very test on the parent commit's build (free after cycle 2 minus free after
# cycle 5); the slack is the largest of them plus one 2 MiB granule.  One cycle's tables (debug_table_bytes(0)) are several MiB, three leaked
# caches many times the slack.
PARENT_DRIFT_MIB = (0, 0, 0)
SLACK = (max(PARENT_DRIFT_MIB) + 2) * MIB


def _cycle(gpqhe_amd, torch, ops, readings, fail_peer=False):
    """One context from creation to close(); returns the words it computed."""
    logn, logq, W, dims, dimevk, cts5, cts8, rlk, small = ops
    want_lanes = 1 if fail_peer else 2
    out = []
    g = gpqhe_amd.PolyContext(logn, dimevk)
    try:
        g.set_overlap(True)
        if fail_peer:
            g.debug_fail_peer(1)
        g.set_chunk(2)                      # 5 ciphertexts, 3 groups: the peer, the wave words, the redo flags, every table of the route
        out += _run(g, torch, cts5, rlk, W, logq, dims)
        assert g.last_lanes() == want_lanes
        g.set_chunk(4)                      # 8 ciphertexts, 2 groups: redo flags and peer workspace grow, the old blocks are retired
        out += _run(g, torch, cts8, rlk, W, logq, dims)
        assert g.last_lanes() == want_lanes
        g.set_stream_bridge(False)          # the relinearisation-front tables
        out += _run(g, torch, cts8, rlk, W, logq, dims)
        assert g.last_lanes() == want_lanes
        readings["table_bytes"] = g.debug_table_bytes(0)
        assert g.debug_table_bytes(1) == 0
    finally:
        g.close()
    s = gpqhe_amd.PolyContext(7, 1)         # 4097 polynomials of one limb: the zero flags outgrow their first 4096 words
    try:
        x = small.clone()
        s.poly_ntt(x, 1)
        torch.cuda.synchronize()
        out.append(x)
    finally:
        s.close()
    torch.cuda.synchronize()
    readings.setdefault("free", []).append(torch.cuda.mem_get_info()[0])
    return out


def test_contexts_created_used_and_destroyed_leave_the_device_memory_where_it_was():
    """Five cycles plus one whose peer is refused (gpq_debug_fail_peer(1): the only failure provoked).  Parent build, three runs: free memory after
    cycle 2 minus after cycle 5 = 0, 0, 0 MiB (PARENT_DRIFT_MIB), so the slack is 2 MiB; debug_table_bytes(0) before the last close() is printed,
    not pinned."""
    import torch
    import gpqhe_amd
    logn, logq = 13, 300
    probe = gpqhe_amd.PolyContext(logn, 20)
    dimP, dimA, dimB, dimevk = probe.he_dims(logq, logq)
    n, p, W = probe.n, list(probe.p), (logq + 64) // 64
    probe.close()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(47)
    cts8 = [_centred(torch, gen, 8, W, n, logq) for _ in range(4)]
    cts5 = [t[: 5 * W * n] for t in cts8]
    rlk = [torch.cat([torch.randint(0, p[d], (n,), dtype=torch.int64, device="cuda", generator=gen) for d in range(dimB)]) for _ in range(2)]
    small = torch.randint(0, (1 << 59) + 1, (4097 * 128,), dtype=torch.int64, device="cuda", generator=gen)
    ops = (logn, logq, W, (dimA, dimB, dimP), dimevk, cts5, cts8, rlk, small)
    readings = {}
    first = _cycle(gpqhe_amd, torch, ops, readings)
    last = None
    for _ in range(4):
        last = None                         # (released before the next cycle allocates: torch's allocator stays where cycle 2 left it)
        last = _cycle(gpqhe_amd, torch, ops, readings)
    assert len(first) == len(last) == 13
    for i, (a, b) in enumerate(zip(first, last)):
        assert torch.equal(a, b), "result %d of cycle 5 differs from cycle 1" % i
    assert bool((first[0] != 0).any()) and bool((first[11] != 0).any()) and bool((first[12] != small).any())
    last = None
    refused = _cycle(gpqhe_amd, torch, ops, readings, fail_peer=True)
    for i, (a, b) in enumerate(zip(first, refused)):
        assert torch.equal(a, b), "result %d on one lane (peer refused) differs" % i
    free = readings["free"]
    print("free MiB after each cycle: %s; cycle 2 - cycle 5 = %.2f MiB; table bytes before the last close: %d"
          % ([f // MIB for f in free], (free[1] - free[4]) / MIB, readings["table_bytes"]))
    assert free[1] - free[4] <= SLACK, "device memory fell by %.2f MiB over three create/destroy cycles" % ((free[1] - free[4]) / MIB)
