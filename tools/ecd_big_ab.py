"""gpq_he_ecd / gpq_he_dcd above 8192 slots against the single-workgroup kernels at 8192 slots, interleaved on ONE device.

Shape: n = 2^16, W = 14, count = 64: every encoder call writes the same 64 * 14 * 2^16 * 8 bytes = 448 MiB whatever the slot count.
(A) 32768 slots: he_ecd_cols + he_ecd_block + he_ecd_slab; the decoder he_dcd_block + he_dcd_cols;
(B)  8192 slots: he_ecd_lds / he_dcd_lds, one workgroup per vector -- what a build without the two-pass kernels runs too;
(C)  8192 slots in blocks of 1024 (gpq_ecd_plan_set_block): the two-pass kernels on (B)'s own inputs; its words are compared with (B)'s;
(D) 32768 slots in blocks of 4096: (A) with twice the workgroups at half the LDS each.
Every repetition runs A, B, C, D in turn, each as `inner` calls between two HIP events after a synchronisation; medians, spreads and the time
per output byte are printed, beside gpq_probe_stream's copy of as many bytes in the same process.

`python tools/ecd_big_ab.py [reps] [inner]`; `--parent PATH` loads another build of the library that has no two-pass kernels (the
parent commit's) and measures (B) alone with it, for the process-to-process comparison."""
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gpqhe_amd import _native  # noqa: E402

LOGN, W, COUNT, LOGDELTA = 16, 14, 64, 30


def event_ms(fn, inner):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def interleave(label, fns, reps, inner, nbytes):
    for f in fns.values():                      # warm-up: hand-off memory, LDS attributes, code objects
        f()
        f()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(event_ms(f, inner))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print("%-8s %-34s median %9.4f ms  spread %9.4f .. %9.4f   %8.2f ps per output byte  %8.1f GB/s out" % (
            label, k, med[k], min(v), max(v), med[k] * 1e9 / nbytes[k], nbytes[k] / med[k] / 1e6))
    sys.stdout.flush()
    return med


def main():
    args = sys.argv[1:]
    parent = None
    if "--parent" in args:
        k = args.index("--parent")
        parent = args[k + 1]
        del args[k:k + 2]
        _native.use_variant(parent)
        older = ctypes.CDLL(_native.LIB_PATH)                                # an older build lacks the newer entry points: bind what it has
        lacks = [name for name in _native.SIGNATURES if not hasattr(older, name)]
        for name in lacks:
            del _native.SIGNATURES[name]
        print("# not in %s: %s" % (parent, ", ".join(lacks) or "nothing"))
    reps = int(args[0]) if args else 9
    inner = int(args[1]) if len(args) > 1 else 20
    import gpqhe_amd
    torch.cuda.set_device(0)
    g = gpqhe_amd.PolyContext(LOGN, 2)
    n = g.n
    slab_bytes = COUNT * W * n * 8
    print("# device %s, library %s" % (torch.cuda.get_device_name(0), parent or "this build"))
    print("# n = 2^%d, W = %d, count = %d: %d bytes per encoder call; %d interleaved repetitions of %d calls" % (LOGN, W, COUNT, slab_bytes, reps, inner))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(16)
    out = torch.empty(COUNT * W * n, dtype=torch.int64, device="cuda")
    legs = {"B 8192 slots, one workgroup": (8192, 0)} if parent else {
        "A 32768 slots, two-pass": (32768, 0), "B 8192 slots, one workgroup": (8192, 0), "C 8192 slots, blocks of 1024": (8192, 1024),
        "D 32768 slots, blocks of 4096": (32768, 4096)}
    plans, zs, zouts = {}, {}, {}
    for name, (slots, block) in legs.items():
        plans[name] = g.ecd_plan(slots) if parent else g.ecd_plan(slots, block=block)
        if slots not in zs:
            zs[slots] = (2.0 ** 20 * (torch.rand(COUNT, slots, 2, dtype=torch.float64, device="cuda", generator=gen) - 0.5)).contiguous()
            zouts[slots] = torch.empty(COUNT, slots, 2, dtype=torch.float64, device="cuda")
    enc = {name: (lambda name=name: g.he_ecd(plans[name], out, zs[legs[name][0]], LOGDELTA, W)) for name in legs}
    interleave("he_ecd", enc, reps, inner, {name: slab_bytes for name in legs})

    src, dst = torch.empty(slab_bytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(slab_bytes // 2, dtype=torch.uint8, device="cuda")
    copy = lambda: _native.check(g.lib.gpq_probe_stream(g._ptr(dst), g._ptr(src), slab_bytes // 2, 0, 2048, 256, 4, g._stream()), "gpq_probe_stream")
    copy(); copy()
    tc = statistics.median(event_ms(copy, inner) for _ in range(reps))
    print("copy     gpq_probe_stream, %d bytes read + %d written: median %9.4f ms  %8.1f GB/s moved" % (slab_bytes // 2, slab_bytes // 2, tc, slab_bytes / tc / 1e6))
    del src, dst

    # the decoder on each leg's own encoded slab; output bytes = 16 slots per plaintext
    slabs = {}
    for name in legs:
        enc[name]()
        slabs[name] = out.clone()
    torch.cuda.synchronize()
    dec = {name: (lambda name=name: g.he_dcd(plans[name], zouts[legs[name][0]], slabs[name], 2.0 ** LOGDELTA, W)) for name in legs}
    interleave("he_dcd", dec, reps, inner, {name: COUNT * 16 * legs[name][0] for name in legs})
    if not parent:
        b, c = "B 8192 slots, one workgroup", "C 8192 slots, blocks of 1024"
        same_slab = torch.equal(slabs[b], slabs[c])
        dec[b](); torch.cuda.synchronize(); zb = zouts[8192].clone()
        dec[c](); torch.cuda.synchronize()
        print("# B and C: same words: %s; same doubles: %s" % (same_slab, torch.equal(zb.view(torch.int64), zouts[8192].view(torch.int64))))
    for p in plans.values():
        p.close()
    g.close()


if __name__ == "__main__":
    main()
