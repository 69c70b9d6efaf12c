"""Hoisted rotations against the per-call composition, interleaved on ONE device (one context, one caller stream, one lane):

* gpq_he_rot_hoisted with K rotations against K x (gpq_poly_rot x 2 + gpq_he_swk), K = 1, 4, 16, at n = 2^16 / q_l = 2^850 and at
  n = 2^17 / 44 limbs (q_l = 2^835), batch 16;
* gpq_he_gemv against the same loop spelled with the slab entry points (src/he-algo.c:47-93 + he_rs) at logn 14 / 2^438 / slots 16 and
  logn 16 / 2^850 / slots 64, batch 1.

Every repetition runs A then B (then the next repetition), each timed by HIP events on the caller's stream after a synchronisation.
Prints the median ms per call, per rotation, the spread (min .. max) of the repetitions and the ratio of the medians.
`python tools/rot_hoist_ab.py [reps]`."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import gpqhe_amd  # noqa: E402
from gpqhe_amd import gemv_steps  # noqa: E402

LOGDELTA = 50


def rand_keys(ctx, dimB, count, gen):
    p = torch.tensor([int(x) - (1 << 64) if int(x) >= 1 << 63 else int(x) for x in ctx.p[:dimB]], dtype=torch.int64, device="cuda")
    out = []
    for _ in range(count):
        k = torch.randint(0, 1 << 59, (dimB, ctx.n), dtype=torch.int64, device="cuda", generator=gen)
        out.append((k % p[:, None]).reshape(-1).contiguous())
    return out


def centred(ctx, W, batch, gen, top_bits=16):
    big = torch.randint(-(1 << 62), 1 << 62, (batch, W, ctx.n), dtype=torch.int64, device="cuda", generator=gen)
    big[:, W - 1] = torch.randint(-(1 << top_bits), 1 << top_bits, (batch, ctx.n), dtype=torch.int64, device="cuda", generator=gen)
    return big.reshape(-1).contiguous()


def event_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleave(label, fns, reps, per):
    for f in fns.values():                      # warm-up: workspaces, tables, code objects
        f()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(event_ms(f))
    med = {k: statistics.median(v) for k, v in times.items()}
    (ka, kb) = list(fns)
    for k in fns:
        v = times[k]
        print("%-44s %-10s median %9.3f ms  per rotation %8.3f ms  spread %9.3f .. %9.3f" % (label, k, med[k], med[k] / per, min(v), max(v)))
    print("%-44s ratio %s / %s = %.3f" % (label, ka, kb, med[ka] / med[kb]))
    sys.stdout.flush()
    return med


def rot_leg(logn, logq, batch, reps):
    probe = gpqhe_amd.PolyContext(logn, 20)
    dimP, _, dimB, _ = probe.he_dims(logq, logq)
    probe.close()
    g = gpqhe_amd.PolyContext(logn, dimB)
    W = logq // 64 + 1
    gen = torch.Generator(device="cuda")
    gen.manual_seed(logn)
    c0, c1 = centred(g, W, batch, gen), centred(g, W, batch, gen)
    keys = rand_keys(g, dimB, 32, gen)
    k0, k1 = keys[:16], keys[16:]
    out0 = torch.empty(16 * c0.numel(), dtype=torch.int64, device="cuda")
    out1 = torch.empty_like(out0)
    d0, d1 = torch.empty_like(c0), torch.empty_like(c1)
    swk_ws = torch.empty(g.lib.gpq_he_swk_workspace_bytes(g.h, W, dimB, dimP, batch) // 8 + 8, dtype=torch.int64, device="cuda")
    g.set_overlap(0)                            # one lane for both sides
    print("# n = 2^%d, q_l = 2^%d, dimB %d, dimP %d, W %d, batch %d" % (logn, logq, dimB, dimP, W, batch))
    for K in (1, 4, 16):
        rots = [1 + 3 * r for r in range(K)]
        hws = torch.empty(g.lib.gpq_he_rot_hoisted_workspace_bytes(g.h, W, dimB, dimP, K, batch) // 8 + 8, dtype=torch.int64, device="cuda")
        import ctypes as C
        rr = (C.c_uint * K)(*rots)
        p0 = (C.c_void_p * K)(*[k.data_ptr() for k in k0[:K]])
        p1 = (C.c_void_p * K)(*[k.data_ptr() for k in k1[:K]])
        s = g._stream()

        def hoisted():
            gpqhe_amd._native.check(g.lib.gpq_he_rot_hoisted(g.h, g._ptr(out0), g._ptr(out1), g._ptr(c0), g._ptr(c1), rr, p0, p1, K, W, logq, dimB, dimP,
                                                             batch, g._ptr(hws), s), "gpq_he_rot_hoisted")

        def composed():
            per = c0.numel()
            for r in range(K):
                g.lib.gpq_poly_rot(g.h, g._ptr(d0), g._ptr(c0), W, rots[r], batch, s)
                g.lib.gpq_poly_rot(g.h, g._ptr(d1), g._ptr(c1), W, rots[r], batch, s)
                gpqhe_amd._native.check(g.lib.gpq_he_swk(g.h, g._ptr(out0[r * per:]), g._ptr(out1[r * per:]), g._ptr(d0), g._ptr(d1), g._ptr(k0[r]),
                                                         g._ptr(k1[r]), W, logq, dimB, dimP, batch, g._ptr(swk_ws), s), "gpq_he_swk")

        interleave("he_rot x%d n=2^%d batch %d" % (K, logn, batch), {"hoisted": hoisted, "composed": composed}, reps, K)
        hoisted()
        h0, h1 = out0[: K * c0.numel()].clone(), out1[: K * c0.numel()].clone()
        composed()
        torch.cuda.synchronize()
        print("# same words: %s" % (torch.equal(h0, out0[: K * c0.numel()]) and torch.equal(h1, out1[: K * c0.numel()])))
        del hws
    g.set_overlap(-1)
    g.close()


def gemv_leg(logn, logq, slots, reps):
    probe = gpqhe_amd.PolyContext(logn, 20)
    dimP, _, dimB, _ = probe.he_dims(logq, logq)
    probe.close()
    dimpt = (logq + 1 + LOGDELTA + logn) // 59 + 1
    g = gpqhe_amd.PolyContext(logn, max(dimB, dimpt))
    W = logq // 64 + 1
    batch = 1
    n1, n2 = gemv_steps(slots)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(100 + logn)
    c0, c1 = centred(g, W, batch, gen), centred(g, W, batch, gen)
    diag = torch.zeros(slots, W, g.n, dtype=torch.int64, device="cuda")
    diag[:, 0] = torch.randint(0, 1 << LOGDELTA, (slots, g.n), dtype=torch.int64, device="cuda", generator=gen)
    diag = diag.reshape(-1)
    keys = rand_keys(g, dimB, 2 * slots, gen)
    k0, k1 = keys[:slots], keys[slots:]
    out0, out1 = torch.empty_like(c0), torch.empty_like(c1)
    big = W * g.n
    s = g._stream()
    swk_ws = torch.empty(g.lib.gpq_he_swk_workspace_bytes(g.h, W, dimB, dimP, batch) // 8 + 8, dtype=torch.int64, device="cuda")
    mpt_ws = torch.empty(g.lib.gpq_he_mulpt_workspace_bytes(g.h, dimpt, batch) // 8 + 8, dtype=torch.int64, device="cuda")
    gws = torch.empty(g.lib.gpq_he_gemv_workspace_bytes(g.h, W, slots, dimB, dimP, dimpt, batch) // 8 + 8, dtype=torch.int64, device="cuda")
    t = [torch.empty_like(c0) for _ in range(8)]
    g.set_overlap(0)
    import ctypes as C
    p0 = (C.c_void_p * slots)(*[k.data_ptr() for k in k0])
    p1 = (C.c_void_p * slots)(*[k.data_ptr() for k in k1])
    P = g._ptr
    print("# he_gemv n = 2^%d, q_l = 2^%d, slots %d (n1 %d, n2 %d), dimB %d, dimpt %d" % (logn, logq, slots, n1, n2, dimB, dimpt))

    def fused():
        gpqhe_amd._native.check(g.lib.gpq_he_gemv(g.h, P(out0), P(out1), P(c0), P(c1), P(diag), p0, p1, slots, W, logq, LOGDELTA, dimB, dimP, dimpt,
                                                  batch, P(gws), s), "gpq_he_gemv")

    def rot(a0, a1, r, o0, o1):
        g.lib.gpq_poly_rot(g.h, P(t[6]), P(a0), W, r, batch, s)
        g.lib.gpq_poly_rot(g.h, P(t[7]), P(a1), W, r, batch, s)
        g.lib.gpq_he_swk(g.h, P(o0), P(o1), P(t[6]), P(t[7]), P(k0[r]), P(k1[r]), W, logq, dimB, dimP, batch, P(swk_ws), s)

    def loop():                                  # src/he-algo.c:62-87 call by call
        for i in range(n2):
            for j in range(n1):
                rot(c0, c1, j, t[0], t[1])
                dst = (t[2], t[3]) if j == 0 else (t[0], t[1])
                g.lib.gpq_he_mulpt(g.h, P(dst[0]), P(dst[1]), P(t[0]), P(t[1]), P(diag[(i * n1 + j) * big:]), W, logq, dimpt, batch, P(mpt_ws), s)
                if j:
                    g.lib.gpq_big_add(g.h, P(t[2]), P(t[2]), P(t[0]), W, logq, batch, s)
                    g.lib.gpq_big_add(g.h, P(t[3]), P(t[3]), P(t[1]), W, logq, batch, s)
            if i == 0:
                rot(t[2], t[3], 0, t[4], t[5])
            else:
                rot(t[2], t[3], i * n1, t[0], t[1])
                g.lib.gpq_big_add(g.h, P(t[4]), P(t[4]), P(t[0]), W, logq, batch, s)
                g.lib.gpq_big_add(g.h, P(t[5]), P(t[5]), P(t[1]), W, logq, batch, s)
        g.lib.gpq_he_rs(g.h, P(t[4]), P(t[5]), W, LOGDELTA, logq - LOGDELTA, batch, s)

    interleave("he_gemv n=2^%d slots %d" % (logn, slots), {"gemv": fused, "loop": loop}, reps, 1)
    fused()
    loop()
    torch.cuda.synchronize()
    print("# same words: %s" % (torch.equal(out0, t[4]) and torch.equal(out1, t[5])))
    g.set_overlap(-1)
    g.close()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    torch.cuda.set_device(0)
    print("# device %s, %d interleaved repetitions per pair" % (torch.cuda.get_device_name(0), reps))
    rot_leg(16, 850, 16, reps)
    rot_leg(17, 835, 16, reps)
    gemv_leg(14, 438, 16, reps)
    gemv_leg(16, 850, 64, reps)


if __name__ == "__main__":
    main()
