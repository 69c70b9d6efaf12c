"""gpq_he_gemv against gpq_he_gemv_planned (plan already made), interleaved on ONE device (one context, one caller stream, one lane), at
(logn 14, q = 2^438, slots 16) and (logn 16, q = 2^850, slots 64), batch 1 and 16, 30-bit diagonals.

Every repetition runs the per-call entry point, then the planned one (then the next repetition), each timed by HIP events on the caller's
stream after a synchronisation.  Prints the medians, the spread of the repetitions, the ratio of every pair (min .. max) and whether the
planned call won every pair; the time to make the plan and the bytes it holds; the per-kernel table of one call of each kind from
gpq_profile_collect; and whether the two produce the same words.

`python tools/gemv_plan_ab.py [reps]`            the comparison
`python tools/gemv_plan_ab.py planned LOGN LOGQ SLOTS BATCH CALLS`   planned calls only: the program to put behind `rocprofv3 --kernel-trace --stats --`
                                                 or `rocprofv3 --pmc ... --` (counters in a run of their own) to look at gemv_mac."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import gpqhe_amd  # noqa: E402
from gpqhe_amd import gemv_steps  # noqa: E402

LOGDELTA = 30


def rand_keys(ctx, dimB, count, gen):
    p = torch.tensor([int(x) - (1 << 64) if int(x) >= 1 << 63 else int(x) for x in ctx.p[:dimB]], dtype=torch.int64, device="cuda")
    out = []
    for _ in range(count):
        k = torch.randint(0, 1 << 59, (dimB, ctx.n), dtype=torch.int64, device="cuda", generator=gen)
        out.append((k % p[:, None]).reshape(-1).contiguous())
    return out


def centred(ctx, W, batch, gen, top_bits):
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


class Leg:
    def __init__(self, logn, logq, slots, batch):
        probe = gpqhe_amd.PolyContext(logn, 20)
        self.dimP, _, self.dimB, _ = probe.he_dims(logq, logq)
        probe.close()
        self.logn, self.logq, self.slots, self.batch = logn, logq, slots, batch
        self.dimpt = (logq + 1 + LOGDELTA + logn) // 59 + 1
        g = self.g = gpqhe_amd.PolyContext(logn, max(self.dimB, self.dimpt))
        W = self.W = logq // 64 + 1
        self.n1, self.n2 = gemv_steps(slots)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(100 + logn + batch)
        top = logq - 1 - 64 * (W - 1)
        self.c0, self.c1 = centred(g, W, batch, gen, top), centred(g, W, batch, gen, top)
        diag = torch.zeros(slots, W, g.n, dtype=torch.int64, device="cuda")
        diag[:, 0] = torch.randint(0, 1 << LOGDELTA, (slots, g.n), dtype=torch.int64, device="cuda", generator=gen)
        self.diag = diag.reshape(-1)
        need = sorted(set(range(self.n1)) | {i * self.n1 for i in range(self.n2)})
        keys = rand_keys(g, self.dimB, 2 * len(need), gen)
        self.k0, self.k1 = [None] * slots, [None] * slots
        for t, r in enumerate(need):
            self.k0[r], self.k1[r] = keys[2 * t], keys[2 * t + 1]
        self.out = [torch.empty_like(self.c0) for _ in range(4)]
        g.set_overlap(0)                        # one lane for both sides
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.plan = g.gemv_plan(self.diag, slots, W, logq, self.dimpt)
        torch.cuda.synchronize()
        self.plan_ms = (time.perf_counter() - t0) * 1e3
        lib = g.lib
        self.ws_a = torch.empty(lib.gpq_he_gemv_workspace_bytes(g.h, W, slots, self.dimB, self.dimP, self.dimpt, batch) // 8 + 8, dtype=torch.int64, device="cuda")
        self.ws_b = torch.empty(lib.gpq_he_gemv_planned_workspace_bytes(g.h, self.plan.h, W, self.dimB, self.dimP, batch) // 8 + 8, dtype=torch.int64, device="cuda")
        self.p0, self.p1 = g._key_ptrs(self.k0), g._key_ptrs(self.k1)

    def per_call(self):
        g, P = self.g, self.g._ptr
        gpqhe_amd._native.check(g.lib.gpq_he_gemv(g.h, P(self.out[0]), P(self.out[1]), P(self.c0), P(self.c1), P(self.diag), self.p0, self.p1, self.slots, self.W,
                                                  self.logq, LOGDELTA, self.dimB, self.dimP, self.dimpt, self.batch, P(self.ws_a), g._stream()), "gpq_he_gemv")

    def planned(self):
        g, P = self.g, self.g._ptr
        gpqhe_amd._native.check(g.lib.gpq_he_gemv_planned(g.h, P(self.out[2]), P(self.out[3]), P(self.c0), P(self.c1), self.plan.h, self.p0, self.p1, self.W,
                                                          LOGDELTA, self.dimB, self.dimP, self.batch, P(self.ws_b), g._stream()), "gpq_he_gemv_planned")

    def close(self):
        torch.cuda.synchronize()
        self.plan.close()
        self.g.set_overlap(-1)
        self.g.close()


def compare(logn, logq, slots, batch, reps):
    leg = Leg(logn, logq, slots, batch)
    label = "n=2^%d q=2^%d slots %d batch %d" % (logn, logq, slots, batch)
    print("# %s: n1 %d, n2 %d, dimB %d, dimpt %d, plan dim %d, plan %.1f MiB made in %.1f ms (one time), exact %s"
          % (label, leg.n1, leg.n2, leg.dimB, leg.dimpt, leg.plan.dim, leg.plan.bytes / 2.0 ** 20, leg.plan_ms, leg.plan.exact))
    for f in (leg.per_call, leg.planned):       # warm-up: tables, code objects
        f()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(event_ms(leg.per_call))
        tb.append(event_ms(leg.planned))
    ratios = [a / b for a, b in zip(ta, tb)]
    for name, v in (("gpq_he_gemv", ta), ("gpq_he_gemv_planned", tb)):
        print("%-40s %-20s median %10.3f ms  spread %10.3f .. %10.3f" % (label, name, statistics.median(v), min(v), max(v)))
    print("%-40s gpq_he_gemv / planned: median of medians %.3f, pairs %.3f .. %.3f, planned faster in every pair: %s"
          % (label, statistics.median(ta) / statistics.median(tb), min(ratios), max(ratios), all(r > 1 for r in ratios)))
    torch.cuda.synchronize()
    print("# same words: %s" % (torch.equal(leg.out[0], leg.out[2]) and torch.equal(leg.out[1], leg.out[3])))
    for name, f in (("gpq_he_gemv", leg.per_call), ("gpq_he_gemv_planned", leg.planned)):
        leg.g.profile(True)
        f()
        prof = leg.g.profile_collect()
        leg.g.profile(False)
        print("# per-kernel, one %s call (%s): total %.3f ms" % (name, label, sum(v[0] for v in prof.values())))
        for k, (ms, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
            print("#   %-26s %5d launches %10.3f ms" % (k, cnt, ms))
    if "gemv_mac" in prof:
        ms, cnt = prof["gemv_mac"]
        # bytes gemv_mac must move: every live term reads both rotations' limbs for every ciphertext and the diagonal's once; both sums are written
        words = leg.plan.dim * (1 << logn)
        algo = (slots * (2 * batch + 1) + leg.n2 * 2 * batch) * words * 8
        print("# gemv_mac: %.1f MiB algorithmic per call, %.3f ms in %d launches -> %.2f TB/s" % (algo / 2.0 ** 20, ms, cnt, algo / ms / 1e9))
    sys.stdout.flush()
    leg.close()


def main():
    torch.cuda.set_device(0)
    if len(sys.argv) > 1 and sys.argv[1] == "planned":
        logn, logq, slots, batch, calls = [int(x) for x in sys.argv[2:7]]
        leg = Leg(logn, logq, slots, batch)
        for _ in range(calls):
            leg.planned()
        leg.close()
        return
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    print("# device %s, %d interleaved repetitions per pair" % (torch.cuda.get_device_name(0), reps))
    for logn, logq, slots in ((14, 438, 16), (16, 850, 64)):
        for batch in (1, 16):
            compare(logn, logq, slots, batch, reps)


if __name__ == "__main__":
    main()
