"""k sequential gpq_he_gemv_planned calls against ONE gpq_he_gemv_multi over the same k plans, interleaved on ONE device (one context, one
caller stream, one lane), at (logn 14, q = 2^438, slots 16) and (logn 16, q = 2^850, slots 64), batch 1 and 16, k = 2 and 4, dense 30-bit
diagonals.

Every repetition runs the k planned calls, the multi call, and the k planned calls again, each timed by HIP events on the caller's stream
after a synchronisation: the two baseline runs of a repetition give the A/A spread.  Prints the medians, min .. max, the ratio of every
pair, the A/A spread (the difference of the two baseline series' medians, and the largest difference inside one repetition) and whether the
multi call's median stays within the baseline's plus that spread; whether all words are equal; and the per-kernel table of one call of each
kind from gpq_profile_collect.

`python tools/gemv_multi_ab.py [reps] [--lib PATH]`     --lib: another build of libgpqhe_hip.so (make -C gpqhe_amd/csrc variant NAME=..
                                                        DEFS="-DGPQ_GEMV_MULTI_BT=2 -DGPQ_GEMV_MULTI_NP=4") to time another (BT, NP)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import gpqhe_amd  # noqa: E402
from gpqhe_amd import _native, gemv_steps  # noqa: E402
from gemv_plan_ab import LOGDELTA, centred, event_ms, rand_keys  # noqa: E402


class Leg:
    def __init__(self, logn, logq, slots, batch, k):
        probe = gpqhe_amd.PolyContext(logn, 20)
        self.dimP, _, self.dimB, _ = probe.he_dims(logq, logq)
        probe.close()
        self.logn, self.logq, self.slots, self.batch, self.k = logn, logq, slots, batch, k
        self.dimpt = (logq + 1 + LOGDELTA + logn) // 59 + 1
        g = self.g = gpqhe_amd.PolyContext(logn, max(self.dimB, self.dimpt))
        W = self.W = logq // 64 + 1
        self.n1, self.n2 = gemv_steps(slots)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(200 + logn + batch + k)
        top = logq - 1 - 64 * (W - 1)
        self.c0, self.c1 = centred(g, W, batch, gen, top), centred(g, W, batch, gen, top)
        need = sorted(set(range(self.n1)) | {i * self.n1 for i in range(self.n2)})
        keys = rand_keys(g, self.dimB, 2 * len(need), gen)
        k0, k1 = [None] * slots, [None] * slots
        for t, r in enumerate(need):
            k0[r], k1[r] = keys[2 * t], keys[2 * t + 1]
        self.keys = keys
        g.set_overlap(0)                        # one lane for both sides
        self.plans = []
        for _ in range(k):
            diag = torch.zeros(slots, W, g.n, dtype=torch.int64, device="cuda")
            diag[:, 0] = torch.randint(0, 1 << LOGDELTA, (slots, g.n), dtype=torch.int64, device="cuda", generator=gen)
            self.plans.append(g.gemv_plan(diag.reshape(-1), slots, W, logq, self.dimpt))
            torch.cuda.synchronize()
        self.multi_set = g.gemv_multi(self.plans)
        self.base = [(torch.empty_like(self.c0), torch.empty_like(self.c1)) for _ in range(k)]
        self.outs = [(torch.empty_like(self.c0), torch.empty_like(self.c1)) for _ in range(k)]
        lib = g.lib
        self.ws_a = torch.empty(max(lib.gpq_he_gemv_planned_workspace_bytes(g.h, p.h, W, self.dimB, self.dimP, batch) for p in self.plans) // 8 + 8,
                                dtype=torch.int64, device="cuda")
        self.ws_b = torch.empty(lib.gpq_he_gemv_multi_workspace_bytes(g.h, self.multi_set.h, W, self.dimB, self.dimP, batch) // 8 + 8, dtype=torch.int64, device="cuda")
        self.p0, self.p1 = g._key_ptrs(k0), g._key_ptrs(k1)
        self.o0, self.o1 = g._key_ptrs([o[0] for o in self.outs]), g._key_ptrs([o[1] for o in self.outs])

    def planned(self):
        g, P = self.g, self.g._ptr
        for t, plan in enumerate(self.plans):
            _native.check(g.lib.gpq_he_gemv_planned(g.h, P(self.base[t][0]), P(self.base[t][1]), P(self.c0), P(self.c1), plan.h, self.p0, self.p1, self.W,
                                                    LOGDELTA, self.dimB, self.dimP, self.batch, P(self.ws_a), g._stream()), "gpq_he_gemv_planned")

    def multi(self):
        g, P = self.g, self.g._ptr
        _native.check(g.lib.gpq_he_gemv_multi(g.h, self.o0, self.o1, P(self.c0), P(self.c1), self.multi_set.h, self.p0, self.p1, self.W,
                                              LOGDELTA, self.dimB, self.dimP, self.batch, P(self.ws_b), g._stream()), "gpq_he_gemv_multi")

    def close(self):
        torch.cuda.synchronize()
        self.multi_set.close()
        for p in self.plans:
            p.close()
        self.g.set_overlap(-1)
        self.g.close()


def compare(logn, logq, slots, batch, k, reps):
    leg = Leg(logn, logq, slots, batch, k)
    label = "n=2^%d q=2^%d slots %d batch %d k %d" % (logn, logq, slots, batch, k)
    print("# %s: n1 %d, n2 %d, dimB %d, dimpt %d, plan dims %s, set: %d baby rotations, dim %d, %d bytes of tables, %d plans per launch"
          % (label, leg.n1, leg.n2, leg.dimB, leg.dimpt, [p.dim for p in leg.plans], leg.multi_set.baby, leg.multi_set.dim, leg.multi_set.bytes,
             gpqhe_amd.gemv_multi_width()))
    for f in (leg.planned, leg.multi):          # warm-up: tables, code objects
        f()
    a1, b, a2 = [], [], []
    for _ in range(reps):
        a1.append(event_ms(leg.planned))
        b.append(event_ms(leg.multi))
        a2.append(event_ms(leg.planned))
    a = a1 + a2
    ratios = [(x + y) / 2 / z for x, y, z in zip(a1, a2, b)]
    for name, v in (("%d x gpq_he_gemv_planned" % k, a), ("gpq_he_gemv_multi", b)):
        print("%-46s %-26s median %10.3f ms  min .. max %10.3f .. %10.3f" % (label, name, statistics.median(v), min(v), max(v)))
    aa_medians = abs(statistics.median(a1) - statistics.median(a2))
    aa_pairs = max(abs(x - y) for x, y in zip(a1, a2))
    over = statistics.median(b) - statistics.median(a)
    print("%-46s planned / multi: median of medians %.3f, pairs %.3f .. %.3f; A/A spread %.3f ms between the series' medians, %.3f ms at most inside a repetition"
          % (label, statistics.median(a) / statistics.median(b), min(ratios), max(ratios), aa_medians, aa_pairs))
    print("%-46s multi - baseline = %+.3f ms: within the A/A spread of the medians: %s" % (label, over, over <= aa_medians))
    torch.cuda.synchronize()
    print("# same words: %s" % all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(leg.base, leg.outs)))
    for name, f in (("%d x gpq_he_gemv_planned" % k, leg.planned), ("gpq_he_gemv_multi", leg.multi)):
        leg.g.profile(True)
        f()
        prof = leg.g.profile_collect()
        leg.g.profile(False)
        print("# per-kernel, one %s (%s): total %.3f ms" % (name, label, sum(v[0] for v in prof.values())))
        for kern, (ms, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
            print("#   %-26s %5d launches %10.3f ms" % (kern, cnt, ms))
    sys.stdout.flush()
    leg.close()


def main():
    args = sys.argv[1:]
    if "--lib" in args:
        at = args.index("--lib")
        _native.use_variant(args[at + 1])
        del args[at:at + 2]
    torch.cuda.set_device(0)
    reps = int(args[0]) if args else 7
    print("# device %s, %d interleaved repetitions (baseline, multi, baseline), library %s" % (torch.cuda.get_device_name(0), reps, os.path.basename(_native.LIB_PATH)))
    for logn, logq, slots in ((14, 438, 16), (16, 850, 64)):
        for batch in (1, 16):
            for k in (2, 4):
                compare(logn, logq, slots, batch, k, reps)


if __name__ == "__main__":
    main()
