"""he_cmp (src/he-algo.c:460-530) three ways, interleaved on ONE device (one context, one caller stream), at (logn 14, q = 2^438, iter 1, t 1:
8 levels) and (logn 16, q = 2^850, iter 1, t 2: 12 levels), Delta = 2^50, batch 1 and 16.

  A    the reference's sequence call by call over the slab calls that existed before gpq_he_cmp (tools/algo_ab.py's PerCall: gpq_he_mul_rs,
       gpq_he_mulpt_const, gpq_he_addpt_const, gpq_big_addsub + gpq_he_rs(.., 0, .), the nested he_inv tests/algo_model.py's text), every buffer
       allocated beforehand; an and bn live in the two halves of a double-width buffer and each round squares them with TWO gpq_he_mul_rs;
  A2   the same, the two squarings as ONE gpq_he_mul_rs over 2 batch ciphertexts (c0 halves adjacent, c1 halves adjacent): the only difference;
  B    ONE gpq_he_cmp.
Every round runs A, A2, B, A, each as one window timed by HIP events on the caller's stream after a synchronisation; the table gives the p50
over the rounds, min .. max, the ratios and the A/A spread of the two A series (the noise a difference has to exceed).  The words of all three
are compared.  Then, MPI level: tests/c/cmp_host.c `time` -- he_cmppt's call sequence over the library's per-call symbols on resident operands
against ONE gpq_shim_he_cmppt, same (iter, t).

`python tools/cmp_ab.py [rounds] [--no-mpi]`"""
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import gpqhe_amd  # noqa: E402
from gpqhe_amd import _native  # noqa: E402
from algo_ab import LOGDELTA, PerCall  # noqa: E402
from gemv_plan_ab import centred, event_ms, rand_keys  # noqa: E402
from tests import algo_model as am  # noqa: E402

SHAPES = ((14, 438, 1, 1), (16, 850, 1, 2))                   # logn, logq, iter, t


class Leg:
    def __init__(self, logn, logq, batch, iter, t):
        self.logn, self.logq, self.batch, self.iter, self.t = logn, logq, batch, iter, t
        probe = gpqhe_amd.PolyContext(logn, 20)
        dimevk = probe.he_dims(logq, logq)[3]
        probe.close()
        g = self.g = gpqhe_amd.PolyContext(logn, dimevk)
        W = self.W = logq // 64 + 1
        gen = torch.Generator(device="cuda")
        gen.manual_seed(700 + logn + batch)
        top = logq - 1 - 64 * (W - 1)
        self.c0, self.c1 = centred(g, W, batch, gen, top), centred(g, W, batch, gen, top)        # PerCall's pool is sized by these
        self.b = (centred(g, W, batch, gen, top), centred(g, W, batch, gen, top))
        self.rlk = rand_keys(g, dimevk, 2, gen)
        self._dims = {}
        dimP, dimA, dimB, _ = self.dims(logq)
        need = [g.he_cmp_workspace_bytes(False, W, logq, logq, LOGDELTA, iter, t, batch), g.lib.gpq_he_mul_workspace_bytes(g.h, W, dimA, dimB, dimP, 2 * batch)]
        assert all(need), g.lib.gpq_last_error().decode()
        self.ws = torch.empty(max(need) // 8 + 8, dtype=torch.int64, device="cuda")
        self.out = (torch.empty_like(self.c0), torch.empty_like(self.c1))
        self.half = self.c0.numel()
        self.D = [(torch.empty(2 * self.half, dtype=torch.int64, device="cuda"), torch.empty(2 * self.half, dtype=torch.int64, device="cuda")) for _ in range(2)]
        self.S = (torch.empty_like(self.c0), torch.empty_like(self.c1))
        self.ops = PerCall(self)
        self.res = {}

    def dims(self, lq):
        if lq not in self._dims:
            self._dims[lq] = self.g.he_dims(self.logq, lq)
        return self._dims[lq]

    def view(self, d, k):
        return tuple(x[k * self.half:(k + 1) * self.half] for x in self.D[d])

    def ct(self, c, l):
        x = am.Ct(c, l)
        x.nu, x.B = False, None                               # PerCall: no fused rescale pending; not one of its pool's buffers
        return x

    def mul_rs(self, out, a, b, l, batch):
        g, P, lq = self.g, self.g._ptr, self.ops.logql(l)
        dimP, dimA, dimB, _ = self.dims(lq)
        _native.check(g.lib.gpq_he_mul_rs(g.h, P(out[0]), P(out[1]), P(a[0]), P(a[1]), P(b[0]), P(b[1]), P(self.rlk[0]), P(self.rlk[1]), self.W, lq,
                                          dimA, dimB, dimP, LOGDELTA, batch, P(self.ws), g._stream()), "gpq_he_mul_rs")

    def inverse(self, src):
        self.ops.reset()
        return am.he_inv(self.ops, src, self.iter)

    def per_call(self, paired):
        """he_cmp call by call; an | bn in the halves of D[cur], every product into the other double buffer"""
        ops, iter = self.ops, self.iter
        L, cur = ops.L, 0
        S = self.ct(self.S, L)
        ops.add(S, self.ct((self.c0, self.c1), L), self.ct(self.b, L))              # :525
        ops.mulpt_const(S, S, 0.5); ops.rs(S)                                        # :473-474
        inv = self.inverse(S)                                                        # :475
        an = self.ct(self.view(cur, 0), L)
        ops.mulpt_const(an, self.ct((self.c0, self.c1), L), 0.5); ops.rs(an)         # :477-478
        for _ in range(iter + 1):
            ops.moddown(an)                                                          # :479-480
        self.mul_rs(self.view(1 - cur, 0), an.c, inv.c, an.l, self.batch)            # :482-483
        cur, l = 1 - cur, an.l - 1
        for r in range(self.t):
            an, bn = self.ct(self.view(cur, 0), l), self.ct(self.view(cur, 1), l)
            ops.subpt(bn, an, 1); ops.neg(bn)                                        # :485-486 / :499-500
            if paired:                                                               # :489-492
                self.mul_rs(self.D[1 - cur], self.D[cur], self.D[cur], l, 2 * self.batch)
            else:
                self.mul_rs(self.view(1 - cur, 0), an.c, an.c, l, self.batch)
                self.mul_rs(self.view(1 - cur, 1), bn.c, bn.c, l, self.batch)
            cur, l = 1 - cur, l - 1
            an, bn = self.ct(self.view(cur, 0), l), self.ct(self.view(cur, 1), l)
            S.l = l
            ops.add(S, an, bn)                                                       # :493
            inv = self.inverse(S)                                                    # :494
            for _ in range(iter + 1):
                ops.moddown(an)                                                      # :495-496
            self.mul_rs(self.view(1 - cur, 0), an.c, inv.c, an.l, self.batch)        # :497-498
            cur, l = 1 - cur, an.l - 1
        self.res["A2" if paired else "A"] = self.view(cur, 0)

    def one_call(self):
        rc = self.g.he_cmp_call(self.out[0], self.out[1], self.c0, self.c1, self.b, self.rlk[0], self.rlk[1], self.W, self.logq, self.logq, LOGDELTA,
                                self.iter, self.t, self.ws)
        _native.check(rc, "gpq_he_cmp")
        self.res["B"] = self.out

    def close(self):
        torch.cuda.synchronize()
        self.g.close()


def compare(logn, logq, iter, t, batch, rounds):
    leg = Leg(logn, logq, batch, iter, t)
    label = "n=2^%d q=2^%d batch %-2d he_cmp iter %d t %d" % (logn, logq, batch, iter, t)
    inner = 4 if batch == 1 else 1                            # calls per timed window: a window of a few milliseconds at least
    legs = {"A": lambda: leg.per_call(False), "A2": lambda: leg.per_call(True), "B": leg.one_call}
    words = {}
    for name, f in legs.items():                              # warm: tables, scratch, every shape of the window; and the words
        f()
        torch.cuda.synchronize()
        words[name] = tuple(x.clone() for x in leg.res[name])
    same = {name: torch.equal(words[name][0], words["A"][0]) and torch.equal(words[name][1], words["A"][1]) for name in ("A2", "B")}
    ts = {"A": [], "A2": [], "B": [], "A'": []}
    for _ in range(rounds):
        for name in ("A", "A2", "B", "A'"):
            ts[name].append(event_ms(lambda: [legs[name[0] if name == "A'" else name]() for _ in range(inner)]) / inner)
    torch.cuda.synchronize()
    p50 = {k: statistics.median(v) for k, v in ts.items()}
    a = statistics.median(ts["A"] + ts["A'"])
    spread = abs(p50["A"] - p50["A'"])
    fmt = lambda k, v: "%s p50 %9.3f ms (%9.3f .. %9.3f)" % (k, statistics.median(v), min(v), max(v))
    print("%s  %s  %s  %s  A - A2 %+.3f ms  A - B %+.3f ms  A / A2 %.3f  A / B %.3f  A/A spread %.3f ms  same words: A2 %s, B %s"
          % (label, fmt("A", ts["A"] + ts["A'"]), fmt("A2", ts["A2"]), fmt("B", ts["B"]), a - p50["A2"], a - p50["B"], a / p50["A2"], a / p50["B"], spread,
             same["A2"], same["B"]))
    sys.stdout.flush()
    leg.close()
    return dict(batch=batch, logn=logn, a=a, a2=p50["A2"], b=p50["B"], spread=spread, same=all(same.values()))


def mpi_level(rounds):
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "cmp_host")
        subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "cmp_host.c"),
                               "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                               "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        for logn, logq, iter, t in SHAPES:
            res = subprocess.run([exe, "time", str(logn), str(logq), str(LOGDELTA), str(iter), str(t), str(rounds)], capture_output=True, text=True, timeout=500)
            print("# MPI level, cmp_host time %d %d %d %d %d (exit %d)" % (logn, logq, LOGDELTA, iter, t, res.returncode))
            print(res.stdout.rstrip())
            if res.returncode:
                print(res.stderr[-2000:])
                return
            sys.stdout.flush()


def main():
    args = sys.argv[1:]
    mpi = "--no-mpi" not in args
    args = [x for x in args if x != "--no-mpi"]
    torch.cuda.set_device(0)
    rounds = int(args[0]) if args else 7
    print("# device %s, %d interleaved rounds (A, A2, B, A), Delta = 2^%d, library %s"
          % (torch.cuda.get_device_name(0), rounds, LOGDELTA, os.path.basename(_native.LIB_PATH)))
    rows = [compare(logn, logq, iter, t, batch, rounds) for logn, logq, iter, t in SHAPES for batch in (1, 16)]
    # the rule the pairing is kept or dropped by: A2 faster than A by more than the A/A spread at batch 1 at both shapes, and not slower beyond
    # it at batch 16; and B not slower than A beyond the spread anywhere
    wins = all(r["a"] - r["a2"] > r["spread"] for r in rows if r["batch"] == 1)
    holds = all(r["a2"] - r["a"] <= r["spread"] for r in rows if r["batch"] == 16)
    print("# pairing: A2 beats A beyond the A/A spread at batch 1 at both shapes: %s; not slower beyond it at batch 16: %s -> %s"
          % (wins, holds, "keep" if wins and holds else "drop"))
    print("# B not slower than A beyond the A/A spread at every shape: %s; same words everywhere: %s"
          % (all(r["b"] - r["a"] <= r["spread"] for r in rows), all(r["same"] for r in rows)))
    if mpi:
        mpi_level(rounds)


if __name__ == "__main__":
    main()
