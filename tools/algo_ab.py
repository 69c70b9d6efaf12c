"""The evaluators of include/gpqhe_hip_algo.h against what a caller had before them, interleaved on ONE device (one context, one caller stream),
at (logn 14, q = 2^438) and (logn 16, q = 2^850), Delta = 2^50.

(a) Slab level, batch 1 and 16: the reference's sequence (tests/algo_model.py) issued call by call over the calls that existed -- gpq_he_mul_rs,
    gpq_he_mulpt_const, gpq_he_mulpt + gpq_he_rs, gpq_he_addpt_const, gpq_big_addsub + gpq_he_rs(.., 0, .) for he_add / he_neg,
    gpq_he_rs(.., 0, .) for he_moddown, device copies for he_copy_ct, every buffer allocated beforehand -- against ONE gpq_he_inv /
    gpq_he_sqrt / gpq_he_sigmoid / gpq_he_log / gpq_he_exp.  Every round runs baseline, new, baseline, each as one window timed by HIP events
    on the caller's stream after a synchronisation; the table gives the p50 over the rounds, min .. max, the ratio, and the A/A spread of the
    two baseline series (the noise a ratio has to exceed).  The words of both sides are compared.
(b) MPI level: tests/c/algo_host.c `time` -- he_inv's call sequence over the library's per-call symbols on resident operands against ONE
    gpq_shim_he_inv, alternating, same iteration count.

`python tools/algo_ab.py [rounds] [--no-mpi]`"""
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import gpqhe_amd  # noqa: E402
from gpqhe_amd import _native  # noqa: E402
from gemv_plan_ab import centred, event_ms, rand_keys  # noqa: E402
from tests import algo_model as am  # noqa: E402

LOGDELTA = 50


class PerCall:
    """tests/algo_model.py's operations over the slab calls that existed before the evaluators, on buffers allocated once.  he_mul + he_rs and
    he_mulpt by a constant + he_rs are the fused calls a slab caller already had: `rs` behind them only counts the level."""

    def __init__(self, leg):
        self.leg, self.g = leg, leg.g
        self.logn, self.logqL, self.s, self.W = leg.logn, leg.logq, LOGDELTA, leg.W
        self.L = leg.logq // LOGDELTA
        self.pool = [(torch.empty_like(leg.c0), torch.empty_like(leg.c1)) for _ in range(12)]
        self.next = 0

    logql = am.BigintOps.logql
    mulpt_dim = am.BigintOps.mulpt_dim

    def reset(self):
        self.next = 0

    def alloc(self):
        ct = am.Ct(self.pool[self.next], 0)
        ct.nu, ct.B = False, self.next                        # (used as "a fused rescale is pending" and as the buffer's place in the pool)
        self.next += 1
        return ct

    def value(self, ct):
        return ct.c

    def copy(self, dst, src):
        dst.c[0].copy_(src.c[0]); dst.c[1].copy_(src.c[1])
        dst.l = src.l

    def neg(self, ct):
        self.g.big_addsub(ct.c[0], ct.c[0], None, self.W, 2); self.g.big_addsub(ct.c[1], ct.c[1], None, self.W, 2)
        self.g.he_rs(ct.c[0], ct.c[1], self.W, 0, self.logql(ct.l))

    def add(self, dst, a, b):
        self.g.big_addsub(dst.c[0], a.c[0], b.c[0], self.W, 0); self.g.big_addsub(dst.c[1], a.c[1], b.c[1], self.W, 0)
        self.g.he_rs(dst.c[0], dst.c[1], self.W, 0, self.logql(a.l))
        dst.l = a.l

    def addpt(self, dst, src, re, sub=False):
        self.g.he_addpt_const(dst.c[0], dst.c[1], src.c[0], src.c[1], am.const_int(re, self.s), 0, self.W, self.logql(src.l), sub)
        dst.l = src.l

    def subpt(self, dst, src, re):
        self.addpt(dst, src, re, True)

    def moddown(self, ct):
        ct.l -= 1
        self.g.he_rs(ct.c[0], ct.c[1], self.W, 0, self.logql(ct.l))

    def rs(self, ct):
        if not ct.nu:
            self.g.he_rs(ct.c[0], ct.c[1], self.W, self.s, self.logql(ct.l - 1))
        ct.nu = False
        ct.l -= 1

    def mul(self, dst, a, b):
        g, leg, lq = self.g, self.leg, self.logql(a.l)
        dimP, dimA, dimB, _ = leg.dims(lq)
        out = self.pool[-1] if dst is a or dst is b else dst.c      # gpq_he_mul_rs: outputs may not alias inputs
        P = g._ptr
        _native.check(g.lib.gpq_he_mul_rs(g.h, P(out[0]), P(out[1]), P(a.c[0]), P(a.c[1]), P(b.c[0]), P(b.c[1]), P(leg.rlk[0]), P(leg.rlk[1]), self.W, lq,
                                          dimA, dimB, dimP, self.s, leg.batch, P(leg.ws), g._stream()), "gpq_he_mul_rs")
        if out is not dst.c:                                        # the spare and the destination's buffers change places
            self.pool[dst.B], self.pool[-1], dst.c = out, dst.c, out
        dst.l, dst.nu = a.l, True

    def mulpt_const(self, dst, src, re):
        lq = self.logql(src.l)
        self.g.he_mulpt_const(dst.c[0], dst.c[1], src.c[0], src.c[1], am.const_int(re, self.s), 0, self.W, lq, self.mulpt_dim(src.l), self.s)
        dst.l, dst.nu = src.l, True

    def mulpt(self, dst, src, m):
        g, leg, P = self.g, self.leg, self.g._ptr
        _native.check(g.lib.gpq_he_mulpt(g.h, P(dst.c[0]), P(dst.c[1]), P(src.c[0]), P(src.c[1]), P(leg.mrep), self.W, self.logql(src.l), self.mulpt_dim(src.l),
                                         leg.batch, P(leg.ws), g._stream()), "gpq_he_mulpt")
        dst.l, dst.nu = src.l, False


class Leg:
    def __init__(self, logn, logq, batch):
        self.logn, self.logq, self.batch = logn, logq, batch
        probe = gpqhe_amd.PolyContext(logn, 20)
        dimevk = probe.he_dims(logq, logq)[3]
        probe.close()
        g = self.g = gpqhe_amd.PolyContext(logn, dimevk)
        W = self.W = logq // 64 + 1
        gen = torch.Generator(device="cuda")
        gen.manual_seed(500 + logn + batch)
        top = logq - 1 - 64 * (W - 1)
        self.c0, self.c1 = centred(g, W, batch, gen, top), centred(g, W, batch, gen, top)
        self.rlk = rand_keys(g, dimevk, 2, gen)
        self.dimpt = (logq + 1 + LOGDELTA + logn) // 59 + 1
        m = torch.randint(-(1 << LOGDELTA), 1 << LOGDELTA, (g.n,), dtype=torch.int64, device="cuda", generator=gen)      # a dense plaintext below Delta
        self.m = torch.cat([m, (m >> 63).repeat(W - 1)]).contiguous()
        self.mrep = self.m.repeat(batch).contiguous()
        self._dims = {}
        need = [g.he_algo_workspace_bytes(k, W, logq, logq, LOGDELTA, self.iters(k), batch) for k in am.KINDS]
        assert all(need), g.lib.gpq_last_error().decode()
        self.ws = torch.empty(max(need) // 8 + 8, dtype=torch.int64, device="cuda")       # holds gpq_he_mul_workspace_bytes / gpq_he_mulpt_workspace_bytes of every level too
        self.out = (torch.empty_like(self.c0), torch.empty_like(self.c1))
        self.ops = PerCall(self)

    def iters(self, kind):
        L = self.logq // LOGDELTA
        return {"inv": min(8, L - 1), "sqrt": min(4, (L - 1) // 2), "exp": min(4, L - 5)}.get(kind, 0)

    def dims(self, lq):
        if lq not in self._dims:
            self._dims[lq] = self.g.he_dims(self.logq, lq)
        return self._dims[lq]

    def per_call(self, kind):
        self.ops.reset()
        self.base = am.run(kind, self.ops, am.Ct((self.c0, self.c1), self.ops.L), self.iters(kind), self.m)

    def one_call(self, kind):
        rc = self.g.he_algo_call(kind, self.out[0], self.out[1], self.c0, self.c1, self.rlk[0], self.rlk[1], self.W, self.logq, self.logq, LOGDELTA,
                                 self.iters(kind), self.ws, self.m, self.dimpt)
        _native.check(rc, "gpq_he_" + kind)

    def close(self):
        torch.cuda.synchronize()
        self.g.close()


def compare(logn, logq, batch, rounds):
    leg = Leg(logn, logq, batch)
    label = "n=2^%d q=2^%d batch %d" % (logn, logq, batch)
    inner = 4 if batch == 1 else 1                            # calls per timed window: a window of a few milliseconds at least
    for kind in am.KINDS:
        it = leg.iters(kind)
        for f in (leg.per_call, leg.one_call):                # warm: tables, scratch, every shape of the window
            f(kind)
        a1, new, a2 = [], [], []
        for _ in range(rounds):
            a1.append(event_ms(lambda: [leg.per_call(kind) for _ in range(inner)]) / inner)
            new.append(event_ms(lambda: [leg.one_call(kind) for _ in range(inner)]) / inner)
            a2.append(event_ms(lambda: [leg.per_call(kind) for _ in range(inner)]) / inner)
        torch.cuda.synchronize()
        same = torch.equal(leg.base.c[0], leg.out[0]) and torch.equal(leg.base.c[1], leg.out[1])
        base = a1 + a2
        ratios = [(x + y) / 2 / z for x, y, z in zip(a1, a2, new)]
        name = "he_%s%s" % (kind, " iter %d" % it if kind in ("inv", "sqrt", "exp") else "")
        print("%-28s %-16s per-call p50 %9.3f ms (%9.3f .. %9.3f)  one call p50 %9.3f ms (%9.3f .. %9.3f)  per-call / one call %.3f (pairs %.3f .. %.3f)  "
              "A/A spread %.3f ms  same words: %s" % (label, name, statistics.median(base), min(base), max(base), statistics.median(new), min(new), max(new),
                                                      statistics.median(base) / statistics.median(new), min(ratios), max(ratios),
                                                      abs(statistics.median(a1) - statistics.median(a2)), same))
        sys.stdout.flush()
    leg.close()


def mpi_level(rounds):
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "algo_host")
        subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "algo_host.c"),
                               "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                               "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        for logn, logq in ((14, 438), (16, 850)):
            res = subprocess.run([exe, "time", str(logn), str(logq), str(LOGDELTA), str(rounds)], capture_output=True, text=True, timeout=500)
            print("# MPI level, algo_host time %d %d %d (exit %d)" % (logn, logq, LOGDELTA, res.returncode))
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
    print("# device %s, %d interleaved rounds (per-call, one call, per-call), Delta = 2^%d, library %s"
          % (torch.cuda.get_device_name(0), rounds, LOGDELTA, os.path.basename(_native.LIB_PATH)))
    for logn, logq in ((14, 438), (16, 850)):
        for batch in (1, 16):
            compare(logn, logq, batch, rounds)
    if mpi:
        mpi_level(rounds)


if __name__ == "__main__":
    main()
