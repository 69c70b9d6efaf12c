"""he_mulpt + he_rs by a constant plaintext a + b x^(n/2): the dense path (gpq_he_mulpt + gpq_he_rs with the plaintext as a polynomial) against
the one-pass gpq_he_mulpt_const, interleaved on ONE device (one context, one caller stream), at (logn 14, q = 2^438) and (logn 16,
q = 2^850), batch 1 and 16, b = 0 and b != 0, Delta = 2^30 -- and gpq_big_addsub (mode 2: one read and one write of the same two slabs, no
arithmetic to speak of) as the yardstick for how close the new kernel is to a copy.

Every repetition runs baseline, new, baseline, each as one window of `inner` calls timed by HIP events on the caller's stream after a
synchronisation; times are per call.  Prints medians, min .. max, the ratio of every pair, the A/A spread of the two baseline series,
whether all words are equal, and the per-kernel table of one call of each kind.

Then the MPI level: tests/c/constpt_host.c `time` -- he_mulpt / he_addpt by a constant on a chained (resident) ciphertext and he_inv's call
sequence over the library's symbols, with gpq_mpi_shim_set_const_pt on and off -- at (14, 438) and (16, 850).

`python tools/const_pt_ab.py [reps] [--no-mpi]`"""
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
from gemv_plan_ab import LOGDELTA, centred, event_ms  # noqa: E402

INNER = 20


class Leg:
    def __init__(self, logn, logq, batch, a, b):
        self.logn, self.logq, self.batch, self.a, self.b = logn, logq, batch, a, b
        self.dim = (logq + 1 + LOGDELTA + logn) // 59 + 1
        g = self.g = gpqhe_amd.PolyContext(logn, self.dim)
        W = self.W = logq // 64 + 1
        gen = torch.Generator(device="cuda")
        gen.manual_seed(300 + logn + batch)
        top = logq - 1 - 64 * (W - 1)
        self.c0, self.c1 = centred(g, W, batch, gen, top), centred(g, W, batch, gen, top)
        m = torch.zeros(batch, W, g.n, dtype=torch.int64, device="cuda")           # the plaintext as the dense path takes it: sign-extended words
        m[:, :, 0], m[:, :, g.n // 2] = a >> 63, b >> 63
        m[:, 0, 0], m[:, 0, g.n // 2] = a, b
        self.m = m.reshape(-1).contiguous()
        self.base = (torch.empty_like(self.c0), torch.empty_like(self.c1))
        self.new = (torch.empty_like(self.c0), torch.empty_like(self.c1))
        self.copy = (torch.empty_like(self.c0), torch.empty_like(self.c1))
        self.ws = torch.empty(g.lib.gpq_he_mulpt_workspace_bytes(g.h, self.dim, batch) // 8 + 8, dtype=torch.int64, device="cuda")
        self.bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert g.he_mulpt_const_fits(a, b, logq, self.dim)

    def dense(self):
        g, P = self.g, self.g._ptr
        for _ in range(INNER):
            _native.check(g.lib.gpq_he_mulpt(g.h, P(self.base[0]), P(self.base[1]), P(self.c0), P(self.c1), P(self.m), self.W, self.logq, self.dim, self.batch,
                                             P(self.ws), g._stream()), "gpq_he_mulpt")
            _native.check(g.lib.gpq_he_rs(g.h, P(self.base[0]), P(self.base[1]), self.W, LOGDELTA, self.logq - LOGDELTA, self.batch, g._stream()), "gpq_he_rs")

    def const(self):
        for _ in range(INNER):
            self.g.he_mulpt_const(self.new[0], self.new[1], self.c0, self.c1, self.a, self.b, self.W, self.logq, self.dim, LOGDELTA, self.bad)

    def yardstick(self):
        for _ in range(INNER):
            self.g.big_addsub(self.copy[0], self.c0, None, self.W, 2)
            self.g.big_addsub(self.copy[1], self.c1, None, self.W, 2)

    def close(self):
        torch.cuda.synchronize()
        self.g.close()


def per_call(fn):
    return event_ms(fn) / INNER


def compare(logn, logq, batch, a, b, reps):
    global INNER
    leg = Leg(logn, logq, batch, a, b)
    label = "n=2^%d q=2^%d batch %d %s" % (logn, logq, batch, "b = 0" if not b else "b != 0")
    nbytes = 2 * 2 * batch * leg.W * leg.g.n * 8                     # both polynomials read once and written once
    print("# %s: W %d, dim %d, a = %d, b = %d, %d calls per timed window, %.2f MB read + written per call" % (label, leg.W, leg.dim, a, b, INNER, nbytes / 1e6))
    for f in (leg.dense, leg.const, leg.yardstick):
        f()
    a1, new, a2, yard = [], [], [], []
    for _ in range(reps):
        a1.append(per_call(leg.dense))
        new.append(per_call(leg.const))
        a2.append(per_call(leg.dense))
        yard.append(per_call(leg.yardstick))
    base = a1 + a2
    ratios = [(x + y) / 2 / z for x, y, z in zip(a1, a2, new)]
    for name, v in (("gpq_he_mulpt + gpq_he_rs", base), ("gpq_he_mulpt_const", new), ("2 x gpq_big_addsub (-a)", yard)):
        print("%-34s %-26s median %9.4f ms  min .. max %9.4f .. %9.4f  (%.0f GB/s of the slabs' bytes)" % (label, name, statistics.median(v), min(v), max(v),
                                                                                                          nbytes / statistics.median(v) / 1e6))
    print("%-34s dense / const: median of medians %.2f, pairs %.2f .. %.2f; A/A spread %.4f ms between the baseline series' medians, %.4f ms at most inside a repetition"
          % (label, statistics.median(base) / statistics.median(new), min(ratios), max(ratios), abs(statistics.median(a1) - statistics.median(a2)),
             max(abs(x - y) for x, y in zip(a1, a2))))
    print("%-34s const / yardstick: %.2f (median over median)" % (label, statistics.median(new) / statistics.median(yard)))
    torch.cuda.synchronize()
    print("# same words: %s (non-centred inputs counted: %d)" % (torch.equal(leg.base[0], leg.new[0]) and torch.equal(leg.base[1], leg.new[1]), int(leg.bad.item())))
    keep, INNER = INNER, 1
    for name, f in (("gpq_he_mulpt + gpq_he_rs", leg.dense), ("gpq_he_mulpt_const", leg.const)):
        leg.g.profile(True)
        f()
        prof = leg.g.profile_collect()
        leg.g.profile(False)
        print("# per-kernel, one %s (%s): total %.4f ms" % (name, label, sum(v[0] for v in prof.values())))
        for kern, (ms, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
            print("#   %-26s %5d launches %10.4f ms" % (kern, cnt, ms))
    INNER = keep
    sys.stdout.flush()
    leg.close()


def mpi_level():
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "constpt_host")
        subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "constpt_host.c"),
                               "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                               "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        for logn, logq in ((14, 438), (16, 850)):
            res = subprocess.run([exe, "time", str(logn), str(logq)], capture_output=True, text=True, timeout=500)
            print("# MPI level, constpt_host time %d %d (exit %d)" % (logn, logq, res.returncode))
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
    reps = int(args[0]) if args else 7
    print("# device %s, %d interleaved repetitions (baseline, new, baseline, yardstick), library %s" % (torch.cuda.get_device_name(0), reps, os.path.basename(_native.LIB_PATH)))
    for logn, logq in ((14, 438), (16, 850)):
        for batch in (1, 16):
            for a, b in (((13 << 28) + 12345, 0), ((13 << 28) + 12345, -(5 << 27) - 7)):
                compare(logn, logq, batch, a, b, reps)
    if mpi:
        mpi_level()


if __name__ == "__main__":
    main()
