"""The FIRST call of he_gemv with a matrix, at the MPI level (real libgcrypt integers, tests/c/ecd_host.c): the parent commit's library, whose
first call encodes `slots` diagonals with the host's he_ecd, converts slots x n integers and uploads slots x W x n words, against this
build with gpq_mpi_shim_set_device_ecd(1), which uploads the slots^2 matrix entries and encodes on the device.

Every leg is a worker process (`ecd_host firstcall`) that sets up once -- context, keys, ciphertext, warm-up -- and then serves commands; the
driver takes turns between them, so the legs are interleaved on ONE device: per repetition parent, this build (switch on), a second
parent process (the parent-against-parent spread) and this build with the switch off (the default must be the parent's path).  Every
`first` drops all plans and uses a matrix not seen before.  Printed: per leg the medians and spread, the he_ecd time inside the call, the
ratio of every pair, whether the device path won every pair by more than the parent-against-parent spread, and the repeat-call times
(a plan hit: unchanged by this work).  Then, in this process, the device side alone: gpq_he_ecd_diagonals and
gpq_gemv_plan_create_from_matrix against gpq_gemv_plan_create on a slab that is already on the device, by HIP events.

  python tools/ecd_first_call_ab.py PARENT_LIB_DIR [pairs [rotate]]    `rotate` k: the legs start and take turns in an order rotated by k; PARENT_LIB_DIR holds the parent commit's libgpqhe_hip.so and libgpqhe_hip_ctx.so
                                                              (a checkout of the parent, `make -C gpqhe_amd/csrc`, then its gpqhe_amd/)
  python tools/ecd_first_call_ab.py kernel CALLS              he_ecd_lds alone at 64 slots (logn 16) and 8192 slots (logn 14), 64 vectors per
                                                              call: the program to put behind `rocprofv3 --kernel-trace --stats --`"""
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(14, 438, 16), (16, 850, 64)]       # DESIGN.md section 6's two shapes: logn, logq, slots
LOGDELTA = 30


def build_host(lib_dir, out):
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "ecd_host.c"),
                           "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                           "-Wl,-rpath,/opt/rocm/lib", "-o", out])
    return out


class Worker:
    def __init__(self, name, exe, shape, on):
        self.name = name
        self.p = subprocess.Popen([exe, "firstcall"] + [str(v) for v in shape] + [str(on)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)
        self.first, self.ecd, self.calls, self.repeat = [], [], [], []
        try:
            self.answer("ready")
        except BaseException:
            self.p.kill()
            self.p.wait()
            raise

    def answer(self, word):
        """the worker's next line that starts with `word` (the library's key generation reports on stdout too)"""
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError("%s: the worker ended (exit code %s) before saying %r" % (self.name, self.p.wait(), word))
            if line.split()[:1] == [word]:
                return line.split()

    def ask(self, what):
        self.p.stdin.write(what + "\n")
        self.p.stdin.flush()
        f = self.answer(what)
        if what == "first":
            self.first.append(float(f[1])); self.ecd.append(float(f[2])); self.calls.append(int(f[3]))
        else:
            self.repeat.append(float(f[1]))
            assert int(f[3]) == 0, "%s: a repeat call encoded" % self.name

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
            self.p.wait(timeout=120)
        finally:
            if self.p.poll() is None:
                self.p.kill()
                self.p.wait()


def mpi_level(parent_dir, pairs, rotate=0):
    with tempfile.TemporaryDirectory() as td:
        parent = build_host(parent_dir, os.path.join(td, "host_parent"))
        this = build_host(os.path.join(ROOT, "gpqhe_amd"), os.path.join(td, "host_this"))
        for shape in SHAPES:
            label = "logn %d q=2^%d slots %d" % shape
            legs = []
            try:
                specs = [("parent", parent, 0), ("this build, device_ecd 1", this, 1), ("parent again", parent, 0), ("this build, device_ecd 0", this, 0)]
                for name, exe, on in specs[rotate % 4:] + specs[:rotate % 4]:   # (the order the processes start and take their turns in)
                    legs.append(Worker(name, exe, shape, on))          # one after another: the set-ups do not compete for the host's cores
                for _ in range(pairs):
                    for w in legs:
                        w.ask("first")
                for _ in range(pairs):
                    for w in legs:
                        w.ask("repeat")
            finally:
                for w in legs:
                    w.close()
            P, N, P2, N0 = (legs[(k - rotate) % 4] for k in range(4))
            for w in legs:
                print("%-28s %-26s first call median %9.2f ms (%9.2f .. %9.2f), of which he_ecd %8.2f ms in %d calls; repeat call median %7.2f ms (%7.2f .. %7.2f)"
                      % (label, w.name, statistics.median(w.first), min(w.first), max(w.first), statistics.median(w.ecd), w.calls[0],
                         statistics.median(w.repeat), min(w.repeat), max(w.repeat)))
            ratio = [a / b for a, b in zip(P.first, N.first)]
            spread = [max(a / b, b / a) for a, b in zip(P.first, P2.first)]
            default = [a / b for a, b in zip(P.first, N0.first)]
            print("%-28s parent / device path: median of medians %.3f, pairs %.3f .. %.3f; parent against parent: pairs within %.3f; "
                  "device path faster in every pair by more than that spread: %s"
                  % (label, statistics.median(P.first) / statistics.median(N.first), min(ratio), max(ratio), max(spread), min(ratio) > max(spread)))
            print("%-28s parent / this build with the switch off (default): pairs %.3f .. %.3f; he_ecd calls per first call: %d (parent %d, device path %d)"
                  % (label, min(default), max(default), N0.calls[0], P.calls[0], N.calls[0]))
            print("%-28s repeat call, parent / device path: %.3f (medians)" % (label, statistics.median(P.repeat) / statistics.median(N.repeat)))
            sys.stdout.flush()


def event_ms(torch, fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def device_level(reps=7):
    import time

    import torch

    import gpqhe_amd
    for logn, logq, slots in SHAPES:
        dimpt = (logq + 1 + LOGDELTA + logn) // 59 + 1
        g = gpqhe_amd.PolyContext(logn, dimpt)
        W = logq // 64 + 1
        gen = torch.Generator(device="cuda")
        gen.manual_seed(logn)
        A = (torch.rand(slots, slots, 2, dtype=torch.float64, device="cuda", generator=gen) - 0.5) * 1024
        one = torch.empty(slots * g.n, dtype=torch.int64, device="cuda")
        wide = torch.empty(slots * W * g.n, dtype=torch.int64, device="cuda")
        with g.ecd_plan(slots) as ecd:
            g.he_ecd_diagonals(ecd, one, A, LOGDELTA, 1)
            g.he_ecd_diagonals(ecd, wide, A, LOGDELTA, W)
            t1 = [event_ms(torch, lambda: g.he_ecd_diagonals(ecd, one, A, LOGDELTA, 1)) for _ in range(reps)]
            tw = [event_ms(torch, lambda: g.he_ecd_diagonals(ecd, wide, A, LOGDELTA, W)) for _ in range(reps)]
            label = "logn %d q=2^%d slots %d" % (logn, logq, slots)
            print("%-28s gpq_he_ecd_diagonals, %d vectors: W = 1 median %.4f ms = %.2f us per vector (%.1f MiB written); W = %d median %.4f ms = %.2f us per vector (%.1f MiB)"
                  % (label, slots, statistics.median(t1), 1e3 * statistics.median(t1) / slots, slots * g.n * 8 / 2.0 ** 20, W, statistics.median(tw),
                     1e3 * statistics.median(tw) / slots, slots * W * g.n * 8 / 2.0 ** 20))
            wall = {"slab": [], "matrix": []}
            for _ in range(reps):
                for kind in ("slab", "matrix"):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    plan = g.gemv_plan(wide, slots, W, logq, dimpt) if kind == "slab" else g.gemv_plan_from_matrix(ecd, A, LOGDELTA, logq, dimpt)
                    torch.cuda.synchronize()
                    wall[kind].append((time.perf_counter() - t0) * 1e3)
                    assert plan.exact
                    plan.close()
            print("%-28s plan creation, wall: gpq_gemv_plan_create on a %d-word slab already on the device median %.3f ms; gpq_gemv_plan_create_from_matrix (encodes first) median %.3f ms"
                  % (label, W, statistics.median(wall["slab"]), statistics.median(wall["matrix"])))
        g.close()
        sys.stdout.flush()


def kernel_only(calls):
    import torch

    import gpqhe_amd
    for logn, slots in ((16, 64), (14, 8192)):
        g = gpqhe_amd.PolyContext(logn, 2)
        z = torch.rand(64, slots, 2, dtype=torch.float64, device="cuda") - 0.5
        out = torch.empty(64 * g.n, dtype=torch.int64, device="cuda")
        with g.ecd_plan(slots) as ecd:
            for _ in range(calls):
                g.he_ecd(ecd, out, z, LOGDELTA, 1)
            torch.cuda.synchronize()
        g.close()


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "kernel":
        kernel_only(int(sys.argv[2]))
        return
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    pairs = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    print("# %d interleaved repetitions per leg" % pairs)
    mpi_level(os.path.abspath(sys.argv[1]), pairs, int(sys.argv[3]) if len(sys.argv) > 3 else 0)      # (before this process opens the device itself)
    import torch
    print("# device %s" % torch.cuda.get_device_name(0))
    device_level()


if __name__ == "__main__":
    main()
