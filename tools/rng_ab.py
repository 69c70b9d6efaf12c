"""The device generator of the reference's deterministic randombytes: its rate, and what it does to whole key generation and encryption.

1. gpq_surf_bytes at 1 MiB and 256 MiB into an aligned buffer from position 0 (the 16-byte-store path), timed by HIP events: bytes/s.
2. he_genrk (8 and 64 rotation keys) and he_enc_sk through the MPI-typed surface at n = 2^16, q_L = 2^850, wall time of the whole call in
   a C host (tools/rng_ab_host.c) whose randombytes forwards to gpq_randombytes, device samplers on in both legs:
     (A) the bytes come from that randombytes on the host and are uploaded -- the path before the device generator;
     (B) gpq_mpi_shim_set_device_rng(1).
   Both legs start every call at stream position 0, so they make the same keys: the checksums must agree.  Each (leg, shape) is ONE run
   of the host under a time limit; the host prints its generator's rate on this machine first.
`python tools/rng_ab.py [reps]` (reps of the short shapes, default 3; the 64-key leg A runs once after its warm-up)."""
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import gpqhe_amd  # noqa: E402

LOGN, LOGQ = 16, 850


def event_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rates(reps):
    g = gpqhe_amd.PolyContext(7, 2)
    for size in (1 << 20, 256 << 20):
        buf = torch.empty(size, dtype=torch.uint8, device="cuda")
        fn = lambda: g.surf_bytes(buf, 0)
        fn(); fn()
        t = [event_ms(fn) for _ in range(max(reps, 5))]
        med = statistics.median(t)
        print("gpq_surf_bytes %4d MiB  median %9.4f ms  spread %9.4f .. %9.4f   %8.2f GB/s" % (size >> 20, med, min(t), max(t), size / med / 1e6))
        sys.stdout.flush()
    g.close()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    torch.cuda.set_device(0)
    print("# device %s; n = 2^%d, q_L = 2^%d" % (torch.cuda.get_device_name(0), LOGN, LOGQ))
    rates(reps)
    torch.cuda.synchronize()
    lib_dir = os.path.join(ROOT, "gpqhe_amd")
    with tempfile.TemporaryDirectory() as tmp:
        host = os.path.join(tmp, "rng_ab_host")
        subprocess.check_call(["gcc", "-O2", "-std=gnu11", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "rng_ab_host.c"),
                               "-L", lib_dir, "-lgpqhe_hip", "-lgpqhe_hip_ctx", "-l:libgcrypt.so.20", "-lm", "-Wl,-rpath," + lib_dir,
                               "-Wl,-rpath,/opt/rocm/lib", "-o", host])
        for slots, reps_a in ((8, reps), (64, 1)):
            for leg, r in (("A", reps_a), ("B", reps)):
                print("# ---- leg %s, %d rotation keys, %d timed repetition(s)" % (leg, slots, r))
                sys.stdout.flush()
                res = subprocess.run([host, leg, str(LOGN), str(LOGQ), str(slots), str(r)], capture_output=True, text=True, timeout=900)
                for line in res.stdout.split("\n"):
                    line = line.replace("Generating rk ... ", "").replace("done.", "").strip()
                    if line:
                        print(line)
                if res.returncode != 0:
                    print("# the host ended with status %d: %s" % (res.returncode, res.stderr[-1000:]))
                    return 1
                sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
