"""gpq_he_enc_pk / gpq_he_enc_sk against the sequence the library had before them, interleaved on ONE device, and the three samplers
against the copy rate.

(A) the existing entry points: gpq_poly_mul with the key replicated per ciphertext (twice for he_enc_pk), gpq_small_to_big of the sampled
    polynomials, gpq_big_addsub, gpq_he_rs(logDelta 0) -- what tests/test_he_enc_gpu.py compares the new calls with word for word;
(B) gpq_he_enc_pk / gpq_he_enc_sk.
Shape: n = 2^16, q = 2^438 (8 limbs, 7 words), batch 64.  Every repetition runs A then B, each timed by HIP events after a synchronisation;
the median, the spread and the ratio of the medians are printed, and whether both gave the same words.
The samplers (gpq_sample_zo / gpq_sample_error / gpq_sample_uniform at the same shape) are reported as GB/s of INPUT bytes and of all
bytes moved, beside gpq_probe_stream's copy rate over the same number of bytes.  The shader clock is read (rocm-smi, read only) while the
encryptors run.  `python tools/enc_ab.py [reps] [logn] [logq] [batch]`."""
import os
import re
import shutil
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import gpqhe_amd  # noqa: E402
from gpqhe_amd import _native  # noqa: E402


def event_ms(fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleave(label, fns, reps):
    for f in fns.values():                      # warm-up: workspaces, tables, code objects
        f()
        f()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(event_ms(f))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print("%-26s %-10s median %9.3f ms  spread %9.3f .. %9.3f" % (label, k, med[k], min(v), max(v)))
    ka, kb = list(fns)
    print("%-26s ratio %s / %s = %.3f" % (label, ka, kb, med[ka] / med[kb]))
    sys.stdout.flush()
    return med


def sclk(step):
    """median shader clock (MHz) of a few read-only rocm-smi polls while `step` keeps the device busy; None without rocm-smi"""
    if shutil.which("rocm-smi") is None:
        return None
    seen = []
    for _ in range(4):
        for _ in range(6):
            step()
        try:
            out = subprocess.run(["rocm-smi", "-d", str(torch.cuda.current_device()), "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        except Exception:
            return None
        m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
        if m:
            seen.append(int(m.group(1)))
    torch.cuda.synchronize()
    return sorted(seen[1:])[len(seen[1:]) // 2] if len(seen) > 1 else None


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    logn, logq, batch = (int(v) for v in (sys.argv[2:5] + ["16", "438", "64"][len(sys.argv[2:5]):]))
    torch.cuda.set_device(0)
    dim, W, nbits = (logq + 1 + logn) // 59 + 1, logq // 64 + 1, logq + 1
    if 64 * W <= nbits:
        W += 1
    g = gpqhe_amd.PolyContext(logn, dim)
    n, nb = g.n, nbits // 8 + 1
    gen = torch.Generator(device="cuda")
    gen.manual_seed(13)
    print("# device %s, %d interleaved repetitions; n = 2^%d, q = 2^%d, dim %d, W %d, batch %d" % (torch.cuda.get_device_name(0), reps, logn, logq, dim, W, batch))
    rand_bytes = lambda count: torch.randint(0, 256, (count,), dtype=torch.uint8, device="cuda", generator=gen)
    small = lambda: torch.empty(batch * n, dtype=torch.int8, device="cuda")
    big = lambda k=batch: torch.empty(k * W * n, dtype=torch.int64, device="cuda")
    zb, eb, ub = rand_bytes(batch * n // 4), rand_bytes(batch * n), rand_bytes(batch * n * nb)
    v, e0, e1, a = g.sample_zo(small(), zb), g.sample_error(small(), eb), g.sample_error(small(), rand_bytes(batch * n)), g.sample_uniform(big(), ub, nbits, W)
    m = big()
    m.zero_()
    m.view(batch, W, n)[:, 0] = torch.randint(-(1 << 40), 1 << 40, (batch, n), dtype=torch.int64, device="cuda", generator=gen)
    m.view(batch, W, n)[:, 1:] = (m.view(batch, W, n)[:, :1] >> 63)

    # one key pair: sk ternary, (p0, p1) = he_keypair's arithmetic on the device
    sk1 = torch.zeros(W * n, dtype=torch.int64, device="cuda")
    t = torch.randint(-1, 2, (n,), dtype=torch.int64, device="cuda", generator=gen)
    sk1.view(W, n)[0], sk1.view(W, n)[1:] = t, (t >> 63)[None, :]

    def pack(src):
        out = torch.empty(dim * n, dtype=torch.int64, device="cuda")
        _native.check(g.lib.gpq_evk_pack(g.h, g._ptr(out), g._ptr(src), W, dim, 1, g._stream()), "gpq_evk_pack")
        return out

    sk_ntt = pack(sk1)
    p0, p1 = g.he_enc_sk(big(1), big(1), None, a[:W * n], e0[:n], sk_ntt, W, logq, dim)
    pk_ntt = (pack(p0), pack(p1))
    rep = lambda one: one.view(1, -1).expand(batch, -1).reshape(-1).contiguous()
    sk_rep, p0_rep, p1_rep = rep(sk1), rep(p0), rep(p1)

    ws_pk = torch.empty(g.lib.gpq_he_enc_workspace_bytes(g.h, dim, batch, 1) // 8 + 8, dtype=torch.int64, device="cuda")
    ws_sk = torch.empty(g.lib.gpq_he_enc_workspace_bytes(g.h, dim, batch, 0) // 8 + 8, dtype=torch.int64, device="cuda")
    ws_mul = torch.empty(g.lib.gpq_poly_mul_workspace_bytes(g.h, dim, batch) // 8 + 8, dtype=torch.int64, device="cuda")
    A0, A1, B0, B1, t0, t1 = big(), big(), big(), big(), big(), big()
    P, s, L = g._ptr, g._stream(), g.lib
    ck = _native.check

    def new_pk():
        ck(L.gpq_he_enc_pk(g.h, P(B0), P(B1), P(m), P(v), P(e0), P(e1), P(pk_ntt[0]), P(pk_ntt[1]), W, logq, dim, batch, P(ws_pk), s), "gpq_he_enc_pk")

    def old_pk():
        ck(L.gpq_small_to_big(g.h, P(t0), P(v), W, batch, s), "gpq_small_to_big")
        ck(L.gpq_poly_mul(g.h, P(A0), P(p0_rep), P(t0), W, dim, logq, batch, P(ws_mul), s), "gpq_poly_mul")
        ck(L.gpq_poly_mul(g.h, P(A1), P(p1_rep), P(t0), W, dim, logq, batch, P(ws_mul), s), "gpq_poly_mul")
        ck(L.gpq_big_addsub(g.h, P(A0), P(A0), P(m), W, batch, 0, s), "gpq_big_addsub")
        ck(L.gpq_small_to_big(g.h, P(t0), P(e0), W, batch, s), "gpq_small_to_big")
        ck(L.gpq_big_addsub(g.h, P(A0), P(A0), P(t0), W, batch, 0, s), "gpq_big_addsub")
        ck(L.gpq_small_to_big(g.h, P(t1), P(e1), W, batch, s), "gpq_small_to_big")
        ck(L.gpq_big_addsub(g.h, P(A1), P(A1), P(t1), W, batch, 0, s), "gpq_big_addsub")
        ck(L.gpq_he_rs(g.h, P(A0), P(A1), W, 0, logq, batch, s), "gpq_he_rs")

    def new_sk():
        ck(L.gpq_he_enc_sk(g.h, P(B0), P(B1), P(m), P(a), P(e0), P(sk_ntt), W, logq, dim, batch, P(ws_sk), s), "gpq_he_enc_sk")

    def old_sk():
        ck(L.gpq_poly_mul(g.h, P(A0), P(a), P(sk_rep), W, dim, logq, batch, P(ws_mul), s), "gpq_poly_mul")
        ck(L.gpq_big_addsub(g.h, P(A0), P(A0), None, W, batch, 2, s), "gpq_big_addsub")
        ck(L.gpq_big_addsub(g.h, P(A0), P(A0), P(m), W, batch, 0, s), "gpq_big_addsub")
        ck(L.gpq_small_to_big(g.h, P(t0), P(e0), W, batch, s), "gpq_small_to_big")
        ck(L.gpq_big_addsub(g.h, P(A0), P(A0), P(t0), W, batch, 0, s), "gpq_big_addsub")
        ck(L.gpq_copy(P(A1), P(a), a.numel() * 8, s), "gpq_copy")
        ck(L.gpq_he_rs(g.h, P(A0), P(A1), W, 0, logq, batch, s), "gpq_he_rs")

    for label, old, new in (("he_enc_pk", old_pk, new_pk), ("he_enc_sk", old_sk, new_sk)):
        interleave(label, {"existing": old, "new": new}, reps)
        old()
        new()
        torch.cuda.synchronize()
        print("# %s: same words: %s" % (label, torch.equal(A0, B0) and torch.equal(A1, B1)))
    mhz = sclk(new_pk)
    print("# shader clock while gpq_he_enc_pk runs: %s" % ("%d MHz" % mhz if mhz else "not read (no rocm-smi)"))

    # the samplers: input bytes per second, all bytes moved per second, and the copy of as many bytes
    outs, outb = small(), big()
    legs = (("gpq_sample_zo", lambda: g.sample_zo(outs, zb), zb.numel(), outs.numel()),
            ("gpq_sample_error", lambda: g.sample_error(outs, eb), eb.numel(), outs.numel()),
            ("gpq_sample_uniform", lambda: g.sample_uniform(outb, ub, nbits, W), ub.numel(), outb.numel() * 8))
    for name, fn, nin, nout in legs:
        moved = (nin + nout) // 32 * 16                                    # the copy reads and writes this many bytes each
        src, dst = torch.empty(moved, dtype=torch.uint8, device="cuda"), torch.empty(moved, dtype=torch.uint8, device="cuda")
        copy = lambda: ck(L.gpq_probe_stream(P(dst), P(src), moved, 0, 2048, 256, 4, s), "gpq_probe_stream")
        fn(); fn(); copy(); copy()
        tf, tc = [], []
        for _ in range(reps):
            tf.append(event_ms(fn))
            tc.append(event_ms(copy))
        mf, mc = statistics.median(tf), statistics.median(tc)
        print("%-20s median %8.4f ms  input %7.1f GB/s  in + out %7.1f GB/s   | copy of %d bytes in + out: %8.4f ms  %7.1f GB/s" % (
            name, mf, nin / mf / 1e6, (nin + nout) / mf / 1e6, 2 * moved, mc, 2 * moved / mc / 1e6))
    g.close()


if __name__ == "__main__":
    main()
