"""gpq_he_genswk_batch against the path the library had before it, interleaved on ONE device.

(A) the existing entry points, key by key: gpq_poly_rot of the secret as the hidden polynomial, then gpq_he_genswk (the general product
    mod P q_L, two Barrett passes, two host synchronisations) -- what tests/test_he_genswk_batch_gpu.py compares the new call with word for
    word;
(B) one gpq_he_genswk_batch for all keys: the secret packed once, the hidden polynomials gathered by the kernel.
Shape: n = 2^16, q_L = 2^438, 64 rotation keys, every input resident on the device (A's error polynomials as big slabs, converted outside the
timed region).  Every repetition runs A then B, each timed by HIP events after a synchronisation; the median, the spread and the ratio of the
medians are printed, and whether both gave the same words.  `python tools/keygen_ab.py [reps] [logn] [logqL] [keys]`."""
import os
import statistics
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


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    logn, logq, keys = (int(v) for v in (sys.argv[2:5] + ["16", "438", "64"][len(sys.argv[2:5]):]))
    torch.cuda.set_device(0)
    probe = gpqhe_amd.PolyContext(logn, 12)
    dimP, _, _, dimevk = probe.he_dims(logq, logq)
    probe.close()
    g = gpqhe_amd.PolyContext(logn, dimevk)
    n = g.n
    P = 1
    for p in g.p[:dimP]:
        P *= p
    nbits = (P << logq).bit_length()
    W, nb, dimmul = nbits // 64 + 1, nbits // 8 + 1, g.he_genswk_dimmul(dimP, logq)
    print("# device %s, %d interleaved repetitions; n = 2^%d, q_L = 2^%d, dimP %d, dimmul %d, dimevk %d, W %d, %d rotation keys" % (
        torch.cuda.get_device_name(0), reps, logn, logq, dimP, dimmul, dimevk, W, keys))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(15)
    rand_bytes = lambda count: torch.randint(0, 256, (count,), dtype=torch.uint8, device="cuda", generator=gen)
    sk_small = torch.randint(-1, 2, (n,), dtype=torch.int8, device="cuda", generator=gen)
    sk_big = g.small_to_big(torch.empty(W * n, dtype=torch.int64, device="cuda"), sk_small, W)
    e = g.sample_error(torch.empty(keys * n, dtype=torch.int8, device="cuda"), rand_bytes(keys * n))
    e_big = g.small_to_big(torch.empty(keys * W * n, dtype=torch.int64, device="cuda"), e, W)
    p1 = torch.empty(keys * W * n, dtype=torch.int64, device="cuda")
    for j in range(keys):
        g.sample_uniform(p1[j * W * n:(j + 1) * W * n], rand_bytes(n * nb), nbits, W)
    sk_ntt = torch.empty(dimmul * n, dtype=torch.int64, device="cuda")
    _native.check(g.lib.gpq_evk_pack(g.h, g._ptr(sk_ntt), g._ptr(sk_big), W, dimmul, 1, g._stream()), "gpq_evk_pack")
    A0, A1, B0, B1 = (torch.empty(keys * dimevk * n, dtype=torch.int64, device="cuda") for _ in range(4))
    sp = torch.empty(W * n, dtype=torch.int64, device="cuda")
    ws_a = torch.empty(g.lib.gpq_he_genswk_workspace_bytes(g.h, W, dimP, logq) // 8 + 8, dtype=torch.int64, device="cuda")
    ws_b = torch.empty(g.lib.gpq_he_genswk_batch_workspace_bytes(g.h, W, dimP, logq, dimevk, keys) // 8 + 8, dtype=torch.int64, device="cuda")
    galois = (_native.C.c_uint64 * keys)(*[pow(5, r, 1 << 64) for r in range(keys)])
    Pt, s, L, ck = g._ptr, g._stream(), g.lib, _native.check
    big, evk = W * n, dimevk * n

    def existing():
        for j in range(keys):
            ck(L.gpq_poly_rot(g.h, Pt(sp), Pt(sk_big), W, j, 1, s), "gpq_poly_rot")
            ck(L.gpq_he_genswk(g.h, Pt(A0[j * evk:(j + 1) * evk]), Pt(A1[j * evk:(j + 1) * evk]), Pt(p1[j * big:(j + 1) * big]), Pt(sk_big),
                               Pt(e_big[j * big:(j + 1) * big]), Pt(sp), W, dimP, logq, dimevk, Pt(ws_a), s), "gpq_he_genswk")

    def batch():
        ck(L.gpq_he_genswk_batch(g.h, Pt(B0), Pt(B1), Pt(p1), Pt(e), Pt(sk_ntt), Pt(sk_small), galois, None, 0, W, dimP, logq, dimevk, keys, Pt(ws_b), s),
           "gpq_he_genswk_batch")

    fns = {"existing": existing, "batch": batch}
    for f in fns.values():                      # warm-up: workspaces, tables, code objects
        f()
        f()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            times[k].append(event_ms(f))
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print("%-10s median %10.3f ms  spread %10.3f .. %10.3f   %8.3f ms per key" % (k, med[k], min(v), max(v), med[k] / keys))
    print("ratio existing / batch = %.3f" % (med["existing"] / med["batch"]))
    torch.cuda.synchronize()
    print("# same words: %s" % (torch.equal(A0, B0) and torch.equal(A1, B1)))
    print("# per call of %d keys, from the shapes: forward transforms of the secret %d -> 0, host synchronisations %d -> 0, Barrett passes %d -> 0, "
          "uploads of sp %d -> 0" % (keys, keys, 2 * keys, 2 * keys, keys))
    g.close()


if __name__ == "__main__":
    main()
