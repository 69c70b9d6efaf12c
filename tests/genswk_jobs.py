"""What tests/test_genswk_model.py runs inside a reference worker process (oracle/ref.py: one reference context per process): he_genswk's
body (src/he-kem.c:83-110) chained from the EXECUTED reference's own pieces -- poly_rot / poly_conj, poly_mul, mpi_smod, rns_decompose,
ntt -- next to the model (tests/genswk_model.py).  Returns the list of differences."""
import random

import numpy as np

from oracle import ref
from tests import genswk_model as gm


def check_genswk(arg):
    logn, logq, hidden, seed = arg
    R = ref.Ref().init(logn, 1 << logq, 8, 1 << 30)
    n, rng = R.n, random.Random(seed)
    P, PqL = R.he_P()
    primes = [R.node(d)["p"] for d in range(R.dimub)]
    assert PqL == P << logq and P == gm.product_of(primes[:R.dim])
    dimmul = gm.dimmul_of(P, logq, logn)
    W = PqL.bit_length() // 64 + 1
    sk = [rng.choice((-1, 0, 1)) for _ in range(n)]
    p1 = [rng.randrange(1 << PqL.bit_length()) for _ in range(n)]        # the raw sample: below 2^nbits, not below P q_L
    e = [rng.randrange(-11, 12) for _ in range(n)]
    if hidden == "s2":
        sp = R.poly_mul(sk, sk, (logq + 1) // 59 + 1, 1 << logq)          # he_genrlk, src/he-kem.c:130
        model_sp = gm.poly_mul(primes, sk, sk, (logq + 1) // 59 + 1, 1 << logq)
    elif hidden == "conj":
        sp, model_sp = R.poly_conj(sk, W), gm.galois_image(sk, 2 * n - 1)
    else:
        sp, model_sp = R.poly_rot(sk, int(hidden), W), gm.galois_image(sk, pow(5, int(hidden), 1 << 64))
    diffs = []
    if list(sp) != list(model_sp):
        diffs.append("hidden polynomial (%s)" % hidden)
    x = R.poly_mul(p1, sk, dimmul, PqL, Win=W)                            # :95
    v = [(-a + b + P * c) % PqL for a, b, c in zip(x, e, sp)]             # :89-90, :97-99
    p0, p1c = R.mpi_smod(v, PqL), R.mpi_smod(p1, PqL)                     # :100-101
    m0, m1 = gm.genswk(P, logq, primes, p1, e, model_sp, sk, dimmul, R.dimevk)
    if p0 != m0:
        diffs.append("swk.p0 (%s): %d coefficients" % (hidden, sum(a != b for a, b in zip(p0, m0))))
    if p1c != m1:
        diffs.append("swk.p1 (%s)" % hidden)
    s0, s1 = gm.genswk(P, logq, primes, p1, e, model_sp, sk, dimmul, R.dimevk, ntt=lambda d, r: R.ntt(np.array(r, dtype=np.uint64), d))
    for d in range(R.dimevk):                                             # :103-110
        for name, poly, slab in (("p0", p0, s0), ("p1", p1c, s1)):
            if not np.array_equal(R.ntt(R.rns_decompose(poly, d, W), d), slab[d]):
                diffs.append("stored %s, limb %d" % (name, d))
    return diffs
