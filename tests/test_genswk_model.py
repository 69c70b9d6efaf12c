"""The model of he_genswk (tests/genswk_model.py) against the EXECUTED reference, the structured reduction of gpq_he_genswk_batch
against the model, and the window inputs against their own list.  No GPU."""
import random

import pytest

from oracle import ref
from tests import genswk_jobs
from tests import genswk_model as gm
from tests.ref_jobs import require_reference

KS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
LOGN = 7


@pytest.fixture(scope="module")
def primes(oracle_ctx):
    return [int(p) for p in oracle_ctx(LOGN, 12).p]


def _dimP(k):
    return (k + 1 + LOGN) // 59 + 1                                      # hectx.dim, src/precomp.c:401


def test_model_equals_the_executed_reference_pieces():
    """(a) logn 7: poly_rot / poly_conj / poly_mul / mpi_smod / rns_decompose / ntt of the reference, chained as src/he-kem.c:83-110"""
    require_reference()
    jobs = [(7, 120, "s2", 1), (7, 120, "0", 2), (7, 120, "5", 3), (7, 63, "conj", 4), (7, 64, "67", 5)]
    for job, diffs in zip(jobs, ref.run(genswk_jobs.check_genswk, jobs, workers=5)):
        assert not diffs, "%s: %s" % (job, diffs)


@pytest.mark.parametrize("k", KS)
def test_structured_steps_equal_the_model(primes, k):
    """(b) steps 2-4 in integers on the window inputs (both hidden forms) and on random inputs, ternary and large hidden polynomials"""
    n, dimP = 1 << LOGN, _dimP(k)
    P = gm.product_of(primes[:dimP])
    dimmul = gm.dimmul_of(P, k, LOGN)
    assert dimmul <= len(primes)
    one = [1] + [0] * (n - 1)
    for sp in (None, one):
        p1, e, spv = gm.window_inputs(P, k, n, sp=sp)
        assert gm.structured(P, k, primes, p1, e, spv, one, dimmul) == gm.genswk(P, k, primes, p1, e, spv, one, dimmul, dimmul)
    rng = random.Random(k)
    for trial in range(2):
        sk = [rng.choice((-1, 0, 1)) for _ in range(n)]
        p1 = [rng.randrange(1 << gm.nbits_of(P, k)) for _ in range(n)]
        e = [rng.randrange(-11, 12) for _ in range(n)]
        sp = gm.galois_image(sk, pow(5, 3, 1 << 64)) if trial else [rng.randrange(-(1 << k), 1 << k) for _ in range(n)]
        assert gm.structured(P, k, primes, p1, e, sp, sk, dimmul) == gm.genswk(P, k, primes, p1, e, sp, sk, dimmul, dimmul)
    # a "secret" large enough for p1 sk to wrap the dimmul-limb basis: both follow the value centred mod P'
    sk = [rng.randrange(-(1 << 60), 1 << 60) for _ in range(n)]
    p1 = [rng.randrange(1 << gm.nbits_of(P, k)) for _ in range(n)]
    Pp = gm.product_of(primes[:dimmul])
    assert any(abs(v) > Pp // 2 for v in gm.negacyclic(p1, sk))
    assert gm.structured(P, k, primes, p1, e, sp, sk, dimmul) == gm.genswk(P, k, primes, p1, e, sp, sk, dimmul, dimmul)


@pytest.mark.parametrize("k", KS)
def test_window_inputs_hit_every_window(primes, k):
    """(c) every listed window occurs at least once, in both hidden forms: the GPU test cannot pass without exercising them"""
    n, dimP = 1 << LOGN, _dimP(k)
    P = gm.product_of(primes[:dimP])
    one = [1] + [0] * (n - 1)
    for sp in (None, one):
        p1, e, spv = gm.window_inputs(P, k, n, sp=sp)
        stats = {}
        gm.structured(P, k, primes, p1, e, spv, one, gm.dimmul_of(P, k, LOGN), stats=stats)
        assert stats["aX"] == [v % P for v in p1]                         # sk = 1: X = p1
        assert not gm.windows_missing(P, k, stats, p1)


def test_galois_image_is_poly_rot_and_poly_conj():
    from oracle import bigint_ref as br
    rng = random.Random(5)
    a = [rng.randrange(-9, 10) for _ in range(64)]
    for rot in (0, 1, 5, 31, 32, 40):
        assert gm.galois_image(a, pow(5, rot, 1 << 64)) == br.poly_rot(a, rot)
    assert gm.galois_image(a, 2 * 64 - 1) == br.poly_conj(a)
