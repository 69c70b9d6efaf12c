"""gpq_he_dec: he_dec (src/he-encrypt.c:105-125) on big slabs with ONE NTT-domain key slab shared by the batch.

Word for word against the sequence the library already had -- gpq_poly_mul with the key replicated per ciphertext, gpq_big_addsub,
gpq_he_rs(logDelta 0) -- at a single-pass ring with two and three limbs and at the first two-pass ring; with ternary keys, with a dense
key in {-1, 1}^n whose product exceeds the basis, and against the Python-integer restatement with a sparse key; against the model
(tests/enc_model.he_dec) at the encryptor's shapes -- q_l of one bit up to 2^850, at and next to word boundaries, with slack words -- and
one level down in the top level's words; at n = 2^13 with eight limbs; and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpqhe_amd import to_device, to_host
from oracle import bigint_ref
from oracle.expect import ints_to_words, words_to_ints
from tests import enc_model
from tests.test_he_enc_gpu import MODEL_SHAPES

pytestmark = pytest.mark.gpu


def _centred(rng, logql, count):
    """uniform centred coefficients mod 2^logql as Python integers"""
    half = 1 << (logql - 1)
    return [int.from_bytes(rng.bytes((logql + 7) // 8), "little") % (1 << logql) - half for _ in range(count)]


def _big(values, W, n):
    return to_device(np.concatenate([ints_to_words(values[k * n:(k + 1) * n], W) for k in range(len(values) // n)]))


def _key_slab(g, sk, W, dim):
    """gpq_evk_pack of the key's big slab, batch 1: uint64[dim][n]"""
    big, out = _big(sk, W, g.n), torch.empty(dim * g.n, dtype=torch.int64, device="cuda")
    assert g.lib.gpq_evk_pack(g.h, C.c_void_p(out.data_ptr()), C.c_void_p(big.data_ptr()), W, dim, 1, g._stream()) == 0
    return out


def _existing(g, c0, c1, sk, W, logql, dim, batch):
    """m by the entry points the library already had, the key replicated `batch` times"""
    skrep = _big(sk * batch, W, g.n)
    r, dummy = torch.empty_like(c1), torch.zeros_like(c1)
    g.poly_mul(r, c1, skrep, W, dim, logql)
    g.big_addsub(r, r, c0, W, 0)
    g.he_rs(r, dummy, W, 0, logql)
    torch.cuda.synchronize()
    return to_host(r)


def _run(g, c0, c1, sk, W, logql, dim, batch):
    m = torch.full_like(c1, 0x5A5A5A5A5A5A5A5A)
    g.he_dec(m, c0, c1, _key_slab(g, sk, W, dim), W, logql, dim)
    torch.cuda.synchronize()
    return to_host(m)


@pytest.mark.parametrize("logn,logql,batch,dense", [(9, 100, 3, False), (9, 117, 3, False), (13, 100, 2, False), (9, 116, 2, True)],
                         ids=["logn9_dim2", "logn9_dim3", "logn13_two_pass", "dense_key_wraps_the_basis"])
def test_words_equal_poly_mul_add_smod_with_the_key_replicated(engine_ctx, logn, logql, batch, dense):
    dim, W = (logql + 1) // 59 + 1, (logql + 64) // 64
    assert dim == {100: 2, 116: 2, 117: 3}[logql]
    g = engine_ctx(logn, 6)
    rng = np.random.default_rng(1000 * logn + logql + dense)
    sk = [int(v) for v in (rng.choice([-1, 1], g.n) if dense else rng.integers(-1, 2, g.n))]
    ints0, ints1 = _centred(rng, logql, batch * g.n), _centred(rng, logql, batch * g.n)
    if dense:                                                                 # the exact product does not fit the dim-limb basis: coefficient n - 1 (no wrapped term) exceeds P/2
        top = sum(ints1[i] * sk[g.n - 1 - i] for i in range(g.n))
        assert 2 * abs(top) > int(g.p[0]) * int(g.p[1]) and dim == 2
    c0, c1 = _big(ints0, W, g.n), _big(ints1, W, g.n)
    got, exp = _run(g, c0, c1, sk, W, logql, dim, batch), _existing(g, c0, c1, sk, W, logql, dim, batch)
    bad = np.flatnonzero(got != exp)
    assert not len(bad), "%d words differ, first at %d" % (len(bad), bad[0])
    assert np.array_equal(to_host(c0), np.concatenate([ints_to_words(ints0[k * g.n:(k + 1) * g.n], W) for k in range(batch)]))    # inputs preserved
    assert len(set(got.reshape(batch, -1)[:, 0].tolist())) == batch          # (the ciphertexts of the batch differ)


def test_sparse_key_against_python_integers(engine_ctx):
    logn, logql, batch = 9, 100, 2
    dim, W = (logql + 1) // 59 + 1, (logql + 64) // 64
    g = engine_ctx(logn, 6)
    n, rng = g.n, np.random.default_rng(216)
    terms = {0: 1, 5: -1, n - 1: 1}                                           # the key of tests/test_mpi_surface_gpu.py: 1 - x^5 + x^(n-1)
    sk = [terms.get(i, 0) for i in range(n)]
    ints0, ints1 = _centred(rng, logql, batch * n), _centred(rng, logql, batch * n)
    got = _run(g, _big(ints0, W, n), _big(ints1, W, n), sk, W, logql, dim, batch).reshape(batch, -1)
    for k in range(batch):
        want = bigint_ref.he_dec_sparse((ints0[k * n:(k + 1) * n], ints1[k * n:(k + 1) * n]), terms, 1 << logql)
        assert words_to_ints(got[k], W, n) == want, "ciphertext %d" % k


def _model_case(g, o, rng, logql, W, dim, batch):
    """gpq_he_dec of `batch` seeded ciphertexts centred mod 2^logql in W words against enc_model.he_dec: Python integers through the oracle's
    poly_mul.  A few c0 coefficients are built so that c1 s + c0 lands on 2^(logql-1) (smod wraps it down) and on -2^(logql-1) - 1 (up)"""
    n, ql, half = g.n, 1 << logql, 1 << (logql - 1)
    assert dim == (logql + 1) // 59 + 1                                       # the model's own dim, src/he-encrypt.c:113
    sk = [int(v) for v in rng.integers(-1, 2, n)]
    ints0, ints1 = _centred(rng, logql, batch * n), _centred(rng, logql, batch * n)
    ups = downs = 0
    for k in range(batch):
        x = enc_model.poly_mul(o, ints1[k * n:(k + 1) * n], sk, dim, ql)      # centred: c0 = +-half -+ ... - x stays inside [-half, half)
        up, down = [i for i, v in enumerate(x) if v > 0][:2], [i for i, v in enumerate(x) if v < 0][:2]
        for i in up:
            ints0[k * n + i] = half - x[i]
        for i in down:
            ints0[k * n + i] = -half - 1 - x[i]
        ups, downs = ups + len(up), downs + len(down)
    assert downs == 2 * batch and (ups == 2 * batch or logql == 1)            # (mod 2: x + c0 <= 0 never reaches half = 1)
    assert all(-half <= v < half for v in ints0 + ints1) and min(ints0) < 0 and min(ints1) < 0
    assert logql == 1 or (max(ints0) > 0 and max(ints1) > 0)                  # both signs (mod 2 the centred values are -1 and 0)
    c0, c1 = _big(ints0, W, n), _big(ints1, W, n)
    kept = c0.clone(), c1.clone()
    got = _run(g, c0, c1, sk, W, logql, dim, batch)                           # (into a poisoned output)
    want = [v for k in range(batch) for v in enc_model.he_dec(o, (ints0[k * n:(k + 1) * n], ints1[k * n:(k + 1) * n]), sk, ql)]
    assert all(-half <= v < half for v in want)
    bad = np.flatnonzero(got != np.concatenate([ints_to_words(want[k * n:(k + 1) * n], W) for k in range(batch)]))
    assert not len(bad), "%d words differ from the model, first at %d (ciphertext, word, coefficient = %s)" % (
        len(bad), bad[0], (bad[0] // (W * n), bad[0] // n % W, bad[0] % n))
    assert torch.equal(c0, kept[0]) and torch.equal(c1, kept[1])              # inputs preserved


DEC_SHAPES = [t for t in MODEL_SHAPES if "p" in t[2]]                         # gpq_he_enc_pk's shapes: 64 W > logql is all gpq_he_dec asks


@pytest.mark.parametrize("logql,W,which,branch", DEC_SHAPES, ids=["q%d_w%d" % t[:2] for t in DEC_SHAPES])
def test_words_equal_the_model_at_word_edges_and_wide_slabs(engine_ctx, oracle_ctx, logql, W, which, branch):
    """the encryptor's shapes (test_he_enc_gpu.MODEL_SHAPES, where each one's word-position branch and its precondition are listed): one
    word, logql one below / on / one above a word boundary, the workload's 2^438 and 2^850 with 8 and 15 limbs, and slack words"""
    assert branch(logql, W) and 64 * W > logql
    g, o = engine_ctx(7, 16), oracle_ctx(7, 16)
    assert g.p == o.p
    _model_case(g, o, np.random.default_rng(3000 + 40 * logql + W), logql, W, (logql + 1) // 59 + 1, 3)


@pytest.mark.parametrize("logql,W,fill", [(88, 7, 5), (64, 7, 6), (388, 7, 0), (30, 2, 1)], ids=["q88_w7", "q64_w7", "q388_w7", "q30_w2"])
def test_level_down_in_the_words_of_the_top_level(engine_ctx, oracle_ctx, logql, W, fill):
    """a rescaled ciphertext keeps the top level's W while logql shrinks: words centred mod 2^logql and sign-extended.  `fill` whole words
    lie at or above logql (the sign-fill branch of the final add): five after a straddling word, six after a full word (logql % 64 == 0),
    none at 2^388 (one level below 2^438: the same seven words, seven limbs where the top level has eight), one after a single word"""
    assert fill == W - (logql + 63) // 64 and (logql % 64 == 0) == (logql == 64)
    g, o = engine_ctx(7, 16), oracle_ctx(7, 16)
    _model_case(g, o, np.random.default_rng(4000 + 40 * logql + W), logql, W, logql // 59 + 1, 3)


def test_two_pass_ring_with_eight_limbs_against_sparse_products(engine_ctx):
    """logn 13, q = 2^438, W = 7, batch 2: the two-pass NTT and gpq_rns_mul_shared with eight limbs, against exact shifted sums"""
    logn, logql, W, batch = 13, 438, 7, 2
    dim = (logql + 1) // 59 + 1
    assert dim == 8 and W == logql // 64 + 1
    g = engine_ctx(logn, dim)
    n, rng = g.n, np.random.default_rng(13439)
    terms = {0: -1, 7: 1, 4099: 1, n - 2: -1, n - 1: 1}
    sk = [terms.get(i, 0) for i in range(n)]
    P = 1
    for p in g.p[:dim]:
        P *= int(p)
    assert 2 * len(terms) << (logql - 1) < P                                  # the product fits the basis: he_dec_sparse's exact sum is poly_mul's
    ints0, ints1 = _centred(rng, logql, batch * n), _centred(rng, logql, batch * n)
    got = _run(g, _big(ints0, W, n), _big(ints1, W, n), sk, W, logql, dim, batch).reshape(batch, -1)
    for k in range(batch):
        want = bigint_ref.he_dec_sparse((ints0[k * n:(k + 1) * n], ints1[k * n:(k + 1) * n]), terms, 1 << logql)
        assert np.array_equal(got[k], ints_to_words(want, W)), "ciphertext %d" % k


def test_refusals(engine_ctx):
    logn, logql, batch = 9, 100, 1
    dim, W = 2, 2
    g = engine_ctx(logn, 6)
    n = g.n
    c0, c1, m = (torch.zeros(batch * W * n, dtype=torch.int64, device="cuda") for _ in range(3))
    key = torch.zeros(6 * n, dtype=torch.int64, device="cuda")
    ws = torch.empty(g.lib.gpq_he_dec_workspace_bytes(g.h, 7, batch) // 8, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(m_, c0_, c1_, W_, logql_, dim_):
        return g.lib.gpq_he_dec(g.h, p(m_), p(c0_), p(c1_), p(key), W_, logql_, dim_, batch, p(ws), g._stream())
    assert call(m, c0, c1, W, 128, 3) == -1                                   # 64 W <= logql
    assert call(m, c0, c1, 1, 64, dim) == -1
    assert call(c0, c0, c1, W, logql, dim) == -1                              # an aliased output
    assert call(c1, c0, c1, W, logql, dim) == -1
    assert call(m, c0, c1, W, logql, 7) == -1                                 # dim beyond the context's limbs
    assert call(m, c0, c1, W, logql, 0) == -1
    assert call(m, c0, c1, W, logql, dim) == 0
    torch.cuda.synchronize()
