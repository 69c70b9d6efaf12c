"""gpq_he_dec: he_dec (src/he-encrypt.c:105-125) on big slabs with ONE NTT-domain key slab shared by the batch.

Word for word against the sequence the library already had -- gpq_poly_mul with the key replicated per ciphertext, gpq_big_addsub,
gpq_he_rs(logDelta 0) -- at a single-pass ring with two and three limbs and at the first two-pass ring; with ternary keys, with a dense
key in {-1, 1}^n whose product exceeds the basis, and against the Python-integer restatement with a sparse key; and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpqhe_amd import to_device, to_host
from oracle import bigint_ref
from oracle.expect import ints_to_words, words_to_ints

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
