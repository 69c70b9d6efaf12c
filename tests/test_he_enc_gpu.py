"""gpq_he_enc_pk / gpq_he_enc_sk: he_enc_pk, he_enc_sk (src/he-encrypt.c:37-103) and he_keypair's arithmetic (src/he-kem.c:59-65) on the device.

Word for word against the sequence the library already had -- gpq_poly_mul with the key replicated per ciphertext, gpq_big_addsub,
gpq_he_rs(logDelta 0), which the existing tests pin to the reference -- at test_he_dec_gpu.py's shapes, the dense key whose product with the
RAW uniform sample exceeds the basis included; against the record of the executed reference (tests/golden/ref_enc.json) fed with the
recorded stream's slices; against the Python-integer model (tests/enc_model.py) at logn 7 with q of one bit up to 2^850, at, one below and
one above a word boundary, with more words than q needs, and at n = 2^13 with eight limbs; over more launch groups than one; inputs
preserved; the refusals; and encode -> encrypt -> decrypt -> decode on the device inside the reference's own noise bound, at the top level
and one level down."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest
import torch

from gpqhe_amd import to_device, to_host
from oracle.expect import ints_to_words
from tests import enc_model, enc_record

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A5A5A5A5A


def _big(values, W, n):
    return to_device(np.concatenate([ints_to_words(values[k * n:(k + 1) * n], W) for k in range(len(values) // n)]))


def _centred(rng, logq, count):
    half = 1 << (logq - 1)
    return [int.from_bytes(rng.bytes((logq + 7) // 8), "little") % (1 << logq) - half for _ in range(count)]


def _raw(rng, logq, count):
    """what sample_uniform(q = 2^logq) hands out: logq + 1 bits, not reduced"""
    return [int.from_bytes(rng.bytes((logq + 8) // 8), "little") % (1 << (logq + 1)) for _ in range(count)]


def _small(rng, lo, hi, count):
    return torch.from_numpy(rng.integers(lo, hi + 1, count, dtype=np.int8)).cuda()


def _key_slab(g, big, W, dim):
    """gpq_evk_pack of ONE polynomial's big slab: uint64[dim][n]"""
    out = torch.empty(dim * g.n, dtype=torch.int64, device="cuda")
    assert g.lib.gpq_evk_pack(g.h, C.c_void_p(out.data_ptr()), C.c_void_p(big.data_ptr()), W, dim, 1, g._stream()) == 0
    return out


def _outputs(like):
    return torch.full_like(like, PATTERN), torch.full_like(like, PATTERN)


def _small_big(g, small, W):
    """an int8 small slab as a big slab, converted on the HOST (the reference path uses nothing of the new entry points)"""
    return _big([int(t) for t in small.cpu().numpy()], W, g.n)


def _existing_sk(g, m, a, e, sk, W, logq, dim, batch):
    """(c0, c1) by the entry points the library already had, the key replicated `batch` times"""
    c0, c1 = torch.empty_like(a), a.clone()
    g.poly_mul(c0, a, _big(sk * batch, W, g.n), W, dim, logq)                   # the RAW sample is multiplied, src/he-encrypt.c:91
    g.big_addsub(c0, c0, None, W, 2)                                           # :93
    g.big_addsub(c0, c0, m, W, 0)                                              # :94
    g.big_addsub(c0, c0, _small_big(g, e, W), W, 0)                            # :95
    g.he_rs(c0, c1, W, 0, logq)                                                # :96-97
    torch.cuda.synchronize()
    return to_host(c0), to_host(c1)


def _existing_pk(g, m, v, e0, e1, pk, W, logq, dim, batch):
    vb = _small_big(g, v, W)
    c0, c1 = torch.empty_like(m), torch.empty_like(m)
    g.poly_mul(c0, _big(pk[0] * batch, W, g.n), vb.clone(), W, dim, logq)      # src/he-encrypt.c:58
    g.poly_mul(c1, _big(pk[1] * batch, W, g.n), vb.clone(), W, dim, logq)      # :59
    g.big_addsub(c0, c0, m, W, 0)                                              # :61
    g.big_addsub(c0, c0, _small_big(g, e0, W), W, 0)                           # :62
    g.big_addsub(c1, c1, _small_big(g, e1, W), W, 0)                           # :63
    g.he_rs(c0, c1, W, 0, logq)                                                # :64-65
    torch.cuda.synchronize()
    return to_host(c0), to_host(c1)


def _inputs(g, rng, logq, W, batch, dense):
    n = g.n
    sk = [int(t) for t in (rng.choice([-1, 1], n) if dense else rng.integers(-1, 2, n))]
    a_ints = _raw(rng, logq, batch * n)
    return dict(sk=sk, a_ints=a_ints, a=_big(a_ints, W, n), m=_big([int(t) for t in rng.integers(-(1 << 40), 1 << 40, batch * n)], W, n),
                e=_small(rng, -11, 11, batch * n), e1=_small(rng, -11, 11, batch * n), v=_small(rng, -1, 1, batch * n),
                pk=(_centred(rng, logq, n), _centred(rng, logq, n)))


@pytest.mark.parametrize("logn,logq,batch,dense", [(9, 100, 3, False), (9, 117, 3, False), (13, 100, 2, False), (9, 116, 2, True)],
                         ids=["logn9_dim2", "logn9_dim3", "logn13_two_pass", "dense_key_wraps_the_basis"])
def test_words_equal_the_existing_entry_points(engine_ctx, logn, logq, batch, dense):
    dim, W = (logq + 1) // 59 + 1, (logq + 64) // 64
    assert dim == {100: 2, 116: 2, 117: 3}[logq]
    g = engine_ctx(logn, 6)
    n, rng = g.n, np.random.default_rng(2000 * logn + logq + dense)
    x = _inputs(g, rng, logq, W, batch, dense)
    if dense:                                                                  # the exact product of the RAW sample does not fit the dim-limb basis:
        top = sum(x["a_ints"][i] * x["sk"][n - 1 - i] for i in range(n))       # coefficient n - 1 (no wrapped term) exceeds P/2
        assert 2 * abs(top) > int(g.p[0]) * int(g.p[1]) and dim == 2
        assert sum(t >= 1 << logq for t in x["a_ints"]) > n // 4                # and the sample really is uncentred
    x["sk_slab"] = _key_slab(g, _big(x["sk"], W, n), W, dim)
    x["pk0_slab"], x["pk1_slab"] = [_key_slab(g, _big(p, W, n), W, dim) for p in x["pk"]]
    sk_slab, pk_slabs = x["sk_slab"], [x["pk0_slab"], x["pk1_slab"]]
    before = {k: x[k].clone() for k in ("a", "m", "e", "e1", "v", "sk_slab", "pk0_slab", "pk1_slab")}
    c0, c1 = _outputs(x["a"])
    g.he_enc_sk(c0, c1, x["m"], x["a"], x["e"], sk_slab, W, logq, dim)
    d0, d1 = _outputs(x["a"])
    g.he_enc_pk(d0, d1, x["m"], x["v"], x["e"], x["e1"], pk_slabs[0], pk_slabs[1], W, logq, dim)
    k0, k1 = _outputs(x["a"])
    g.he_enc_sk(k0, k1, None, x["a"], x["e"], sk_slab, W, logq, dim)           # he_keypair: no plaintext
    torch.cuda.synchronize()
    got = [to_host(t) for t in (c0, c1, d0, d1, k0, k1)]
    exp = list(_existing_sk(g, x["m"], x["a"], x["e"], x["sk"], W, logq, dim, batch))
    exp += list(_existing_pk(g, x["m"], x["v"], x["e"], x["e1"], x["pk"], W, logq, dim, batch))
    exp += list(_existing_sk(g, torch.zeros_like(x["m"]), x["a"], x["e"], x["sk"], W, logq, dim, batch))
    for name, a, b in zip(("enc_sk c0", "enc_sk c1", "enc_pk c0", "enc_pk c1", "keypair p0", "keypair p1"), got, exp):
        bad = np.flatnonzero(a != b)
        assert not len(bad), "%s: %d words differ, first at %d" % (name, len(bad), bad[0])
    for k, t in before.items():                                                # inputs preserved
        assert torch.equal(t, x[k]), k
    assert len(set(got[0].reshape(batch, -1)[:, 0].tolist())) == batch          # (the ciphertexts of the batch differ)
    assert not np.array_equal(got[1], to_host(x["a"]))                         # (c1 is the CENTRED sample)


def _sha(words):
    return hashlib.sha256(np.ascontiguousarray(words).tobytes()).hexdigest()


@pytest.mark.parametrize("case", enc_record.CASES, ids=enc_record.case_name)
def test_words_equal_the_record_of_the_executed_reference(engine_ctx, case):
    """he_keypair, he_enc_sk, he_enc_pk and he_dec on the slices of the recorded stream the reference's own calls consumed (sample_sk is the
    host's: the model's, from the same stream)"""
    logn, logq = case
    rec = enc_record.enc_golden()["cases"][enc_record.case_name(case)]
    dim, dimdec = enc_model.he_dim(logn, 1 << logq), (logq + 1) // 59 + 1
    g = engine_ctx(logn, max(6, dim))                                          # (7, 438) needs eight limbs
    n, W, nbits = g.n, rec["W"], logq + 1
    nb = nbits // 8 + 1
    assert W == enc_record.words(logq) and dimdec <= dim <= len(g.p)
    host = enc_model.Stream(enc_record.stored_stream())
    dev = torch.from_numpy(host.data).cuda()

    def take(count):
        pos = host.pos
        host.take(count)
        return dev[pos:pos + count]

    def check(names, tensors):
        torch.cuda.synchronize()
        for name, t in zip(names, tensors):
            assert _sha(to_host(t)) == rec["sha256"][name], name

    small = lambda: torch.empty(n, dtype=torch.int8, device="cuda")
    big = lambda: torch.full((W * n,), PATTERN, dtype=torch.int64, device="cuda")
    sk = enc_model.sample_hwt(host, n)
    assert enc_record.sha(sk, W) == rec["sha256"]["sk"]
    sk_big = _big(sk, W, n)
    e, a = g.sample_error(small(), take(n)), g.sample_uniform(big(), take(n * nb), nbits, W)
    p0, p1 = g.he_enc_sk(big(), big(), None, a, e, _key_slab(g, sk_big, W, dim), W, logq, dim)
    check(("p0", "p1"), (p0, p1))
    assert host.pos == rec["pos"]["he_keypair"]
    host.take(enc_record.PROBE)
    m = _big(enc_record.case_plaintext(case), W, n)
    e, a = g.sample_error(small(), take(n)), g.sample_uniform(big(), take(n * nb), nbits, W)
    s0, s1 = g.he_enc_sk(big(), big(), m, a, e, _key_slab(g, sk_big, W, dim), W, logq, dim)
    check(("sk_c0", "sk_c1"), (s0, s1))
    assert host.pos == rec["pos"]["he_enc_sk"]
    host.take(enc_record.PROBE)
    v, e0, e1 = g.sample_zo(small(), take(n // 4)), g.sample_error(small(), take(n)), g.sample_error(small(), take(n))
    q0, q1 = g.he_enc_pk(big(), big(), m, v, e0, e1, _key_slab(g, p0, W, dim), _key_slab(g, p1, W, dim), W, logq, dim)
    check(("pk_c0", "pk_c1"), (q0, q1))
    assert host.pos == rec["pos"]["he_enc_pk"]
    key = _key_slab(g, sk_big, W, dimdec)
    check(("dec_sk", "dec_pk"), (g.he_dec(big(), s0, s1, key, W, logq, dimdec), g.he_dec(big(), q0, q1, key, W, logq, dimdec)))


# (logq, W, which entry points, the enc_tail_k branch the shape is there for, the precondition that makes it take that branch)
#   "p" = gpq_he_enc_pk, "s" = gpq_he_enc_sk (64 W > logq + 1: the raw sample of logq + 1 bits stays non-negative), he_keypair's form with it
_ONE_WORD = lambda logq, W: W == 1 and logq < 64                              # the only word holds bit logq - 1 AND straddles logq
_ONE_WORD_MOST = lambda logq, W: W == 1 and logq in (62, 63)                  # the most one word takes: 64 W > logq (enc_pk), > logq + 1 (enc_sk)
_TOP_BIT = lambda logq, W: logq % 64 == 63 and 64 * W - logq >= 64            # bit logq - 1 is bit 62 of a word; with W > 1 a sign-fill word follows
_FULL_WORD = lambda logq, W: logq % 64 == 0 and W == logq // 64 + 1           # no word straddles logq: the masking branch is skipped, the last word is sign fill
_ONE_BIT = lambda logq, W: logq % 64 == 1 and W == logq // 64 + 1             # the straddling word keeps ONE bit, which is the sign bit
_WORKLOAD = lambda logq, W: W == logq // 64 + 1 and (logq + 1) // 59 + 1 >= 8  # the workload's moduli: the least W, eight limbs or more
_SLACK = lambda logq, W: 64 * W - logq >= 128                                 # two words or more at or above logq: sign fill (lo >= logq), a rescaled level
MODEL_SHAPES = [(1, 1, "p", _ONE_WORD), (2, 1, "ps", _ONE_WORD), (62, 1, "s", _ONE_WORD_MOST), (63, 1, "p", _ONE_WORD_MOST),
                (63, 2, "ps", _TOP_BIT), (64, 2, "ps", _FULL_WORD), (65, 2, "ps", _ONE_BIT),
                (127, 3, "ps", _TOP_BIT), (128, 3, "ps", _FULL_WORD), (129, 3, "ps", _ONE_BIT),
                (438, 7, "ps", _WORKLOAD), (850, 14, "ps", _WORKLOAD),
                (100, 4, "ps", _SLACK), (64, 3, "ps", _SLACK), (438, 9, "ps", _SLACK)]


def _crossing(x, e, half, picks=2):
    """{i: m_i} for a few coefficients of ONE polynomial, chosen so that sign x_i + m_i + e_i lands on half or just above (smod wraps it down)
    and on -half - 1 or just below (wraps it up); `x` is the centred product with its sign applied, so |m_i| <= half + 14 fits logq + 1 bits"""
    up = [i for i, v in enumerate(x) if v >= 0][:picks]
    down = [i for i, v in enumerate(x) if v < 0][:picks]
    assert len(up) == picks and len(down) == picks
    m = {i: half - x[i] - int(e[i]) + 3 * k for k, i in enumerate(up)}
    m.update({i: -half - 1 - x[i] - int(e[i]) - 3 * k for k, i in enumerate(down)})
    return m


def _wraps(sums, half):
    return sum(v >= half for v in sums), sum(v < -half for v in sums)


@pytest.mark.parametrize("logq,W,which,branch", MODEL_SHAPES, ids=["q%d_w%d" % t[:2] for t in MODEL_SHAPES])
def test_words_equal_the_model_at_word_edges_and_wide_slabs(engine_ctx, oracle_ctx, logq, W, which, branch):
    """gpq_he_enc_sk (with and without a plaintext) and gpq_he_enc_pk against Python integers (enc_model.enc_sk_from / enc_pk_from) at logn 7,
    batch 3 (the key switch of enc_pk runs its pair form and its single form); a few plaintext coefficients are built so that the sum
    crosses +-2^(logq-1) in both directions"""
    logn, batch = 7, 3
    assert branch(logq, W) and 64 * W > logq
    q, half = 1 << logq, 1 << (logq - 1)
    dim = enc_model.he_dim(logn, q)
    g, o = engine_ctx(logn, 16), oracle_ctx(logn, 16)
    assert g.p == o.p and dim <= 16
    n, rng = g.n, np.random.default_rng(7000 + 40 * logq + W)
    x = _inputs(g, rng, logq, W, batch, False)
    e, e1, v = (x[k].cpu().numpy().reshape(batch, n) for k in ("e", "e1", "v"))
    a = [x["a_ints"][k * n:(k + 1) * n] for k in range(batch)]
    assert e.min() < 0 < e.max() and e1.min() < 0 < e1.max()
    names, got, exp, before = [], [], [], {}

    def run(call, name, m_ints, tensors):
        m = None if m_ints is None else _big([t for row in m_ints for t in row], W, n)
        if m_ints is not None:
            flat = [t for row in m_ints for t in row]
            assert min(flat) < 0 < max(flat)                                    # the plaintext has both signs
            tensors = dict(tensors, m=m)
        before.update({name + " " + k: (t, t.clone()) for k, t in tensors.items()})
        c0, c1 = _outputs(x["a"])                                               # poisoned
        call(c0, c1, m)
        names.extend((name + " c0", name + " c1"))
        got.extend((c0, c1))

    def plaintext(built):
        m = [int(t) for t in rng.integers(-(1 << 40), 1 << 40, n)]
        for i, t in built.items():
            m[i] = t
        return m

    if "s" in which:
        assert 64 * W > logq + 1
        sk_slab = _key_slab(g, _big(x["sk"], W, n), W, dim)
        xs = [[-t for t in enc_model.poly_mul(o, a[k], x["sk"], dim, q)] for k in range(batch)]                 # -a s, src/he-encrypt.c:91-93
        m_sk = [plaintext(_crossing(xs[k], e[k], half)) for k in range(batch)]
        up, down = _wraps([xs[k][i] + m_sk[k][i] + int(e[k][i]) for k in range(batch) for i in range(n)], half)
        assert up >= 2 * batch and down >= 2 * batch                            # smod wraps in both directions
        assert sum(t >= half for t in x["a_ints"]) > n // 4                     # and c1 = smod(a) wraps the raw sample
        ins = {"a": x["a"], "e": x["e"], "sk": sk_slab}
        run(lambda c0, c1, m: g.he_enc_sk(c0, c1, m, x["a"], x["e"], sk_slab, W, logq, dim), "enc_sk", m_sk, ins)
        run(lambda c0, c1, m: g.he_enc_sk(c0, c1, None, x["a"], x["e"], sk_slab, W, logq, dim), "keypair", None, ins)
        for m_rows in (m_sk, [None] * batch):
            pairs = [enc_model.enc_sk_from(o, m_rows[k], a[k], e[k], x["sk"], dim, q) for k in range(batch)]
            exp.extend(([t for c in pairs for t in c[0]], [t for c in pairs for t in c[1]]))
    if "p" in which:
        pk_slabs = [_key_slab(g, _big(p, W, n), W, dim) for p in x["pk"]]
        x0 = [enc_model.poly_mul(o, x["pk"][0], [int(t) for t in v[k]], dim, q) for k in range(batch)]          # pk0 v, src/he-encrypt.c:58
        m_pk = [plaintext(_crossing(x0[k], e[k], half)) for k in range(batch)]
        up, down = _wraps([x0[k][i] + m_pk[k][i] + int(e[k][i]) for k in range(batch) for i in range(n)], half)
        assert up >= 2 * batch and down >= 2 * batch
        ins = {"v": x["v"], "e0": x["e"], "e1": x["e1"], "pk0": pk_slabs[0], "pk1": pk_slabs[1]}
        run(lambda c0, c1, m: g.he_enc_pk(c0, c1, m, x["v"], x["e"], x["e1"], pk_slabs[0], pk_slabs[1], W, logq, dim), "enc_pk", m_pk, ins)
        pairs = [enc_model.enc_pk_from(o, m_pk[k], v[k], e[k], e1[k], x["pk"], dim, q) for k in range(batch)]
        exp.extend(([t for c in pairs for t in c[0]], [t for c in pairs for t in c[1]]))
    torch.cuda.synchronize()
    for name, t, want in zip(names, got, exp):
        assert all(-half <= w < half for w in want)
        words, want = to_host(t), np.concatenate([ints_to_words(want[k * n:(k + 1) * n], W) for k in range(batch)])
        bad = np.flatnonzero(words != want)
        assert not len(bad), "%s: %d words differ from the model, first at %d (ciphertext, word, coefficient = %s)" % (
            name, len(bad), bad[0], (bad[0] // (W * n), bad[0] // n % W, bad[0] % n))
    for name, (t, kept) in before.items():                                      # inputs preserved
        assert torch.equal(t, kept), name


def _sparse_terms(rng, n, count):
    """`count` distinct positions with signs: a sparse polynomial in {-1, 0, 1}^n, x^0 and x^(n-1) among the positions"""
    pos = [0, n - 1] + [int(t) for t in rng.choice(np.arange(1, n - 1), count - 2, replace=False)]
    return [(k, int(rng.choice([-1, 1]))) for k in pos]


def test_two_pass_ring_with_eight_limbs_against_sparse_products(engine_ctx):
    """logn 13, q = 2^438, W = 7, batch 2: the two-pass NTT, gpq_rns_mul_shared, small_to_rns_k and the key switch of enc_pk with eight limbs.
    The secret and v are sparse, so the products are exact shifted sums of Python integers (_sparse_negacyclic); they fit the basis, so
    poly_rns2mpi's centring mod P is the identity and the model is smod(product + ..., q)"""
    from tests.test_ckks_roundtrip_gpu import _dense_of, _sparse_negacyclic
    logn, logq, W, batch = 13, 438, 7, 2
    q, dim = 1 << logq, enc_model.he_dim(logn, 1 << logq)
    assert dim == 8 and W == logq // 64 + 1
    g = engine_ctx(logn, dim)
    n, rng = g.n, np.random.default_rng(13438)
    P = 1
    for p in g.p[:dim]:
        P *= int(p)
    smod = lambda t: enc_model.br.mpi_smod(t, q)
    sk_terms, v_terms = _sparse_terms(rng, n, 5), [_sparse_terms(rng, n, 4) for _ in range(batch)]
    sk = _dense_of(sk_terms, n)
    a = [_raw(rng, logq, n) for _ in range(batch)]
    pk = (_centred(rng, logq, n), _centred(rng, logq, n))
    m = [[int(t) for t in rng.integers(-(1 << 40), 1 << 40, n)] for _ in range(batch)]
    e, e1 = (rng.integers(-11, 12, (batch, n), dtype=np.int8) for _ in range(2))
    v = np.array([_dense_of(t, n) for t in v_terms], dtype=np.int8)
    xs = [_sparse_negacyclic(a[k], sk_terms, n) for k in range(batch)]
    x0, x1 = ([_sparse_negacyclic(p, v_terms[k], n) for k in range(batch)] for p in pk)
    assert all(2 * abs(t) < P for rows in (xs, x0, x1) for row in rows for t in row)                            # the products fit the basis
    want = [[smod(-xs[k][i] + m[k][i] + int(e[k][i])) for k in range(batch) for i in range(n)], [smod(t) for row in a for t in row],
            [smod(x0[k][i] + m[k][i] + int(e[k][i])) for k in range(batch) for i in range(n)],
            [smod(x1[k][i] + int(e1[k][i])) for k in range(batch) for i in range(n)]]
    flat = lambda rows: [t for row in rows for t in row]
    dm, da = _big(flat(m), W, n), _big(flat(a), W, n)
    de, de1, dv = (torch.from_numpy(t.reshape(-1)).cuda() for t in (e, e1, v))
    c0, c1 = _outputs(da)
    g.he_enc_sk(c0, c1, dm, da, de, _key_slab(g, _big(sk, W, n), W, dim), W, logq, dim)
    d0, d1 = _outputs(da)
    g.he_enc_pk(d0, d1, dm, dv, de, de1, _key_slab(g, _big(pk[0], W, n), W, dim), _key_slab(g, _big(pk[1], W, n), W, dim), W, logq, dim)
    torch.cuda.synchronize()
    for name, t, w in zip(("enc_sk c0", "enc_sk c1", "enc_pk c0", "enc_pk c1"), (c0, c1, d0, d1), want):
        bad = np.flatnonzero(to_host(t) != np.concatenate([ints_to_words(w[k * n:(k + 1) * n], W) for k in range(batch)]))
        assert not len(bad), "%s: %d words differ from the model, first at %d" % (name, len(bad), bad[0])


def test_batch_larger_than_the_launch_group(engine_ctx):
    """gpq_set_chunk(2) with batch 5 at the first two-pass ring: three launch groups, the same words"""
    logn, logq, batch = 13, 100, 5
    dim, W = 2, 2
    g = engine_ctx(logn, 6)
    n, rng = g.n, np.random.default_rng(135)
    x = _inputs(g, rng, logq, W, batch, False)
    sk_slab = _key_slab(g, _big(x["sk"], W, n), W, dim)
    pk_slabs = [_key_slab(g, _big(p, W, n), W, dim) for p in x["pk"]]
    runs = []
    try:
        for chunk in (32, 2):
            g.set_chunk(chunk)
            c0, c1 = _outputs(x["a"])
            g.he_enc_sk(c0, c1, x["m"], x["a"], x["e"], sk_slab, W, logq, dim)
            d0, d1 = _outputs(x["a"])
            g.he_enc_pk(d0, d1, x["m"], x["v"], x["e"], x["e1"], pk_slabs[0], pk_slabs[1], W, logq, dim)
            torch.cuda.synchronize()
            runs.append([to_host(t) for t in (c0, c1, d0, d1)])
    finally:
        g.set_chunk(32)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert not (runs[0][2] == np.uint64(PATTERN)).all()


def test_refusals(engine_ctx):
    logn, logq, batch, dim, W = 9, 100, 1, 2, 2
    g = engine_ctx(logn, 6)
    n = g.n
    c0, c1, m, a = (torch.zeros(batch * W * n, dtype=torch.int64, device="cuda") for _ in range(4))
    v, e0, e1 = (torch.zeros(batch * n, dtype=torch.int8, device="cuda") for _ in range(3))
    key0, key1 = (torch.zeros(6 * n, dtype=torch.int64, device="cuda") for _ in range(2))
    ws = torch.empty(max(g.lib.gpq_he_enc_workspace_bytes(g.h, 6, batch, 1), 8) // 8, dtype=torch.int64, device="cuda")
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def pk(c0_=c0, c1_=c1, m_=m, v_=v, e0_=e0, e1_=e1, k0=key0, k1=key1, W_=W, logq_=logq, dim_=dim, batch_=batch, ws_=ws):
        return g.lib.gpq_he_enc_pk(g.h, p(c0_), p(c1_), p(m_), p(v_), p(e0_), p(e1_), p(k0), p(k1), W_, logq_, dim_, batch_, p(ws_), g._stream())

    def sk(c0_=c0, c1_=c1, m_=m, a_=a, e_=e0, k=key0, W_=W, logq_=logq, dim_=dim, batch_=batch, ws_=ws):
        return g.lib.gpq_he_enc_sk(g.h, p(c0_), p(c1_), p(m_), p(a_), p(e_), p(k), W_, logq_, dim_, batch_, p(ws_), g._stream())

    for call in (pk, sk):
        assert call(W_=0) == -1 and call(W_=33) == -1 and call(W_=1) == -1     # W outside 1..32, 64 W <= logq
        assert call(logq_=128) == -1 and call(logq_=0) == -1
        assert call(batch_=0) == -1
        assert call(dim_=0) == -1 and call(dim_=7) == -1                       # a dim the context lacks
        assert call(c0_=None) == -1 and call(c1_=None) == -1 and call(ws_=None) == -1
        assert call(c0_=m) == -1 and call(c1_=m) == -1                         # an output overlaps an input
        assert call(c1_=c0) == -1                                              # the outputs overlap
    assert pk(v_=None) == -1 and pk(e0_=None) == -1 and pk(e1_=None) == -1 and pk(k0=None) == -1 and pk(k1=None) == -1
    assert pk(c0_=key0) == -1 and pk(c1_=key1) == -1
    assert sk(a_=None) == -1 and sk(e_=None) == -1 and sk(k=None) == -1
    assert sk(c0_=a) == -1 and sk(c1_=a) == -1 and sk(c0_=key0) == -1
    assert sk(logq_=127) == -1                                                 # the raw sample of 128 bits is not non-negative in two words
    assert g.lib.gpq_he_enc_workspace_bytes(None, dim, batch, 1) == 0
    assert pk() == 0 and sk() == 0 and pk(m_=None) == 0 and sk(m_=None) == 0   # the plaintext is optional
    torch.cuda.synchronize()


def _round_trip(engine_ctx, logq, logql, W):
    """gpq_he_ecd -> gpq_he_enc_pk at 2^logq -> (logql < logq: gpq_he_rs by 0 bits, the centring mod 2^logql he_rs leaves behind) ->
    gpq_he_dec at 2^logql -> gpq_he_dcd, all in W words, at logn 9, 16 slots, Delta 2^30: every slot within Bclean / Delta of the
    message, Bclean the reference's own bound for a key of Hamming weight 64 (src/precomp.c:413-415), evaluated here"""
    logn, slots, logDelta, batch = 9, 16, 30, 3
    dim, dimdec = enc_model.he_dim(logn, 1 << logq), (logql + 1) // 59 + 1
    g = engine_ctx(logn, max(6, dim))
    n, nbits = g.n, logq + 1
    nb = nbits // 8 + 1
    rng = np.random.default_rng(930)
    dev_bytes = lambda count: torch.from_numpy(rng.integers(0, 256, count + 1, dtype=np.uint8)).cuda()[1:]      # (odd addresses)
    sk = enc_model.sample_hwt(enc_model.Stream(rng.integers(0, 256, 4096, dtype=np.uint8)), n)
    sk_big = _big(sk, W, n)
    small = lambda k: torch.empty(k * n, dtype=torch.int8, device="cuda")
    big = lambda k: torch.empty(k * W * n, dtype=torch.int64, device="cuda")
    e, a = g.sample_error(small(1), dev_bytes(n)), g.sample_uniform(big(1), dev_bytes(n * nb), nbits, W)
    p0, p1 = g.he_enc_sk(big(1), big(1), None, a, e, _key_slab(g, sk_big, W, dim), W, logq, dim)                  # he_keypair
    z = torch.from_numpy(rng.uniform(-1, 1, (batch, slots)) + 1j * rng.uniform(-1, 1, (batch, slots))).cuda()
    with g.ecd_plan(slots) as plan:
        m = g.he_ecd(plan, big(batch), z, logDelta=logDelta, W=W)
        v, e0, e1 = g.sample_zo(small(batch), dev_bytes(batch * n // 4)), g.sample_error(small(batch), dev_bytes(batch * n)), g.sample_error(small(batch), dev_bytes(batch * n))
        c0, c1 = g.he_enc_pk(big(batch), big(batch), m, v, e0, e1, _key_slab(g, p0, W, dim), _key_slab(g, p1, W, dim), W, logq, dim)
        if logql < logq:
            g.he_rs(c0, c1, W, 0, logql)
        back = g.he_dec(big(batch), c0, c1, _key_slab(g, sk_big, W, dimdec), W, logql, dimdec)
        out = g.he_dcd(plan, torch.empty_like(z), back, float(1 << logDelta), W)
        torch.cuda.synchronize()
    sigma, h = enc_model.SIGMA, 64
    Bclean = 8 * math.sqrt(2) * sigma * n + 6 * sigma * math.sqrt(n) + 16 * sigma * math.sqrt(h * n)
    err = (out - z).abs().max().item()
    print("largest slot error %.3e, Bclean / Delta %.3e" % (err, Bclean / 2.0 ** logDelta))
    assert err <= Bclean / 2.0 ** logDelta
    assert not torch.equal(c0, m)                                              # (it is a ciphertext)
    assert err > 0


def test_encode_encrypt_decrypt_decode_on_the_device(engine_ctx):
    """q = 2^100 in two words, decrypted at the level it was encrypted at"""
    _round_trip(engine_ctx, 100, 100, 2)


def test_encode_encrypt_decrypt_decode_one_level_down(engine_ctx):
    """the hand-off a program makes after he_rs: encrypted at 2^438 in seven words, decrypted at 2^388 in the same seven words with seven
    limbs instead of eight; the same bound"""
    logq, logql, W = 438, 388, 7
    assert W == logq // 64 + 1 == logql // 64 + 1 and (logql + 1) // 59 + 1 < enc_model.he_dim(9, 1 << logq)
    _round_trip(engine_ctx, logq, logql, W)
