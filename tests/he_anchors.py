"""Oracle anchors for the tests that compare two device settings with each other over several launch groups (gpq_set_chunk): the first and
the last ciphertext of every group, the short last group included, checked against the restated reference (oracle/expect.py, worker
processes).  A fault shared by both settings -- in how a group after the first, or the ragged tail, is handled -- fails here."""
import numpy as np

from oracle import expect


def group_ends(batch, chunk):
    """indices of the first and the last ciphertext of every launch group of `chunk` ciphertexts"""
    return sorted({k for k0 in range(0, batch, chunk) for k in (k0, min(k0 + chunk, batch) - 1)})


def _host(t):
    return t.detach().cpu().numpy().view(np.uint64)


def he_mul_tasks(logn, logq, W, dims, cts, rlk, idx, rs=None):
    """src/he-mult.c:88-156 (and src/he-rescale.c:33-54 with rs = log2 Delta) for ciphertexts idx of the device slabs
    cts = [ct1.c0, ct1.c1, ct2.c0, ct2.c1] under the key slabs rlk"""
    dimA, dimB, dimP = dims
    per = W << logn
    ins, keys = [_host(t) for t in cts], [_host(t) for t in rlk]
    return [dict(kind="he_mul", logn=logn, dimP=dimP, dimA=dimA, dimB=dimB, W=W, logq=logq, rs=rs,
                 ct=[np.ascontiguousarray(x[j * per:(j + 1) * per]) for x in ins], rlk0=keys[0], rlk1=keys[1]) for j in idx]


def he_swk_tasks(logn, logq, W, dims, d, swk, idx):
    """src/he-automorphism.c:40-85 for the pairs idx of the device slabs d = [d0, d1] under the key slabs swk"""
    _, dimB, dimP = dims
    per = W << logn
    ins, keys = [_host(t) for t in d], [_host(t) for t in swk]
    return [dict(kind="he_swk", logn=logn, dimP=dimP, dimB=dimB, W=W, logq=logq, d0=np.ascontiguousarray(ins[0][j * per:(j + 1) * per]),
                 d1=np.ascontiguousarray(ins[1][j * per:(j + 1) * per]), swk0=keys[0], swk1=keys[1]) for j in idx]


def expect_all(tasks, workers=8):
    return expect.expect_many(tasks, workers=min(workers, 8))


def assert_anchored(what, got, want, key, idx, per):
    """got: device slab of the whole batch; want: expect results for ciphertexts idx, in order"""
    h = _host(got)
    for r, j in enumerate(idx):
        bad = np.flatnonzero(h[j * per:(j + 1) * per] != want[r][key])
        assert bad.size == 0, "%s of ciphertext %d: %d words differ from the restated reference, first at %s" % (what, j, bad.size, bad[:4])
