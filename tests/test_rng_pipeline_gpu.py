"""The device generator feeding the device samplers and encryptor, against the record of the EXECUTED reference (tests/golden/ref_enc.json,
written by tests/enc_record.py): no byte comes from a stored stream or from the host.

For every recorded case, from stream position 0 as a fresh reference process starts: sample_zo, sample_error and sample_uniform alone;
then he_keypair -> he_enc_sk -> he_enc_pk in one run, where sample_sk is the model's sample_hwt on gpq_rng_host_bytes of the same stream
object and every other byte is made by gpq_rng_device_bytes where the samplers read it.  The sha256 of every output and the stream
position after every call are the recorded reference's (the record drew PROBE bytes after each call; they are skipped by a seek)."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

import gpqhe_amd
from gpqhe_amd import to_device, to_host
from oracle.expect import ints_to_words
from tests import enc_model, enc_record

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A5A5A5A5A


class HostDraws:
    """enc_model's Stream interface on the host path of a stream object"""

    def __init__(self, rng):
        self.rng = rng

    def take(self, count):
        return self.rng.host_bytes(count)


def _sha(words):
    return hashlib.sha256(np.ascontiguousarray(words).tobytes()).hexdigest()


def _drawn(g, rng, count):
    """the next `count` bytes of the stream, generated on the device"""
    return rng.device_bytes(g, torch.empty(count, dtype=torch.uint8, device="cuda"))


def _key_slab(g, big, W, dim):
    out = torch.empty(dim * g.n, dtype=torch.int64, device="cuda")
    assert g.lib.gpq_evk_pack(g.h, C.c_void_p(out.data_ptr()), C.c_void_p(big.data_ptr()), W, dim, 1, g._stream()) == 0
    return out


@pytest.mark.parametrize("case", enc_record.CASES, ids=enc_record.case_name)
def test_samplers_alone_from_position_0(engine_ctx, case):
    logn, logq = case
    rec = enc_record.enc_golden()["cases"][enc_record.case_name(case)]
    g = engine_ctx(logn, max(6, enc_model.he_dim(logn, 1 << logq)))
    n, W, nbits = g.n, rec["W"], logq + 1
    small = lambda: torch.empty(n, dtype=torch.int8, device="cuda")
    for name, count in (("sample_zo", n // 4), ("sample_error", n)):
        r = gpqhe_amd.Rng()
        out = getattr(g, name)(small(), _drawn(g, r, count))
        torch.cuda.synchronize()
        assert enc_record.sha(out.cpu().numpy().tolist(), W) == rec["sha256"][name], name
        assert r.tell() == rec["pos"][name]
    r = gpqhe_amd.Rng()
    big = g.sample_uniform(torch.full((W * n,), PATTERN, dtype=torch.int64, device="cuda"), _drawn(g, r, n * (nbits // 8 + 1)), nbits, W)
    torch.cuda.synchronize()
    assert _sha(to_host(big)) == rec["sha256"]["sample_uniform"]
    assert r.tell() == rec["pos"]["sample_uniform"]


@pytest.mark.parametrize("case", enc_record.CASES, ids=enc_record.case_name)
def test_keypair_and_both_encryptions_from_position_0(engine_ctx, case):
    logn, logq = case
    rec = enc_record.enc_golden()["cases"][enc_record.case_name(case)]
    dim = enc_model.he_dim(logn, 1 << logq)
    g = engine_ctx(logn, max(6, dim))
    n, W, nbits = g.n, rec["W"], logq + 1
    nb = nbits // 8 + 1
    r = gpqhe_amd.Rng()

    def check(names, tensors):
        torch.cuda.synchronize()
        for name, t in zip(names, tensors):
            assert _sha(to_host(t)) == rec["sha256"][name], name

    def after(call):
        assert r.tell() == rec["pos"][call], call
        r.seek(r.tell() + enc_record.PROBE)

    small = lambda: torch.empty(n, dtype=torch.int8, device="cuda")
    big = lambda: torch.full((W * n,), PATTERN, dtype=torch.int64, device="cuda")
    sk = enc_model.sample_hwt(HostDraws(r), n)                                  # sample_sk: the host's, on the same stream
    assert enc_record.sha(sk, W) == rec["sha256"]["sk"]
    sk_big = to_device(ints_to_words(sk, W))
    # he_keypair and he_enc_sk: error, uniform -- one device draw each, sliced where the samplers read
    for m, names, call in ((None, ("p0", "p1"), "he_keypair"), (to_device(ints_to_words(enc_record.case_plaintext(case), W)), ("sk_c0", "sk_c1"), "he_enc_sk")):
        b = _drawn(g, r, n + n * nb)
        e, a = g.sample_error(small(), b[:n]), g.sample_uniform(big(), b[n:], nbits, W)
        out = g.he_enc_sk(big(), big(), m, a, e, _key_slab(g, sk_big, W, dim), W, logq, dim)
        check(names, out)
        after(call)
        if m is None:
            p0, p1 = out
    b = _drawn(g, r, n // 4 + 2 * n)                                             # he_enc_pk: zo, error, error
    v, e0, e1 = g.sample_zo(small(), b[:n // 4]), g.sample_error(small(), b[n // 4:n // 4 + n]), g.sample_error(small(), b[n // 4 + n:])
    check(("pk_c0", "pk_c1"), g.he_enc_pk(big(), big(), m, v, e0, e1, _key_slab(g, p0, W, dim), _key_slab(g, p1, W, dim), W, logq, dim))
    assert r.tell() == rec["pos"]["he_enc_pk"]
