"""gpq_he_inv / gpq_he_sigmoid / gpq_he_exp (include/gpqhe_hip_algo.h) under every "same words" switch of tests/bridge_settings.py.  An evaluator is
host code around gpq_he_mul_rs, gpq_he_mulpt_const, gpq_he_mulpt and gpq_he_lin_const at a different modulus per level, from ONE workspace sized
on the host before a switch is looked at: a switch could reach it wrongly while each of those calls, which the other settings tests run at one
level, stays right.

Three shapes, the ones of tests/test_settings_derived_gpu.py (dims = he_dims(logq, logq)), the input at the top level:
  S3  logn 7,  q_L = 2^438, Delta 2^30   dims 8/16/24 at the top, fewer limbs at every level below; inv-2, sigmoid, exp-1
  S2  logn 10, q_L = 2^120, Delta 2^20   dims 3/5/8: no matrix-core front, integer-VALU tail; inv-2, sigmoid, exp-1 (which ends at 2^20)
  S1  logn 13, q_L = 2^200, Delta 2^30   two-pass ring: the key switch pre-weights limbs, the tail streams; inv-1, sigmoid
Batch 3 on contexts of bridge_settings.Cells, i.e. in launch groups of 2.  Without a tolerance:
1. under every entry of SETTINGS, every word of every output equals the "default" entry's run, and the inputs are unchanged;
2. the default run equals the restated reference (Python integers) on ciphertexts 0 and 2;
3. the workspace is exactly gpq_he_algo_workspace_bytes between two bands of poison, outputs framed the same way: no guard word changes;
4. gpq_he_algo_workspace_bytes is the same number under every entry."""
import pytest
import torch

from gpqhe_amd import big_to_ints, to_host
from tests import bridge_settings as bs
from tests.algo_device import Env

pytestmark = pytest.mark.gpu

SHAPES = {"S3": (7, 438, 30, [("inv", 2), ("sigmoid", 0), ("exp", 1)]),
          "S2": (10, 120, 20, [("inv", 2), ("sigmoid", 0), ("exp", 1)]),
          "S1": (13, 200, 30, [("inv", 1), ("sigmoid", 0)])}
BATCH = 3

_ENVS, _RUNS = {}, {}
_contexts = bs.Cells()


@pytest.fixture(scope="module", autouse=True)
def _close_cells():
    yield
    torch.cuda.synchronize()
    _RUNS.clear()
    _ENVS.clear()
    _contexts.close()


def _env(shape, setting, engine_ctx, oracle_ctx):
    """the shape's inputs (made once, on the session's default context) on the context that carries `setting`"""
    logn, logq, logdelta, _ = SHAPES[shape]
    if shape not in _ENVS:
        _ENVS[shape] = Env(engine_ctx, oracle_ctx, logn, logq, logdelta, BATCH, 90 + len(shape) + logn, sets="A")
    base = _ENVS[shape]
    if (shape, setting) not in _ENVS:
        _ENVS[shape, setting] = base.on(_contexts.get(logn, base.dimevk, setting))
    return _ENVS[shape, setting]


def _run(shape, setting, engine_ctx, oracle_ctx):
    """every kind of the shape under `setting` -> {(kind, iter): (c0, c1, bytes of the workspace)}; checked for its frames once, then cached"""
    if (shape, setting) not in _RUNS:
        env = _env(shape, setting, engine_ctx, oracle_ctx)
        words = BATCH * env.W * env.g.n
        res = {}
        for kind, iter in SHAPES[shape][3]:
            nbytes = env.workspace_bytes(kind, iter)
            assert nbytes, "%s, %s-%d under `%s`: %s" % (shape, kind, iter, setting, env.g.lib.gpq_last_error().decode())
            bufs = {"output c0": bs.Guarded(8 * words), "output c1": bs.Guarded(8 * words), "workspace (%d bytes reported)" % nbytes: bs.Guarded(nbytes)}
            o0, o1 = bufs["output c0"].t, bufs["output c1"].t
            rc = env.call(kind, iter, env.dev["A"][0], env.dev["A"][1], o0, o1, bufs["workspace (%d bytes reported)" % nbytes].t)
            torch.cuda.synchronize()
            assert rc == 0, "%s, %s-%d under `%s` refused: %s" % (shape, kind, iter, setting, env.g.lib.gpq_last_error().decode())
            bs.assert_guards(bufs, "%s, %s-%d under `%s`" % (shape, kind, iter, setting))
            res[kind, iter] = (o0, o1, nbytes)
        _RUNS[shape, setting] = res
    return _RUNS[shape, setting]


def _differences(a, b):
    bad = torch.nonzero(a != b).flatten()
    return "%d words differ, first at %s" % (bad.numel(), bad[:4].tolist()) if bad.numel() else ""


@pytest.mark.parametrize("setting", list(bs.SETTINGS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_evaluators_write_the_default_words(engine_ctx, oracle_ctx, shape, setting):
    env = _env(shape, setting, engine_ctx, oracle_ctx)
    pristine = [t.clone() for t in env.dev["A"] + env.rlk + (env.m,)]
    res = _run(shape, setting, engine_ctx, oracle_ctx)
    assert all(torch.equal(a, b) for a, b in zip(env.dev["A"] + env.rlk + (env.m,), pristine)), "%s under `%s`: a call wrote to its inputs" % (shape, setting)
    base = _run(shape, "default", engine_ctx, oracle_ctx)
    assert set(res) == set(base) == set(SHAPES[shape][3])
    for (kind, iter), (o0, o1, nbytes) in res.items():
        assert bool(o0.any()) and bool(o1.any())
        assert nbytes == base[kind, iter][2], "%s, %s-%d: gpq_he_algo_workspace_bytes says %d under `%s` and %d by default" % (
            shape, kind, iter, nbytes, setting, base[kind, iter][2])
        for side, got in enumerate((o0, o1)):
            diff = _differences(got, base[kind, iter][side])
            assert not diff, "%s, %s-%d under `%s`: c%d against the default run: %s" % (shape, kind, iter, setting, side, diff)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_default_run_is_the_restated_reference(engine_ctx, oracle_ctx, shape):
    env = _env(shape, "default", engine_ctx, oracle_ctx)
    res = _run(shape, "default", engine_ctx, oracle_ctx)
    for (kind, iter), (o0, o1, _) in res.items():
        got = [big_to_ints(to_host(t), env.W, env.g.n) for t in (o0, o1)]
        for k in (0, 2):
            c = env.restated(kind, iter, "A", k)
            assert got[0][k] == c[0] and got[1][k] == c[1], "%s, %s-%d: ciphertext %d differs from the restated reference" % (shape, kind, iter, k)
