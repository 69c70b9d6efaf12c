"""gpq_he_cmp (iter 1, t 0) and gpq_he_cmppt (iter 0, t 1) under every "same words" switch of tests/bridge_settings.py, at one small cell: logn 7,
q_L = 2^200, Delta = 2^20, batch 3 on contexts of bridge_settings.Cells, i.e. in launch groups of 2.  Without a tolerance: under every entry
of SETTINGS every word of both outputs equals the "default" entry's run, the inputs are unchanged, the workspace is exactly
gpq_he_cmp_workspace_bytes between two bands of poison (the same number under every entry), and the default run equals the same text over
separate public calls."""
import pytest
import torch

from tests import bridge_settings as bs
from tests.cmp_device import CmpEnv

pytestmark = pytest.mark.gpu

LOGN, LOGQ, LOGDELTA, BATCH = 7, 200, 20, 3
CALLS = [("cmp", 1, 0), ("cmppt", 0, 1)]

_ENVS, _RUNS = {}, {}
_contexts = bs.Cells()


@pytest.fixture(scope="module", autouse=True)
def _close_cells():
    yield
    torch.cuda.synchronize()
    _RUNS.clear()
    _ENVS.clear()
    _contexts.close()


def _env(setting, engine_ctx, oracle_ctx):
    if "base" not in _ENVS:
        _ENVS["base"] = CmpEnv(engine_ctx, oracle_ctx, LOGN, LOGQ, LOGDELTA, BATCH, 97)
    base = _ENVS["base"]
    if setting not in _ENVS:
        e = base.on(_contexts.get(LOGN, base.dimevk, setting))
        e._sep = {}
        _ENVS[setting] = e
    return _ENVS[setting]


def _run(setting, engine_ctx, oracle_ctx):
    if setting not in _RUNS:
        env = _env(setting, engine_ctx, oracle_ctx)
        words = BATCH * env.W * env.g.n
        res = {}
        for fn, iter, t in CALLS:
            nbytes = env.g.he_cmp_workspace_bytes(fn == "cmppt", env.W, LOGQ, LOGQ, LOGDELTA, iter, t, BATCH)
            assert nbytes, "he_%s under `%s`: %s" % (fn, setting, env.g.lib.gpq_last_error().decode())
            bufs = {"output c0": bs.Guarded(8 * words), "output c1": bs.Guarded(8 * words), "workspace (%d bytes reported)" % nbytes: bs.Guarded(nbytes)}
            o0, o1 = bufs["output c0"].t, bufs["output c1"].t
            rc = env.cmp_call(fn, iter, t, env.dev["A"][0], env.dev["A"][1], env.other(fn), o0, o1, bufs["workspace (%d bytes reported)" % nbytes].t)
            torch.cuda.synchronize()
            assert rc == 0, "he_%s under `%s` refused: %s" % (fn, setting, env.g.lib.gpq_last_error().decode())
            bs.assert_guards(bufs, "he_%s under `%s`" % (fn, setting))
            res[fn] = (o0, o1, nbytes)
        _RUNS[setting] = res
    return _RUNS[setting]


@pytest.mark.parametrize("setting", list(bs.SETTINGS))
def test_comparisons_write_the_default_words(engine_ctx, oracle_ctx, setting):
    env = _env(setting, engine_ctx, oracle_ctx)
    ins = env.dev["A"] + env.dev["B"] + env.rlk + (env.pt["m1"],)
    pristine = [x.clone() for x in ins]
    res = _run(setting, engine_ctx, oracle_ctx)
    assert all(torch.equal(a, b) for a, b in zip(ins, pristine)), "under `%s`: a call wrote to its inputs" % setting
    base = _run("default", engine_ctx, oracle_ctx)
    for fn, (o0, o1, nbytes) in res.items():
        assert bool(o0.any()) and bool(o1.any())
        assert nbytes == base[fn][2], "he_%s: gpq_he_cmp_workspace_bytes says %d under `%s` and %d by default" % (fn, nbytes, setting, base[fn][2])
        for side, got in enumerate((o0, o1)):
            bad = torch.nonzero(got != base[fn][side]).flatten()
            assert not bad.numel(), "he_%s under `%s`: c%d: %d words differ from the default run, first at %s" % (fn, setting, side, bad.numel(), bad[:4].tolist())


def test_the_default_run_is_the_separate_calls(engine_ctx, oracle_ctx):
    base = _env("default", engine_ctx, oracle_ctx)
    res = _run("default", engine_ctx, oracle_ctx)
    for fn, iter, t in CALLS:
        want = _ENVS["base"].separate(fn, iter, t)
        assert torch.equal(res[fn][0], want[0]) and torch.equal(res[fn][1], want[1]), fn
    assert base.g is not _ENVS["base"].g
