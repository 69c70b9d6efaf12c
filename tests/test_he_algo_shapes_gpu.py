"""The evaluators (include/gpqhe_hip_algo.h) away from the one point tests/test_he_algo_gpu.py runs them at (q_L = 2^200, Delta = 2^30, W = 4, the
input at the top level): tests/algo_model.py's SLAB_SHAPES.

  A   2^200, Delta 2^30, the input 2 levels down (2^140), W 4      logql != logqL in every operation: Book::logql, gpq_he_dims(c, logqL, logql(level)),
                                                                   mulpt_dim, the dimpt of the workspace; he_exp ends at 2^20
  B   2^200, Delta 2^20, 2 down (2^160)                            three iterations: AlgoDevice's place / settle go round a third time; another scale
  C   2^300, Delta 2^59, the top, W 5                              constants up to 12 * 2^59 next to INT64_MAX, shifts of 59; depth 4 ends at exactly
                                                                   2^64: the sign on a word's first bit
  D   2^200, Delta 2^4, 40 down (2^40), W 1                        one word; he_const_pt of -1/48, -17/80640 and 31/1451520 is 0: a zero constant into
                                                                   gpq_he_mulpt_const, and he_sigmoid's result is he_const_pt(1/2) alone
  E1  2^438, Delta 2^30, the top, W 7                              bases of 8/16/24 limbs, the matrix-core front, limb counts that fall with the level
  E2  2^438, Delta 2^30, 8 down (2^198), W 4                       P sized for a q_L far above q_l
  F   2^850, Delta 2^30, the top, W 14                             a 16-word P: the wide tail behind a derived call
  G   logn 13, 2^200, Delta 2^30, 1 down, batch 3 in groups of 2   a two-pass ring below the top
(logn 7 and batch 2 unless said.)  Every cell hands the call a workspace of exactly gpq_he_algo_workspace_bytes between two bands of poison
(tests/bridge_settings.py's Guarded), inputs and outputs framed the same way, and asserts, without a tolerance: the words of the same sequence as
separate public calls (tests/algo_device.py's DeviceOps); the words of the restated reference (Python integers) on the first and the last
ciphertext; inputs unchanged; every guard word intact; outputs in mpi_smod's range of the output's level.

Also: every kind of cell A in place; per kind the largest logDelta the library must accept and the smallest it must refuse, computed here from
Python integers, the first run against the restated reference, the second answered "constant"; and the launch classes of one he_sigmoid and one
he_inv call against their products called separately."""
import pytest

from gpqhe_amd import big_to_ints, to_host
from tests import algo_model as am
from tests import bridge_settings as bs
from tests.algo_device import DeviceOps, Env

pytestmark = pytest.mark.gpu

GPQ_ERR_INVALID = -1
INT64_MAX = (1 << 63) - 1


def _torch():
    import torch
    return torch


_ENVS = {}


def _env(cell, engine_ctx, oracle_ctx):
    if cell not in _ENVS:
        logn, logq, logdelta, down, W, batch, _ = am.SLAB_SHAPES[cell]
        e = Env(engine_ctx, oracle_ctx, logn, logq, logdelta, batch, 40 + list(am.SLAB_SHAPES).index(cell), down=down, W=W, sets="A")
        assert e.logql0 == logq - down * logdelta and e.W == W
        _ENVS[cell] = e
    return _ENVS[cell]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    _torch().cuda.synchronize()
    _ENVS.clear()


class Framed:
    """one evaluator call with every buffer between two bands of poison: the inputs (copies of set A), the outputs (poison, or the inputs
    themselves) and a workspace of exactly the declared size"""

    def __init__(self, env, kind, iter, in_place=False):
        torch = _torch()
        self.env, self.what = env, "%s-%d" % (kind, iter)
        words = env.batch * env.W * env.g.n
        self.bufs = {"c0": bs.Guarded(8 * words), "c1": bs.Guarded(8 * words)}
        self.ins = (self.bufs["c0"].t, self.bufs["c1"].t)
        for t, src in zip(self.ins, env.dev["A"]):
            t.copy_(src)
        if in_place:
            self.outs = self.ins
        else:
            self.bufs.update(o0=bs.Guarded(8 * words), o1=bs.Guarded(8 * words))
            self.outs = (self.bufs["o0"].t, self.bufs["o1"].t)
        self.nbytes = env.workspace_bytes(kind, iter)
        assert self.nbytes and self.nbytes % 8 == 0, "%s: gpq_he_algo_workspace_bytes refuses: %s" % (self.what, env.g.lib.gpq_last_error().decode())
        self.bufs["workspace"] = bs.Guarded(self.nbytes)
        self.rc = env.call(kind, iter, self.ins[0], self.ins[1], self.outs[0], self.outs[1], self.bufs["workspace"].t)
        torch.cuda.synchronize()

    def ints(self):
        """[c0 | c1][ciphertext] -> the coefficients as Python integers"""
        return [big_to_ints(to_host(t), self.env.W, self.env.g.n) for t in self.outs]


def _assert_cell(env, kind, iter, in_place=False):
    torch = _torch()
    run = Framed(env, kind, iter, in_place)
    assert run.rc == 0, "%s refused: %s" % (run.what, env.g.lib.gpq_last_error().decode())
    bs.assert_guards(run.bufs, run.what)
    want = env.separate(kind, iter, "A")
    assert torch.equal(run.outs[0], want[0]) and torch.equal(run.outs[1], want[1]), "%s: not the words of the separate calls" % run.what
    if not in_place:
        assert torch.equal(run.ins[0], env.dev["A"][0]) and torch.equal(run.ins[1], env.dev["A"][1]), "%s: the inputs changed" % run.what
    assert env.g.he_algo_depth(kind, iter) == am.depth(kind, iter)
    logqo = env.logql0 - am.depth(kind, iter) * env.logdelta
    assert 1 <= logqo <= 64 * env.W
    h = 1 << (logqo - 1)
    got = run.ints()
    for side in (0, 1):
        for k in range(env.batch):
            assert all(-h <= v < h for v in got[side][k]), "%s: c%d of ciphertext %d leaves mpi_smod's range at 2^%d" % (run.what, side, k, logqo)
    for k in sorted({0, env.batch - 1}):
        c = env.restated(kind, iter, "A", k)
        assert got[0][k] == c[0] and got[1][k] == c[1], "%s: ciphertext %d differs from the restated reference" % (run.what, k)
    return got


CELL_CASES = [(cell, kind, iter) for cell, shape in am.SLAB_SHAPES.items() for kind, iter in shape[6]]


@pytest.mark.parametrize("cell,kind,iter", CELL_CASES, ids=["%s-%s-%d" % c for c in CELL_CASES])
def test_cell(engine_ctx, oracle_ctx, cell, kind, iter):
    env = _env(cell, engine_ctx, oracle_ctx)
    chunked = cell == "G"
    if chunked:
        env.g.set_chunk(2)                           # batch 3: two launch groups with an odd last one
    try:
        got = _assert_cell(env, kind, iter)
    finally:
        _torch().cuda.synchronize()
        if chunked:
            env.g.set_chunk(32)
    if cell == "A" and kind == "exp":
        assert env.logql0 - am.depth(kind, iter) * env.logdelta == 20
    if cell == "C" and am.depth(kind, iter) == 4:
        assert env.logql0 - 4 * env.logdelta == 64   # the output's sign is bit 63 of the first of W words
    if cell == "D" and kind == "sigmoid":
        # every constant product is by 0 and so is every product behind it: what is left is he_const_pt(1/2) at coefficient 0 of c0
        assert [am.const_int(re, env.logdelta) for re in (-1. / 48, -17. / 80640, 31. / 1451520)] == [0, 0, 0]
        n = env.g.n
        for k in range(env.batch):
            assert got[0][k] == [am.const_int(0.5, env.logdelta)] + [0] * (n - 1) and got[1][k] == [0] * n


@pytest.mark.parametrize("kind,iter", am.SLAB_SHAPES["A"][6], ids=["%s-%d" % c for c in am.SLAB_SHAPES["A"][6]])
def test_in_place_below_the_top(engine_ctx, oracle_ctx, kind, iter):
    _assert_cell(_env("A", engine_ctx, oracle_ctx), kind, iter, in_place=True)


@pytest.mark.parametrize("cell", ["A", "E2"])
def test_dimpt_is_bounded_by_the_limb_count_at_the_inputs_level(engine_ctx, oracle_ctx, cell):
    """he_exp's dimpt is "at most the reference's value" (src/he-mult.c:168) -- at the INPUT's modulus: one limb more, which q_L's count would still
    allow, is refused with the outputs untouched.  (The count itself runs: test_cell.)"""
    torch = _torch()
    env = _env(cell, engine_ctx, oracle_ctx)
    kind, iter = [c for c in am.SLAB_SHAPES[cell][6] if c[0] == "exp"][0]
    at_the_top = (env.logq + 1 + env.logdelta + env.logn) // 59 + 1
    assert env.dimpt == (env.logql0 + 1 + env.logdelta + env.logn) // 59 + 1 < at_the_top <= env.dimevk
    o0, o1 = bs.Guarded(8 * env.dev["A"][0].numel()), bs.Guarded(8 * env.dev["A"][1].numel())
    ws = torch.empty(env.workspace_bytes(kind, iter) // 8 + 8, dtype=torch.int64, device="cuda")
    g = env.g
    rc = g.he_algo_call(kind, o0.t, o1.t, env.dev["A"][0], env.dev["A"][1], env.rlk[0], env.rlk[1], env.W, env.logq, env.logql0, env.logdelta, iter, ws, env.m,
                        env.dimpt + 1)
    torch.cuda.synchronize()
    assert rc == GPQ_ERR_INVALID and "dimpt" in g.lib.gpq_last_error().decode(), (rc, g.lib.gpq_last_error().decode())
    assert o0.untouched() and o1.untouched() and o0.guards_intact() and o1.guards_intact()


# ---------------------------------------------------------------------------
# the largest Delta a kind's constants allow, and the first they do not
# ---------------------------------------------------------------------------
class Constants:
    """tests/algo_model.py's operations with levels alone: records (re, level of the operand, is it a factor) of every he_const_pt"""

    def __init__(self, L):
        self.L, self.seen = L, []

    def alloc(self):
        return am.Ct()

    def copy(self, dst, src):
        dst.l = src.l

    def neg(self, ct):
        pass

    def add(self, dst, a, b):
        assert a.l == b.l
        dst.l = a.l

    def addpt(self, dst, src, re):
        self.seen.append((re, src.l, False))
        dst.l = src.l

    subpt = addpt

    def moddown(self, ct):
        ct.l -= 1

    rs = moddown

    def mul(self, dst, a, b):
        assert a.l == b.l
        dst.l = a.l

    def mulpt(self, dst, src, m):
        dst.l = src.l

    def mulpt_const(self, dst, src, re):
        self.seen.append((re, src.l, True))
        dst.l = src.l


def _constants(kind, iter, L):
    ops = Constants(L)
    am.run(kind, ops, am.Ct(None, L), iter, None)
    seen = ops.seen
    if kind == "sqrt" and iter:
        # the last round's bn (src/he-algo.c:196-202: he_const_pt(3), he_const_pt(0.25)) feeds nothing; the library's sequence stops before it
        assert [x[0] for x in seen[-2:]] == [3, 0.25]
        seen = seen[:-2]
    return seen


EDGE_KINDS = [("inv", 1), ("sqrt", 1), ("sqrt", 2), ("sigmoid", 0), ("log", 0), ("exp", 0)]
EDGE_LOGN, EDGE_SPARE = 7, 20


def _edge_logq(kind, iter, logdelta):
    """q_L for a chain of exactly depth levels of Delta = 2^logdelta that ends at 2^EDGE_SPARE"""
    return am.depth(kind, iter) * logdelta + EDGE_SPARE


def _accepted(kind, iter, logdelta, logq, primes):
    """every constant of the sequence is an int64_t, and every constant FACTOR a keeps he_mulpt's words: a 2^(logql - 1) < floor(P / 2) over
    the reference's limb count at the operand's level (the rule above gpq_he_mulpt_const_fits, include/gpqhe_hip.h)"""
    L = logq // logdelta
    for re, l, factor in _constants(kind, iter, L):
        a = abs(am.const_int(re, logdelta))
        if a > INT64_MAX:
            return False
        if factor:
            logql = logq - (L - l) * logdelta
            dim = (logql + 1 + logdelta + EDGE_LOGN) // 59 + 1
            P = 1
            for p in primes[:dim]:
                P *= int(p)
            if not a << (logql - 1) < P // 2:
                return False
    return True


@pytest.mark.parametrize("kind,iter", EDGE_KINDS, ids=["%s-%d" % c for c in EDGE_KINDS])
def test_constant_edges(engine_ctx, oracle_ctx, kind, iter):
    torch = _torch()
    depth = am.depth(kind, iter)
    primes = oracle_ctx(EDGE_LOGN, am.primes_for(EDGE_LOGN, _edge_logq(kind, iter, 63))).p
    ok = [d for d in range(1, 64) if _accepted(kind, iter, d, _edge_logq(kind, iter, d + 1), primes)]
    top = ok[-1]
    print("%s-%d: logDelta accepted up to %d" % (kind, iter, top))
    assert ok == list(range(1, top + 1)) and EDGE_SPARE + depth < top < 63
    # one context for both edges: q_L is sized for the refused scale, a chain of exactly `depth` levels at either
    logq = _edge_logq(kind, iter, top + 1)
    assert logq // top == depth == logq // (top + 1)
    key = ("edge", kind, iter)
    if key not in _ENVS:
        _ENVS[key] = Env(engine_ctx, oracle_ctx, EDGE_LOGN, logq, top, 2, 70 + EDGE_KINDS.index((kind, iter)), sets="A")
    env = _ENVS[key]
    got = _assert_cell(env, kind, iter)
    assert any(v for v in got[0][0])
    # the same call one bit of Delta further
    g, W = env.g, env.W
    assert g.he_algo_workspace_bytes(kind, W, logq, logq, top + 1, iter, env.batch) == 0
    assert "constant" in g.lib.gpq_last_error().decode()
    o0, o1 = bs.Guarded(8 * env.dev["A"][0].numel()), bs.Guarded(8 * env.dev["A"][1].numel())
    ws = torch.empty(env.workspace_bytes(kind, iter) // 8, dtype=torch.int64, device="cuda")
    dimpt = (logq + 1 + top + 1 + EDGE_LOGN) // 59 + 1
    rc = g.he_algo_call(kind, o0.t, o1.t, env.dev["A"][0], env.dev["A"][1], env.rlk[0], env.rlk[1], W, logq, logq, top + 1, iter, ws, env.m, dimpt)
    torch.cuda.synchronize()
    assert rc == GPQ_ERR_INVALID and "constant" in g.lib.gpq_last_error().decode(), (rc, g.lib.gpq_last_error().decode())
    assert o0.untouched() and o1.untouched() and o0.guards_intact() and o1.guards_intact()


# ---------------------------------------------------------------------------
# launch classes
# ---------------------------------------------------------------------------
class Products(DeviceOps):
    """DeviceOps whose products are the calls an evaluator makes -- gpq_he_mul_rs, gpq_he_mulpt_const with the rescale riding -- each profiled on
    its own; the additive calls in between are not counted"""

    def __init__(self, env):
        DeviceOps.__init__(self, env)
        self.counts, self.pending = {}, {}

    def _counted(self, call):
        torch = _torch()
        torch.cuda.synchronize()
        self.g.profile_collect()
        call()
        torch.cuda.synchronize()
        for name, (_, launches) in self.g.profile_collect().items():
            self.counts[name] = self.counts.get(name, 0) + int(launches)

    def mul(self, dst, a, b):
        assert a.l == b.l
        self.pending[id(dst)] = ("mul", a.c, b.c, a.l)
        dst.l = a.l

    def mulpt_const(self, dst, src, re):
        self.pending[id(dst)] = ("mulc", src.c, am.const_int(re, self.s), src.l)
        dst.l = src.l

    def rs(self, ct):
        torch = _torch()
        what, x, y, l = self.pending.pop(id(ct))          # every product of he_sigmoid and he_inv is rescaled at once
        assert l == ct.l
        c = (torch.empty_like(x[0]), torch.empty_like(x[0]))
        if what == "mul":
            dimP, dimA, dimB, _ = self.g.he_dims(self.logqL, self.logql(l))
            self._counted(lambda: self.g.he_mul_rs(c[0], c[1], x[0], x[1], y[0], y[1], self.e.rlk[0], self.e.rlk[1], self.W, self.logql(l), dimA, dimB, dimP, self.s))
        else:
            self._counted(lambda: self.g.he_mulpt_const(c[0], c[1], x[0], x[1], y, 0, self.W, self.logql(l), self.mulpt_dim(l), self.s))
        ct.c, ct.l = c, l - 1


@pytest.mark.parametrize("kind,iter", [("sigmoid", 0), ("inv", 2)])
def test_launch_classes(engine_ctx, oracle_ctx, kind, iter):
    """An evaluator launches what its products launch when called separately with the same arguments, and gpq_he_lin_const: nothing else is
    recorded (no rescale of its own; gpq_big_addsub has no profile class, so its absence shows as the absence of anything unaccounted for),
    and gpq_he_lin_const at most once per sum that tests/algo_model.py's LazyOps materialises, plus one for the result's copy."""
    torch = _torch()
    env = _env("A", engine_ctx, oracle_ctx)
    g = env.g
    want = env.separate(kind, iter, "A")
    Framed(env, kind, iter)                               # warm
    g.profile(True)
    try:
        g.profile_collect()
        run = Framed(env, kind, iter)
        prof = {name: int(v[1]) for name, v in g.profile_collect().items()}
        ops = Products(env)
        d = env.dev["A"]
        out = am.run(kind, ops, am.Ct((d[0].clone(), d[1].clone()), ops.L - env.down), iter, env.m)
        torch.cuda.synchronize()
    finally:
        g.profile(False)
    assert run.rc == 0 and not ops.pending
    assert torch.equal(run.outs[0], want[0]) and torch.equal(out.c[0], want[0]) and torch.equal(out.c[1], want[1])
    print("%s-%d: the call %s; its products alone %s" % (kind, iter, prof, ops.counts))
    lin = prof.pop("he_lin_const", 0)
    assert "big_addsub" not in prof
    assert prof == ops.counts and "he_lin_const" not in ops.counts
    lazy = am.LazyOps(env.o, env.logn, env.logq, env.logdelta, env.rlk_host)
    ct = env.cts["A"][0]
    lazy.value(am.run(kind, lazy, am.Ct((ct[0], ct[1]), lazy.L - env.down), iter, env.m_host))
    assert 1 <= lin <= lazy.sums + 1, (lin, lazy.sums)
