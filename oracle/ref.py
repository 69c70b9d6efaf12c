"""ctypes binding of oracle/ref_driver.c: the EXECUTED reference (oracle/_ref/, built by `make -C oracle ref`).

TEST INFRASTRUCTURE ONLY.  Where oracle.py / bigint_ref.py restate the reference, this module runs it.  The reference keeps its
context in globals, so one process holds one context: `Ref(path).init(...)` once, then calls.  `run(fn, args)` gives every argument
a fresh worker process (multiprocessing, `spawn`: nothing of the caller is inherited, in particular no GPU state) in which
`fn(arg)` runs; `fn` is a module-level function that opens its own `Ref`.  A worker that dies (the reference abort()s on what it
does not like) raises here with the worker's stderr.

Which build: libgpqhe_ref.so is the reference as the runtime libgcrypt behaves; libgpqhe_ref_floor.so routes mpi_fdiv through
oracle_fdiv (ref_driver.c).  `which()` PROBES the loaded libgcrypt (-1000503 fdiv 1000 must give q = -1001, r = 497; 1.9.4 gives
+1001) and returns the as-is build on a library that floor-divides and the _floor build otherwise -- never decided by version.
"""
import ctypes as C
import multiprocessing as _mp
import os
import tempfile

import numpy as np

from oracle.expect import ints_to_words, words_to_ints

_HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(_HERE, "_ref")
AS_IS = os.path.join(DIR, "libgpqhe_ref.so")
FLOOR = os.path.join(DIR, "libgpqhe_ref_floor.so")
BUILD_JSON = os.path.join(DIR, "BUILD.json")

ERRORS = {-1: "a value does not fit the words given", -2: "q above the reference's cap for this ring",
          -3: "parameters the reference aborts on", -4: "not initialised, or a slot / key is missing"}

u64p = np.ctypeslib.ndpointer(dtype=np.uint64, flags="C_CONTIGUOUS")
f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")


class RefError(RuntimeError):
    def __init__(self, what, code):
        RuntimeError.__init__(self, "%s: %d (%s)" % (what, code, ERRORS.get(code, "?")))
        self.code = code


def available():
    return os.path.exists(AS_IS) and os.path.exists(FLOOR)


def _words(v, W=None):
    """non-negative int -> little-endian uint64 words"""
    v = int(v)
    assert v >= 0
    W = W or max(1, (v.bit_length() + 63) // 64)
    return np.array([(v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(W)], dtype=np.uint64)


def _int(words):
    return sum(int(w) << (64 * j) for j, w in enumerate(words))


def bits(x):
    """a double as its 64 bits: nu and B are compared as bits, not as values"""
    return int(np.array([x], dtype=np.float64).view(np.uint64)[0])


_SIG = {
    "ref_gcrypt_version": (C.c_char_p, []),
    "ref_floor_fixed": (C.c_int, []),
    "ref_init": (C.c_int, [C.c_uint, u64p, C.c_uint, C.c_uint, C.c_uint64]),
    "ref_dimub": (C.c_uint, []),
    "ref_logqub": (C.c_uint, []),
    "ref_node": (C.c_int, [C.c_uint, u64p]),
    "ref_zetas": (C.c_int, [C.c_uint, C.c_int, u64p]),
    "ref_prefix": (C.c_int, [C.c_uint, u64p, u64p, C.c_uint]),
    "ref_he_info": (C.c_int, [u32p]),
    "ref_he_q": (C.c_int, [C.c_uint, u64p, C.c_uint]),
    "ref_he_P": (C.c_int, [u64p, u64p, C.c_uint]),
    "ref_he_bounds": (C.c_int, [f64p, C.c_uint]),
    "ref_ntt": (C.c_int, [C.c_uint, u64p, C.c_int]),
    "ref_poly_rns": (C.c_int, [C.c_uint, C.c_int, u64p, u64p, u64p]),
    "ref_montgomery_inv": (C.c_uint64, [C.c_uint64]),
    "ref_barrett_inv": (C.c_uint64, [C.c_uint64]),
    "ref_reduce": (C.c_int, [C.c_uint, C.c_int, u64p, u64p, u64p, C.c_size_t]),
    "ref_rns_decompose": (C.c_int, [C.c_uint, u64p, u64p, C.c_uint]),
    "ref_rns_reconstruct": (C.c_int, [u64p, C.c_uint, u64p, C.c_uint]),
    "ref_poly_rns2mpi": (C.c_int, [u64p, C.c_uint, u64p, C.c_uint, u64p, C.c_uint]),
    "ref_poly_mul": (C.c_int, [u64p, u64p, u64p, C.c_uint, C.c_uint, u64p, C.c_uint]),
    "ref_poly_auto": (C.c_int, [u64p, u64p, C.c_uint, C.c_int, C.c_size_t]),
    "ref_mpi_smod": (C.c_int, [u64p, u64p, C.c_uint, C.c_size_t, u64p, C.c_uint]),
    "ref_mpi_rdiv": (C.c_int, [u64p, u64p, C.c_uint, C.c_size_t, u64p, C.c_uint, C.c_int]),
    "ref_fdiv": (C.c_int, [u64p, u64p, u64p, C.c_uint, C.c_size_t, u64p, C.c_uint, C.c_int]),
    "ref_ct_set": (C.c_int, [C.c_int, u64p, u64p, C.c_uint, C.c_uint, C.c_double, C.c_double]),
    "ref_ct_get": (C.c_int, [C.c_int, u64p, u64p, C.c_uint, u32p, f64p]),
    "ref_pt_set": (C.c_int, [C.c_int, u64p, C.c_uint, C.c_double]),
    "ref_pt_get": (C.c_int, [C.c_int, u64p, C.c_uint, f64p]),
    "ref_he_ecd": (C.c_int, [C.c_int, f64p]),
    "ref_evk_set": (C.c_int, [C.c_uint, u64p, u64p]),
    "ref_he_addsub": (C.c_int, [C.c_int] * 4),
    "ref_he_neg": (C.c_int, [C.c_int]),
    "ref_he_pt_op": (C.c_int, [C.c_int] * 4),
    "ref_he_mul": (C.c_int, [C.c_int] * 3),
    "ref_he_rs": (C.c_int, [C.c_int, C.c_int]),
    "ref_he_rot": (C.c_int, [C.c_int, C.c_uint]),
    "ref_he_conj": (C.c_int, [C.c_int]),
    "ref_he_gemv": (C.c_int, [C.c_int, f64p, C.c_int]),
    "ref_he_sum": (C.c_int, [C.c_int, C.c_int]),
    "ref_he_idx": (C.c_int, [C.c_int, C.c_int, C.c_uint]),
}

_LIBS = {}


def _load(path):
    if path not in _LIBS:
        L = C.CDLL(path)
        for name, (res, args) in _SIG.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        _LIBS[path] = L
    return _LIBS[path]


def _big(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


class Ref:
    """One build of the reference in this process.  Coefficient vectors go in and out as Python ints; residue limbs as uint64 arrays."""

    def __init__(self, path=None):
        self.path = path or which()
        self.L = _load(self.path)
        self.n = None

    def _ck(self, what, rc):
        if rc != 0:
            raise RefError(what, rc)

    # -- context
    def init(self, logn, q, slots=0, Delta=0):
        qw = _words(q)
        self._ck("ref_init(%d, 2^%d.., %d, %d)" % (logn, int(q).bit_length() - 1, slots, Delta), self.L.ref_init(logn, qw, len(qw), slots, Delta))
        self.logn, self.n, self.q, self.slots, self.Delta = logn, 1 << logn, int(q), slots, Delta
        self.dimub = self.L.ref_dimub()
        self.W = (int(q).bit_length() + 1 + 63) // 64      # words that hold any centred coefficient mod q
        self.WP = self.dimub + 1                           # words that hold any product of the chain's primes
        if slots:
            info = np.zeros(4, dtype=np.uint32)
            self._ck("ref_he_info", self.L.ref_he_info(info))
            self.dim, self.dimevk, self.Lmax = int(info[0]), int(info[1]), int(info[2])
        return self

    def gcrypt_version(self):
        return self.L.ref_gcrypt_version().decode()

    def node(self, d):
        out = np.zeros(4, dtype=np.uint64)
        self._ck("ref_node", self.L.ref_node(d, out))
        return dict(zip(("p", "pinv_mont", "pinv_barr", "ninv"), (int(x) for x in out)))

    def zetas(self, d, inverse=False):
        out = np.empty(self.n, dtype=np.uint64)
        self._ck("ref_zetas", self.L.ref_zetas(d, int(inverse), out))
        return out

    def prefix(self, d):
        """(phat_invmp[0..d], P) of the prefix of d + 1 primes"""
        inv, P = np.zeros(d + 1, dtype=np.uint64), np.zeros(self.WP, dtype=np.uint64)
        self._ck("ref_prefix", self.L.ref_prefix(d, inv, P, self.WP))
        return [int(x) for x in inv], _int(P)

    def he_q(self, l):
        out = np.zeros(self.W, dtype=np.uint64)
        self._ck("ref_he_q", self.L.ref_he_q(l, out, self.W))
        return _int(out)

    def he_bounds(self):
        """(Brs, [Bmult[0..L]]) as doubles"""
        out = np.zeros(self.Lmax + 2, dtype=np.float64)
        self._ck("ref_he_bounds", self.L.ref_he_bounds(out, out.size))
        return float(out[0]), [float(x) for x in out[1:]]

    def he_P(self):
        W = self.WP + self.W
        P, PqL = np.zeros(W, dtype=np.uint64), np.zeros(W, dtype=np.uint64)
        self._ck("ref_he_P", self.L.ref_he_P(P, PqL, W))
        return _int(P), _int(PqL)

    # -- limb level
    def ntt(self, a, d, inverse=False):
        a = _big(a).copy()
        self._ck("ref_ntt", self.L.ref_ntt(d, a, int(inverse)))
        return a

    def invntt(self, a, d):
        return self.ntt(a, d, inverse=True)

    def rns_mul(self, a, b, d, mul=True):
        r = np.empty(self.n, dtype=np.uint64)
        self._ck("ref_poly_rns", self.L.ref_poly_rns(d, int(mul), r, _big(a), _big(b)))
        return r

    def rns_add(self, a, b, d):
        return self.rns_mul(a, b, d, mul=False)

    def reduce(self, d, lo, hi, barrett):
        lo, hi = _big(lo), _big(hi)
        out = np.empty(lo.size, dtype=np.uint64)
        self._ck("ref_reduce", self.L.ref_reduce(d, int(barrett), out, lo, hi, lo.size))
        return out

    # -- polynomial level (lists of Python ints)
    def rns_decompose(self, a, d, W=None):
        W = W or self.W
        out = np.empty(self.n, dtype=np.uint64)
        self._ck("ref_rns_decompose", self.L.ref_rns_decompose(d, out, ints_to_words(a, W), W))
        return out

    def rns_reconstruct(self, rhat, dim):
        out = np.empty(self.WP * self.n, dtype=np.uint64)
        self._ck("ref_rns_reconstruct", self.L.ref_rns_reconstruct(out, self.WP, _big(rhat), dim))
        m = 1 << (64 * self.WP)
        return [v % m for v in words_to_ints(out, self.WP, self.n)]

    def poly_rns2mpi(self, rhat, dim, q):
        qw, W = _words(q), (int(q).bit_length() + 64) // 64
        out = np.empty(W * self.n, dtype=np.uint64)
        self._ck("ref_poly_rns2mpi", self.L.ref_poly_rns2mpi(out, W, _big(rhat), dim, qw, len(qw)))
        return words_to_ints(out, W, self.n)

    def poly_mul(self, a, b, dim, q, Win=None):
        qw, W = _words(q), max(Win or 0, (int(q).bit_length() + 64) // 64)
        out = np.empty(W * self.n, dtype=np.uint64)
        self._ck("ref_poly_mul", self.L.ref_poly_mul(out, ints_to_words(a, W), ints_to_words(b, W), W, dim, qw, len(qw)))
        return words_to_ints(out, W, self.n)

    def poly_rot(self, a, rot, W=None):
        W = W or self.W
        out = np.empty(W * self.n, dtype=np.uint64)
        self._ck("ref_poly_auto", self.L.ref_poly_auto(out, ints_to_words(a, W), W, 0, rot))
        return words_to_ints(out, W, self.n)

    def poly_conj(self, a, W=None):
        W = W or self.W
        out = np.empty(W * self.n, dtype=np.uint64)
        self._ck("ref_poly_auto", self.L.ref_poly_auto(out, ints_to_words(a, W), W, 1, 0))
        return words_to_ints(out, W, self.n)

    @staticmethod
    def _Wfor(values, m):
        top = max([abs(int(v)) for v in values] + [int(m)])
        return (top.bit_length() + 2 + 63) // 64

    def mpi_smod(self, values, q):
        W, mw = self._Wfor(values, q), _words(q)
        out = np.empty(W * len(values), dtype=np.uint64)
        self._ck("ref_mpi_smod", self.L.ref_mpi_smod(out, ints_to_words(values, W), W, len(values), mw, len(mw)))
        return words_to_ints(out, W, len(values))

    def mpi_rdiv(self, values, m, alias=True):
        W, mw = self._Wfor(values, m), _words(m)
        out = np.empty(W * len(values), dtype=np.uint64)
        self._ck("ref_mpi_rdiv", self.L.ref_mpi_rdiv(out, ints_to_words(values, W), W, len(values), mw, len(mw), int(alias)))
        return words_to_ints(out, W, len(values))

    def fdiv(self, values, m, which):
        """[(q, r)]; which: 0 the library's gcry_mpi_div(.., -1), 1 oracle_fdiv, 2 oracle_fdiv with q aliasing a and a NULL remainder (r = 0)"""
        W, mw = self._Wfor(values, m), _words(m)
        q, r = np.empty(W * len(values), dtype=np.uint64), np.empty(W * len(values), dtype=np.uint64)
        self._ck("ref_fdiv", self.L.ref_fdiv(q, r, ints_to_words(values, W), W, len(values), mw, len(mw), which))
        return list(zip(words_to_ints(q, W, len(values)), words_to_ints(r, W, len(values))))

    # -- ciphertext level: numbered slots on the C side
    def ct_set(self, k, ct, l, nu=1.0, B=0.0, W=None):
        W = W or self.W
        self._ck("ref_ct_set", self.L.ref_ct_set(k, ints_to_words(ct[0], W), ints_to_words(ct[1], W), W, l, nu, B))

    def ct_get(self, k, W=None):
        """((c0, c1), l, bits(nu), bits(B))"""
        W = W or self.W
        c0, c1 = np.empty(W * self.n, dtype=np.uint64), np.empty(W * self.n, dtype=np.uint64)
        l, nb = np.zeros(1, dtype=np.uint32), np.zeros(2, dtype=np.float64)
        self._ck("ref_ct_get", self.L.ref_ct_get(k, c0, c1, W, l, nb))
        return (words_to_ints(c0, W, self.n), words_to_ints(c1, W, self.n)), int(l[0]), bits(nb[0]), bits(nb[1])

    def ct_get_words(self, k, W):
        c0, c1 = np.empty(W * self.n, dtype=np.uint64), np.empty(W * self.n, dtype=np.uint64)
        l, nb = np.zeros(1, dtype=np.uint32), np.zeros(2, dtype=np.float64)
        self._ck("ref_ct_get", self.L.ref_ct_get(k, c0, c1, W, l, nb))
        return c0, c1

    def ct_set_words(self, k, c0, c1, W, l, nu=1.0, B=0.0):
        self._ck("ref_ct_set", self.L.ref_ct_set(k, _big(c0), _big(c1), W, l, nu, B))

    def pt_set(self, k, m, nu, W=None):
        W = W or self.W
        self._ck("ref_pt_set", self.L.ref_pt_set(k, ints_to_words(m, W), W, float(nu)))

    def pt_get(self, k, W=None):
        W = W or self.W
        m, nu = np.empty(W * self.n, dtype=np.uint64), np.zeros(1, dtype=np.float64)
        self._ck("ref_pt_get", self.L.ref_pt_get(k, m, W, nu))
        return words_to_ints(m, W, self.n), float(nu[0])

    def he_ecd(self, k, z):
        reim = np.ascontiguousarray(np.asarray(z, dtype=np.complex128)).view(np.float64)
        assert reim.size == 2 * self.slots
        self._ck("ref_he_ecd", self.L.ref_he_ecd(k, reim))

    def evk_set(self, which, p0, p1):
        """which: 'rlk', 'ck' or a rotation index; residue slabs uint64[dimevk][n]"""
        idx = {"rlk": 0, "ck": 1}.get(which, None)
        idx = idx if idx is not None else 2 + int(which)
        p0, p1 = _big(p0), _big(p1)
        assert p0.size == p1.size == self.dimevk * self.n
        self._ck("ref_evk_set", self.L.ref_evk_set(idx, p0, p1))

    def he_add(self, dst, a, b): self._ck("he_add", self.L.ref_he_addsub(0, dst, a, b))
    def he_sub(self, dst, a, b): self._ck("he_sub", self.L.ref_he_addsub(1, dst, a, b))
    def he_neg(self, k): self._ck("he_neg", self.L.ref_he_neg(k))
    def he_addpt(self, dst, src, pt): self._ck("he_addpt", self.L.ref_he_pt_op(0, dst, src, pt))
    def he_subpt(self, dst, src, pt): self._ck("he_subpt", self.L.ref_he_pt_op(1, dst, src, pt))
    def he_mulpt(self, dst, src, pt): self._ck("he_mulpt", self.L.ref_he_pt_op(2, dst, src, pt))
    def he_mul(self, dst, a, b): self._ck("he_mul", self.L.ref_he_mul(dst, a, b))
    def he_rs(self, k): self._ck("he_rs", self.L.ref_he_rs(k, 0))
    def he_moddown(self, k): self._ck("he_moddown", self.L.ref_he_rs(k, 1))
    def he_rot(self, k, rot): self._ck("he_rot", self.L.ref_he_rot(k, rot))
    def he_conj(self, k): self._ck("he_conj", self.L.ref_he_conj(k))
    def he_sum(self, dst, src): self._ck("he_sum", self.L.ref_he_sum(dst, src))
    def he_idx(self, dst, src, idx): self._ck("he_idx", self.L.ref_he_idx(dst, src, idx))

    def he_gemv(self, dst, A, src):
        reim = np.ascontiguousarray(np.asarray(A, dtype=np.complex128)).reshape(-1).view(np.float64)
        assert reim.size == 2 * self.slots * self.slots
        self._ck("he_gemv", self.L.ref_he_gemv(dst, reim, src))


# ---------------------------------------------------------------------------
# which build
# ---------------------------------------------------------------------------
_NATIVE = None


def floor_is_native():
    """does the LOADED libgcrypt floor-divide a negative dividend correctly?  (-1000503 fdiv 1000 = -1001 rem 497)"""
    global _NATIVE
    if _NATIVE is None:
        (q, r), = Ref(AS_IS).fdiv([-1000503], 1000, 0)
        assert r == 497 and abs(q) == 1001, "unknown floor-division behaviour of this libgcrypt: q = %d, r = %d" % (q, r)
        _NATIVE = q == -1001
    return _NATIVE


def which():
    return AS_IS if floor_is_native() else FLOOR


# ---------------------------------------------------------------------------
# worker processes
# ---------------------------------------------------------------------------
def _child(fn, arg, conn, errpath):
    fd = os.open(errpath, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
    os.dup2(fd, 2)
    try:
        conn.send(("ok", fn(arg)))
    except BaseException as e:                       # noqa: the parent re-raises it with the text
        import traceback
        conn.send(("error", "%s\n%s" % (repr(e), traceback.format_exc())))
    conn.close()


def run(fn, args, workers=8, timeout=1500):
    """[fn(a) for a in args], each call in a fresh spawned process, at most min(workers, 8) at a time"""
    ctx = _mp.get_context("spawn")
    workers = max(1, min(int(workers), 8))
    results = [None] * len(args)
    pending, running = list(enumerate(args)), []
    with tempfile.TemporaryDirectory() as td:
        try:
            while pending or running:
                while pending and len(running) < workers:
                    i, a = pending.pop(0)
                    recv, send = ctx.Pipe(duplex=False)
                    err = os.path.join(td, "err%d.txt" % i)
                    p = ctx.Process(target=_child, args=(fn, a, send, err))
                    p.start()
                    send.close()
                    running.append((i, p, recv, err))
                i, p, recv, err = running.pop(0)
                msg = None
                try:
                    if recv.poll(timeout):
                        msg = recv.recv()
                except EOFError:
                    msg = None
                p.join(30 if msg else 5)
                if p.is_alive():
                    p.kill()
                    p.join()
                with open(err) as f:
                    stderr = f.read()
                if msg is None:
                    raise RuntimeError("reference worker %d (%s) died with exit code %s; its stderr:\n%s" % (i, getattr(fn, "__name__", fn), p.exitcode, stderr[-4000:]))
                if msg[0] != "ok":
                    raise RuntimeError("reference worker %d (%s) failed: %s\nits stderr:\n%s" % (i, getattr(fn, "__name__", fn), msg[1], stderr[-4000:]))
                results[i] = msg[1]
        finally:
            for _, p, _, _ in running:
                p.kill()
                p.join()
    return results
