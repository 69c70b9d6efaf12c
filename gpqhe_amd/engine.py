"""Host-side mirror of the reference's RNS interface on top of the C ABI.

Names follow the reference: `PolyContext` is the RNS part of `polyctx`
(src/poly.h:49-65), `poly_ntt` / `poly_invntt` / `poly_rns_mul` / `poly_rns_add`
are src/ntt.c:37,54 and src/poly.c:71-82 applied to whole limb-major slabs
`uint64[batch][dim][n]` in HBM, `he_mul_tensor` / `he_keyswitch` are the limb
loops of src/he-mult.c:116-138 and :58-66.  Slabs are torch int64 CUDA tensors
carrying the uint64 bit patterns (torch is the allocator/stream provider; the
arithmetic happens in libgpqhe_hip.so).
"""
import ctypes as C

import numpy as np

from . import _native


def _torch():
    import torch
    return torch


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    torch = _torch()
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_device(a, device=None):
    """numpy uint64 array -> int64 CUDA tensor with the same bits."""
    torch = _torch()
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(device or "cuda")


def to_host(t):
    """int64 CUDA tensor -> numpy uint64 array."""
    return t.detach().cpu().numpy().view(np.uint64)


class PolyContext:
    """`polyctx_init(logn, q)` restricted to what the hot path reads: ring
    degree, the prime chain and the per-prime NTT tables (src/precomp.c:244-264,
    :354-380).  `nprimes` is `polyctx.dimub`; pass `logq` instead to get the
    reference's own bound (src/precomp.c:357)."""

    def __init__(self, logn, nprimes=None, logq=None, device=None):
        self.lib = _native.load()
        if nprimes is None:
            if logq is None:
                raise ValueError("PolyContext needs nprimes or logq")
            nprimes = self.lib.gpq_dimub(logn, logq)
        torch = _torch()
        if not torch.cuda.is_available():
            raise _native.GpqError("gpqhe_amd needs a HIP device; there is no CPU path")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self._dev = torch.device("cuda", self.device)     # workspaces and streams belong to the context's device, not the current one
        h = C.c_void_p()
        _native.check(self.lib.gpq_ctx_create(C.byref(h), logn, nprimes, self.device), "gpq_ctx_create")
        self.h = h
        self.logn, self.n, self.nprimes = logn, 1 << logn, nprimes
        self.p = [self.lib.gpq_ctx_const(h, d, 0) for d in range(nprimes)]

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _ptr(self, t):
        """device pointer of a slab, which must live on this context's device"""
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError("slab on %s, context on cuda:%d" % (t.device, self.device))
        return C.c_void_p(t.data_ptr())

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpq_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def const(self, name, d):
        which = {"p": 0, "pinv_mont": 1, "pinv_barr": 2, "ninv": 3, "psi": 4}[name]
        return self.lib.gpq_ctx_const(self.h, d, which)

    def zetas(self, d, inverse=False):
        ptr = self.lib.gpq_ctx_zetas(self.h, d, 1 if inverse else 0)
        return np.ctypeslib.as_array(ptr, shape=(self.n,)).copy()

    def set_chunk(self, chunk):
        _native.check(self.lib.gpq_set_chunk(self.h, chunk), "gpq_set_chunk")

    def set_limb_classes(self, wide, split):
        """first `wide` limbs wide-split butterflies, up to `split` split-twiddle ones, the rest 7-mad (clamped; bit-identical)"""
        _native.check(self.lib.gpq_set_limb_classes(self.h, wide, split), "gpq_set_limb_classes")

    def set_limb_block(self, limbs):
        _native.check(self.lib.gpq_set_limb_block(self.h, limbs), "gpq_set_limb_block")

    # --- MPI <-> RNS bridge on big slabs uint64[batch][W][n] ---
    def rns_decompose(self, slab, big, W, dim):
        """src/rns.c:37-48 for all limbs."""
        batch = big.numel() // (W * self.n)
        _native.check(self.lib.gpq_rns_decompose(self.h, self._ptr(slab), self._ptr(big), W, dim, batch, self._stream()), "gpq_rns_decompose")
        return slab

    def rns_reconstruct(self, big, Wout, slab, dim, logq):
        """src/poly.c:109-120 with q = 2^logq (0: centre mod P only)."""
        batch = self._shape(slab, dim)
        _native.check(self.lib.gpq_rns_reconstruct(self.h, self._ptr(big), Wout, self._ptr(slab), dim, batch, logq, self._stream()), "gpq_rns_reconstruct")
        return big

    def set_bridge_mfma(self, on):
        """matrix-core (default) or integer-VALU rns_decompose (off: also the CRT sum and the tail on the integer VALU); read by every call that
        decomposes or reconstructs -- the he_mul / he_swk / he_rot_hoisted / he_gemv family, he_mulpt, poly_mul, he_dec, he_enc_*, he_genswk*, gemv plans; same words"""
        _native.check(self.lib.gpq_set_bridge_mfma(self.h, 1 if on else 0), "gpq_set_bridge_mfma")

    PRESCALE_DEFAULT = 3

    def set_prescale(self, mode):
        """he_mul / he_swk: what the inverse transforms pre-multiply for the kernels behind them -- 3 (default, also True): the weights of the
        key switch's whole basis, the relinearisation tail is one product; 2: per-basis CRT weights + w_j for the relinearisation front;
        1: per-basis CRT weights; 0 / False: nothing.  All exact; the tests compare them.  Two-pass rings only; he_rot_hoisted and, through it,
        he_gemv / he_gemv_planned / he_gemv_multi make the same choice.  Calls without a key switch do not read it."""
        mode = self.PRESCALE_DEFAULT if mode is True else int(mode)
        _native.check(self.lib.gpq_set_prescale(self.h, mode), "gpq_set_prescale")

    def set_stream_bridge(self, on):
        """he_mul / he_swk, and the tail of every rotation of he_rot_hoisted / he_gemv / he_gemv_planned / he_gemv_multi: the fused streaming bridge
        kernels (default) or round 3's separate kernels; same words.  Calls without a key switch do not read it."""
        _native.check(self.lib.gpq_set_stream_bridge(self.h, 1 if on else 0), "gpq_set_stream_bridge")

    def set_lazy_decompose(self, on):
        """he_mul and he_swk (so also he_rot_hoisted of one rotation and the giant steps of the he_gemv family) on two-pass rings: their
        rns_decompose output may stay in (0, 3p) for the forward transforms (default) or be canonical; same results.  The hoisted decomposition
        of he_rot_hoisted and the plans are always canonical."""
        _native.check(self.lib.gpq_set_lazy_decompose(self.h, 1 if on else 0), "gpq_set_lazy_decompose")

    def set_overlap(self, on):
        """he_mul / he_swk / tensor / key switch over several launch groups: -1 = two lanes when affordable (default), 0 / False = one, 1 / True = two; same words.
        he_rot_hoisted and the he_gemv family keep their groups in order on the caller's stream whatever this says."""
        v = -1 if (on is not True and on is not False and int(on) < 0) else (1 if on else 0)
        _native.check(self.lib.gpq_set_overlap(self.h, v), "gpq_set_overlap")

    def debug_fail_peer(self, on=True):
        """tests: the next creation of the peer lane (True / 1) or the next allocation of its workspace (2) fails like an allocation would"""
        _native.check(self.lib.gpq_debug_fail_peer(self.h, int(on)), "gpq_debug_fail_peer")

    def debug_table_bytes(self, which=0):
        """read-only device bytes owned by the context (0) / by its peer lane (1: zero, the peer borrows); 2: a peer exists; 3: the peer's table pointers are the context's"""
        return int(self.lib.gpq_debug_table_bytes(self.h, which))

    def last_lanes(self):
        """lanes (1 or 2) the last multi-group call on this context ran on"""
        return int(self.lib.gpq_last_lanes(self.h))

    def set_nt_policy(self, mode):
        """slab traffic of the transform kernels non-temporal: -1 by working set (default), 0 never, 1 always; never changes a word"""
        _native.check(self.lib.gpq_set_nt_policy(self.h, int(mode)), "gpq_set_nt_policy")

    def debug_force_redo(self, every):
        """tests: the streaming bridge kernels (he_mul's CRT -> decompose, the one-product tail of he_mul / he_swk / he_rot_hoisted / he_gemv*) also
        flag every coefficient whose index is a multiple of `every` (0: off)"""
        _native.check(self.lib.gpq_debug_force_redo(self.h, int(every)), "gpq_debug_force_redo")

    def debug_zero_watch(self, on=True):
        """tests: keep copies of gpq_ntt's zero-flag words before and after the redo kernel (src/ntt.c:45-48)"""
        _native.check(self.lib.gpq_debug_zero_watch(self.h, 1 if on else 0), "gpq_debug_zero_watch")

    def debug_zero_flags(self, count):
        """(before, after) flag words of the last gpq_ntt launch group, word [polynomial * dim + limb]"""
        before, after = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
        got = self.lib.gpq_debug_zero_flags(self.h, before.ctypes.data_as(C.c_void_p), after.ctypes.data_as(C.c_void_p), count)
        if got != count:
            raise RuntimeError("gpq_debug_zero_flags: %d words watched, %d asked for" % (got, count))
        return before, after

    def set_exact_crt(self, on):
        """tests: the full-width CRT kernel for every coefficient of every reconstruction (rns_reconstruct, poly_mul, he_mulpt, he_dec, he_enc_*,
        gemv_inner, the relinearisation tail of the he_mul / he_swk / he_rot_hoisted / he_gemv family); same words"""
        _native.check(self.lib.gpq_set_exact_crt(self.h, 1 if on else 0), "gpq_set_exact_crt")

    def poly_mul(self, r, a, b, W, dim, logq):
        """src/poly.c:84-107 on big slabs, q = 2^logq."""
        torch = _torch()
        batch = a.numel() // (W * self.n)
        ws = torch.empty(self.lib.gpq_poly_mul_workspace_bytes(self.h, dim, batch) // 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_poly_mul(self.h, self._ptr(r), self._ptr(a), self._ptr(b), W, dim, logq, batch, self._ptr(ws), self._stream()), "gpq_poly_mul")
        return r

    def poly_mul_general(self, r, a, b, W, dim, q):
        """src/poly.c:84-107 on big slabs for an arbitrary modulus q (Python int)."""
        torch = _torch()
        batch = a.numel() // (W * self.n)
        Lq = (q.bit_length() + 63) // 64
        qw = (_native.u64 * Lq)(*[(q >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(Lq)])
        ws = torch.empty(self.lib.gpq_poly_mul_general_workspace_bytes(self.h, dim, batch) // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_poly_mul_general(self.h, self._ptr(r), self._ptr(a), self._ptr(b), W, dim, qw, Lq, batch, self._ptr(ws), self._stream()),
                      "gpq_poly_mul_general")
        return r

    def big_addsub(self, out, a, b, W, mode):
        """out = a + b (mode 0), a - b (1), -a (2) on big slabs of W words, wrapping: src/he-add.c:32-140 before its mpi_smod."""
        polys = a.numel() // (W * self.n)
        _native.check(self.lib.gpq_big_addsub(self.h, self._ptr(out), self._ptr(a), self._ptr(b) if b is not None else None, W, polys, mode, self._stream()),
                      "gpq_big_addsub")
        return out

    def he_rs(self, c0, c1, W, logDelta, logql):
        """src/he-rescale.c:33-54 with Delta = 2^logDelta, q_l = 2^logql, in place."""
        batch = c0.numel() // (W * self.n)
        _native.check(self.lib.gpq_he_rs(self.h, self._ptr(c0), self._ptr(c1), W, logDelta, logql, batch, self._stream()), "gpq_he_rs")

    def he_dims(self, logqL, logql):
        """(dimP, dimA, dimB, dimevk) as src/precomp.c:401,407 and src/he-mult.c:99,51 compute them."""
        v = [C.c_uint() for _ in range(4)]
        _native.check(self.lib.gpq_he_dims(self.h, logqL, logql, *[C.byref(x) for x in v]), "gpq_he_dims")
        return tuple(x.value for x in v)

    def he_mul(self, out_c0, out_c1, ct1c0, ct1c1, ct2c0, ct2c1, rlk0, rlk1, W, logql, dimA, dimB, dimP):
        """src/he-mult.c:88-156 on big slabs, q_l = 2^logql."""
        torch = _torch()
        batch = ct1c0.numel() // (W * self.n)
        nbytes = self.lib.gpq_he_mul_workspace_bytes(self.h, W, dimA, dimB, dimP, batch)
        ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_mul(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(ct1c0), self._ptr(ct1c1), self._ptr(ct2c0), self._ptr(ct2c1),
                                          self._ptr(rlk0), self._ptr(rlk1), W, logql, dimA, dimB, dimP, batch, self._ptr(ws), self._stream()), "gpq_he_mul")
        return ws

    def he_mul_rs(self, out_c0, out_c1, ct1c0, ct1c1, ct2c0, ct2c1, rlk0, rlk1, W, logql, dimA, dimB, dimP, logDelta):
        """he_mul then he_rs (src/he-mult.c:88-156, src/he-rescale.c:33-54) in one call: the rescale rides in the relinearisation tail."""
        torch = _torch()
        batch = ct1c0.numel() // (W * self.n)
        nbytes = self.lib.gpq_he_mul_workspace_bytes(self.h, W, dimA, dimB, dimP, batch)
        ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_mul_rs(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(ct1c0), self._ptr(ct1c1), self._ptr(ct2c0), self._ptr(ct2c1),
                                             self._ptr(rlk0), self._ptr(rlk1), W, logql, dimA, dimB, dimP, logDelta, batch, self._ptr(ws), self._stream()), "gpq_he_mul_rs")
        return ws

    def relin_tail(self, out, chat, d, W, logql, dimB, dimP):
        """src/he-mult.c:67-77 alone (d = None: nothing added)."""
        torch = _torch()
        batch = self._shape(chat, dimB)
        ws = torch.empty(self.lib.gpq_relin_tail_workspace_bytes(self.h, W, dimB, dimP, batch) // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_relin_tail(self.h, self._ptr(out), self._ptr(chat), self._ptr(d) if d is not None else None, W, logql, dimB, dimP,
                                              batch, self._ptr(ws), self._stream()), "gpq_relin_tail")
        return out

    def relin_tail_overwriting(self, out, chat, d, W, logql, dimB, dimP):
        """src/he-mult.c:67-77 with `chat` given up as scratch: the tail as one product over all dimB limbs."""
        torch = _torch()
        batch = self._shape(chat, dimB)
        ws = torch.empty(self.lib.gpq_relin_tail_workspace_bytes(self.h, W, dimB, dimP, batch) // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_relin_tail_overwriting(self.h, self._ptr(out), self._ptr(chat), self._ptr(d) if d is not None else None, W, logql, dimB, dimP,
                                                          batch, self._ptr(ws), self._stream()), "gpq_relin_tail_overwriting")
        return out

    def he_swk(self, out_c0, out_c1, d0, d1, swk0, swk1, W, logql, dimB, dimP):
        """src/he-automorphism.c:40-85 on big slabs, q_l = 2^logql."""
        torch = _torch()
        batch = d0.numel() // (W * self.n)
        nbytes = self.lib.gpq_he_swk_workspace_bytes(self.h, W, dimB, dimP, batch)
        ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_swk(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(d0), self._ptr(d1), self._ptr(swk0), self._ptr(swk1),
                                          W, logql, dimB, dimP, batch, self._ptr(ws), self._stream()), "gpq_he_swk")
        return ws

    @staticmethod
    def _words(q, Lq=None):
        """q as little-endian words; Lq > the words q needs passes zero top words"""
        L = Lq or (q.bit_length() + 63) // 64
        return (_native.u64 * L)(*[(q >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(L)]), L

    def rns_reconstruct_general(self, big, Wout, slab, dim, q, Lq=None):
        """src/poly.c:109-120 for an arbitrary modulus q (Python int): centred mod P, then mpi_smod(., q)."""
        torch = _torch()
        batch = self._shape(slab, dim)
        qw, L = self._words(q, Lq)
        scratch = torch.empty(self.lib.gpq_poly_mul_general_workspace_bytes(self.h, dim, batch) // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_rns_reconstruct_general(self.h, self._ptr(big), Wout, self._ptr(slab), dim, batch, qw, L, self._ptr(scratch), self._stream()),
                      "gpq_rns_reconstruct_general")
        return big

    def relin_tail_general(self, out, chat, d, W, ql, dimB, dimP):
        """src/he-mult.c:67-77 alone for an arbitrary q_l (d = None: nothing added)."""
        torch = _torch()
        batch = self._shape(chat, dimB)
        qw, L = self._words(ql)
        # the tail runs all `batch` polynomials in one group; the one-polynomial general workspace times batch covers it
        nbytes = batch * self.lib.gpq_he_general_workspace_bytes(self.h, W, 0, dimB, dimP, 1)
        ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_relin_tail_general(self.h, self._ptr(out), self._ptr(chat), self._ptr(d) if d is not None else None, W, qw, L, dimB, dimP,
                                                      batch, self._ptr(ws), self._stream()), "gpq_relin_tail_general")
        return out

    def he_mul_general(self, out_c0, out_c1, ct1c0, ct1c1, ct2c0, ct2c1, rlk0, rlk1, W, ql, dimA, dimB, dimP):
        """src/he-mult.c:88-156 for an arbitrary q_l (Python int)."""
        torch = _torch()
        batch = ct1c0.numel() // (W * self.n)
        qw, L = self._words(ql)
        ws = torch.empty(self.lib.gpq_he_general_workspace_bytes(self.h, W, dimA, dimB, dimP, batch) // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_mul_general(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(ct1c0), self._ptr(ct1c1), self._ptr(ct2c0), self._ptr(ct2c1),
                                                  self._ptr(rlk0), self._ptr(rlk1), W, qw, L, dimA, dimB, dimP, batch, self._ptr(ws), self._stream()),
                      "gpq_he_mul_general")

    def he_swk_general(self, out_c0, out_c1, d0, d1, swk0, swk1, W, ql, dimB, dimP):
        torch = _torch()
        batch = d0.numel() // (W * self.n)
        qw, L = self._words(ql)
        ws = torch.empty(self.lib.gpq_he_general_workspace_bytes(self.h, W, 0, dimB, dimP, batch) // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_swk_general(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(d0), self._ptr(d1), self._ptr(swk0), self._ptr(swk1),
                                                  W, qw, L, dimB, dimP, batch, self._ptr(ws), self._stream()), "gpq_he_swk_general")

    def he_rs_general(self, c0, c1, W, delta, ql):
        """src/he-rescale.c:33-54 for any Delta (< 2^64) and any q_l."""
        torch = _torch()
        batch = c0.numel() // (W * self.n)
        qw, L = self._words(ql)
        scratch = torch.empty(192, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_rs_general(self.h, self._ptr(c0), self._ptr(c1), W, delta, qw, L, batch, self._ptr(scratch), self._stream()), "gpq_he_rs_general")

    def he_mulpt(self, out_c0, out_c1, c0, c1, m, W, logql, dim):
        """src/he-mult.c:159-196 on big slabs."""
        torch = _torch()
        batch = c0.numel() // (W * self.n)
        ws = torch.empty(self.lib.gpq_he_mulpt_workspace_bytes(self.h, dim, batch) // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_mulpt(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(c0), self._ptr(c1), self._ptr(m), W, logql, dim, batch,
                                            self._ptr(ws), self._stream()), "gpq_he_mulpt")

    def he_mulpt_general(self, out_c0, out_c1, c0, c1, m, W, ql, dim):
        """src/he-mult.c:159-196 for an arbitrary q_l (Python int)."""
        torch = _torch()
        batch = c0.numel() // (W * self.n)
        qw, L = self._words(ql)
        nbytes = self.lib.gpq_he_mulpt_workspace_bytes(self.h, dim, batch) + self.lib.gpq_poly_mul_general_workspace_bytes(self.h, dim, batch)
        ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_mulpt_general(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(c0), self._ptr(c1), self._ptr(m), W, qw, L, dim,
                                                    batch, self._ptr(ws), self._stream()), "gpq_he_mulpt_general")

    @staticmethod
    def const_pt(re, im, logDelta):
        """(a, b) of he_const_pt (src/he-encode.c:119-125) for Delta = 2^logDelta: the plaintext is a + b x^(n/2).  Host only."""
        a, b = C.c_int64(), C.c_int64()
        _native.check(_native.load().gpq_const_pt(float(re), float(im), logDelta, C.byref(a), C.byref(b)), "gpq_const_pt")
        return a.value, b.value

    def he_mulpt_const_fits(self, a, b, logql, dim):
        """does the constant path give he_mulpt's words for inputs centred mod 2^logql on `dim` limbs?"""
        return bool(self.lib.gpq_he_mulpt_const_fits(self.h, a, b, logql, dim))

    def he_mulpt_const(self, out_c0, out_c1, c0, c1, a, b, W, logql, dim, logDelta=0, bad=None):
        """he_mulpt by a + b x^(n/2) and, logDelta != 0, he_rs (src/he-mult.c:159-196, src/he-rescale.c:33-54) in one pass over the big slabs;
        out may be the input.  bad: None or a zeroed int32 device tensor that counts input coefficients not centred mod 2^logql."""
        batch = c0.numel() // (W * self.n)
        _native.check(self.lib.gpq_he_mulpt_const(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(c0), self._ptr(c1), a, b, W, logql, dim, logDelta,
                                                  batch, self._ptr(bad) if bad is not None else None, self._stream()), "gpq_he_mulpt_const")

    def he_addpt_const(self, out_c0, out_c1, c0, c1, a, b, W, logql, sub=False):
        """he_addpt / he_subpt (src/he-add.c:80-123) with the plaintext a + b x^(n/2) in one launch; out may be the input."""
        batch = c0.numel() // (W * self.n)
        _native.check(self.lib.gpq_he_addpt_const(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(c0), self._ptr(c1), a, b, 1 if sub else 0, W, logql,
                                                  batch, self._stream()), "gpq_he_addpt_const")

    # --- the evaluators of src/he-algo.c:131-458 (include/gpqhe_hip_algo.h) ---
    ALGO_KINDS = {"inv": 0, "sqrt": 1, "sigmoid": 2, "log": 3, "exp": 4}

    def he_lin_const(self, out_c0, out_c1, terms, W, logql, a=0, b=0):
        """out = smod(sum of sign * (x_c0, x_c1) over the one to three `terms` (x_c0, x_c1, sign) + (a + b x^(n/2)), 2^logql): the collapsed
        chain of he_neg / he_add / he_sub / he_addpt / he_subpt / he_moddown / he_copy_ct, one launch; out may be one of the terms."""
        K = len(terms)
        batch = terms[0][0].numel() // (W * self.n)
        x0 = (C.c_void_p * 3)(*[self._ptr(t[0]).value for t in terms])
        x1 = (C.c_void_p * 3)(*[self._ptr(t[1]).value for t in terms])
        sg = (C.c_int * 3)(*[int(t[2]) for t in terms])
        _native.check(self.lib.gpq_he_lin_const(self.h, self._ptr(out_c0), self._ptr(out_c1), x0, x1, sg, K, a, b, W, logql, batch, self._stream()),
                      "gpq_he_lin_const")

    def he_algo_depth(self, kind, iter=0):
        return int(self.lib.gpq_he_algo_depth(self.ALGO_KINDS[kind], iter))

    def he_algo_workspace_bytes(self, kind, W, logqL, logql, logDelta, iter, batch):
        """bytes of an evaluator call's workspace; 0 when the call would be refused"""
        return int(self.lib.gpq_he_algo_workspace_bytes(self.h, self.ALGO_KINDS[kind], W, logqL, logql, logDelta, iter, batch))

    def he_algo_call(self, kind, out_c0, out_c1, c0, c1, rlk0, rlk1, W, logqL, logql, logDelta, iter, workspace, m=None, dimpt=0):
        """the return code of gpq_he_<kind> on a caller-owned workspace (tests look at refusals and at the workspace's end)"""
        batch = c0.numel() // (W * self.n)
        head = [self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(c0), self._ptr(c1)]
        keys = [self._ptr(rlk0), self._ptr(rlk1)]
        tail = [batch, self._ptr(workspace), self._stream()]
        if kind == "exp":
            return self.lib.gpq_he_exp(*head, self._ptr(m), dimpt, *keys, W, logqL, logql, logDelta, iter, *tail)
        if kind in ("inv", "sqrt"):
            return getattr(self.lib, "gpq_he_" + kind)(*head, *keys, W, logqL, logql, logDelta, iter, *tail)
        return getattr(self.lib, "gpq_he_" + kind)(*head, *keys, W, logqL, logql, logDelta, *tail)

    def he_algo(self, kind, out_c0, out_c1, c0, c1, rlk0, rlk1, W, logqL, logql, logDelta, iter=0, m=None, dimpt=0):
        """he_inv / he_sqrt / he_sigmoid / he_log / he_exp (kind) of the batch as one call; q_l = 2^logql is the input's modulus, the output's
        is 2^(logql - depth logDelta).  he_exp: m = he_ecd of the constant vector a / 2^iter (one big slab), dimpt = he_mulpt's limbs."""
        torch = _torch()
        batch = c0.numel() // (W * self.n)
        nbytes = self.he_algo_workspace_bytes(kind, W, logqL, logql, logDelta, iter, batch)
        if not nbytes:
            raise _native.GpqError("gpq_he_algo_workspace_bytes: " + self.lib.gpq_last_error().decode())
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=self._dev)
        _native.check(self.he_algo_call(kind, out_c0, out_c1, c0, c1, rlk0, rlk1, W, logqL, logql, logDelta, iter, ws, m, dimpt), "gpq_he_" + kind)
        return ws

    def he_lin_pt(self, out_c0, out_c1, terms, m, W, logql, msign=1, a=0, b=0):
        """he_lin_const plus msign * m in c0: he_addpt / he_subpt by ONE dense plaintext m (a big slab of one polynomial, shared by the batch)"""
        K = len(terms)
        batch = terms[0][0].numel() // (W * self.n)
        x0 = (C.c_void_p * 3)(*[self._ptr(t[0]).value for t in terms])
        x1 = (C.c_void_p * 3)(*[self._ptr(t[1]).value for t in terms])
        sg = (C.c_int * 3)(*[int(t[2]) for t in terms])
        _native.check(self.lib.gpq_he_lin_pt(self.h, self._ptr(out_c0), self._ptr(out_c1), x0, x1, sg, K, self._ptr(m), msign, a, b, W, logql, batch,
                                             self._stream()), "gpq_he_lin_pt")

    # --- he_cmp / he_cmppt (src/he-algo.c:460-548) ---
    @staticmethod
    def he_cmp_rounds(alpha):
        """he_cmp's t for alpha in 1..52, -1 otherwise.  Host only."""
        return int(_native.load().gpq_he_cmp_rounds(alpha))

    @staticmethod
    def he_cmp_depth(iter, t):
        """(3 + iter)(1 + t), or -1.  Host only."""
        return int(_native.load().gpq_he_cmp_depth(iter, t))

    def he_cmp_workspace_bytes(self, with_pt, W, logqL, logql, logDelta, iter, t, batch):
        """bytes of a gpq_he_cmp (with_pt false) / gpq_he_cmppt call's workspace; 0 when the call would be refused"""
        return int(self.lib.gpq_he_cmp_workspace_bytes(self.h, 1 if with_pt else 0, W, logqL, logql, logDelta, iter, t, batch))

    def he_cmp_call(self, out_c0, out_c1, a_c0, a_c1, other, rlk0, rlk1, W, logqL, logql, logDelta, iter, t, workspace):
        """the return code of gpq_he_cmp (other = (b_c0, b_c1)) or gpq_he_cmppt (other = the plaintext slab m) on a caller-owned workspace"""
        batch = a_c0.numel() // (W * self.n)
        head = [self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(a_c0), self._ptr(a_c1)]
        tail = [self._ptr(rlk0), self._ptr(rlk1), W, logqL, logql, logDelta, iter, t, batch, self._ptr(workspace), self._stream()]
        if isinstance(other, (tuple, list)):
            return self.lib.gpq_he_cmp(*head, self._ptr(other[0]), self._ptr(other[1]), *tail)
        return self.lib.gpq_he_cmppt(*head, self._ptr(other), *tail)

    def he_cmp(self, out_c0, out_c1, a_c0, a_c1, other, rlk0, rlk1, W, logqL, logql, logDelta, iter, t):
        """he_cmp(a, other = (b_c0, b_c1)) or he_cmppt(a, other = m) of the batch as one call; t from he_cmp_rounds(alpha)"""
        torch = _torch()
        batch = a_c0.numel() // (W * self.n)
        with_pt = not isinstance(other, (tuple, list))
        nbytes = self.he_cmp_workspace_bytes(with_pt, W, logqL, logql, logDelta, iter, t, batch)
        if not nbytes:
            raise _native.GpqError("gpq_he_cmp_workspace_bytes: " + self.lib.gpq_last_error().decode())
        ws = torch.empty(nbytes // 8, dtype=torch.int64, device=self._dev)
        _native.check(self.he_cmp_call(out_c0, out_c1, a_c0, a_c1, other, rlk0, rlk1, W, logqL, logql, logDelta, iter, t, ws),
                      "gpq_he_cmppt" if with_pt else "gpq_he_cmp")
        return ws

    def he_genswk(self, evk0, evk1, p1, sk, e, sp, W, dimP, logqL, dimevk):
        """src/he-kem.c:74-118 from host-sampled p1 / e and the hidden polynomial sp; q_L = 2^logqL."""
        torch = _torch()
        nbytes = self.lib.gpq_he_genswk_workspace_bytes(self.h, W, dimP, logqL)
        if not nbytes:
            raise _native.GpqError("gpq_he_genswk_workspace_bytes: " + self.lib.gpq_last_error().decode())
        ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_genswk(self.h, self._ptr(evk0), self._ptr(evk1), self._ptr(p1), self._ptr(sk), self._ptr(e), self._ptr(sp), W, dimP, logqL, dimevk,
                                             self._ptr(ws), self._stream()), "gpq_he_genswk")

    def he_genswk_dimmul(self, dimP, logqL):
        """limbs of he_genswk's product (src/he-kem.c:83) for q_L = 2^logqL: what sk_ntt of he_genswk_batch is packed over"""
        dimmul = self.lib.gpq_he_genswk_dimmul(self.h, dimP, logqL)
        if not dimmul:
            raise _native.GpqError("gpq_he_genswk_dimmul: " + self.lib.gpq_last_error().decode())
        return dimmul

    def he_genswk_batch(self, evk0, evk1, p1, e, sk_ntt, W, dimP, logqL, dimevk, sk_small=None, galois=None, sp=None, Wsp=0):
        """he_genswk (src/he-kem.c:74-118) for every key of evk0 / evk1 = [count][dimevk][n] in one call, q_L = 2^logqL: p1 = the RAW
        sample_uniform big slabs [count][W][n], e = int8 small slabs [count][n], sk_ntt = the secret as ONE NTT-domain slab [dimmul][n]
        (evk_pack over he_genswk_dimmul limbs).  The hidden polynomials: galois = one odd g per key (5^rot mod 2^64: poly_rot, 2n - 1:
        poly_conj) with sk_small = the int8 secret [n], gathered by the kernel; or sp = big slabs [count][Wsp][n] (he_genrlk's s^2)."""
        torch = _torch()
        count = e.numel() // self.n
        nbytes = self.lib.gpq_he_genswk_batch_workspace_bytes(self.h, W, dimP, logqL, dimevk, count)
        if not nbytes:
            raise _native.GpqError("gpq_he_genswk_batch_workspace_bytes: " + self.lib.gpq_last_error().decode())
        ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        g = None if galois is None else (C.c_uint64 * max(len(galois), 1))(*[int(v) & (2**64 - 1) for v in galois])
        if g is not None and len(galois) != count:
            raise ValueError("%d keys need %d Galois elements, not %d" % (count, count, len(galois)))
        opt = lambda t: None if t is None else self._ptr(t)
        _native.check(self.lib.gpq_he_genswk_batch(self.h, self._ptr(evk0), self._ptr(evk1), self._ptr(p1), self._ptr(e), self._ptr(sk_ntt), opt(sk_small), g,
                                                   opt(sp), Wsp, W, dimP, logqL, dimevk, count, self._ptr(ws), self._stream()), "gpq_he_genswk_batch")
        return ws

    def _key_ptrs(self, keys):
        """host array of device pointers (None stays NULL)"""
        return (C.c_void_p * len(keys))(*[None if k is None else self._ptr(k).value for k in keys])

    def he_rot_hoisted(self, out_c0, out_c1, c0, c1, rots, rk0, rk1, W, logql, dimB, dimP):
        """he_rot (src/he-automorphism.c:101-115) of the batch by every rots[r] with key (rk0[r], rk1[r]); c1 is decomposed and transformed
        once.  Outputs rotation-major: len(rots) x batch big slabs each."""
        torch = _torch()
        batch, nrot = c0.numel() // (W * self.n), len(rots)
        nbytes = self.lib.gpq_he_rot_hoisted_workspace_bytes(self.h, W, dimB, dimP, nrot, batch)
        ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        r = (C.c_uint * max(nrot, 1))(*rots)
        _native.check(self.lib.gpq_he_rot_hoisted(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(c0), self._ptr(c1), r, self._key_ptrs(rk0),
                                                  self._key_ptrs(rk1), nrot, W, logql, dimB, dimP, batch, self._ptr(ws), self._stream()), "gpq_he_rot_hoisted")
        return ws

    def he_gemv(self, out_c0, out_c1, c0, c1, diag, rk0, rk1, slots, W, logql, logDelta, dimB, dimP, dimpt):
        """he_gemv (src/he-algo.c:47-93) + its he_rs on big slabs: diag = slots plaintext big slabs (index i*n1 + j), rk0 / rk1 = per-rotation
        key slabs (lists indexed by the rotation; unused entries may be None)."""
        torch = _torch()
        batch = c0.numel() // (W * self.n)
        nbytes = self.lib.gpq_he_gemv_workspace_bytes(self.h, W, slots, dimB, dimP, dimpt, batch)
        if not nbytes:
            raise _native.GpqError("gpq_he_gemv_workspace_bytes: " + self.lib.gpq_last_error().decode())
        ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_gemv(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(c0), self._ptr(c1), self._ptr(diag), self._key_ptrs(rk0),
                                           self._key_ptrs(rk1), slots, W, logql, logDelta, dimB, dimP, dimpt, batch, self._ptr(ws), self._stream()), "gpq_he_gemv")
        return ws

    def gemv_plan(self, diag, slots, W, logql, dimpt):
        """A plan for he_gemv with a fixed matrix: diag = slots plaintext big slabs (index i*n1 + j) as he_gemv takes them."""
        return GemvPlan(self, diag, slots, W, logql, dimpt)

    # --- he_ecd on the device (include/gpqhe_hip.h, "he_ecd on the device") ---
    def ecd_plan(self, slots, roots=None, roots_slots=None, block=None):
        """The encoder's tables for `slots` slots: roots = a (4 S + 1) x 2 float64 table for S >= slots slots (None: ecd_roots(slots)).
        block = None: gpq_ecd_plan_create, at most 8192 slots; block = slots per workgroup (0: min(slots, 8192)):
        gpq_ecd_plan_create_split, any power of two up to n/2 and 65536."""
        return EcdPlan(self, slots, roots, roots_slots, block)

    def he_ecd(self, plan, out, z, logDelta=None, W=1, bad=None, Delta=None):
        """he_ecd (src/he-encode.c:107-111) of every vector of z = [count][slots] complex128 (or (re, im) float64 pairs) on the device into
        out = [count][W][n]; `bad` = an int32 device word that counts coefficients without an image (stored as 0), or None."""
        logDelta = log_delta(logDelta, Delta)
        count = z.numel() * (2 if z.is_complex() else 1) // (2 * plan.slots)
        if out.numel() != count * W * self.n:
            raise ValueError("out holds %d words, %d vectors need %d" % (out.numel(), count, count * W * self.n))
        _native.check(self.lib.gpq_he_ecd(self.h, plan.h, self._ptr(out), self._ptr(z), logDelta, W, count,
                                          None if bad is None else self._ptr(bad), self._stream()), "gpq_he_ecd")
        return out

    def he_ecd_diagonals(self, plan, out, A, logDelta=None, W=1, bad=None, Delta=None):
        """out[i n1 + j] = he_ecd(zrotdiag(A, i n1 + j, -i n1)) for the slots x slots row-major complex128 matrix A on the device: the `diag`
        of he_gemv and gemv_plan."""
        logDelta = log_delta(logDelta, Delta)
        if out.numel() != plan.slots * W * self.n:
            raise ValueError("out holds %d words, %d diagonals need %d" % (out.numel(), plan.slots, plan.slots * W * self.n))
        _native.check(self.lib.gpq_he_ecd_diagonals(self.h, plan.h, self._ptr(out), self._ptr(A), logDelta, W,
                                                    None if bad is None else self._ptr(bad), self._stream()), "gpq_he_ecd_diagonals")
        return out

    # --- he_dec and he_dcd on the device (include/gpqhe_hip.h, "he_dec and he_dcd on the device") ---
    def he_dcd(self, plan, z_out, big, nu, W):
        """he_dcd (src/he-encode.c:114-117) of every plaintext of big = [count][W][n] on the device into z_out = [count][slots] complex128
        (or (re, im) float64 pairs); nu = pt->nu, any finite double > 0.  The plan is the encoder's (ecd_plan)."""
        count = big.numel() // (W * self.n)
        have = z_out.numel() * (2 if z_out.is_complex() else 1)
        if have != count * 2 * plan.slots:
            raise ValueError("z_out holds %d doubles, %d plaintexts need %d" % (have, count, count * 2 * plan.slots))
        _native.check(self.lib.gpq_he_dcd(self.h, plan.h, self._ptr(z_out), self._ptr(big), float(nu), W, count, self._stream()), "gpq_he_dcd")
        return z_out

    def he_dec(self, m, c0, c1, sk_ntt, W, logql, dim):
        """he_dec (src/he-encrypt.c:105-125) with q_l = 2^logql on big slabs: m = smod(c1 * sk + c0, q_l) for every ciphertext of the batch;
        sk_ntt = the key as ONE NTT-domain slab [dim][n] (evk_pack of its big slab), shared by the batch."""
        torch = _torch()
        batch = c1.numel() // (W * self.n)
        ws = torch.empty(self.lib.gpq_he_dec_workspace_bytes(self.h, dim, batch) // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_dec(self.h, self._ptr(m), self._ptr(c0), self._ptr(c1), self._ptr(sk_ntt), W, logql, dim, batch,
                                          self._ptr(ws), self._stream()), "gpq_he_dec")
        return m

    # --- samplers and encryption on the device (include/gpqhe_hip.h, "samplers and encryption on the device") ---
    def sample_zo(self, out, bytes_dev):
        """sample_zo (src/sample.c:112-131) of the caller's bytes: bytes_dev = uint8 [count][n/4] on the device (any byte address),
        out = int8 [count][n]."""
        count = out.numel() // self.n
        if bytes_dev.numel() != count * (self.n // 4):
            raise ValueError("%d polynomials need %d bytes, not %d" % (count, count * (self.n // 4), bytes_dev.numel()))
        _native.check(self.lib.gpq_sample_zo(self.h, self._ptr(out), self._ptr(bytes_dev), count, self._stream()), "gpq_sample_zo")
        return out

    def sample_error(self, out, bytes_dev):
        """sample_error (src/sample.c:60-82) of the caller's bytes: bytes_dev = uint8 [count][n], out = int8 [count][n]."""
        count = out.numel() // self.n
        if bytes_dev.numel() != count * self.n:
            raise ValueError("%d polynomials need %d bytes, not %d" % (count, count * self.n, bytes_dev.numel()))
        _native.check(self.lib.gpq_sample_error(self.h, self._ptr(out), self._ptr(bytes_dev), count, self._stream()), "gpq_sample_error")
        return out

    def sample_uniform(self, big, bytes_dev, nbits, W):
        """sample_uniform (src/sample.c:133-141) for a q of nbits bits: bytes_dev = uint8 [count][n][nbits // 8 + 1], big = [count][W][n],
        the RAW values in [0, 2^nbits)."""
        count = big.numel() // (W * self.n)
        if bytes_dev.numel() != count * self.n * (nbits // 8 + 1):
            raise ValueError("%d polynomials need %d bytes, not %d" % (count, count * self.n * (nbits // 8 + 1), bytes_dev.numel()))
        _native.check(self.lib.gpq_sample_uniform(self.h, self._ptr(big), self._ptr(bytes_dev), nbits, W, count, self._stream()), "gpq_sample_uniform")
        return big

    def surf_bytes(self, bytes_dev, pos=0, seed=None):
        """bytes [pos, pos + len) of the reference's deterministic randombytes stream (src/rng.c:36-77) for `seed` (32 words; None: the
        reference's) into bytes_dev, a uint8 tensor on the device at any byte address.  pos: a Python integer below 2^128."""
        _native.check(self.lib.gpq_surf_bytes(self.h, self._ptr(bytes_dev), bytes_dev.numel(), _seed_words(seed), pos & _M64, pos >> 64, self._stream()),
                      "gpq_surf_bytes")
        return bytes_dev

    def small_to_big(self, big, small, W):
        """an int8 small slab [count][n] sign-extended into a big slab [count][W][n]"""
        _native.check(self.lib.gpq_small_to_big(self.h, self._ptr(big), self._ptr(small), W, small.numel() // self.n, self._stream()), "gpq_small_to_big")
        return big

    def he_enc_pk(self, out_c0, out_c1, m, v, e0, e1, pk0_ntt, pk1_ntt, W, logq, dim):
        """he_enc_pk (src/he-encrypt.c:37-73) with q = 2^logq: m = plaintext big slabs (None: none), v / e0 / e1 = int8 small slabs
        (sample_zo, sample_error, sample_error), pk0_ntt / pk1_ntt = the public key as ONE NTT-domain slab pair [dim][n]."""
        torch = _torch()
        batch = v.numel() // self.n
        ws = torch.empty(self.lib.gpq_he_enc_workspace_bytes(self.h, dim, batch, 1) // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_enc_pk(self.h, self._ptr(out_c0), self._ptr(out_c1), None if m is None else self._ptr(m), self._ptr(v), self._ptr(e0),
                                             self._ptr(e1), self._ptr(pk0_ntt), self._ptr(pk1_ntt), W, logq, dim, batch, self._ptr(ws), self._stream()),
                      "gpq_he_enc_pk")
        return out_c0, out_c1

    def he_enc_sk(self, out_c0, out_c1, m, a, e, sk_ntt, W, logq, dim):
        """he_enc_sk (src/he-encrypt.c:75-103) with q = 2^logq: a = the RAW sample_uniform big slabs, e = an int8 small slab, sk_ntt = the
        secret key as he_dec takes it; m = None is he_keypair's pk.p0, pk.p1 (src/he-kem.c:59-65)."""
        torch = _torch()
        batch = e.numel() // self.n
        ws = torch.empty(self.lib.gpq_he_enc_workspace_bytes(self.h, dim, batch, 0) // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_enc_sk(self.h, self._ptr(out_c0), self._ptr(out_c1), None if m is None else self._ptr(m), self._ptr(a), self._ptr(e),
                                             self._ptr(sk_ntt), W, logq, dim, batch, self._ptr(ws), self._stream()), "gpq_he_enc_sk")
        return out_c0, out_c1

    def gemv_plan_from_matrix(self, ecd, A, logDelta=None, logql=None, dimpt=None, Delta=None):
        """A plan for he_gemv straight from the slots x slots complex128 matrix A on the device: the diagonals are encoded there."""
        return GemvPlan.from_matrix(self, ecd, A, log_delta(logDelta, Delta), logql, dimpt)

    def gemv_inner(self, out_c0, out_c1, R0, R1, plan, giant, W):
        """One giant step's inner sum smod(sum_j R_j * diag[giant n1 + j], 2^logql); R0 / R1 = n1 x batch big slabs, rotation-major."""
        torch = _torch()
        batch = out_c0.numel() // (W * self.n)
        nbytes = self.lib.gpq_gemv_inner_workspace_bytes(self.h, plan.h, batch)
        ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_gemv_inner(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(R0), self._ptr(R1), plan.h, giant, W, batch,
                                              self._ptr(ws), self._stream()), "gpq_gemv_inner")
        return ws

    def he_gemv_planned(self, out_c0, out_c1, c0, c1, plan, rk0, rk1, W, logDelta, dimB, dimP, workspace=None):
        """he_gemv + he_rs as `he_gemv` computes them, with the matrix held by `plan`; keys of rotations the plan does not need may be None."""
        torch = _torch()
        batch = c0.numel() // (W * self.n)
        ws = workspace
        if ws is None:
            nbytes = self.lib.gpq_he_gemv_planned_workspace_bytes(self.h, plan.h, W, dimB, dimP, batch)
            if not nbytes:
                raise _native.GpqError("gpq_he_gemv_planned_workspace_bytes: " + self.lib.gpq_last_error().decode())
            ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_gemv_planned(self.h, self._ptr(out_c0), self._ptr(out_c1), self._ptr(c0), self._ptr(c1), plan.h, self._key_ptrs(rk0),
                                                   self._key_ptrs(rk1), W, logDelta, dimB, dimP, batch, self._ptr(ws), self._stream()), "gpq_he_gemv_planned")
        return ws

    def gemv_multi(self, plans):
        """A set of GemvPlans of this context (same slots and logql) that he_gemv_multi applies to the same ciphertexts; it borrows them."""
        return GemvMulti(self, plans)

    def he_gemv_multi(self, outs0, outs1, c0, c1, multi, rk0, rk1, W, logDelta, dimB, dimP, workspace=None):
        """he_gemv_planned for every plan of `multi` on the same ciphertexts, with the baby rotations and their transforms shared: outs0[t] /
        outs1[t] get what he_gemv_planned writes for plan t.  Keys outside multi.rotations() may be None."""
        torch = _torch()
        batch = c0.numel() // (W * self.n)
        if len(outs0) != multi.count or len(outs1) != multi.count:
            raise ValueError("%d plans need %d outputs, not %d and %d" % (multi.count, multi.count, len(outs0), len(outs1)))
        ws = workspace
        if ws is None:
            nbytes = self.lib.gpq_he_gemv_multi_workspace_bytes(self.h, multi.h, W, dimB, dimP, batch)
            if not nbytes:
                raise _native.GpqError("gpq_he_gemv_multi_workspace_bytes: " + self.lib.gpq_last_error().decode())
            ws = torch.empty(nbytes // 8 + 8, dtype=torch.int64, device=self._dev)
        _native.check(self.lib.gpq_he_gemv_multi(self.h, self._key_ptrs(outs0), self._key_ptrs(outs1), self._ptr(c0), self._ptr(c1), multi.h, self._key_ptrs(rk0),
                                                 self._key_ptrs(rk1), W, logDelta, dimB, dimP, batch, self._ptr(ws), self._stream()), "gpq_he_gemv_multi")
        return ws

    def poly_rot(self, r, a, W, rot):
        _native.check(self.lib.gpq_poly_rot(self.h, self._ptr(r), self._ptr(a), W, rot, a.numel() // (W * self.n), self._stream()), "gpq_poly_rot")
        return r

    def poly_conj(self, r, a, W):
        _native.check(self.lib.gpq_poly_conj(self.h, self._ptr(r), self._ptr(a), W, a.numel() // (W * self.n), self._stream()), "gpq_poly_conj")
        return r

    def phat_invmp(self, dim):
        return [self.lib.gpq_ctx_phat_invmp(self.h, dim, d) for d in range(dim)]

    def profile(self, on):
        _native.check(self.lib.gpq_profile_enable(self.h, 1 if on else 0), "gpq_profile_enable")

    def profile_collect(self):
        """{kernel name: (total ms, launches)} of the launches recorded since the last call."""
        k = self.lib.gpq_profile_kernels()
        ms = (C.c_double * k)()
        cnt = (C.c_ulonglong * k)()
        _native.check(self.lib.gpq_profile_collect(self.h, ms, cnt), "gpq_profile_collect")
        return {self.lib.gpq_profile_kernel_name(i).decode(): (ms[i], cnt[i]) for i in range(k) if cnt[i]}

    def _shape(self, slab, dim):
        per = dim * self.n
        if slab.numel() % per:
            raise ValueError("slab of %d words is not a multiple of dim*n = %d" % (slab.numel(), per))
        return slab.numel() // per

    # --- src/ntt.c:37,54 over slabs, in place ---
    def poly_ntt(self, slab, dim):
        _native.check(self.lib.gpq_ntt(self.h, self._ptr(slab), dim, self._shape(slab, dim), self._stream()), "gpq_ntt")
        return slab

    def poly_invntt(self, slab, dim):
        _native.check(self.lib.gpq_invntt(self.h, self._ptr(slab), dim, self._shape(slab, dim), self._stream()), "gpq_invntt")
        return slab

    def poly_ntt_reference(self, slab, dim, inverse=False):
        """src/ntt.c executed as written on the device (any input words): the kernel gpq_ntt redoes flagged limbs with."""
        _native.check(self.lib.gpq_ntt_reference(self.h, self._ptr(slab), dim, self._shape(slab, dim), 1 if inverse else 0, self._stream()), "gpq_ntt_reference")
        return slab

    # --- src/poly.c:71-82 over slabs ---
    def poly_rns_mul(self, r, a, b, dim):
        _native.check(self.lib.gpq_rns_mul(self.h, self._ptr(r), self._ptr(a), self._ptr(b), dim, self._shape(a, dim), self._stream()), "gpq_rns_mul")
        return r

    def poly_rns_add(self, r, a, b, dim):
        _native.check(self.lib.gpq_rns_add(self.h, self._ptr(r), self._ptr(a), self._ptr(b), dim, self._shape(a, dim), self._stream()), "gpq_rns_add")
        return r

    # --- limb loop of poly_mul, src/poly.c:96-103 ---
    def poly_mul_rns(self, r, a, b, dim):
        _native.check(self.lib.gpq_poly_mul_rns(self.h, self._ptr(r), self._ptr(a), self._ptr(b), dim, self._shape(a, dim), self._stream()),
                      "gpq_poly_mul_rns")
        return r

    def mulpt_rns(self, r0, r1, m, x0, x1, dim):
        _native.check(self.lib.gpq_mulpt_rns(self.h, self._ptr(r0), self._ptr(r1), self._ptr(m), self._ptr(x0), self._ptr(x1), dim, self._shape(m, dim), self._stream()),
                      "gpq_mulpt_rns")
        return r0, r1

    # --- he_mul RNS core ---
    def tensor_workspace(self, dim, batch):
        torch = _torch()
        nbytes = self.lib.gpq_tensor_workspace_bytes(self.h, dim, batch)
        return torch.empty(nbytes // 8, dtype=torch.int64, device=self._dev)

    def keyswitch_workspace(self, dim, batch):
        torch = _torch()
        nbytes = self.lib.gpq_keyswitch_workspace_bytes(self.h, dim, batch)
        return torch.empty(nbytes // 8, dtype=torch.int64, device=self._dev)

    def he_mul_tensor(self, d0, d1, d2, a0, a1, b0, b1, dim, workspace=None):
        """src/he-mult.c:116-138 on decomposed inputs: d0=a0*b0, d1=a0*b1+a1*b0, d2=a1*b1."""
        batch = self._shape(a0, dim)
        ws = workspace if workspace is not None else self.tensor_workspace(dim, batch)
        _native.check(self.lib.gpq_he_mul_tensor(self.h, self._ptr(d0), self._ptr(d1), self._ptr(d2), self._ptr(a0), self._ptr(a1), self._ptr(b0), self._ptr(b1),
                                                 dim, batch, self._ptr(ws), self._stream()), "gpq_he_mul_tensor")
        return d0, d1, d2

    def he_keyswitch(self, c0, c1, x, evk0, evk1, dim, workspace=None):
        """src/he-mult.c:58-66 / src/he-automorphism.c:59-67 on a decomposed input."""
        batch = self._shape(x, dim)
        ws = workspace if workspace is not None else self.keyswitch_workspace(dim, batch)
        _native.check(self.lib.gpq_keyswitch(self.h, self._ptr(c0), self._ptr(c1), self._ptr(x), self._ptr(evk0), self._ptr(evk1),
                                             dim, batch, self._ptr(ws), self._stream()), "gpq_keyswitch")
        return c0, c1


class GemvMulti:
    """gpq_gemv_multi: a set of GemvPlans applied to the same ciphertexts by Context.he_gemv_multi.  `.count` plans, `.baby` rotations in the
    union of their live baby steps, `.dim` the largest of their dims, `.bytes` of index tables on the device.  The set borrows the plans
    (it keeps them referenced); `close()` (or leaving a `with` block) frees its tables."""

    def __init__(self, ctx, plans):
        self.lib, self.h, self.plans = ctx.lib, C.c_void_p(), list(plans)
        self.slots = self.plans[0].slots if self.plans else 0
        ptrs = (C.c_void_p * max(len(self.plans), 1))(*[p.h.value for p in self.plans])
        _native.check(self.lib.gpq_gemv_multi_create(ctx.h, C.byref(self.h), ptrs, len(self.plans), ctx._stream()), "gpq_gemv_multi_create")
        count, baby, dim, nbytes = C.c_uint(), C.c_uint(), C.c_uint(), C.c_size_t()
        _native.check(self.lib.gpq_gemv_multi_info(self.h, C.byref(count), C.byref(baby), C.byref(dim), C.byref(nbytes)), "gpq_gemv_multi_info")
        self.count, self.baby, self.dim, self.bytes = count.value, baby.value, dim.value, nbytes.value

    def rotations(self):
        """needed[r] for every rotation r < slots whose key he_gemv_multi reads: the union over the plans"""
        needed = (C.c_ubyte * self.slots)()
        _native.check(self.lib.gpq_gemv_multi_rotations(self.h, needed), "gpq_gemv_multi_rotations")
        return [int(v) for v in needed]

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpq_gemv_multi_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class GemvPlan:
    """gpq_gemv_plan: the diagonals of a fixed matrix, decomposed and forward-transformed once.  `.dim` limbs of the inner sum, `.bytes` held
    on the device, `.live` non-zero diagonals, `.exact` False when the plan cannot reproduce he_gemv (the calls then refuse it).  `close()`
    (or leaving a `with` block) frees the device memory at once."""

    def __init__(self, ctx, diag, slots, W, logql, dimpt):
        self.lib, self.h = ctx.lib, C.c_void_p()
        _native.check(self.lib.gpq_gemv_plan_create(ctx.h, C.byref(self.h), ctx._ptr(diag), slots, W, logql, dimpt, ctx._stream()), "gpq_gemv_plan_create")
        self._describe(slots, logql, dimpt)

    @classmethod
    def from_matrix(cls, ctx, ecd, A, logDelta, logql, dimpt):
        """gpq_gemv_plan_create_from_matrix: the diagonals of the device matrix A, encoded on the device with the EcdPlan `ecd`"""
        self = cls.__new__(cls)
        self.lib, self.h = ctx.lib, C.c_void_p()
        _native.check(self.lib.gpq_gemv_plan_create_from_matrix(ctx.h, C.byref(self.h), ecd.h, ctx._ptr(A), logDelta, logql, dimpt, ctx._stream()),
                      "gpq_gemv_plan_create_from_matrix")
        self._describe(ecd.slots, logql, dimpt)
        return self

    def _describe(self, slots, logql, dimpt):
        dim, nbytes, live, exact = C.c_uint(), C.c_size_t(), C.c_uint(), C.c_int()
        _native.check(self.lib.gpq_gemv_plan_info(self.h, C.byref(dim), C.byref(nbytes), C.byref(live), C.byref(exact)), "gpq_gemv_plan_info")
        self.dim, self.bytes, self.live, self.exact = dim.value, nbytes.value, live.value, bool(exact.value)
        self.diag_bits = int(self.lib.gpq_gemv_plan_diag_bits(self.h))
        self.slots, self.logql, self.dimpt = slots, logql, dimpt

    def rotations(self):
        """needed[r] for every rotation r < slots whose key he_gemv_planned reads"""
        needed = (C.c_ubyte * self.slots)()
        _native.check(self.lib.gpq_gemv_plan_rotations(self.h, needed), "gpq_gemv_plan_rotations")
        return [int(v) for v in needed]

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpq_gemv_plan_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class EcdPlan:
    """gpq_ecd_plan: the root table and the powers of 5 the encoder reads for `slots` slots, on the device.  `roots` = a (4 S + 1) x 2
    float64 array for S = roots_slots >= slots slots (S is taken from the array's length when not given); None = ecd_roots(slots).
    block = None: at most 8192 slots, one workgroup per vector.  block = slots per workgroup (0: min(slots, 8192)): gpq_ecd_plan_create_split,
    slots = any power of two up to n/2 and 65536, a vector of more slots than `block` split over workgroups (include/gpqhe_hip.h)."""

    def __init__(self, ctx, slots, roots=None, roots_slots=None, block=None):
        self.lib, self.h, self.slots = ctx.lib, C.c_void_p(), slots
        if roots is not None:
            roots = np.ascontiguousarray(roots, dtype=np.float64).reshape(-1, 2)
            roots_slots = roots_slots or (roots.shape[0] - 1) // 4
            if roots.shape[0] != 4 * roots_slots + 1:
                raise ValueError("a root table for %d slots has %d rows, not %d" % (roots_slots, 4 * roots_slots + 1, roots.shape[0]))
        table = None if roots is None else roots.ctypes.data_as(C.c_void_p)
        if block is None:
            _native.check(self.lib.gpq_ecd_plan_create(ctx.h, C.byref(self.h), slots, table, roots_slots or 0), "gpq_ecd_plan_create")
        else:
            _native.check(self.lib.gpq_ecd_plan_create_split(ctx.h, C.byref(self.h), slots, block, table, roots_slots or 0), "gpq_ecd_plan_create_split")

    def set_block(self, block_slots=0):
        """gpq_ecd_plan_set_block: slots per workgroup for he_ecd and he_dcd on this plan (0: the default, min(slots, 8192)); a power of
        two in 2..min(slots, 8192) with slots / block_slots <= 8.  The words never depend on it."""
        _native.check(self.lib.gpq_ecd_plan_set_block(self.h, block_slots), "gpq_ecd_plan_set_block")
        return self

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpq_ecd_plan_destroy(self.h)
            self.h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def ecd_roots(slots):
    """(4 slots + 1) x 2 float64: T[t] = (cos, sin)(2 PI t / (4 slots)) by the C library's sincos (include/gpqhe_hip.h: gpq_ecd_roots).  No device."""
    table = np.empty((4 * slots + 1, 2), dtype=np.float64)
    _native.check(_native.load().gpq_ecd_roots(table.ctypes.data_as(C.c_void_p), slots), "gpq_ecd_roots")
    return table


_M64 = (1 << 64) - 1


def _seed_words(seed):
    if seed is None:
        return None
    words = np.ascontiguousarray(seed, dtype=np.uint32)
    if words.shape != (32,):
        raise ValueError("a seed is 32 words of 32 bits")
    return words.ctypes.data_as(C.c_void_p)


def surf_bytes_host(length, pos=0, seed=None):
    """bytes [pos, pos + length) of the reference's deterministic randombytes stream on the CPU (gpq_surf_bytes_host): no device needed"""
    out = np.empty(length, dtype=np.uint8)
    _native.check(_native.load().gpq_surf_bytes_host(out.ctypes.data_as(C.c_void_p), length, _seed_words(seed), pos & _M64, pos >> 64), "gpq_surf_bytes_host")
    return out


class Rng:
    """gpq_rng: one stream of the reference's deterministic randombytes with a position; host and device draws advance it alike."""

    def __init__(self, seed=None, pos=0):
        self.lib = _native.load()
        h = C.c_void_p()
        _native.check(self.lib.gpq_rng_create(C.byref(h), _seed_words(seed)), "gpq_rng_create")
        self.h = h
        if pos:
            self.seek(pos)

    def seek(self, pos):
        _native.check(self.lib.gpq_rng_seek(self.h, pos & _M64, pos >> 64), "gpq_rng_seek")

    def tell(self):
        pos = (C.c_uint64 * 2)()
        _native.check(self.lib.gpq_rng_tell(self.h, pos), "gpq_rng_tell")
        return int(pos[0]) | (int(pos[1]) << 64)

    def host_bytes(self, length):
        out = np.empty(length, dtype=np.uint8)
        _native.check(self.lib.gpq_rng_host_bytes(self.h, out.ctypes.data_as(C.c_void_p), length), "gpq_rng_host_bytes")
        return out

    def device_bytes(self, ctx, bytes_dev):
        """the next bytes_dev.numel() bytes into a uint8 tensor on ctx's device, on the current stream"""
        _native.check(self.lib.gpq_rng_device_bytes(ctx.h, self.h, ctx._ptr(bytes_dev), bytes_dev.numel(), ctx._stream()), "gpq_rng_device_bytes")
        return bytes_dev

    def close(self):
        if getattr(self, "h", None):
            self.lib.gpq_rng_destroy(self.h)
            self.h = None

    __del__ = close


def sample_error_table():
    """65536 x 2 int8: T[b0][b1] of sample_error's byte pairs, (0, 0) for b1 = 0 (include/gpqhe_hip.h: gpq_sample_error_table).  No device."""
    table = np.empty((65536, 2), dtype=np.int8)
    _native.check(_native.load().gpq_sample_error_table(table.ctypes.data_as(C.c_void_p)), "gpq_sample_error_table")
    return table


def log_delta(logDelta=None, Delta=None):
    """the logDelta the device encoder takes: Delta must be a power of two >= 2 (any other needs the reference's x87 product and is refused)"""
    if Delta is None:
        if logDelta is None:
            raise ValueError("logDelta or Delta")
        return int(logDelta)
    m, e = np.frexp(float(Delta))
    if m != 0.5 or e < 2 or (logDelta is not None and int(logDelta) != e - 1):
        raise _native.GpqError("he_ecd on the device: Delta = %r is not a power of two (GPQ_ERR_INVALID)" % (Delta,))
    return int(e) - 1


def gemv_acc_dim(logql, diag_bits, logn, n1):
    """limbs the accumulated inner sum of a planned he_gemv needs to be exact (include/gpqhe_hip.h: gpq_gemv_acc_dim).  No device."""
    return int(_native.load().gpq_gemv_acc_dim(logql, diag_bits, logn, n1))


def automorphism_index(logn, g):
    """sigma of X -> X^g in the NTT domain (include/gpqhe_hip.h: gpq_automorphism_index): NTT(a o X^g)[j] = NTT(a)[idx[j]].  No device."""
    lib = _native.load()
    idx = np.empty(1 << logn, dtype=np.uint32)
    _native.check(lib.gpq_automorphism_index(logn, g, idx.ctypes.data_as(C.c_void_p)), "gpq_automorphism_index")
    return idx


def gemv_multi_width():
    """plans that share one gemv_mac_multi launch in he_gemv_multi (include/gpqhe_hip.h: gpq_gemv_multi_width).  No device."""
    return int(_native.load().gpq_gemv_multi_width())


def gemv_steps(slots):
    """(n1, n2) of he_gemv, src/he-algo.c:51-54"""
    import math
    n1 = int(math.sqrt(slots))
    if slots != n1 * n1:
        n1 = int(math.sqrt(2 * slots))
    return n1, slots // n1


def ints_to_big(values, W):
    """Python ints (signed) -> numpy uint64 big slab [W][n], two's complement."""
    n = len(values)
    out = np.empty((W, n), dtype=np.uint64)
    mod = 1 << (64 * W)
    for i, v in enumerate(values):
        v = int(v) % mod
        for j in range(W):
            out[j, i] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return out.reshape(-1)


def big_to_ints(big, W, n):
    """numpy uint64 big slab(s) [..][W][n] -> list of signed Python ints per polynomial."""
    arr = np.asarray(big, dtype=np.uint64).reshape(-1, W, n)
    res = []
    for poly in arr:
        vals = []
        for i in range(n):
            v = 0
            for j in range(W):
                v |= int(poly[j, i]) << (64 * j)
            if v >> (64 * W - 1):
                v -= 1 << (64 * W)
            vals.append(v)
        res.append(vals)
    return res


class StreamTimer:
    """HIP-event timer on the stream the kernels are launched on."""

    def __init__(self):
        self.lib = _native.load()
        self.h = C.c_void_p()
        _native.check(self.lib.gpq_timer_create(C.byref(self.h)), "gpq_timer_create")

    def start(self):
        _native.check(self.lib.gpq_timer_start(self.h, _stream()), "gpq_timer_start")

    def stop(self):
        _native.check(self.lib.gpq_timer_stop(self.h, _stream()), "gpq_timer_stop")

    def elapsed_ms(self):
        ms = C.c_float()
        _native.check(self.lib.gpq_timer_elapsed_ms(self.h, C.byref(ms)), "gpq_timer_elapsed_ms")
        return ms.value

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.gpq_timer_destroy(self.h)
            self.h = None
