"""The inline device primitives of gpqhe_amd/csrc/modarith.hpp -- and gs_last / TwTraits / ref_fqmul of ntt_kernels.hpp, horner59 of
bridge_kernels.hpp -- run on the device one call per lane (libgpqhe_modprobe.so, built from the product's own headers) and pinned to
Python integers at the edges of their lazy ranges.

tests/test_lazy_ranges.py and tests/test_inject_ranges.py prove the algebra on a restatement in Python; the parity tests run whole
transforms from canonical words, where an intermediate at 6p - 1, 8p - 1, 2^62 + 2^31 - 2, a zero tl or a full low column is a
2^-30 event per word.  This module runs the HIP text itself there.  For every op of the probe one row of tests/modarith_cases.py
gives domain -> post-condition, quoted from the headers:

  multiplies, butterflies, horner59   every output == the exact integer (a*w, x +- y*w, (x +- y)*w, r 2^59 + d) mod p AND inside the
                                      range the header promises, so that the next stage's input is legal
  canonicalising ops                  canon4 / canon8 / canon_fold, gs_last x 3, mulmod_canon*, addmod_canon, ref_fqmul and the canon_*
                                      members equal the residue in [0, p) exactly
  conditional subtractions            csubN == x - m [x >= m] exactly, on both sides of m

The checks are on the device output alone -- congruence and an integer bound, never a comparison with a Python model of the
algorithm -- so another correct formulation of a primitive passes.  No tolerance anywhere.

Moduli: the first and last prime of the chains for logn 7, 13 and 17 (the last of logn 17's 45 limbs has the largest real c) and the
class limits c = 257, GPQ_WIDE_CMAX - 1, GPQ_SPLIT_CMAX - 1, GPQ_FOLD_CMAX - 1 (parsed out of the header; not prime, and they need
not be: the identities hold for any odd modulus 2^59 + c), each for the ops whose class admits its c.  Operands: the cross product
of the directed multiplicands and multipliers of tests/modarith_cases.py, the constructed pairs (chosen xh, tl = 0 / 1 / 2^59 - 1,
xl = 0 / 2^59 - 1), and 2^13 seeded uniform tuples over the domain.  Wide ops run only pairs that split_entry_fits_wide accepts."""
import ctypes as C

import numpy as np
import pytest

from tests import modarith_cases as mc

pytestmark = pytest.mark.gpu
u64p = C.POINTER(C.c_uint64)


@pytest.fixture(scope="module")
def probe():
    try:
        import torch  # noqa: F401  (one HIP runtime for the whole process, as gpqhe_amd._native.load)
    except ImportError:
        pass
    lib = C.CDLL(mc.PROBE_PATH)
    lib.gpq_modprobe_nops.restype = C.c_int
    lib.gpq_modprobe_op_name.restype = C.c_char_p
    lib.gpq_modprobe_op_name.argtypes = [C.c_int]
    lib.gpq_modprobe_run.restype = C.c_int
    lib.gpq_modprobe_run.argtypes = [C.c_int, C.c_uint64] + [u64p] * 6 + [C.c_size_t]
    lib.op_index = {lib.gpq_modprobe_op_name(i).decode(): i for i in range(lib.gpq_modprobe_nops())}
    return lib


def run_on_device(lib, row, mod, t):
    """one probe call for the whole case; returns one list of Python integers per result"""
    n = len(t)
    arrs = [np.array(v, dtype=np.uint64) for v in (t.x, t.y, t.w0, t.w1)]
    outs = [np.full(n, 0xDEADBEEFDEADBEEF, dtype=np.uint64) for _ in range(2)]
    rc = lib.gpq_modprobe_run(lib.op_index[row.op], mod.p, *[a.ctypes.data_as(u64p) for a in arrs + outs], n)
    assert rc == 0, "gpq_modprobe_run(%s) returned HIP error %d" % (row.op, rc)
    return [o.tolist() for o in outs[:row.results]]


@pytest.mark.parametrize("row,mod", mc.cases(), ids=lambda v: repr(v).replace(" ", ""))
def test_primitive_keeps_its_post_condition_on_the_device(probe, row, mod):
    t = row.tuples(mod)
    assert t.ndirected > 0 and len(t) == t.ndirected + mc.NRANDOM
    outs = run_on_device(probe, row, mod, t)
    bad = row.violations(mod, t, outs)
    if bad:
        directed = sum(i < t.ndirected for i in bad)
        lines = ["%s mod %s (p = 2^59 + %d): %d of %d tuples break `%s` (%d directed, %d random); first:"
                 % (row.name, mod.label, mod.c, len(bad), len(t), row.quote, directed, len(bad) - directed)]
        for i in bad[:6]:
            lines.append("  #%d %r -> %r, bounds %r" % (i, t.at(i), [o[i] for o in outs], [row.bounds(mod, j) for j in range(row.results)]))
        pytest.fail("\n".join(lines))
