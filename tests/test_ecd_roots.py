"""gpq_ecd_roots (host only): the root table the device encoder reads when the caller supplies none is the C library's sincos table --
what the reference's ring_init holds once gcc has merged its cos and sin calls (src/precomp.c:306-309) -- and a table for S slots serves
every power of two below S by stride.  No GPU."""
import numpy as np
import pytest

import gpqhe_amd
from gpqhe_amd import engine
from tests import ecd_model


@pytest.mark.parametrize("slots", [1, 2, 64, 512, 8192])
def test_table_is_the_c_librarys_sincos(slots):
    T = gpqhe_amd.ecd_roots(slots)
    assert T.shape == (4 * slots + 1, 2)
    assert np.array_equal(T, ecd_model.roots_via_sincos(slots))
    assert np.array_equal(T[0], [1.0, 0.0]) and np.array_equal(T[4 * slots], T[0])


def test_a_larger_table_serves_smaller_slot_counts_by_stride():
    T = gpqhe_amd.ecd_roots(8192)
    for slots in (1, 4, 128, 4096):
        assert np.array_equal(T[::8192 // slots], gpqhe_amd.ecd_roots(slots))


def test_bad_arguments():
    lib = gpqhe_amd.load()
    buf = np.zeros(64)
    assert lib.gpq_ecd_roots(buf.ctypes.data, 3) == -1 and lib.gpq_ecd_roots(buf.ctypes.data, 0) == -1 and lib.gpq_ecd_roots(None, 4) == -1
    assert not buf.any()
    assert engine.log_delta(Delta=2.0 ** 30) == 30 and engine.log_delta(logDelta=20) == 20 and engine.log_delta(Delta=1 << 50) == 50
    for delta in (3.0, 2.0 ** 30 + 1, 1e9, 0.5, 1.0):
        with pytest.raises(gpqhe_amd.GpqError):
            engine.log_delta(Delta=delta)
