"""gpqhe_amd -- MI355X-native engine for GPQHE's RNS/NTT hot path.

The product is libgpqhe_hip.so (hand-written HIP for gfx950 behind the C ABI
of include/gpqhe_hip.h); this package is the thin host-side mirror of the
reference's interface used by the tests and the benchmark.
"""
from ._native import GpqError, LIB_PATH, load  # noqa: F401
from .engine import EcdPlan, GemvMulti, GemvPlan, PolyContext, Rng, surf_bytes_host, ecd_roots, sample_error_table, StreamTimer, gemv_acc_dim, gemv_multi_width, automorphism_index, big_to_ints, gemv_steps, ints_to_big, to_device, to_host  # noqa: F401
