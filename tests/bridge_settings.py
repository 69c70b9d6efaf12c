"""The switches of the library that are documented as "same words", once: the table the settings tests iterate over
(tests/test_settings_derived_gpu.py, tests/test_settings_bridge_calls_gpu.py), contexts that carry one setting each, and the guarded
buffers those tests hand to the C entry points.  A plain module: nothing here is collected.

A setting is applied to a context of its own (setting_context); the session-cached engine_ctx contexts never see a non-default one.
Every such context runs with gpq_set_chunk(2): a batch of 3 is two launch groups with an odd last one, which runs the single-polynomial
instantiations of the key-switch kernels.

tests/test_bridge_settings_cover.py (no device) reads include/gpqhe_hip.h and fails when a switch is neither used by an entry of SETTINGS nor
listed, with a reason, in NOT_A_WORD_SETTING."""
import contextlib

CHUNK = 2

# name -> (apply(g), tags).  tags: "bridge" = the bridge-only calls (he_mulpt, poly_mul, he_dec, he_enc_*, he_genswk*, gemv plans) run under
# the entry too.  For the matrix-core decompose, the exact CRT, the limb block and the limb classes that is because launch_decompose /
# launch_reconstruct and the transforms read them.  "stream bridge off" and the forced redos carry the tag as a CONTROL: only the streaming
# kernels read them (crt_decompose_stream of gpq_he_mul, tail_stream, relin_tail), none of which a bridge-only call reaches, so those calls
# must not notice them.  "tail" = the entry (also) re-routes the key switch or the relinearisation tail, which only the key-switching calls
# have.  tests/test_bridge_settings_cover.py pins every entry's name, switches and tags: an entry cannot leave or change unnoticed.
SETTINGS = {
    "default": (lambda g: None, ("bridge", "tail")),
    "stream bridge off": (lambda g: g.set_stream_bridge(False), ("bridge", "tail")),
    "prescale 2": (lambda g: g.set_prescale(2), ("tail",)),
    "prescale 1": (lambda g: g.set_prescale(1), ("tail",)),
    "prescale 0": (lambda g: g.set_prescale(0), ("tail",)),
    "integer-VALU decompose": (lambda g: g.set_bridge_mfma(False), ("bridge", "tail")),
    "exact CRT": (lambda g: g.set_exact_crt(True), ("bridge", "tail")),
    "canonical decompose": (lambda g: g.set_lazy_decompose(False), ("tail",)),
    "force redo 1": (lambda g: g.debug_force_redo(1), ("bridge", "tail")),      # every coefficient through the exact kernels
    "force redo 7": (lambda g: g.debug_force_redo(7), ("bridge", "tail")),
    "nt always": (lambda g: g.set_nt_policy(1), ("tail",)),
    "general butterflies": (lambda g: g.set_limb_classes(0, 0), ("bridge", "tail")),
    "limb block 2": (lambda g: g.set_limb_block(2), ("bridge", "tail")),
    "two lanes": (lambda g: g.set_overlap(1), ("tail",)),
    "stream bridge off + prescale 0 + exact CRT": (lambda g: (g.set_stream_bridge(False), g.set_prescale(0), g.set_exact_crt(True)), ("tail",)),
    "integer-VALU decompose + force redo 3": (lambda g: (g.set_bridge_mfma(False), g.debug_force_redo(3)), ("bridge", "tail")),
    "prescale 2 + canonical decompose + limb block 2": (lambda g: (g.set_prescale(2), g.set_lazy_decompose(False), g.set_limb_block(2)), ("tail",)),
}

# what every context of setting_context gets besides its setting
ALWAYS = {"gpq_set_chunk": "setting_context: every context runs in launch groups of CHUNK"}

# int gpq_set_*(...) of include/gpqhe_hip.h that are not switches between kernels computing the same words
NOT_A_WORD_SETTING = {
    "gpq_set_device": "the calling thread's current device, not a property of a context",
}


def tagged(tag):
    """the names of SETTINGS that carry `tag`, in the table's order"""
    return [name for name, (_, tags) in SETTINGS.items() if tag in tags]


class Recorder:
    """stands in for a PolyContext where no device is: records the C name behind every method an apply() calls"""

    def __init__(self):
        self.called, self.calls = [], []             # the C names; (method, arguments) as the entry wrote them

    def __getattr__(self, name):
        def record(*args):
            self.called.append("gpq_" + name)
            self.calls.append((name,) + args)
        return record


def switches_used():
    """{C name: [settings that call it]} over SETTINGS, plus ALWAYS"""
    used = {name: ["(every context)"] for name in ALWAYS}
    for setting, (apply, _) in SETTINGS.items():
        r = Recorder()
        apply(r)
        for name in r.called:
            used.setdefault(name, []).append(setting)
    return used


@contextlib.contextmanager
def setting_context(logn, nprimes, setting="default"):
    """a PolyContext of its own under SETTINGS[setting], closed afterwards"""
    import torch
    import gpqhe_amd
    g = gpqhe_amd.PolyContext(logn, nprimes)
    try:
        g.set_chunk(CHUNK)
        SETTINGS[setting][0](g)
        yield g
    finally:
        torch.cuda.synchronize()
        g.close()


class Cells:
    """contexts by (key, setting), made on first use and closed together: one per cell of a test module, shared by that cell's calls"""

    def __init__(self):
        self.stack, self.ctx = contextlib.ExitStack(), {}

    def get(self, logn, nprimes, setting):
        key = (logn, nprimes, setting)
        if key not in self.ctx:
            self.ctx[key] = self.stack.enter_context(setting_context(logn, nprimes, setting))
        return self.ctx[key]

    def close(self):
        self.stack.close()
        self.ctx.clear()


# ---------------------------------------------------------------------------
# buffers of exactly the reported size between two bands of poison
# ---------------------------------------------------------------------------
GUARD_BYTES = 64 * 1024
POISON = 0x5A5AC3C35A5AC3C3


class Guarded:
    """`nbytes` (rounded up to 8) of device memory, 64-byte aligned, with GUARD_BYTES of POISON words in front and behind, all inside ONE
    allocation: a kernel that writes past either end of what it was given changes a guard word instead of a neighbouring allocation.
    The body starts as poison too, so an entry point that refuses its arguments can be shown to have written nothing."""

    def __init__(self, nbytes, device="cuda"):
        import torch
        self.words = (nbytes + 7) // 8
        g = GUARD_BYTES // 8
        self.buf = torch.full((2 * g + self.words + 8,), POISON, dtype=torch.int64, device=device)
        self.start = ((-self.buf.data_ptr()) % 64) // 8 + g
        self.t = self.buf[self.start:self.start + self.words]
        assert self.t.data_ptr() % 64 == 0

    def guards_intact(self):
        lo, hi = self.buf[:self.start], self.buf[self.start + self.words:]
        return bool((lo == POISON).all()) and bool((hi == POISON).all())

    def untouched(self):
        return bool((self.t == POISON).all())


def assert_guards(bufs, what):
    """after torch.cuda.synchronize(): every guard word of every buffer still holds the poison"""
    for name, b in bufs.items():
        assert b.guards_intact(), "%s: a guard word next to `%s` (%d bytes) was overwritten" % (what, name, 8 * b.words)
