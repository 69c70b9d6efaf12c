"""What tests/test_modarith_device_gpu.py rests on, checked without a device: the probe library covers every inline device function of
modarith.hpp (a primitive added later fails here until it is probed), every op has a row in tests/modarith_cases.py with directed
operands for every modulus its class admits, and the generator itself stays inside the domains and -- through the integer models of
the primitives -- inside the bounds the rows quote from the headers.  Loading the probe needs no device."""
import ctypes as C
import os
import re

import pytest

from tests import modarith_cases as mc


@pytest.fixture(scope="module")
def op_names():
    lib = C.CDLL(mc.PROBE_PATH)
    lib.gpq_modprobe_op_name.restype = C.c_char_p
    lib.gpq_modprobe_op_name.argtypes = [C.c_int]
    names = [lib.gpq_modprobe_op_name(i).decode() for i in range(lib.gpq_modprobe_nops())]
    assert lib.gpq_modprobe_op_name(-1) is None and lib.gpq_modprobe_op_name(len(names)) is None
    return names


def device_functions(header):
    with open(os.path.join(mc.CSRC, header)) as f:
        return re.findall(r"__device__\s+(?:static\s+)?__forceinline__\s+[\w:<> ]+?[\s&*](\w+)\s*\(", f.read())


def test_every_device_function_of_the_headers_is_probed_or_a_listed_helper(op_names):
    found = device_functions("modarith.hpp")
    assert len(found) >= 25 and {"mulmod_raw_t", "mulmod_split", "ct_bfly_wide", "canon_fold", "csub_by", "not_low27"} <= set(found)
    assert {"gs_last", "ref_fqmul", "slab_ld"} <= set(device_functions("ntt_kernels.hpp")) and "horner59" in device_functions("bridge_kernels.hpp")
    for name in sorted(set(found) | {"gs_last", "ref_fqmul", "horner59"}):
        if name in mc.HELPERS:
            assert name not in op_names and name not in mc.PROBED_AS, name
            continue
        wanted = mc.PROBED_AS.get(name, [name])
        assert set(wanted) <= set(op_names), "%s: no probe op (add one to modarith_probe.hip and a row to tests/modarith_cases.py, or list it in HELPERS with the reason)" % name
    assert set(mc.HELPERS) <= set(found)
    # the members of the three TwTraits: an op for each one that is not the identity
    with open(os.path.join(mc.CSRC, "ntt_kernels.hpp")) as f:
        text = f.read()
    for tw in ("uint64_t", "TwS", "TwW"):
        body = text[text.index("template <> struct TwTraits<%s> {" % tw):]
        body = body[:body.index("\n};")]
        members = re.findall(r"__forceinline__ uint64_t (\w+)\(uint64_t x, const PrimeK &(k?)\) \{ return ([^;]+); \}", body)
        assert sorted(m[0] for m in members) == ["canon_fwd", "canon_inv", "inv_from4", "inv_from8", "left", "right"], (tw, members)
        for member, uses_k, expr in members:
            assert (expr == "x") == (not uses_k)
            assert (("TwTraits<%s>::%s" % (tw, member)) in op_names) == (expr != "x"), (tw, member, expr)


def test_ops_and_rows_match(op_names):
    assert len(set(op_names)) == len(op_names)
    assert {r.op for r in mc.ROWS} == set(op_names)
    assert len({r.name for r in mc.ROWS}) == len(mc.ROWS)
    for r in mc.ROWS:
        assert r.quote and r.klass in mc.CLASS_CMAX and r.results in (1, 2)
    assert mc.WIDE_CMAX <= mc.SPLIT_CMAX <= mc.FOLD_CMAX
    labels = [m.label for m in mc.moduli()]
    assert len(labels) == len(set(labels)) and sum(bool(m.table) for m in mc.moduli()) >= 5
    assert max(m.c for m in mc.moduli() if m.table) == 222822401              # the last of logn 17's 45 limbs
    for klass, cmax in mc.CLASS_CMAX.items():
        assert any(m.c == cmax - 1 and m.admits(klass) for m in mc.moduli()) and not any(m.c >= cmax and m.admits(klass) for m in mc.moduli())


@pytest.mark.parametrize("row", mc.ROWS, ids=lambda r: r.name.replace(" ", ""))
def test_generated_operands_stay_in_the_domain_and_the_model_inside_the_bounds(row):
    """For every tuple of every modulus the row admits: it lies in the row's domain, and the integer model of the primitive (every
    register bound asserted on the way) satisfies the row's post-condition -- so the reference alone passes the device test."""
    mods = [m for m in mc.moduli() if m.admits(row.klass)]
    assert mods
    for mod in mods:
        t = row.tuples(mod)
        assert t.ndirected > 0 and len(t) == t.ndirected + mc.NRANDOM
        p = mod.p
        assert all(row.in_domain(mod, t, i) for i in range(len(t)))
        model = [row.model(p, x, y, w0, w1) for x, y, w0, w1 in zip(t.x, t.y, t.w0, t.w1)]
        outs = [[m[j] for m in model] for j in range(row.results)]
        assert all(0 <= v <= mc.M64 for o in outs for v in o)
        bad = row.violations(mod, t, outs)
        assert not bad, (mod, t.at(bad[0]), model[bad[0]])


def test_directed_sets_reach_the_edges_they_are_for():
    """The constructed pairs hit the xh, tl and xl they aim at; the cross products contain the top multiplicand against the pair
    that maximises al*X + ah*Y (w = 1, or the last member of the q 2^28 + j family that the table check lets through)."""
    for mod in mc.moduli():
        p, c = mod.p, mod.c
        tls = set()
        for a, w in mc.constructed_mul7(mod, 8 * p - 1):
            x = a * w + c + 1
            tls.add(c * (x >> 59) % mc.B59)
            tls.add(("xl", x % mc.B59))
        assert {0, 1, mc.M59, ("xl", 0), ("xl", mc.M59)} <= tls
        if mod.admits("split"):
            assert {mc.split_fold(a, *mc.pair_of(p, w), p)[1] for a, w in mc.constructed_split(mod)} == {0, 1, mc.M59}
            row = next(r for r in mc.ROWS if r.name == "mulmod_split<TwS>")
            t = row.tuples(mod)
            seen = set(zip(t.x[:t.ndirected], t.w[:t.ndirected]))
            top = 6 * p - 1
            assert (top, 1) in seen and (((((top >> 31) - 1) << 31) | 0x7FFFFFFF), 1) in seen
        if mod.admits("wide"):
            row = next(r for r in mc.ROWS if r.name == "mulmod_split<TwW>")
            t = row.tuples(mod)
            seen = set(zip(t.x[:t.ndirected], t.w[:t.ndirected]))
            best = max((w for w in set(t.w[:t.ndirected])), key=lambda w: max(mc.split_fold(a, *mc.pair_of(p, w), p)[0] for a in mc.wide_extremal_multiplicands(p)))
            assert all((a, best) in seen for a in mc.wide_extremal_multiplicands(p))
            assert max(mc.split_fold(a, *mc.pair_of(p, best), p)[0] for a in mc.wide_extremal_multiplicands(p)) >= (1 << 32) - (1 << 24)


def test_wide_table_check_is_exact_on_the_pairs_the_probe_runs():
    """Wide ops run only pairs that split_entry_fits_wide accepts.  The library's predicate (what upload_tables runs) agrees with the
    restated one on every pair; a rejected pair does overflow -- th >= 2^32 at one of the two extremal multiplicands -- and an accepted
    one does not, so the predicate is exact, not merely safe; every rejected w is below 2^34 and is 1, 2 or of the family q 2^28 + j;
    no entry of a real prime's tables is rejected (a random pair never is: Row.tuples asserts it)."""
    from gpqhe_amd import _native
    lib = _native.load()
    row = next(r for r in mc.ROWS if r.name == "mulmod_split<TwW>")
    for mod in mc.moduli():
        if not mod.admits("wide"):
            continue
        p = mod.p
        t = row.tuples(mod)
        family, rejected = set(mc.wide_family(p)) | {1, 2}, set(t.rejected)
        assert rejected <= family and all(w < (1 << 34) for w in t.rejected) and not set(t.rejected) & set(mod.table)
        assert {1, 2} <= set(t.rejected)
        for w in set(t.w) | set(t.rejected):
            X, Y = mc.pair_of(p, w)
            ok = mc.fits_wide(p, X, Y)
            assert ok == (w not in rejected)
            assert lib.gpq_debug_split_entry_fits_wide(p, X, Y) == int(ok), (p, w)
        for w in set(t.w[:t.ndirected]) | set(t.rejected):
            th = max(mc.split_fold(a, *mc.pair_of(p, w), p)[0] for a in mc.wide_extremal_multiplicands(p))
            assert (th >= (1 << 32)) == (w in rejected), (p, w, th)
