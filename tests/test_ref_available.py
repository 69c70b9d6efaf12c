"""Guard against silent skipping: where the reference checkout exists, oracle/_ref/ must be built and current.

The test_ref_* modules compare the oracle (and, on the GPU, the device) with the EXECUTED reference that `make -C oracle ref` leaves
in oracle/_ref/.  They may skip only on a bare checkout (no sources, no oracle/_ref/).  This module FAILS when the sources are there
and a library or BUILD.json is missing or older than what it was built from."""
import json
import os

import pytest

from oracle import ref
from tests.ref_jobs import ROOT, reference_sources


def test_reference_build_is_present_and_current():
    src = reference_sources()
    if src is None and not os.path.isdir(ref.DIR):
        pytest.skip("bare checkout: neither a reference checkout nor oracle/_ref/")
    products = [ref.AS_IS, ref.FLOOR, ref.BUILD_JSON]
    missing = [p for p in products if not os.path.exists(p)]
    assert not missing, "not built: %s -- run __graft_entry__.build() (make -C oracle ref)" % ", ".join(os.path.relpath(p, ROOT) for p in missing)
    inputs = [os.path.join(ROOT, "oracle", "ref_driver.c"), os.path.join(ROOT, "oracle", "gcrypt_decl", "gcrypt.h")]
    if src is not None:                                   # only compared where the tree was built here; the libraries travel without their sources
        for p in products:
            stale = [i for i in inputs if os.path.getmtime(i) > os.path.getmtime(p)]
            assert not stale, "%s is older than %s: rebuild" % (os.path.relpath(p, ROOT), ", ".join(os.path.relpath(i, ROOT) for i in stale))
    with open(ref.BUILD_JSON) as f:
        info = json.load(f)
    assert len(info["reference_sha256"]) >= 22 + 8        # the 22 sources of the reference's library target and its headers
    running = ref.Ref(ref.AS_IS).gcrypt_version()
    # a difference is not a failure: ref.which() decides by probing the loaded library, never by version
    print("libgcrypt: built against %s, running %s; floor division of negative dividends native: %s -> %s"
          % (info["libgcrypt"], running, ref.floor_is_native(), os.path.basename(ref.which())))
    assert ref.Ref(ref.AS_IS).L.ref_floor_fixed() == 0 and ref.Ref(ref.FLOOR).L.ref_floor_fixed() == 1
    assert os.path.basename(ref.which()) == ("libgpqhe_ref.so" if ref.floor_is_native() else "libgpqhe_ref_floor.so")

