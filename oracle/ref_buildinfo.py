"""Writes _ref/BUILD.json after `make -C oracle ref`: what was compiled, with what, against which libgcrypt.

TEST INFRASTRUCTURE ONLY.  Usage: ref_buildinfo.py OUTDIR CC FLAGS SOURCE...   (data, untracked like the rest of _ref/)"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys


def main(outdir, cc, flags, sources):
    lib = ctypes.CDLL(os.path.join(os.path.abspath(outdir), "libgpqhe_ref.so"))
    lib.ref_gcrypt_version.restype = ctypes.c_char_p
    here = os.path.dirname(os.path.abspath(__file__))
    ours = [os.path.join(here, "ref_driver.c"), os.path.join(here, "gcrypt_decl", "gcrypt.h")]

    def sha(path):
        with open(path, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()

    info = {
        "compiler": subprocess.check_output([cc.split()[0], "--version"], text=True).splitlines()[0],
        "flags": flags,
        "libgcrypt": lib.ref_gcrypt_version().decode(),
        "libraries": ["libgpqhe_ref.so", "libgpqhe_ref_floor.so"],
        "reference_sha256": {os.path.basename(p): sha(p) for p in sources},
        "driver_sha256": {os.path.basename(p): sha(p) for p in ours},
    }
    with open(os.path.join(outdir, "BUILD.json"), "w") as f:
        json.dump(info, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4:])
