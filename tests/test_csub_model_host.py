"""tools/csub_model.cpp: the integer model of the masked conditional subtraction (csub_by, gpqhe_amd/csrc/modarith.hpp) equals the select
form and x - m [x >= m] at the edge values under every entry mask, and restores the mask.  A stand-alone host program, built here with
the undefined-behaviour sanitizer; tests/test_masked_csub_gpu.py runs the HIP text on the same values."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_masked_form_equals_select_form_on_the_host(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "hipcc") if shutil.which(c)), None)
    assert cxx, "no C++ compiler on PATH"
    exe = str(tmp_path / "csub_model")
    subprocess.run([cxx, "-std=c++17", "-O1", "-fsanitize=undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "csub_model.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "select form == masked form" in run.stdout
