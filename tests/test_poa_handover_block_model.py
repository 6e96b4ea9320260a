"""The block hand-over as the row loop of the 16-bit LDS forward pass is written
since it runs block by block (an outer loop per block, no per-row hand-over
test), as a host model (CPU only): tests/handover_block_model.cpp steps one
producer against one consumer over csrc/poa_handover.hpp under the four
schedulers of tests/handover_model.cpp, for every V in 1 .. 3*64 + 2*B and B in
{8, 16}.  It asserts that the outer loop's blocks are those of the per-row
tests, that every carry is read after it was written and before its slot is
rewritten, that the sweep's last wave stores carry[1 .. V] once each and
nothing else, and that both sides finish within a step bound.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handover_block_model(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no system C++ compiler")
    exe = str(tmp_path / "handover_block_model")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "claragenomicsanalysis_amd", "csrc"),
                           os.path.join(ROOT, "tests", "handover_block_model.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failed" in r.stdout, r.stdout[-4000:]
