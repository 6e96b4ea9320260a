"""The C++ interface of cudapolish's resident route (FastaParser qualities,
DeviceReads::create with qualities, cudapolish::add_poa_group_resident):
tests/polish_resident_cpp_check.cpp, built against the library and run once on
the host part and once with a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["fastq_qualities", "fasta_has_none", "quality_count_refused", "bad_qualities_refused"]
GPU = ["device_reads_with_qualities", "statuses_equal", "bad_slices_refused", "consensus_equal"]


def build(tmp_path):
    lib = os.path.join(ROOT, "claragenomicsanalysis_amd", "lib")
    exe = str(tmp_path / "polish_resident_cpp_check")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-std=c++17", "-O1", "-Wall",
                           "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           "-x", "c++", os.path.join(ROOT, "tests", "polish_resident_cpp_check.cpp"), "-L", lib,
                           "-lgwamd", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def run(tmp_path, *args):
    r = subprocess.run([build(tmp_path), str(tmp_path / "reads.fastq")] + list(args), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.split()


def test_cpp_interface_host_part(tmp_path):
    assert run(tmp_path) == [word for name in HOST for word in ("ok", name)]


@pytest.mark.gpu
def test_cpp_interface(tmp_path):
    assert run(tmp_path, "gpu") == [word for name in HOST + GPU for word in ("ok", name)]
