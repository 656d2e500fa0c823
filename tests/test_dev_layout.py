"""The one table of an env's device arrays (csrc/tfx_dev_layout.hpp) is plain host arithmetic: a stand-alone program
(tests/dev_layout_check.cpp) carves the scratch arena and asserts its regions disjoint, aligned and inside the
allocation, splits device blocks into halves and asserts they tile every array, and requires sub_dev to give byte for
byte what the hand-written list gave - under AddressSanitizer and UBSan.  No device, no library of the project loaded."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_dev_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "c++"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "dev_layout_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "traffic-env_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "dev_layout_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dev layout ok" in out.stdout
