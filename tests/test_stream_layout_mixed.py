"""The one device allocation of a mixed demand (tfx_set_demand_mixed; csrc/tfx_stream_layout.hpp, the up-front form): a
stand-alone program (tests/stream_layout_mixed_check.cpp) restates the rows rule, asserts the regions in order and inside
the allocation and that a 10-tick decision of cfg2-sized envs fits, under AddressSanitizer and UBSan.  No device, no
library of the project loaded.  tests/test_stream_layout.py pins the other streams' layouts."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_mixed_stream_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or "c++"
    exe = str(tmp_path / "stream_layout_mixed_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "traffic-env_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "stream_layout_mixed_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mixed stream layout ok" in out.stdout
