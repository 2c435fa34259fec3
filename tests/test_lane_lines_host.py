"""The idle-lane rule of the SpMM kernels (sgc_amd/csrc/lane_lines.h), checked
on the host: lane_lines_host.cpp is compiled against the header with the host
C++ compiler and enumerates every lane of every wave instruction of the
multi-row mapping (F in 602, 516, 132, 130, 90, 76 and the quads' widths), the
one-row mapping (V in 1, 2, 4 at F in 500, 1433, 129, 127) and the (col, val)
staging loads.  It asserts that the 128-B lines an instruction's lanes touch
are a subset of the lines its active lanes touch.

The rule the kernels had before -- an idle lane gathers byte 0 of the gathered
row -- fails this at F = 602: slice 4, lanes 23..31 read line 0."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(name) if name else None
        if path:
            return path
    return None


def test_idle_lanes_stay_on_active_lines(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lane_lines_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "sgc_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lane_lines_host.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failures" in res.stdout
