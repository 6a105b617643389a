"""The per-(kernel, device) table behind the dynamic-LDS opt-in (csrc/lds_table.h) as plain host C++: tests/host/lds_table_main.cpp
is compiled with the machine's C++ compiler and run.  8 threads x 4 fake kernels x 3 devices request 32, 70, 150, 70, 150 KiB: the
setter runs exactly twice per (kernel, device), with 70 then 150 KiB, never for 32 KiB; a failed setter is not recorded, is asked
again by the next identical request, and its error value comes back unchanged.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_lds_table_host_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "hipcc", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler found")
    exe = str(tmp_path / "lds_table_main")
    src = os.path.join(REPO, "tests", "host", "lds_table_main.cpp")
    inc = [f"-I{os.path.join(REPO, 'include')}", f"-I{os.path.join(REPO, 'inverseproblemwithdiffusionmodel_amd', 'csrc')}"]
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-pthread", *inc, src, "-o", exe], check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.returncode, p.stdout, p.stderr)
