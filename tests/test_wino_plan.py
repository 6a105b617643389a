"""The launch plan of the 2-D Winograd kernels and the reader of the IPDM_* switches (csrc/wino_plan.h, env_int.h) as plain host
C++: tests/host/wino_plan_main.cpp is compiled with the machine's C++ compiler and run.  It sweeps layer shapes x batch x operand
family x epilogue x alignment x every single switch and checks each served plan against what the kernels' static_asserts and
arguments ask (tile counts, f16x2-only forms, 16-byte DMA only for aligned inputs, no epilogue dropped), the form and partials
queries against the plan, and that 8 threads reading a switch see one value.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def test_wino_plan_host_program(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++", "hipcc", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler found")
    exe = str(tmp_path / "wino_plan_main")
    src = os.path.join(REPO, "tests", "host", "wino_plan_main.cpp")
    inc = [f"-I{os.path.join(REPO, 'include')}", f"-I{os.path.join(REPO, 'inverseproblemwithdiffusionmodel_amd', 'csrc')}"]
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O1", "-pthread", *inc, src, "-o", exe], check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.returncode, p.stdout, p.stderr)
