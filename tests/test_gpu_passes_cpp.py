"""Renders in passes from a C++ process on the GPU (tests/cpp/passes_e2e.cpp): the process loads
the system's HIP runtime, not the one a Python process has loaded, and renders four scenes in a
row. crt_render_progressive and a never-stopping crt_render_adaptive, three passes each, must give
crt_render's frame bit for bit every time: the pass path's scratch may not depend on what the
runtime's default memory pool does between passes."""
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"


def test_passes_from_a_cpp_process_equal_the_one_shot_render(tmp_path):
    exe = tmp_path / "passes_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{ROOT / 'include'}", str(ROOT / "tests" / "cpp" / "passes_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.stdout.count(" 0 of 16800 values differ") == 4 and r.stdout.count(", 0 differ") == 4
