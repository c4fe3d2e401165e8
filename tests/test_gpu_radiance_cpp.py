"""Camera::ray_colors of the C++ drop-in end to end on the GPU: tests/cpp/radiance_e2e.cpp, compiled
by g++ against the drop-in headers (no torch in the process), compares it byte for byte with
crt_radiance called directly, on 4096 rays in the Cornell box."""
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"


def test_ray_colors_equal_crt_radiance(tmp_path):
    exe = tmp_path / "radiance_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "radiance_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    r = subprocess.run([str(exe), "20261"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    lit, dark, n = map(int, re.search(r"^lit (\d+) dark (\d+) of (\d+)$", r.stdout, re.M).groups())
    assert n == 4096 and lit + dark == n and lit >= 100 and dark >= 100  # paths that reach the light, and paths that do not
