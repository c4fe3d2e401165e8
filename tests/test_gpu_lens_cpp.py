"""Camera::render_lens of the C++ drop-in end to end on the GPU: tests/cpp/lens_e2e.cpp, compiled by
g++ against the drop-in headers (no torch in the process), compares it byte for byte with
crt_render_lens called directly, for an equirectangular frame and a cube map inside the Cornell box."""
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"


def test_camera_render_lens_equals_crt_render_lens(tmp_path):
    exe = tmp_path / "lens_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "lens_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    r = subprocess.run([str(exe), "20263"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    el, en, cl, cn = map(int, re.search(r"^lens equirect (\d+) of (\d+) cube (\d+) of (\d+)$", r.stdout, re.M).groups())
    assert en == 128 and cn == 96
    assert el > 0 and cl > 0  # the eye is inside the lit box: neither frame is all black
