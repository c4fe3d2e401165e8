"""Camera::render_lens_progressive and Camera::render_lens_denoised of the C++ drop-in end to end on the
GPU: tests/cpp/lens_passes_e2e.cpp, compiled by g++ against the drop-in headers, compares a fisheye frame
and a cube map rendered in passes with render_lens' images, a render stopped by its callback with
crt_render_lens_passes stopped alike, and the PINHOLE denoised frames with render_denoised's, byte for
byte. Frames are at most 40 x 24."""
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"


def test_lens_passes_of_the_drop_in(tmp_path):
    exe = tmp_path / "lens_passes_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "lens_passes_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    r = subprocess.run([str(exe), "20263"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    passes, stopped, lit = map(int, re.search(r"^lens passes (\d+) stopped (\d+) lit (\d+)$", r.stdout, re.M).groups())
    assert passes == 6 and stopped == 8  # two frames of 24 samples in passes of 8; the callback's stop
    assert lit > 0  # the eye is inside the lit box: the frames are not black
