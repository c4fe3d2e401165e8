"""Camera::render_lens(world, lens, lights) of the C++ drop-in, end to end on the GPU:
tests/cpp/light_nee_e2e.cpp, compiled by g++ against the drop-in headers (no torch in the process),
compares it byte for byte with crt_render_lens_lights called directly, for a cube map inside the Cornell
box, and counts the pixels that differ from the unsampled frame."""
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"


def test_camera_render_lens_lights_equals_crt_render_lens_lights(tmp_path):
    exe = tmp_path / "light_nee_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "light_nee_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    r = subprocess.run([str(exe), "20264"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    got = re.findall(r"^lights differs (\d+) of (\d+)$", r.stdout, re.M)
    assert len(got) == 1 and int(got[0][1]) == 96
    assert int(got[0][0]) > 0  # paths that bounce off a Lambertian draw more numbers: another frame
