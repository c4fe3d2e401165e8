"""Camera::render_lens(world, lens, env) of the C++ drop-in end to end on the GPU: tests/cpp/env_e2e.cpp,
compiled by g++ against the drop-in headers (no torch in the process), compares it byte for byte with
crt_render_lens_env called directly, for a cube map inside the Cornell box lit by a cube-map environment
through both filters, and counts the pixels that differ from the constant-background frame."""
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"


def test_camera_render_lens_env_equals_crt_render_lens_env(tmp_path):
    exe = tmp_path / "env_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "env_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    r = subprocess.run([str(exe), "20263"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    got = re.findall(r"^env (nearest|bilinear) differs (\d+) of (\d+)$", r.stdout, re.M)
    assert [g[0] for g in got] == ["nearest", "bilinear"]
    for _, differs, n in got:
        assert int(n) == 96
        assert int(differs) > 0  # the box's front is open: the environment is seen, the frame is not the flat one
