"""Camera::render_lens(world, lens, env) of the C++ drop-in with an importance-sampled Environment, end
to end on the GPU: tests/cpp/env_nee_e2e.cpp, compiled by g++ against the drop-in headers (no torch in
the process), compares it byte for byte with crt_render_lens_env_sampled called directly, for a cube
map inside the Cornell box lit by a map with one bright texel through both filters, and counts the
pixels that differ from the unsampled frame."""
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"


def test_camera_render_lens_importance_equals_crt_render_lens_env_sampled(tmp_path):
    exe = tmp_path / "env_nee_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "env_nee_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    r = subprocess.run([str(exe), "20264"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    got = re.findall(r"^nee (nearest|bilinear) differs (\d+) of (\d+)$", r.stdout, re.M)
    assert [g[0] for g in got] == ["nearest", "bilinear"]
    for _, differs, n in got:
        assert int(n) == 96
        assert int(differs) > 0  # paths that bounce off a Lambertian draw four more numbers: another frame
