"""Camera::render_adaptive of the C++ drop-in end to end on the GPU: tests/cpp/adaptive_e2e.cpp
renders one small scene with Camera::render, with render_adaptive when no block may stop, and with
a stopping rule, and writes each with Image::send_as_ppm. When no block stops the frame is
Camera::render's bit for bit, so the PPM bytes are equal."""
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
SEED = 4155677120  # tests/test_gpu_cpp_e2e.py: the render's base seed is then 7


def test_adaptive_ppm_equals_render_ppm_when_no_block_stops(tmp_path):
    exe = tmp_path / "adaptive_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "adaptive_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    outs = [tmp_path / f"{n}.ppm" for n in ("render", "never_stop", "adaptive")]
    r = subprocess.run([str(exe), str(SEED), *map(str, outs)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    want, never, adaptive = (p.read_bytes() for p in outs)
    assert want.startswith(b"P3\n100 56\n255\n")
    assert never == want
    # on_pass ran, the ProgressBar ticked, and the mean spp is printed: 12 when nothing stops,
    # fewer with the stopping rule (the sky's blocks stop at 8)
    assert "pass 3: 12 / 12 spp" in r.stdout and "100%" in r.stdout
    means = [float(m) for m in re.findall(r"Rendered ([0-9.]+) spp on average \(of 12\)", r.stdout)]
    print(r.stdout[-1500:])
    assert len(means) == 2 and means[0] == 12 and 8 <= means[1] < 12
    assert len(adaptive) > 0 and adaptive[:14] == want[:14]
