"""Camera::render_progressive of the C++ drop-in end to end on the GPU: tests/cpp/progressive_e2e.cpp
renders config1_e2e.cpp's scene in passes and writes it with Image::send_as_ppm. Rendered to the
end its frame is Camera::render's bit for bit, so the PPM bytes equal config1_e2e's."""
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"
SEED = 4155677120  # tests/test_gpu_cpp_e2e.py: the render's base seed is then 7


def run(tmp_path, name):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / f"{name}.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    out = tmp_path / f"{name}.ppm"
    r = subprocess.run([str(exe), str(SEED), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return out.read_bytes(), r.stdout


def test_progressive_ppm_equals_one_shot_ppm(tmp_path):
    want, _ = run(tmp_path, "config1_e2e")
    got, log = run(tmp_path, "progressive_e2e")
    assert "pass 1: 1 / 1 spp" in log and "100%" in log  # on_pass ran and the ProgressBar ticked
    assert got == want
