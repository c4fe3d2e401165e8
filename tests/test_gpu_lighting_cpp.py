"""Camera::render_lens, render_lens_progressive and render_lens_denoised under a Lighting (the C++
drop-in), end to end on the GPU: tests/cpp/lighting_e2e.cpp, compiled by g++ against the drop-in headers (no
torch in the process), compares each byte for byte with the blocking entry it goes over
(crt_render_lens_lit, crt_render_lens_passes_lit) for a cube map inside the Cornell box under a sampled and
under a plain map with the box's light, and counts the pixels that the map changes. Lights made of another
world end the program with a message."""
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"


def test_the_drop_ins_lit_calls_equal_the_blocking_entries(tmp_path):
    exe = tmp_path / "lighting_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "lighting_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    r = subprocess.run([str(exe), "20264"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    for tag in ("sampled", "plain"):
        got = re.findall(rf"^{tag} render_lens differs (\d+) of (\d+)$", r.stdout, re.M)
        assert len(got) == 1 and int(got[0][1]) == 96 and int(got[0][0]) > 0  # the map is seen beside the light
        assert re.findall(rf"^{tag} render_lens_progressive passes (\d+)$", r.stdout, re.M) == ["4"]
        got = re.findall(rf"^{tag} render_lens_denoised differs (\d+) of (\d+)$", r.stdout, re.M)
        assert len(got) == 1 and int(got[0][0]) > 0  # the filter did something
    assert "nothing set equals crt_render_lens" in r.stdout
    r = subprocess.run([str(exe), "20264", "foreign"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "the Lights were made of another world" in r.stdout, r.stdout[-2000:]
