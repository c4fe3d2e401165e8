"""Camera::probes of the C++ drop-in end to end on the GPU: tests/cpp/probes_e2e.cpp, compiled by g++
against the drop-in headers (no torch in the process), compares it byte for byte with crt_probes
called directly, on 8 floor points of the Cornell box in both modes."""
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"


def test_camera_probes_equal_crt_probes(tmp_path):
    exe = tmp_path / "probes_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "probes_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    r = subprocess.run([str(exe), "20262"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    n, sphere, hemi = map(int, re.search(r"^probes (\d+) sphere (\d+) hemisphere (\d+)$", r.stdout, re.M).groups())
    assert n == 8 and sphere == 8 and hemi == 8  # the box is lit and the sky is not black: every probe receives light
