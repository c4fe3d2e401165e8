"""BVH::hit_by_batch and BVH::occluded_batch of the C++ drop-in end to end on the GPU:
tests/cpp/trace_e2e.cpp, compiled by g++ against the drop-in headers, compares them with
BVH::hit_by called ray by ray (crt_closest_hits) on a sphere world and a box room."""
import re
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
INC = ROOT / "cpp_raytracer_amd" / "include"
LIBDIR = ROOT / "cpp_raytracer_amd" / "lib"


def test_batches_equal_hit_by_ray_by_ray(tmp_path):
    exe = tmp_path / "trace_e2e"
    subprocess.run(["g++", "-std=c++20", "-O2", f"-I{INC}", str(ROOT / "tests" / "cpp" / "trace_e2e.cpp"),
                    "-o", str(exe), f"-L{LIBDIR}", "-lcrt_hip", f"-Wl,-rpath,{LIBDIR}"], check=True, timeout=300)
    r = subprocess.run([str(exe), "20251"], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    cases = re.findall(r"^(\w+) \(.*\) hits (\d+) of (\d+)$", r.stdout, re.M)
    assert [c[0] for c in cases] == ["spheres", "spheres", "room", "room"]
    for name, hits, n in cases:  # hits and misses in every case: neither side of the comparison is empty
        assert int(n) == 200 and 10 <= int(hits) <= 190, (name, hits)
