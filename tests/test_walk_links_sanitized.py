"""The miss-link builder and validator of the stackless walk (cpp_raytracer_amd/csrc/crt_walk_links.h, the
text crt_host.cpp compiles) under AddressSanitizer and UndefinedBehaviorSanitizer: tools/walk_links_check.cpp
compiled as a stand-alone host program and run as a child process, never loaded into Python, on random
trees in the device node order, a root that is a leaf, one interior node, chains up to the u16 limit and
malformed arrays; every table must validate and equal the recursive definition, and none with one entry
changed may. CPU only."""
import shutil
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def test_builder_and_validator_are_clean_under_sanitizers(tmp_path):
    exe = tmp_path / "walk_links_check"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", "-I", str(ROOT / "cpp_raytracer_amd" / "csrc"),
                    str(ROOT / "tools" / "walk_links_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "2000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("walk links ok: 2060 trees, "), r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
