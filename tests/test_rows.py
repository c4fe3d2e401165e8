"""cpp_raytracer_amd/csrc/crt_rows.h, the row-dealing arithmetic the drivers, the gather and the
per-device code share, by brute force against the definition "frame row r belongs to tile
(r / rb) % n" (tests/cpp/rows_check.cpp, a plain g++ program: the header needs no HIP).

H in 0..40, rb in {1, 2, 4, 8}, n in 1..9, every tile: count_owned is the count; owned-to-frame is
the k-th owned row, the identity when packed; the gather's spans cover the owned rows once each, in
order; the block-row mapping agrees with owned-to-frame at rb = 4. pass_len is a multiple of the
chunk length, at least one chunk, and the request rounded up to chunks. For a request of 0 that is
max(1, N // 10) rounded up: the integer quotient, as crt_render_progressive has always cut its
passes (N = 41 in chunks of 4 runs passes of 4, not of 8), so that no render changes its passes."""
import subprocess

from conftest import ROOT


def test_rows_header_against_definition(tmp_path):
    exe = tmp_path / "rows_check"
    subprocess.run(["g++", "-std=c++20", "-O2", "-Wall", "-Werror", f"-I{ROOT / 'cpp_raytracer_amd' / 'csrc'}",
                    str(ROOT / "tests" / "cpp" / "rows_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    # 41 heights x 4 row blocks x (1 + ... + 9) tiles, then 2000 x 4 x 8 pass lengths
    assert int(r.stdout) == 41 * 4 * 45 + 2000 * 4 * 8
