// Row dealing arithmetic of the tilings (crt_tiling{rb, n, d}): frame row r belongs to tile
// (r / rb) % n, and a tile's owned rows are numbered in frame order. No HIP here
// (tests/cpp/rows_check.cpp is a plain g++ program).
#pragma once

#include <cstddef>
#include <cstdint>

namespace crt {

// Tile d's rows of an H-row frame as the gather copies them: `blocks` row blocks, the first at
// frame row `first`, `step` rows apart; the first `full` of them have all rb rows, a short last
// one (full < blocks) starts at frame row `last` and ends with the frame.
struct RowSpans {
    size_t first, step, blocks, full, last;
};
inline RowSpans row_spans(size_t H, size_t rb, size_t n, size_t d) {
    RowSpans s{d * rb, n * rb, 0, 0, 0};
    if (s.first >= H) return s;
    s.blocks = (H - s.first + s.step - 1) / s.step;
    s.last = s.first + (s.blocks - 1) * s.step;
    s.full = s.last + rb <= H ? s.blocks : s.blocks - 1;
    return s;
}

// the number of rows of [0, h) that tile ti of tc owns
inline uint32_t count_owned(uint32_t h, uint32_t rb, uint32_t tc, uint32_t ti) {
    const RowSpans s = row_spans(h, rb, tc, ti);
    return static_cast<uint32_t>(s.full * rb + (s.full < s.blocks ? h - s.last : 0));
}

// The row that holds tile d's k-th owned row: of the frame, or of a packed buffer (row k itself).
inline size_t owned_to_frame_row(size_t k, size_t rb, size_t n, size_t d, bool packed = false) {
    return packed ? k : (k / rb * n + d) * rb + k % rb;
}

// Block row j of tile d (blocks of bh owned rows, rb a multiple of bh) as a block row of the frame.
inline size_t owned_to_frame_block_row(size_t j, size_t bh, size_t rb, size_t n, size_t d) {
    return owned_to_frame_row(j * bh, rb, n, d) / bh;
}

// Samples per pass of a job of N samples in chunks of L: the requested number (0: a tenth of the
// job, N / 10, at least 1) rounded up to whole chunks.
inline uint64_t pass_len(uint32_t N, uint32_t L, uint32_t requested) {
    const uint64_t want = requested ? requested : (N / 10 > 1 ? N / 10 : 1);
    return (want + L - 1) / L * L;
}

}  // namespace crt
