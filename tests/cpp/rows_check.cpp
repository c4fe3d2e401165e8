// Brute-force check of cpp_raytracer_amd/csrc/crt_rows.h against the definition "frame row r belongs
// to tile (r / rb) % n": H in 0..40, rb in {1, 2, 4, 8}, n in 1..9, every tile (tests/test_rows.py).
// Prints the number of cases checked; exits 1 at the first mismatch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "crt_rows.h"

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            std::printf("FAILED %s (line %d): H %zu rb %zu n %zu d %zu\n", #cond, __LINE__, H, rb, n, d);    \
            return 1;                                                                                        \
        }                                                                                                    \
    } while (0)

int main() {
    long cases = 0;
    size_t H = 0, rb = 0, n = 0, d = 0;
    for (H = 0; H <= 40; ++H)
        for (size_t rbi = 0; rbi < 4; ++rbi)
            for (n = 1; n <= 9; ++n)
                for (d = 0; d < n; ++d) {
                    rb = size_t{1} << rbi;
                    std::vector<size_t> owned;  // the definition
                    for (size_t r = 0; r < H; ++r)
                        if ((r / rb) % n == d) owned.push_back(r);
                    CHECK(crt::count_owned(H, rb, n, d) == owned.size());
                    for (size_t k = 0; k < owned.size(); ++k) {
                        CHECK(crt::owned_to_frame_row(k, rb, n, d) == owned[k]);
                        CHECK(crt::owned_to_frame_row(k, rb, n, d, false) == owned[k]);
                        CHECK(crt::owned_to_frame_row(k, rb, n, d, true) == k);
                    }
                    // the gather's spans, walked as gather_packed copies them: packed source row ->
                    // frame row; together they are the owned rows, once each, in order
                    const crt::RowSpans s = crt::row_spans(H, rb, n, d);
                    std::vector<size_t> copied;
                    CHECK(s.full <= s.blocks && s.blocks <= s.full + 1);
                    for (size_t b = 0; b < s.full; ++b)
                        for (size_t i = 0; i < rb; ++i) copied.push_back(s.first + b * s.step + i);
                    CHECK(copied.size() == s.full * rb);  // the short block's source starts at row full * rb
                    if (s.full < s.blocks) {
                        CHECK(s.last == s.first + s.full * s.step && s.last < H && H - s.last < rb);
                        for (size_t r = s.last; r < H; ++r) copied.push_back(r);
                    }
                    CHECK(copied == owned);
                    if (rb == 4)  // 4-row blocks of 4-row tiles: a tile's block row is one of the frame's
                        for (size_t j = 0; j * 4 < owned.size(); ++j) {
                            CHECK(crt::owned_to_frame_block_row(j, 4, rb, n, d) * 4 == crt::owned_to_frame_row(j * 4, rb, n, d));
                            CHECK(crt::owned_to_frame_block_row(j, 4, rb, n, d) == owned[j * 4] / 4);
                        }
                    if (rb == 8)  // two block rows a row block
                        for (size_t j = 0; j * 4 < owned.size(); ++j)
                            CHECK(crt::owned_to_frame_block_row(j, 4, rb, n, d) == owned[j * 4] / 4);
                    ++cases;
                }
    // pass_len(N, L, requested): whole chunks, at least one, not less than asked; 0 asks for a
    // tenth of the job (N / 10 as the drivers have always taken it: the integer quotient, at least 1)
    for (uint32_t N = 1; N <= 2000; ++N)
        for (uint32_t L : {1u, 4u, 5u, 11u})
            for (uint32_t req : {0u, 1u, 3u, 4u, 8u, 22u, 1000u, 4294967295u}) {
                const uint64_t p = crt::pass_len(N, L, req);
                const uint64_t want = req ? req : std::max<uint32_t>(1, N / 10);
                if (p % L != 0 || p < L || p < want || p - want >= L) {
                    std::printf("FAILED pass_len(%u, %u, %u) = %llu\n", N, L, req, static_cast<unsigned long long>(p));
                    return 1;
                }
                ++cases;
            }
    std::printf("%ld\n", cases);
    return 0;
}
