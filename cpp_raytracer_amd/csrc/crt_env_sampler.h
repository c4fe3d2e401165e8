// Luminance sampling of a cube-map environment (include/crt_render.h, crt_env_sampler): the table
// entries, env_pdf and env_sample, one copy for the sampler's build kernels, the NEE instances of
// radiance_kernel and plain_radiance_kernel (crt_device.hip) and a host program. Every operation is
// an IEEE f64 + - * /, a sqrt, a comparison or a floor, and the build never fuses
// (-ffp-contract=off): tests/env_nee_model.py restates it in numpy bit for bit.
//
// Bounds: env_pdf indexes as env_lookup's NEAREST step does (clamped integers after the range
// check). env_sample's searches return a count in [0, len] that is clamped to len - 1 before it
// indexes, so no xi (NaN included: every comparison with it is false) reads outside the tables.
#pragma once

#include "crt_env.h"

namespace crt {

// the tables of a sampler, rows r = face * n + row_in_face as the map's own
struct EnvTables {
    const double* w;  // 6n x n: luminance times the texel centre's solid-angle factor
    const double* c;  // 6n x n: prefix sums along each row
    const double* m;  // 6n: prefix sums of the rows' totals
    double W;         // m[6n - 1]
};

// w[r][col] of a texel (rgb) at column col, row_in_face row of a face of n x n
CRT_HD double env_weight(const double rgb[3], uint32_t col, uint32_t row, uint32_t n) {
    double Y = (0.2126 * rgb[0] + 0.7152 * rgb[1]) + 0.0722 * rgb[2];
    Y = Y > 0 ? Y : 0.0;  // NaN and negative values: 0
    const double g = 2.0 / static_cast<double>(n);
    const double uc = (static_cast<double>(col) + 0.5) * g - 1.0;
    const double vc = (static_cast<double>(row) + 0.5) * g - 1.0;
    const double sc = (1.0 + uc * uc) + vc * vc;
    return Y / (sc * __builtin_sqrt(sc));
}

// the solid-angle density with which env_sample draws the direction d; 0 where d has no major axis
CRT_HD double env_pdf(const crt_env& E, const EnvTables& Tb, const double d[3]) {
    EnvProj J;
    if (!env_project(E, d, J)) return 0.0;
    const int n = static_cast<int>(E.face_size);
    const int col = env_clamp(static_cast<int>(__builtin_floor(J.fx)), n);
    const int row = env_clamp(static_cast<int>(__builtin_floor(J.fy)), n);
    const size_t r = static_cast<size_t>(J.face) * E.face_size + static_cast<size_t>(row);
    const double s = (1.0 + J.u * J.u) + J.v * J.v;
    const double hh = J.h * J.h;
    return ((Tb.w[r * E.face_size + static_cast<size_t>(col)] / Tb.W) * hh) * (s * __builtin_sqrt(s));
}

// how many of the non-decreasing a[0 .. len) are <= x
CRT_HD uint32_t env_count_le(const double* a, uint32_t len, double x) {
    uint32_t lo = 0, hi = len;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the direction of four numbers in [0, 1), unnormalised, in the map's basis
CRT_HD void env_sample(const crt_env& E, const EnvTables& Tb, double xi1, double xi2, double xi3, double xi4,
                       double d[3]) {
    const uint32_t n = E.face_size, rows = 6 * n;
    uint32_t r = env_count_le(Tb.m, rows, xi1 * Tb.W);
    r = r > rows - 1 ? rows - 1 : r;
    const double* cr = Tb.c + static_cast<size_t>(r) * n;
    uint32_t k = env_count_le(cr, n, xi2 * cr[n - 1]);
    k = k > n - 1 ? n - 1 : k;
    const uint32_t face = r / n, rf = r % n;
    const double g = 2.0 / static_cast<double>(n);
    const double fx = static_cast<double>(k) + xi3, fy = static_cast<double>(rf) + xi4;
    const double u = fx * g - 1.0, v = fy * g - 1.0;
    double x, y, z;
    switch (face) {  // crt_lens_rays_async's CUBE table
        case 0: x = 1.0; y = -v; z = -u; break;   // +X
        case 1: x = -1.0; y = -v; z = u; break;   // -X
        case 2: x = u; y = 1.0; z = v; break;     // +Y
        case 3: x = u; y = -1.0; z = -v; break;   // -Y
        case 4: x = u; y = -v; z = 1.0; break;    // +Z
        default: x = -u; y = -v; z = -1.0; break; // -Z
    }
    for (int j = 0; j < 3; ++j) d[j] = (E.right[j] * x + E.up[j] * y) + E.forward[j] * z;
}

}  // namespace crt
