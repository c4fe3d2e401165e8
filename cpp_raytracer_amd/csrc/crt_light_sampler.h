// Sampling of the scene's own lights (include/crt_render.h, crt_light_sampler): the weights,
// light_pick, light_point and light_pdf, one copy for the sampler's build, the lights instances of
// radiance_kernel and plain_radiance_kernel (crt_device.hip) and a host program. Every operation is
// an IEEE f64 + - * /, a sqrt or a comparison, and the build never fuses (-ffp-contract=off):
// tests/light_nee_model.py restates it in numpy bit for bit. No sin or cos: spheres are sampled by
// area (a point on the whole surface from random_unit_vector), not by the cone they subtend.
//
// Bounds: both searches return a count in [0, L] that is clamped to [0, L - 1] before it indexes, so
// no xi (NaN included: every comparison with it is false) and no ref reads outside the tables.
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef CRT_HD
#define CRT_HD inline
#endif

namespace crt {

// the tables of a sampler; L >= 1
struct LightTables {
    const uint32_t* ref;   // pick order (ascending flattened primitive index): light i's slot reference
    const double* cdf;     // pick order: sequential sums of w
    const uint32_t* sref;  // the slot references sorted ascending
    const double* sw;      // w in sref's order
    double W;              // cdf[L - 1]
    uint32_t L;
};

CRT_HD double light_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Y of an emission e = color * param: NaN and negative values give 0
CRT_HD double light_luminance(const double e[3]) {
    const double Y = (0.2126 * e[0] + 0.7152 * e[1]) + 0.0722 * e[2];
    return Y > 0 ? Y : 0.0;
}

// A of a parallelogram with sides s1, s2: |s1 x s2|
CRT_HD double light_area_quad(const double s1[3], const double s2[3]) {
    const double cr[3] = {s1[1] * s2[2] - s1[2] * s2[1], s1[2] * s2[0] - s1[0] * s2[2], s1[0] * s2[1] - s1[1] * s2[0]};
    return __builtin_sqrt(light_dot(cr, cr));
}

// A of a sphere of radius r (hollow spheres have r < 0)
CRT_HD double light_area_sphere(double r) { return (4.0 * 3.141592653589793) * (r * r); }

// how many of the non-decreasing a[0 .. len) are <= x (env_count_le's form)
template <typename T>
CRT_HD uint32_t light_count_le(const T* a, uint32_t len, T x) {
    uint32_t lo = 0, hi = len;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// light i of a number in [0, 1): the count of entries with cdf[k] <= xi1 * W, clamped to L - 1
CRT_HD uint32_t light_pick(const LightTables& Tb, double xi1) {
    const uint32_t i = light_count_le(Tb.cdf, Tb.L, xi1 * Tb.W);
    return i > Tb.L - 1 ? Tb.L - 1 : i;
}

// w of the light in slot `ref`; 0 for a ref that is no light
CRT_HD double light_weight(const LightTables& Tb, uint32_t ref) {
    const uint32_t cnt = light_count_le(Tb.sref, Tb.L, ref);
    const uint32_t k = cnt > 0 ? cnt - 1 : 0;
    return Tb.sref[k] == ref ? Tb.sw[k] : 0.0;
}

// the point of a parallelogram light of two numbers in [0, 1), drawn in that order
CRT_HD void light_point(const double v[3], const double s1[3], const double s2[3], double xi2, double xi3, double p[3]) {
    for (int k = 0; k < 3; ++k) p[k] = (v[k] + s1[k] * xi2) + s2[k] * xi3;
}

// the point of a sphere light of random_unit_vector's u
CRT_HD void light_point(const double c[3], double r, const double u[3], double p[3]) {
    const double ar = __builtin_fabs(r);
    for (int k = 0; k < 3; ++k) p[k] = c[k] + u[k] * ar;
}

// The solid-angle density with which the sampler produces the point where the ray (.., d) hit a
// light at t: w its weight, A its area, n the hit's normal (either side), outside false for a hit on
// the geometric inside of a sphere (the sampler's points are seen from outside only).
CRT_HD double light_pdf(double w, double W, double A, double t, const double n[3], const double d[3], bool outside) {
    if (!outside || !(w > 0)) return 0.0;
    const double v[3] = {d[0] * t, d[1] * t, d[2] * t};
    const double vv = light_dot(v, v);
    return ((w / W) / A) * ((vv * __builtin_sqrt(vv)) / __builtin_fabs(light_dot(n, v)));
}

}  // namespace crt
