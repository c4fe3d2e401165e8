// The cube-map environment lookup E(d) of include/crt_render.h (crt_env), one copy for
// radiance_kernel and plain_radiance_kernel (crt_device.hip), without HIP so that a host program
// can run the same lines. Every operation is an IEEE f64 + - * /, a comparison or a floor, and the
// build never fuses (-ffp-contract=off): tests/env_model.py restates it in numpy bit for bit.
//
// Bounds: the float-to-integer conversions come after the range check on m, where |u|, |v| <= 1,
// so fx, fy lie in [0, n] with n <= 16384, and every index is clamped to [0, n - 1] as an integer:
// no direction reads outside the 6n x n x 3 doubles.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/crt_render.h"

#ifndef CRT_HD
#define CRT_HD inline
#endif

namespace crt {

CRT_HD int env_clamp(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// Steps 1 to 5 of E(d): the face, (u, v), h and (fx, fy) of a direction. One copy for env_lookup and
// for env_pdf (crt_env_sampler.h).
struct EnvProj {
    uint32_t face;
    double u, v, h, fx, fy;
};

// false where d has no major axis (step 2): nothing of J is written then
CRT_HD bool env_project(const crt_env& E, const double d[3], EnvProj& J) {
    const double x = (d[0] * E.right[0] + d[1] * E.right[1]) + d[2] * E.right[2];
    const double y = (d[0] * E.up[0] + d[1] * E.up[1]) + d[2] * E.up[2];
    const double z = (d[0] * E.forward[0] + d[1] * E.forward[1]) + d[2] * E.forward[2];
    const double ax = __builtin_fabs(x), ay = __builtin_fabs(y), az = __builtin_fabs(z);
    double m = ax >= ay ? ax : ay;
    m = m >= az ? m : az;
    // the comparisons above drop a NaN; m must carry it
    const bool ordered = ax == ax && ay == ay && az == az;
    if (!(ordered && m > 0 && m < __builtin_inf())) return false;
    if (ax >= ay && ax >= az) {
        J.face = x > 0 ? 0u : 1u;
        J.u = (x > 0 ? -z : z) / m;
        J.v = -y / m;
    } else if (ay >= az) {
        J.face = y > 0 ? 2u : 3u;
        J.u = x / m;
        J.v = (y > 0 ? z : -z) / m;
    } else {
        J.face = z > 0 ? 4u : 5u;
        J.u = (z > 0 ? x : -x) / m;
        J.v = -y / m;
    }
    J.h = 0.5 * static_cast<double>(E.face_size);
    J.fx = (J.u + 1.0) * J.h;
    J.fy = (J.v + 1.0) * J.h;
    return true;
}

// E(d) into out[3]; bg: the call's constant background, the value where d has no major axis
CRT_HD void env_lookup(const crt_env& E, const double d[3], const double bg[3], double out[3]) {
    EnvProj J;
    if (!env_project(E, d, J)) {
        out[0] = bg[0]; out[1] = bg[1]; out[2] = bg[2];
        return;
    }
    const uint32_t face = J.face;
    const double fx = J.fx, fy = J.fy;
    const int n = static_cast<int>(E.face_size);
    const size_t row0 = static_cast<size_t>(face) * E.face_size;
    if (E.filter == CRT_ENV_NEAREST) {
        const int col = env_clamp(static_cast<int>(__builtin_floor(fx)), n);
        const int row = env_clamp(static_cast<int>(__builtin_floor(fy)), n);
        const double* t = E.texels + ((row0 + static_cast<size_t>(row)) * E.face_size + static_cast<size_t>(col)) * 3;
        out[0] = t[0]; out[1] = t[1]; out[2] = t[2];
        return;
    }
    const double gx = fx - 0.5, gy = fy - 0.5;
    const double x0f = __builtin_floor(gx), y0f = __builtin_floor(gy);
    const double wx = gx - x0f, wy = gy - y0f;
    const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f);
    const size_t ca = static_cast<size_t>(env_clamp(x0, n)), cb = static_cast<size_t>(env_clamp(x0 + 1, n));
    const size_t ra = (row0 + static_cast<size_t>(env_clamp(y0, n))) * E.face_size;
    const size_t rb = (row0 + static_cast<size_t>(env_clamp(y0 + 1, n))) * E.face_size;
    const double* c00 = E.texels + (ra + ca) * 3;
    const double* c10 = E.texels + (ra + cb) * 3;
    const double* c01 = E.texels + (rb + ca) * 3;
    const double* c11 = E.texels + (rb + cb) * 3;
    for (int k = 0; k < 3; ++k) {
        const double a = c00[k] + wx * (c10[k] - c00[k]);
        const double b = c01[k] + wx * (c11[k] - c01[k]);
        out[k] = a + wy * (b - a);
    }
}

}  // namespace crt
