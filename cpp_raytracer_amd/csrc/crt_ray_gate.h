// The per-ray range checks of a traversal set-up (trav_init, leaf_step in crt_device.hip) and the
// one gate that implies them all, without HIP so that the kernels and a host test
// (tests/cpp/ray_gate_check.cpp) run the same lines.
//
// A traversal set-up asks of a ray (o, d), with a = dot(d, d) as the kernels compute it (f64, three
// rounded squares summed left to right, no fused multiply-add) and o32 = RN32(o), d32 = RN32(d):
//   gate_walk_plain   1/d finite and non-zero, o finite: the min/max and f32 walks' slab values are
//                     NaN-free (else the EXACT walk, Trav::neg & kZeroDir)
//   gate_walk_f32     the f32 walk's error analysis holds (else marg = inf: every node test in f64)
//   gate_leaf32       the packed f32 sphere filter's error analysis holds (leaf_ray32)
//   gate_recip        div_a's corrections are exact for this a (else it divides)
// Camera rays and scattered rays of any scene a camera can look at pass all four, and until
// round 8 every set-up spent some forty vector instructions proving it again. ray_gate() is one
// conservative predicate over the three-plus-three f32 conversions the set-up makes anyway; a wave
// whose lanes all pass it takes the four as known, any other wave evaluates them as before.
//
// ray_gate(o32, d32):  sd = (|d32_0| + |d32_1|) + |d32_2| <= 2^29,
//                      so = (|o32_0| + |o32_1|) + |o32_2| <= 2^29,
//                      min_k |d32_k| >= 2^-29                        (f32, round to nearest)
// NaN fails it: a NaN component makes its sum NaN, and every comparison is written so that NaN
// compares false (min() alone would drop a NaN operand, which is why the sums come first: once
// sd <= 2^29 holds no d32_k is NaN and the minimum is exact). +-inf fails the sums.
//
// Proof that the gate implies the four. RN32 (f64 -> f32, round to nearest even) is monotone and
// odd, and a sum of non-negative f32 terms rounds to no less than each term (each term is
// representable and not above the exact sum).
//  (1) sd <= 2^29 gives |d32_k| <= 2^29 for every k. Then |d_k| <= 2^29 (1 + 2^-24) < 2^30: the
//      f64 values that round to at most 2^29 end at the midpoint to the next f32, 2^29 + 2^5.
//  (2) min_k |d32_k| >= 2^-29 gives |d_k| >= 2^-29 (1 - 2^-25) > 2^-30 for every k (below that
//      midpoint RN32 gives at most the f32 before 2^-29), so d_k is neither zero nor NaN.
//  (3) so <= 2^29 gives |o32_k| <= 2^29, so o_k is finite and |o_k| < 2^30 as in (1).
//  gate_walk_plain: 2^-1000 <= |d_k| <= 2^1000 by (1), (2); o finite by (3).
//  gate_walk_f32:   2^-39 <= |d32_k| <= 2^39 and |o32_k| <= 2^40 by (1)-(3) on the f32 values.
//  a:  every RN(d_k^2) lies in [2^-58 (1 - 2^-24), 2^58 (1 + 2^-24)^2 (1 + 2^-53)], and a sum of
//      three such terms, rounded twice, in [2^-58 (1 - 2^-24), 3 * 2^58 (1 + 2^-22)] (a rounded
//      sum of non-negative terms is no less than each term), inside [2^-60, 2^60].
//  gate_leaf32:     a in [2^-60, 2^60] by the line above, |o_k|, |d_k| <= 2^30 by (1), (3).
//  gate_recip:      a in [2^-500, 2^500] likewise.
// tests/test_ray_gate.py checks the implication on 10^6 random rays over the whole f64 exponent
// range and on every threshold's neighbours, zeros, denormals, infinities and NaN.
#pragma once

#ifndef CRT_HD
#define CRT_HD inline
#endif

namespace crt {

CRT_HD bool gate_dir_ok(double x) { return __builtin_fabs(x) >= 0x1p-1000 && __builtin_fabs(x) <= 0x1p1000; }
CRT_HD bool gate_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }

CRT_HD bool gate_walk_plain(const double o[3], const double d[3]) {
    return gate_dir_ok(d[0]) && gate_dir_ok(d[1]) && gate_dir_ok(d[2]) &&
           gate_finite(o[0]) && gate_finite(o[1]) && gate_finite(o[2]);
}

// o32 = RN32(o), d32 = RN32(d)
CRT_HD bool gate_walk_f32(const float o32[3], const float d32[3]) {
    bool ok = true;
    for (int k = 0; k < 3; ++k)
        ok = ok && __builtin_fabsf(d32[k]) <= 0x1p39f && __builtin_fabsf(d32[k]) >= 0x1p-39f &&
             __builtin_fabsf(o32[k]) <= 0x1p40f;
    return ok;
}

CRT_HD bool gate_leaf32(const double o[3], const double d[3], double a) {
    bool ok = a >= 0x1p-60 && a <= 0x1p60;
    for (int k = 0; k < 3; ++k) ok = ok && __builtin_fabs(o[k]) <= 0x1p30 && __builtin_fabs(d[k]) <= 0x1p30;
    return ok;
}

CRT_HD bool gate_recip(double a) { return a >= 0x1p-500 && a <= 0x1p500; }

constexpr float kGateMax = 0x1p29f, kGateMinDir = 0x1p-29f;

CRT_HD bool ray_gate(const float o32[3], const float d32[3]) {
    const float sd = (__builtin_fabsf(d32[0]) + __builtin_fabsf(d32[1])) + __builtin_fabsf(d32[2]);
    const float so = (__builtin_fabsf(o32[0]) + __builtin_fabsf(o32[1])) + __builtin_fabsf(o32[2]);
    const float dmin = __builtin_fminf(__builtin_fminf(__builtin_fabsf(d32[0]), __builtin_fabsf(d32[1])),
                                       __builtin_fabsf(d32[2]));
    return sd <= kGateMax && so <= kGateMax && dmin >= kGateMinDir;
}

}  // namespace crt
