// The contract of a ray query (crt_trace_async), as one predicate without HIP so that the query
// kernels (crt_device.hip) and a host test (tests/cpp/ray_class_check.cpp) run the same lines.
//
// A ray is traced iff its six numbers are finite, its direction is not all zero (+0 and -0 are
// both zero) and its upper bound is not NaN (+inf and -inf are bounds like any other). Denormal
// components are finite and non-zero: such rays are traced. Every other ray is written as a miss
// before any traversal state is set up: the walks never see it.
//
// The same holds for a ray whose interval is empty, t_max <= t_min (t_max = -inf included): every
// primitive test asks t_min < t < t_max, so BVH::hit_by reports no hit whatever it visits. It must
// not reach the render kernel's walks, which end at a sentinel node that every ray has to enter: the
// node test of an empty interval fails there too.
#pragma once

#ifndef CRT_HD
#define CRT_HD inline
#endif

namespace crt {

CRT_HD bool ray_component_finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }  // false for NaN

CRT_HD bool ray_traceable(const double o[3], const double d[3], double t_max) {
    const bool fin = ray_component_finite(o[0]) && ray_component_finite(o[1]) && ray_component_finite(o[2]) &&
                     ray_component_finite(d[0]) && ray_component_finite(d[1]) && ray_component_finite(d[2]);
    const bool dir = d[0] != 0 || d[1] != 0 || d[2] != 0;
    return fin && dir && t_max == t_max;
}

// false: nothing can be accepted in (t_min, t_max) (t_min is finite: crt_trace_async checks it)
CRT_HD bool ray_interval_open(double t_min, double t_max) { return t_min < t_max; }

}  // namespace crt
