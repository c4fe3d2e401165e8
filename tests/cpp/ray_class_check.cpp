// crt_ray_class.h as a C function for tests/test_ray_sets.py (ctypes): the query kernels' ray
// classification, compiled for the host.
#include "crt_ray_class.h"

extern "C" int ray_class_traceable(const double* ray6, double t_max) {
    return crt::ray_traceable(ray6, ray6 + 3, t_max) ? 1 : 0;
}

extern "C" int ray_class_interval_open(double t_min, double t_max) { return crt::ray_interval_open(t_min, t_max) ? 1 : 0; }
