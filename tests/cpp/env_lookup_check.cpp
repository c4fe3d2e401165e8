// csrc/crt_env.h's env_lookup, the lines the radiance kernels run, built for the host
// (-ffp-contract=off) behind one C function: tests/test_env_abi.py holds it to tests/env_model.py's
// numpy restatement bit for bit.
#include "crt_env.h"

extern "C" void env_lookup_many(const crt_env* env, const double* dirs, size_t n, const double* bg, double* out) {
    for (size_t i = 0; i < n; ++i) crt::env_lookup(*env, dirs + 3 * i, bg, out + 3 * i);
}

extern "C" unsigned env_sizeof(void) { return sizeof(crt_env); }
