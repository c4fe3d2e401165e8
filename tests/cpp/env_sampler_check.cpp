// csrc/crt_env_sampler.h's env_weight, env_pdf and env_sample, the lines the sampler's build kernels
// and the NEE instances of the radiance kernels run, built for the host (-ffp-contract=off) behind C
// functions: tests/test_env_nee_model.py holds them to tests/env_nee_model.py's numpy restatement bit
// for bit. The tables' sums here are the build kernels' loops: sequential, from 0.0.
#include "crt_env_sampler.h"

extern "C" void env_tables_host(const crt_env* env, double* w, double* c, double* m) {
    const uint32_t n = env->face_size;
    double total = 0.0;
    for (uint32_t r = 0; r < 6 * n; ++r) {
        double sum = 0.0;
        for (uint32_t k = 0; k < n; ++k) {
            const size_t i = static_cast<size_t>(r) * n + k;
            w[i] = crt::env_weight(env->texels + 3 * i, k, r % n, n);
            sum = sum + w[i];
            c[i] = sum;
        }
        total = total + sum;
        m[r] = total;
    }
}

extern "C" void env_pdf_many(const crt_env* env, const double* w, const double* c, const double* m, double W,
                             const double* dirs, size_t count, double* out) {
    const crt::EnvTables tb{w, c, m, W};
    for (size_t i = 0; i < count; ++i) out[i] = crt::env_pdf(*env, tb, dirs + 3 * i);
}

extern "C" void env_sample_many(const crt_env* env, const double* w, const double* c, const double* m, double W,
                                const double* xi, size_t count, double* out) {
    const crt::EnvTables tb{w, c, m, W};
    for (size_t i = 0; i < count; ++i)
        crt::env_sample(*env, tb, xi[4 * i], xi[4 * i + 1], xi[4 * i + 2], xi[4 * i + 3], out + 3 * i);
}
