// gfx950 build of a crt_env_sampler's tables (include/crt_render.h states every expression and its
// order; crt_env_sampler.h holds the per-texel one). The sums are sequential by contract and the
// build is not a hot path: one thread a row for w and c, one thread for m.
//   env_rows_kernel      thread r < 6n: w[r][k] = env_weight(texel), c[r][k] = c[r][k - 1] + w[r][k]
//   env_marginal_kernel  one thread: m[r] = m[r - 1] + c[r][n - 1]
#include <hip/hip_runtime.h>

#define CRT_HD __host__ __device__ __forceinline__

#include <cmath>
#include <cstdint>
#include <string>

#include "crt_internal.h"
#include "crt_hip_util.h"
#include "crt_env_sampler.h"

#pragma clang fp contract(off)

namespace crt {

namespace es {

__global__ __launch_bounds__(64) void env_rows_kernel(const double* __restrict__ texels, uint32_t n,
                                                      double* __restrict__ w, double* __restrict__ c) {
    const uint32_t r = blockIdx.x * 64 + threadIdx.x;
    if (r >= 6 * n) return;
    const size_t base = static_cast<size_t>(r) * n;
    const uint32_t rf = r % n;
    double sum = 0.0;
    for (uint32_t k = 0; k < n; ++k) {
        const double* t = texels + (base + k) * 3;
        const double rgb[3] = {t[0], t[1], t[2]};
        const double wk = env_weight(rgb, k, rf, n);
        sum = sum + wk;
        w[base + k] = wk;
        c[base + k] = sum;
    }
}

__global__ void env_marginal_kernel(const double* __restrict__ c, uint32_t n, double* __restrict__ m) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double sum = 0.0;
    for (uint32_t r = 0; r < 6 * n; ++r) {
        sum = sum + c[static_cast<size_t>(r) * n + (n - 1)];
        m[r] = sum;
    }
}

}  // namespace es

int device_env_sampler_free(crt_env_sampler* smp) {
    if (!smp) return CRT_OK;
    {
        DeviceGuard g(smp->device);
        (void)hipFree(smp->w);  // w, c and m are one allocation
    }
    delete smp;
    return CRT_OK;
}

int device_env_sampler_create(int device, const crt_env* env, crt_env_sampler** out) {
    const int rc = device_check(device);
    if (rc) return rc;
    DeviceGuard g(device);
    const uint32_t n = env->face_size;
    const size_t cells = size_t{6} * n * n, rows = size_t{6} * n;
    double* base = nullptr;
    HIP_TRY(hipMalloc(&base, (2 * cells + rows) * sizeof(double)));
    crt_env_sampler* smp = new crt_env_sampler{device, *env, base, base + cells, base + 2 * cells, 0.0};
    hipLaunchKernelGGL(es::env_rows_kernel, dim3((static_cast<uint32_t>(rows) + 63) / 64), dim3(64), 0, nullptr,
                       env->texels, n, smp->w, smp->c);
    hipLaunchKernelGGL(es::env_marginal_kernel, dim3(1), dim3(1), 0, nullptr, smp->c, n, smp->m);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(&smp->W, smp->m + (rows - 1), sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        (void)device_env_sampler_free(smp);
        return fail(CRT_E_HIP, std::string("crt_env_sampler_create: ") + hipGetErrorString(e));
    }
    if (!(smp->W > 0 && smp->W < INFINITY)) {
        (void)device_env_sampler_free(smp);
        return fail(CRT_E_INVALID, "crt_env_sampler_create: the map's total weight W must be positive and finite");
    }
    *out = smp;
    return CRT_OK;
}

}  // namespace crt
