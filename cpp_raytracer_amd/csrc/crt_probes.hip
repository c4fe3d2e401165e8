// gfx950 irradiance probes: crt_probes_async, crt_probe_rays_async and crt_sh_eval_async
// (include/crt_render.h states every expression and its order; this file evaluates exactly those,
// in IEEE f64 with -ffp-contract=off, so tests/probe_model.py's numpy restatement gives the same
// bits). Two small kernels around device_radiance, which traces the generated rays unchanged:
//   probe_rays_kernel    one thread a record r = p * S + s: the state crt_sample_seed(base_seed, p, s),
//                        Vec3D::random_unit_vector on it (shade's draw, IEEE sqrt and division), the
//                        ray {P, u} or {P, N + u}, and the state after the draws
//   probe_reduce_kernel  one wave a probe: lane l sums the terms Y_k(d_s) * L_s[j] of samples
//                        s = l, l + 64, ... in order, then a cross-lane tree over steps 32 .. 1; lane 0
//                        writes the sum times W / S. No atomics, so the order is the documented one
//                        for any grid and any batch.
// The host side cuts the probes into batches of whole probes whose scratch (rays, states, radiance:
// 76 bytes a record) comes from the pass pool; nothing is carried between batches.
// sh_eval_kernel evaluates stored coefficients, one thread a query.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "crt_internal.h"
#include "crt_hip_util.h"

#pragma clang fp contract(off)

namespace crt {

namespace pb {

constexpr double kScale = 1 / static_cast<double>(4294967295u - 1);  // rand_util.h:110-112
constexpr uint32_t kWavesPerBlock = 4;                               // probe_reduce_kernel: one probe a wave

// crt_device.hip's sample_seed (crt_sample_seed)
__device__ __forceinline__ uint32_t sample_seed(uint32_t base, uint32_t pixel, uint32_t sample) {
    uint64_t z = (static_cast<uint64_t>(pixel) << 32) | sample;
    z += static_cast<uint64_t>(base) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return static_cast<uint32_t>(z ^ (z >> 32));
}

// crt_device.hip's rnd_pm1: rand_double(s, -1, 1) bit for bit ((1 - -1) * x is exact, and
// RN(2x * kScale) = RN(x * (2 kScale)))
__device__ __forceinline__ double rnd_pm1(uint32_t& s) {
    s = 1664525u * s + 1013904223u;
    return static_cast<double>(s) * (2 * kScale) + -1.0;
}

// Vec3D::random_unit_vector (vec3d.h:64-75) as crt_device.hip's non-FAST instance draws it:
// rejection in the cube, then * (1 / sqrt(|v|^2)) with the IEEE sqrt and division
__device__ __forceinline__ void random_unit_vector(uint32_t& s, double& x, double& y, double& z) {
    double m2;
    do {
        x = rnd_pm1(s);
        y = rnd_pm1(s);
        z = rnd_pm1(s);
        m2 = x * x + y * y + z * z;
    } while (!(m2 < 1));
    const double inv = 1 / sqrt(x * x + y * y + z * z);
    x = x * inv;
    y = y * inv;
    z = z * inv;
}

// Records [0, n) of a batch that starts at probe `first`: record r is sample r % S of probe
// first + r / S. points / normals are the caller's whole arrays (normals null: SPHERE).
__global__ __launch_bounds__(256) void probe_rays_kernel(const double* __restrict__ points,
                                                         const double* __restrict__ normals, uint32_t first,
                                                         uint32_t n, uint32_t S, uint32_t base_seed,
                                                         double* __restrict__ rays, uint32_t* __restrict__ states) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint32_t p = first + r / S, s = r % S;
    uint32_t rng = sample_seed(base_seed, p, s);
    double u[3];
    random_unit_vector(rng, u[0], u[1], u[2]);
    double* out = rays + 6 * static_cast<size_t>(r);
    for (int k = 0; k < 3; ++k) {
        out[k] = points[3 * static_cast<size_t>(p) + k];
        out[3 + k] = normals ? normals[3 * static_cast<size_t>(p) + k] + u[k] : u[k];
    }
    states[r] = rng;
}

// The real SH basis of bands 0..2 at the direction (x, y, z), in crt_probes_async's order
__device__ __forceinline__ void sh_basis(double x, double y, double z, double Y[9]) {
    Y[0] = 0.28209479177387814;
    Y[1] = 0.4886025119029199 * y;
    Y[2] = 0.4886025119029199 * z;
    Y[3] = 0.4886025119029199 * x;
    Y[4] = 1.0925484305920792 * (x * y);
    Y[5] = 1.0925484305920792 * (y * z);
    Y[6] = 0.31539156525252005 * ((3.0 * z) * z - 1.0);
    Y[7] = 1.0925484305920792 * (x * z);
    Y[8] = 0.5462742152960396 * (x * x - y * y);
}

// One wave a probe of the batch: probes [0, count) of rays / rgb (S records each) into
// coeff[probe][k][j]. SH: nine coefficients a channel; otherwise the single term Y = 1, used
// without a multiply. A lane without samples stays 0.0.
template <bool SH>
__global__ __launch_bounds__(64 * kWavesPerBlock) void probe_reduce_kernel(const double* __restrict__ rays,
                                                                           const double* __restrict__ rgb,
                                                                           uint32_t count, uint32_t S, double scale,
                                                                           double* __restrict__ coeff) {
    constexpr int K = SH ? 9 : 1;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t probe = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (probe >= count) return;  // the whole wave
    double acc[K][3];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[k][j] = 0.0;
    const size_t base = static_cast<size_t>(probe) * S;
    for (uint32_t s = lane; s < S; s += 64) {
        const double* L = rgb + 3 * (base + s);
        const double L0 = L[0], L1 = L[1], L2 = L[2];
        if constexpr (SH) {
            const double* d = rays + 6 * (base + s) + 3;
            double Y[9];
            sh_basis(d[0], d[1], d[2], Y);
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                acc[k][0] = acc[k][0] + Y[k] * L0;
                acc[k][1] = acc[k][1] + Y[k] * L1;
                acc[k][2] = acc[k][2] + Y[k] * L2;
            }
        } else {
            acc[0][0] = acc[0][0] + L0;
            acc[0][1] = acc[0][1] + L1;
            acc[0][2] = acc[0][2] + L2;
        }
    }
    // lane l < step becomes lane[l] + lane[l + step]; the lanes at or above step compute values
    // nobody reads
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1)
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[k][j] = acc[k][j] + __shfl_down(acc[k][j], step, 64);
    if (lane == 0) {
        double* out = coeff + static_cast<size_t>(probe) * (K * 3);
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < 3; ++j) out[3 * k + j] = acc[k][j] * scale;
    }
}

// crt_sh_eval_async: query i reads probe index[i]'s 9 x 3 coefficients; band weights A (all 1 for
// radiance)
__global__ __launch_bounds__(256) void sh_eval_kernel(const double* __restrict__ coeff, uint64_t num_probes,
                                                      const uint32_t* __restrict__ index,
                                                      const double* __restrict__ dirs, uint32_t m, double a0,
                                                      double a1, double a2, double* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double r[3] = {0.0, 0.0, 0.0};
    const uint32_t p = index[i];
    if (p < num_probes) {
        const double* d = dirs + 3 * static_cast<size_t>(i);
        const double* c = coeff + 27 * static_cast<size_t>(p);
        double Y[9];
        sh_basis(d[0], d[1], d[2], Y);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const double a = k == 0 ? a0 : (k < 4 ? a1 : a2);
#pragma unroll
            for (int j = 0; j < 3; ++j) r[j] = r[j] + a * (c[3 * k + j] * Y[k]);
        }
    }
    for (int j = 0; j < 3; ++j) out[3 * static_cast<size_t>(i) + j] = r[j];
}

static hipError_t launch_rays(const double* d_points, const double* d_normals, uint32_t first, uint32_t records,
                              const crt_probe_params* prm, double* d_rays, uint32_t* d_states, hipStream_t st) {
    hipLaunchKernelGGL(probe_rays_kernel, dim3((records + 255) / 256), dim3(256), 0, st, d_points,
                       prm->mode == CRT_PROBE_HEMISPHERE ? d_normals : nullptr, first, records, prm->samples,
                       prm->base_seed, d_rays, d_states);
    return hipGetLastError();
}

}  // namespace pb

// probes a batch may hold: the caller's batch_probes, or the most whose scratch stays at or under
// 256 MiB; never fewer than one, never more than 2^31 - 1 records
static uint64_t batch_size(const crt_probe_params* prm) {
    constexpr uint64_t kRecordBytes = 48 + 4 + 24, kBudget = 256ull << 20;
    uint64_t b = prm->batch_probes ? prm->batch_probes : kBudget / (kRecordBytes * prm->samples);
    b = std::min<uint64_t>(b, 0x7fffffffull / prm->samples);
    return std::max<uint64_t>(b, 1);
}

int device_probe_rays(int device, const double* d_points, const double* d_normals, size_t n,
                      const crt_probe_params* prm, double* d_rays, uint32_t* d_states, void* stream) {
    const int rc = device_check(device);
    if (rc) return rc;
    if (n == 0) return CRT_OK;
    DeviceGuard g(device);
    const hipError_t e = pb::launch_rays(d_points, d_normals, 0, static_cast<uint32_t>(n * prm->samples), prm, d_rays,
                                         d_states, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("probe_rays_kernel launch: ") + hipGetErrorString(e));
    return CRT_OK;
}

int device_probes(const crt_scene* s, int device, const double* d_points, const double* d_normals, size_t n,
                  const crt_probe_params* prm, const crt_env* env, double* d_coeff, void* stream,
                  const crt_env_sampler* smp, const crt_light_sampler* lights) {
    int rc = device_check(device);
    if (rc) return rc;
    if (!s->dev[device].valid)
        return fail(CRT_E_NOT_UPLOADED, "scene not uploaded to device " + std::to_string(device));
    if (n == 0) return CRT_OK;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool sh = prm->mode == CRT_PROBE_SPHERE;
    const size_t K = sh ? 9 : 1;
    if (prm->max_depth == 0) {  // every path is +0 (crt_radiance_async): so is every sum
        HIP_TRY(hipMemsetAsync(d_coeff, 0, n * K * 3 * sizeof(double), st));
        return CRT_OK;
    }
    void* pool_v = nullptr;
    rc = device_pass_pool(device, &pool_v);
    if (rc) return rc;
    hipMemPool_t pool = static_cast<hipMemPool_t>(pool_v);
    crt_radiance_params rp{};
    rp.max_depth = prm->max_depth;
    rp.base_seed = prm->base_seed;  // unused: every path has a state
    for (int k = 0; k < 3; ++k) rp.background[k] = prm->background[k];
    rp.t_min = prm->t_min;
    rp.flags = prm->flags;
    const double scale = (sh ? 12.566370614359172 : 3.141592653589793) / static_cast<double>(prm->samples);
    const uint64_t S = prm->samples, per_batch = batch_size(prm);
    for (uint64_t first = 0; first < n; first += per_batch) {
        const uint32_t count = static_cast<uint32_t>(std::min<uint64_t>(per_batch, n - first));
        const size_t records = static_cast<size_t>(count * S);
        // one allocation: the rays, the radiance, then the states
        char* scratch = nullptr;
        HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&scratch), records * (48 + 24 + 4), pool, st));
        double* rays = reinterpret_cast<double*>(scratch);
        double* rgb = reinterpret_cast<double*>(scratch + records * 48);
        uint32_t* states = reinterpret_cast<uint32_t*>(scratch + records * (48 + 24));
        hipError_t e = pb::launch_rays(d_points, d_normals, static_cast<uint32_t>(first), static_cast<uint32_t>(records),
                                       prm, rays, states, st);
        if (e == hipSuccess) rc = device_radiance(s, device, rays, records, states, &rp, env, rgb, st, smp, lights);
        if (e == hipSuccess && rc == CRT_OK) {
            const dim3 grid((count + pb::kWavesPerBlock - 1) / pb::kWavesPerBlock), block(64 * pb::kWavesPerBlock);
            double* out = d_coeff + first * K * 3;
            if (sh)
                hipLaunchKernelGGL(pb::probe_reduce_kernel<true>, grid, block, 0, st, rays, rgb, count, prm->samples, scale, out);
            else
                hipLaunchKernelGGL(pb::probe_reduce_kernel<false>, grid, block, 0, st, rays, rgb, count, prm->samples, scale, out);
            e = hipGetLastError();
        }
        (void)hipFreeAsync(scratch, st);
        if (e != hipSuccess) return fail(CRT_E_HIP, std::string("probe kernels: ") + hipGetErrorString(e));
        if (rc) return rc;
    }
    return CRT_OK;
}

// crt_probes: device_probes for host arrays, blocking: one upload of the points (and normals), the
// bake on a stream of its own, one copy back
int device_probes_host(crt_scene* s, int device, const double* points, const double* normals, size_t n,
                       const crt_probe_params* prm, double* coeff) {
    int rc = device_upload(s, device);
    if (rc) return rc;
    DeviceGuard g(device);
    const size_t in_bytes = n * 3 * sizeof(double);
    const size_t out_bytes = n * (prm->mode == CRT_PROBE_SPHERE ? 9 : 1) * 3 * sizeof(double);
    double *d_points = nullptr, *d_normals = nullptr, *d_coeff = nullptr;
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreate(&st);
    if (e == hipSuccess) e = hipMalloc(&d_points, in_bytes);
    if (e == hipSuccess && normals) e = hipMalloc(&d_normals, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&d_coeff, out_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_points, points, in_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && normals) e = hipMemcpyAsync(d_normals, normals, in_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) rc = device_probes(s, device, d_points, d_normals, n, prm, nullptr, d_coeff, st);
    if (e == hipSuccess && rc == CRT_OK) e = hipMemcpyAsync(coeff, d_coeff, out_bytes, hipMemcpyDeviceToHost, st);
    if (st) {
        const hipError_t se = hipStreamSynchronize(st);
        if (e == hipSuccess) e = se;
        (void)hipStreamDestroy(st);
    }
    (void)hipFree(d_points);
    (void)hipFree(d_normals);
    (void)hipFree(d_coeff);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("crt_probes: ") + hipGetErrorString(e));
    return CRT_OK;
}

int device_sh_eval(int device, const double* d_coeff, size_t num_probes, const uint32_t* d_index,
                   const double* d_dirs, size_t m, uint32_t what, double* d_rgb, void* stream) {
    const int rc = device_check(device);
    if (rc) return rc;
    if (m == 0) return CRT_OK;
    DeviceGuard g(device);
    const bool irr = what == CRT_SH_IRRADIANCE;
    hipLaunchKernelGGL(pb::sh_eval_kernel, dim3((static_cast<uint32_t>(m) + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_coeff, static_cast<uint64_t>(num_probes), d_index, d_dirs, static_cast<uint32_t>(m),
                       irr ? CRT_SH_A0 : 1.0, irr ? CRT_SH_A1 : 1.0, irr ? CRT_SH_A2 : 1.0, d_rgb);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("sh_eval_kernel launch: ") + hipGetErrorString(e));
    return CRT_OK;
}

}  // namespace crt
