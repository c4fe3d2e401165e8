// gfx950 lens renders: crt_lens_rays_async, crt_render_lens_async and crt_render_lens
// (include/crt_render.h states every expression and its order; this file evaluates exactly those,
// in IEEE f64 with -ffp-contract=off, so tests/lens_model.py's numpy restatement gives the same
// bits up to the device library's sin and cos). Two small kernels around device_radiance, which
// traces the generated rays unchanged:
//   lens_rays_kernel    one thread a record r = (pixel - first) * ns + (s - s0): the state
//                       crt_sample_seed(base_seed, row * w + col, s), the kind's draws (PINHOLE:
//                       start_path's, crt_device.hip; the others: the two jitter draws), the ray and
//                       the state after the draws
//   lens_reduce_kernel  one wave a pixel: lane l sums whole chunks l, l + 64, l + 128 of
//                       crt_sample_chunk_len(spp) samples, each in sample order from 0.0, into LDS;
//                       lane 0 adds the chunk sums in chunk order and writes the sum times 1 / spp:
//                       crt_render_async's order. No atomics, so the bits are the same for any grid
//                       and any batch.
// The host side cuts the frame into batches of whole pixels in row-major order whose scratch (rays,
// radiance, states: 76 bytes a record) comes from the pass pool; nothing is carried between batches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "crt_internal.h"
#include "crt_hip_util.h"

#pragma clang fp contract(off)

namespace crt {

namespace ln {

constexpr double kScale = 1 / static_cast<double>(4294967295u - 1);  // rand_util.h:110-112
constexpr uint32_t kWavesPerBlock = 4;                               // lens_reduce_kernel: one pixel a wave
constexpr uint32_t kMaxChunks = 192;                                 // crt_sample_chunk_len: ceil(spp / L) <= 192

// crt_device.hip's sample_seed (crt_sample_seed)
__device__ __forceinline__ uint32_t sample_seed(uint32_t base, uint32_t pixel, uint32_t sample) {
    uint64_t z = (static_cast<uint64_t>(pixel) << 32) | sample;
    z += static_cast<uint64_t>(base) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return static_cast<uint32_t>(z ^ (z >> 32));
}

// crt_device.hip's rnd (crt_rand_double) and rnd_pm1 (rand_double(s, -1, 1) bit for bit)
__device__ __forceinline__ double rnd(uint32_t& s, double lo, double hi) {
    s = 1664525u * s + 1013904223u;
    return lo + (hi - lo) * static_cast<double>(s) * kScale;
}
__device__ __forceinline__ double rnd_pm1(uint32_t& s) {
    s = 1664525u * s + 1013904223u;
    return static_cast<double>(s) * (2 * kScale) + -1.0;
}

// What the generator reads. PINHOLE: the camera's own vectors (R = pixel_delta_x, U = pixel_delta_y,
// F = pixel00, ddx / ddy = the defocus disk); every other kind: the caller's basis and extents.
struct LensView {
    double O[3], R[3], U[3], F[3];
    double ddx[3], ddy[3];
    double defocus_angle;
    double ex, ey;
    double sx, sy;  // 2.0 / (double)w, 2.0 / (double)h_face
    uint32_t w, base_seed;
};

// Records [0, n) of a batch that starts at pixel `first` (row-major in the whole frame): record r is
// sample s0 + r % ns of pixel first + r / ns.
template <uint32_t KIND>
__global__ __launch_bounds__(256) void lens_rays_kernel(LensView V, uint64_t first, uint32_t n, uint32_t s0,
                                                        uint32_t ns, double* __restrict__ rays,
                                                        uint32_t* __restrict__ states) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint64_t pixel = first + r / ns;
    const uint32_t s = s0 + r % ns;
    const uint32_t row = static_cast<uint32_t>(pixel / V.w), col = static_cast<uint32_t>(pixel % V.w);
    uint32_t rng = sample_seed(V.base_seed, row * V.w + col, s);
    double o[3], d[3];
    if constexpr (KIND == CRT_LENS_PINHOLE) {  // start_path (crt_device.hip), random_ray_through_pixel
        if (V.defocus_angle <= 0) {
            o[0] = V.O[0]; o[1] = V.O[1]; o[2] = V.O[2];
        } else {
            double vx, vy;
            do {
                vx = rnd_pm1(rng);
                vy = rnd_pm1(rng);
            } while (!(vx * vx + vy * vy + 0.0 * 0.0 < 1));
            o[0] = (V.O[0] + V.ddx[0] * vx) + V.ddy[0] * vy;
            o[1] = (V.O[1] + V.ddx[1] * vx) + V.ddy[1] * vy;
            o[2] = (V.O[2] + V.ddx[2] * vx) + V.ddy[2] * vy;
        }
        const double fr = static_cast<double>(row), fc = static_cast<double>(col);
        const double uy = rnd(rng, -0.5, 0.5);
        const double ux = rnd(rng, -0.5, 0.5);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double center = (V.F[k] + V.U[k] * fr) + V.R[k] * fc;
            const double sample = (center + V.R[k] * ux) + V.U[k] * uy;
            d[k] = sample - o[k];
        }
    } else {
        uint32_t rf = row, face = 0;
        if constexpr (KIND == CRT_LENS_CUBE) {
            face = row / V.w;
            rf = row % V.w;
        }
        const double uy = rnd(rng, -0.5, 0.5);
        const double ux = rnd(rng, -0.5, 0.5);
        const double fx = (static_cast<double>(col) + 0.5) + ux;
        const double fy = (static_cast<double>(rf) + 0.5) + uy;
        const double a = fx * V.sx - 1.0;
        const double b = 1.0 - fy * V.sy;
        o[0] = V.O[0]; o[1] = V.O[1]; o[2] = V.O[2];
        if constexpr (KIND == CRT_LENS_ORTHOGRAPHIC) {
            const double ax = a * V.ex, by = b * V.ey;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                o[k] = (V.O[k] + V.R[k] * ax) + V.U[k] * by;
                d[k] = V.F[k];
            }
        } else if constexpr (KIND == CRT_LENS_EQUIRECT) {
            const double phi = a * V.ex, theta = b * V.ey;
            const double ct = cos(theta), st = sin(theta);
            const double x = ct * sin(phi), z = ct * cos(phi);
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = (V.R[k] * x + V.U[k] * st) + V.F[k] * z;
        } else if constexpr (KIND == CRT_LENS_FISHEYE) {
            const double px = a * V.ex, py = b * V.ey;
            const double psi = sqrt(px * px + py * py);
            const double kk = psi == 0 ? 1.0 : sin(psi) / psi;
            const double x = px * kk, y = py * kk, z = cos(psi);
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = (V.R[k] * x + V.U[k] * y) + V.F[k] * z;
        } else {  // CUBE: the face table, v pointing down the image
            const double u = a, v = -b;
            double x, y, z;
            switch (face) {
                case 0: x = 1.0; y = -v; z = -u; break;   // +X
                case 1: x = -1.0; y = -v; z = u; break;   // -X
                case 2: x = u; y = 1.0; z = v; break;     // +Y
                case 3: x = u; y = -1.0; z = -v; break;   // -Y
                case 4: x = u; y = -v; z = 1.0; break;    // +Z
                default: x = -u; y = -v; z = -1.0; break; // -Z
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = (V.R[k] * x + V.U[k] * y) + V.F[k] * z;
        }
    }
    double* dst = rays + 6 * static_cast<size_t>(r);
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    dst[3] = d[0]; dst[4] = d[1]; dst[5] = d[2];
    states[r] = rng;
}

// One wave a pixel of the batch: pixels [0, count) of rgb (spp records each) into out[pixel][j].
// Lane l sums chunks l, l + 64, l + 128 (each its samples in order from 0.0) into the wave's LDS
// row; lane 0 then adds the chunk sums in chunk order.
__global__ __launch_bounds__(64 * kWavesPerBlock) void lens_reduce_kernel(const double* __restrict__ rgb,
                                                                          uint32_t count, uint32_t spp, uint32_t L,
                                                                          double inv_spp, double* __restrict__ out) {
    __shared__ double sums[kWavesPerBlock][kMaxChunks * 3];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t pixel = blockIdx.x * kWavesPerBlock + wave;
    const bool live = pixel < count;  // the whole wave
    const uint32_t chunks = (spp + L - 1) / L;
    if (live) {
        const double* px = rgb + 3 * (static_cast<size_t>(pixel) * spp);
        for (uint32_t c = lane; c < chunks; c += 64) {
            const uint32_t s1 = min(spp, (c + 1) * L);
            double u0 = 0.0, u1 = 0.0, u2 = 0.0;
            for (uint32_t s = c * L; s < s1; ++s) {
                const double* q = px + 3 * static_cast<size_t>(s);
                u0 = u0 + q[0];
                u1 = u1 + q[1];
                u2 = u2 + q[2];
            }
            sums[wave][3 * c] = u0;
            sums[wave][3 * c + 1] = u1;
            sums[wave][3 * c + 2] = u2;
        }
    }
    __syncthreads();
    if (live && lane == 0) {
        double t0 = sums[wave][0], t1 = sums[wave][1], t2 = sums[wave][2];
        for (uint32_t c = 1; c < chunks; ++c) {
            t0 = t0 + sums[wave][3 * c];
            t1 = t1 + sums[wave][3 * c + 1];
            t2 = t2 + sums[wave][3 * c + 2];
        }
        double* dst = out + 3 * static_cast<size_t>(pixel);
        dst[0] = t0 * inv_spp;
        dst[1] = t1 * inv_spp;
        dst[2] = t2 * inv_spp;
    }
}

static LensView lens_view(const crt_camera* cam, const crt_lens* lens) {
    LensView v{};
    const bool pinhole = lens->kind == CRT_LENS_PINHOLE;
    for (int k = 0; k < 3; ++k) {
        v.O[k] = pinhole ? cam->origin[k] : lens->origin[k];
        v.R[k] = pinhole ? cam->pixel_delta_x[k] : lens->right[k];
        v.U[k] = pinhole ? cam->pixel_delta_y[k] : lens->up[k];
        v.F[k] = pinhole ? cam->pixel00[k] : lens->forward[k];
        v.ddx[k] = cam->defocus_disk_x[k];
        v.ddy[k] = cam->defocus_disk_y[k];
    }
    v.defocus_angle = cam->defocus_angle;
    v.ex = lens->extent_x;
    v.ey = lens->extent_y;
    v.sx = 2.0 / static_cast<double>(cam->image_w);
    v.sy = 2.0 / static_cast<double>(lens->kind == CRT_LENS_CUBE ? cam->image_w : cam->image_h);
    v.w = cam->image_w;
    v.base_seed = cam->base_seed;
    return v;
}

static hipError_t launch_rays(const LensView& V, uint32_t kind, uint64_t first, uint32_t records, uint32_t s0,
                              uint32_t ns, double* d_rays, uint32_t* d_states, hipStream_t st) {
    const dim3 grid((records + 255) / 256), block(256);
    switch (kind) {
        case CRT_LENS_PINHOLE:
            hipLaunchKernelGGL(lens_rays_kernel<CRT_LENS_PINHOLE>, grid, block, 0, st, V, first, records, s0, ns, d_rays, d_states);
            break;
        case CRT_LENS_ORTHOGRAPHIC:
            hipLaunchKernelGGL(lens_rays_kernel<CRT_LENS_ORTHOGRAPHIC>, grid, block, 0, st, V, first, records, s0, ns, d_rays, d_states);
            break;
        case CRT_LENS_EQUIRECT:
            hipLaunchKernelGGL(lens_rays_kernel<CRT_LENS_EQUIRECT>, grid, block, 0, st, V, first, records, s0, ns, d_rays, d_states);
            break;
        case CRT_LENS_FISHEYE:
            hipLaunchKernelGGL(lens_rays_kernel<CRT_LENS_FISHEYE>, grid, block, 0, st, V, first, records, s0, ns, d_rays, d_states);
            break;
        default:
            hipLaunchKernelGGL(lens_rays_kernel<CRT_LENS_CUBE>, grid, block, 0, st, V, first, records, s0, ns, d_rays, d_states);
            break;
    }
    return hipGetLastError();
}

}  // namespace ln

// pixels a batch may hold: the caller's batch_pixels, or the most whose scratch stays at or under
// 256 MiB; never fewer than one, never more than 2^31 - 1 records (spp <= 2^31 - 1 is checked)
static uint64_t lens_batch_size(const crt_lens* lens, uint64_t spp) {
    constexpr uint64_t kRecordBytes = 48 + 4 + 24, kBudget = 256ull << 20;
    uint64_t b = lens->batch_pixels ? lens->batch_pixels : kBudget / (kRecordBytes * spp);
    b = std::min<uint64_t>(b, 0x7fffffffull / spp);
    return std::max<uint64_t>(b, 1);
}

int device_lens_rays(int device, const crt_camera* cam, const crt_lens* lens, uint32_t first_sample,
                     uint32_t num_samples, double* d_rays, uint32_t* d_states, void* stream) {
    const int rc = device_check(device);
    if (rc) return rc;
    const uint64_t records = static_cast<uint64_t>(cam->image_w) * cam->image_h * num_samples;
    if (records == 0) return CRT_OK;
    DeviceGuard g(device);
    const hipError_t e = ln::launch_rays(ln::lens_view(cam, lens), lens->kind, 0, static_cast<uint32_t>(records),
                                         first_sample, num_samples, d_rays, d_states, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("lens_rays_kernel launch: ") + hipGetErrorString(e));
    return CRT_OK;
}

int device_render_lens(const crt_scene* s, int device, const crt_camera* cam, const crt_lens* lens, double* d_rgb,
                       void* stream) {
    int rc = device_check(device);
    if (rc) return rc;
    if (!s->dev[device].valid)
        return fail(CRT_E_NOT_UPLOADED, "scene not uploaded to device " + std::to_string(device));
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t pixels = static_cast<uint64_t>(cam->image_w) * cam->image_h;
    if (cam->max_depth == 0) {  // every path is +0 (crt_radiance_async): so is every pixel
        HIP_TRY(hipMemsetAsync(d_rgb, 0, pixels * 3 * sizeof(double), st));
        return CRT_OK;
    }
    void* pool_v = nullptr;
    rc = device_pass_pool(device, &pool_v);
    if (rc) return rc;
    hipMemPool_t pool = static_cast<hipMemPool_t>(pool_v);
    crt_radiance_params rp{};
    rp.max_depth = cam->max_depth;
    rp.base_seed = cam->base_seed;  // unused: every path has a state
    for (int k = 0; k < 3; ++k) rp.background[k] = cam->background[k];
    rp.t_min = cam->t_min;
    rp.flags = lens->flags;
    const ln::LensView V = ln::lens_view(cam, lens);
    const uint32_t spp = cam->samples_per_pixel, L = sample_chunk_len(spp);
    const double inv_spp = 1 / static_cast<double>(spp);
    const uint64_t per_batch = lens_batch_size(lens, spp);
    for (uint64_t first = 0; first < pixels; first += per_batch) {
        const uint32_t count = static_cast<uint32_t>(std::min<uint64_t>(per_batch, pixels - first));
        const size_t records = static_cast<size_t>(count) * spp;
        // one allocation: the rays, the radiance, then the states
        char* scratch = nullptr;
        HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&scratch), records * (48 + 24 + 4), pool, st));
        double* rays = reinterpret_cast<double*>(scratch);
        double* rgb = reinterpret_cast<double*>(scratch + records * 48);
        uint32_t* states = reinterpret_cast<uint32_t*>(scratch + records * (48 + 24));
        hipError_t e = ln::launch_rays(V, lens->kind, first, static_cast<uint32_t>(records), 0, spp, rays, states, st);
        if (e == hipSuccess) rc = device_radiance(s, device, rays, records, states, &rp, rgb, st);
        if (e == hipSuccess && rc == CRT_OK) {
            const dim3 grid((count + ln::kWavesPerBlock - 1) / ln::kWavesPerBlock), block(64 * ln::kWavesPerBlock);
            hipLaunchKernelGGL(ln::lens_reduce_kernel, grid, block, 0, st, rgb, count, spp, L, inv_spp, d_rgb + first * 3);
            e = hipGetLastError();
        }
        (void)hipFreeAsync(scratch, st);
        if (e != hipSuccess) return fail(CRT_E_HIP, std::string("lens kernels: ") + hipGetErrorString(e));
        if (rc) return rc;
    }
    return CRT_OK;
}

// crt_render_lens: device_render_lens for a host array, blocking: the render on a stream of its
// own, one copy back
int device_render_lens_host(crt_scene* s, int device, const crt_camera* cam, const crt_lens* lens, double* rgb) {
    int rc = device_upload(s, device);
    if (rc) return rc;
    DeviceGuard g(device);
    const size_t bytes = static_cast<size_t>(cam->image_w) * cam->image_h * 3 * sizeof(double);
    double* d_rgb = nullptr;
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreate(&st);
    if (e == hipSuccess) e = hipMalloc(&d_rgb, bytes);
    if (e == hipSuccess) rc = device_render_lens(s, device, cam, lens, d_rgb, st);
    if (e == hipSuccess && rc == CRT_OK) e = hipMemcpyAsync(rgb, d_rgb, bytes, hipMemcpyDeviceToHost, st);
    if (st) {
        const hipError_t se = hipStreamSynchronize(st);
        if (e == hipSuccess) e = se;
        (void)hipStreamDestroy(st);
    }
    (void)hipFree(d_rgb);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("crt_render_lens: ") + hipGetErrorString(e));
    return CRT_OK;
}

}  // namespace crt
