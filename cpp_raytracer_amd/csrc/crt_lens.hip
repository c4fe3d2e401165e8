// gfx950 lens renders: crt_lens_rays_async, crt_render_lens_async and crt_render_lens, and the lens
// renders in passes: crt_render_lens_pass_async, crt_lens_centre_rays_async, crt_lens_features_async
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
// The passes add four more, all around device_radiance / device_trace as well:
//   lens_list_{count,scan,write}_kernel  the pixels of the 16x4 blocks whose word equals the pass's first
//                       sample, compacted into a row-major list (ballots and a prefix sum, no atomics;
//                       the order of the list decides no bit: every listed pixel is reduced on its own)
//   lens_accumulate_kernel / lens_accumulate_serial_kernel  accumulate_kernel's additions
//                       (crt_device.hip) of one pass into the running sum, the noise state and the
//                       frame so far: one wave a pixel with the pass's chunk sums in LDS
//                       (lens_reduce_kernel's scheme) for a pass of more than 64 samples, one thread
//                       a pixel below that
//   lens_skip_kernel    one wave a block: a skipped block's pixels as accumulate_masked_kernel leaves
//                       them, a rendered block's word set to the pass's end
//   lens_centre_rays_kernel / lens_feature_kernel  the ray through every pixel's centre, and
//                       crt_feature records from the crt_hit records device_trace gives for them
// The host side cuts the frame into batches of whole pixels in row-major order whose scratch (rays,
// radiance, states: 76 bytes a record) is a buffer kept per device (LensScratch); nothing is carried between batches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <limits>
#include <mutex>
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

// The ray of the kinds other than PINHOLE through frame position (fx, fy) of face `face` (0 unless
// CUBE): crt_lens_rays_async's expressions from a and b on.
template <uint32_t KIND>
__device__ __forceinline__ void project(const LensView& V, uint32_t face, double fx, double fy, double o[3],
                                        double d[3]) {
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

// Records [0, n) of a batch that starts at pixel `first` (row-major in the whole frame): record r is
// sample s0 + r % ns of pixel first + r / ns. LISTED (a masked pass): of pixel list[first + r / ns].
template <uint32_t KIND, bool LISTED>
__global__ __launch_bounds__(256) void lens_rays_kernel(LensView V, uint64_t first, uint32_t n, uint32_t s0,
                                                        uint32_t ns, const uint32_t* __restrict__ list,
                                                        double* __restrict__ rays, uint32_t* __restrict__ states) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint64_t pixel = LISTED ? list[first + r / ns] : first + r / ns;
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
        project<KIND>(V, face, fx, fy, o, d);
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

// list == nullptr: the batch's pixels are first, first + 1, ...; else list[first], list[first + 1], ...
static hipError_t launch_rays(const LensView& V, uint32_t kind, uint64_t first, uint32_t records, uint32_t s0,
                              uint32_t ns, double* d_rays, uint32_t* d_states, hipStream_t st,
                              const uint32_t* list = nullptr) {
    const dim3 grid((records + 255) / 256), block(256);
#define CRT_LENS_LAUNCH(KIND)                                                                                        \
    if (list)                                                                                                        \
        hipLaunchKernelGGL((lens_rays_kernel<KIND, true>), grid, block, 0, st, V, first, records, s0, ns, list, d_rays, \
                           d_states);                                                                                \
    else                                                                                                             \
        hipLaunchKernelGGL((lens_rays_kernel<KIND, false>), grid, block, 0, st, V, first, records, s0, ns, list, d_rays, \
                           d_states);                                                                                \
    break
    switch (kind) {
        case CRT_LENS_PINHOLE: CRT_LENS_LAUNCH(CRT_LENS_PINHOLE);
        case CRT_LENS_ORTHOGRAPHIC: CRT_LENS_LAUNCH(CRT_LENS_ORTHOGRAPHIC);
        case CRT_LENS_EQUIRECT: CRT_LENS_LAUNCH(CRT_LENS_EQUIRECT);
        case CRT_LENS_FISHEYE: CRT_LENS_LAUNCH(CRT_LENS_FISHEYE);
        default: CRT_LENS_LAUNCH(CRT_LENS_CUBE);
    }
#undef CRT_LENS_LAUNCH
    return hipGetLastError();
}

// ---- lens renders in passes ---------------------------------------------------------------------
// Blocks are the frame's 16 x 4 blocks (crt_block_count's numbering over the whole frame).
__device__ __forceinline__ uint32_t block_of(uint32_t row, uint32_t col, uint32_t tiles_x) {
    return (row / CRT_BLOCK_H) * tiles_x + col / CRT_BLOCK_W;
}

// The pixels (row * w + col) of the blocks whose word equals `first`, compacted in row-major order in
// three launches, without atomics: list[0] = their number, list[1 + i] = the i-th one, so a pass in
// which every block is active traces its pixels in the order of a pass without blocks.
//   lens_list_count_kernel   a thread block takes kListThreads consecutive pixels: every wave counts its
//                            active ones with a ballot, thread 0 adds the waves' counts: seg[block]
//   lens_list_scan_kernel    one thread block: seg[] to its exclusive prefix sums, kListThreads
//                            segments a round (Hillis-Steele in LDS), the total to list[0]
//   lens_list_write_kernel   the count kernel's ballots again; a lane writes at its segment's offset +
//                            the counts of the waves before its own + the set bits below it
// (A first version reserved list entries with one integer atomic a wave or a block; its list came in
// the atomics' order, and the radiance kernel ran 13 % slower on it than on row-major pixels.)
constexpr uint32_t kListThreads = 1024;
__device__ __forceinline__ bool pixel_active(const uint32_t* __restrict__ blocks, uint32_t p, uint32_t pixels, uint32_t w,
                                             uint32_t tiles_x, uint32_t first) {
    return p < pixels && blocks[block_of(p / w, p % w, tiles_x)] == first;
}

__global__ __launch_bounds__(kListThreads) void lens_list_count_kernel(const uint32_t* __restrict__ blocks, uint32_t w,
                                                                       uint32_t pixels, uint32_t tiles_x, uint32_t first,
                                                                       uint32_t* __restrict__ seg) {
    __shared__ uint32_t wave_count[kListThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(pixel_active(blocks, blockIdx.x * kListThreads + threadIdx.x, pixels, w, tiles_x, first));
    if (lane == 0) wave_count[wave] = static_cast<uint32_t>(__popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t v = 0; v < kListThreads / 64; ++v) all += wave_count[v];
        seg[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kListThreads) void lens_list_scan_kernel(uint32_t* __restrict__ seg, uint32_t nseg,
                                                                      uint32_t* __restrict__ list) {
    __shared__ uint32_t x[2][kListThreads];
    uint32_t base = 0;
    for (uint32_t s0 = 0; s0 < nseg; s0 += kListThreads) {
        const uint32_t i = s0 + threadIdx.x;
        const uint32_t own = i < nseg ? seg[i] : 0;
        uint32_t cur = 0;
        x[0][threadIdx.x] = own;
        __syncthreads();
        for (uint32_t d = 1; d < kListThreads; d <<= 1) {  // inclusive sums, ping-pong
            const uint32_t v = x[cur][threadIdx.x] + (threadIdx.x >= d ? x[cur][threadIdx.x - d] : 0);
            x[cur ^ 1][threadIdx.x] = v;
            cur ^= 1;
            __syncthreads();
        }
        if (i < nseg) seg[i] = base + x[cur][threadIdx.x] - own;
        base += x[cur][kListThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) list[0] = base;
}

__global__ __launch_bounds__(kListThreads) void lens_list_write_kernel(const uint32_t* __restrict__ blocks, uint32_t w,
                                                                       uint32_t pixels, uint32_t tiles_x, uint32_t first,
                                                                       const uint32_t* __restrict__ seg,
                                                                       uint32_t* __restrict__ list) {
    __shared__ uint32_t wave_count[kListThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t p = blockIdx.x * kListThreads + threadIdx.x;
    const bool on = pixel_active(blocks, p, pixels, w, tiles_x, first);
    const uint64_t m = __ballot(on);
    if (lane == 0) wave_count[wave] = static_cast<uint32_t>(__popcll(m));
    __syncthreads();
    if (on) {
        uint32_t before = 0;
        for (uint32_t v = 0; v < wave; ++v) before += wave_count[v];
        const uint32_t below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                         __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
        list[1 + seg[blockIdx.x] + before + below] = p;
    }
}

// accumulate_kernel's additions (crt_device.hip) for one pixel of one pass, in chunk order: a fresh
// pass (first sample 0) starts the running sum from chunk 0's sum and t, q from 0, any other from the
// stored values; every full-length chunk adds y = (r + g) + b and y * y to t and q; out = sum * inv_done.
struct PixelAcc {
    double r, g, b, t, q;
    __device__ __forceinline__ void start(bool fresh, const double* __restrict__ sum, const double* __restrict__ noise,
                                          size_t pix) {
        r = g = b = t = q = 0;
        if (fresh) return;  // chunk 0 sets r, g, b
        r = sum[pix * 3 + 0];
        g = sum[pix * 3 + 1];
        b = sum[pix * 3 + 2];
        if (noise) {
            t = noise[pix * 2 + 0];
            q = noise[pix * 2 + 1];
        }
    }
    __device__ __forceinline__ void chunk(uint32_t c, bool fresh, bool full, double pr, double pg, double pb) {
        if (c > 0 || !fresh) {
            r = r + pr;
            g = g + pg;
            b = b + pb;
        } else {
            r = pr;
            g = pg;
            b = pb;
        }
        if (full) {
            const double y = (pr + pg) + pb;
            t = t + y;
            q = q + y * y;
        }
    }
    __device__ __forceinline__ void store(double* __restrict__ sum, double* __restrict__ noise, double* __restrict__ out,
                                          size_t pix, double inv_done) const {
        sum[pix * 3 + 0] = r;
        sum[pix * 3 + 1] = g;
        sum[pix * 3 + 2] = b;
        if (noise) {
            noise[pix * 2 + 0] = t;
            noise[pix * 2 + 1] = q;
        }
        if (out) {
            out[pix * 3 + 0] = r * inv_done;
            out[pix * 3 + 1] = g * inv_done;
            out[pix * 3 + 2] = b * inv_done;
        }
    }
};

// The sum of samples [s0, s1) of a pixel's records px in sample order from 0.0 (px == nullptr: every
// record is +0, max_depth == 0).
__device__ __forceinline__ void chunk_sum(const double* __restrict__ px, uint32_t s0, uint32_t s1, double u[3]) {
    u[0] = u[1] = u[2] = 0.0;
    for (uint32_t s = s0; s < s1; ++s) {
        const double* q = px + 3 * static_cast<size_t>(s);
        u[0] = u[0] + (px ? q[0] : 0.0);
        u[1] = u[1] + (px ? q[1] : 0.0);
        u[2] = u[2] + (px ? q[2] : 0.0);
    }
}

// A pass of many samples: one wave a pixel of the batch, pixels [0, count): frame pixel
// list[first + i] (list == nullptr: first + i), whose ns records of this pass start at
// rgb + 3 * i * ns. lens_reduce_kernel's scheme: lane l sums the pass's chunks l, l + 64, l + 128
// into the wave's LDS row; lane 0 then makes PixelAcc's additions in chunk order.
__global__ __launch_bounds__(64 * kWavesPerBlock) void lens_accumulate_kernel(
    const double* __restrict__ rgb, const uint32_t* __restrict__ list, uint64_t first, uint32_t count, uint32_t ns,
    uint32_t L, bool fresh, double inv_done, double* __restrict__ sum, double* __restrict__ noise,
    double* __restrict__ out) {
    __shared__ double sums[kWavesPerBlock][kMaxChunks * 3];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * kWavesPerBlock + wave;
    const bool live = i < count;  // the whole wave
    const uint32_t chunks = (ns + L - 1) / L, full_chunks = ns / L;
    if (live) {
        const double* px = rgb ? rgb + 3 * (static_cast<size_t>(i) * ns) : nullptr;
        for (uint32_t c = lane; c < chunks; c += 64) {
            double u[3];
            chunk_sum(px, c * L, min(ns, (c + 1) * L), u);
            sums[wave][3 * c] = u[0];
            sums[wave][3 * c + 1] = u[1];
            sums[wave][3 * c + 2] = u[2];
        }
    }
    __syncthreads();
    if (!live || lane != 0) return;
    const size_t pix = list ? list[first + i] : first + i;
    PixelAcc a;
    a.start(fresh, sum, noise, pix);
    for (uint32_t c = 0; c < chunks; ++c)
        a.chunk(c, fresh, c < full_chunks, sums[wave][3 * c], sums[wave][3 * c + 1], sums[wave][3 * c + 2]);
    a.store(sum, noise, out, pix, inv_done);
}

// A pass of few samples (at most kSerialSamples: a preview pass is a chunk or a few): one thread a
// pixel makes the same additions in the same order, chunk after chunk, with no LDS. One wave a pixel
// keeps 2 lanes of 64 busy on a pass of two chunks and cost 1.1 ms a pass on a 2048 x 1024 frame.
constexpr uint32_t kSerialSamples = 64;
__global__ __launch_bounds__(256) void lens_accumulate_serial_kernel(
    const double* __restrict__ rgb, const uint32_t* __restrict__ list, uint64_t first, uint32_t count, uint32_t ns,
    uint32_t L, bool fresh, double inv_done, double* __restrict__ sum, double* __restrict__ noise,
    double* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const uint32_t chunks = (ns + L - 1) / L, full_chunks = ns / L;
    const double* px = rgb ? rgb + 3 * (static_cast<size_t>(i) * ns) : nullptr;
    const size_t pix = list ? list[first + i] : first + i;
    PixelAcc a;
    a.start(fresh, sum, noise, pix);
    for (uint32_t c = 0; c < chunks; ++c) {
        double u[3];
        chunk_sum(px, c * L, min(ns, (c + 1) * L), u);
        a.chunk(c, fresh, c < full_chunks, u[0], u[1], u[2]);
    }
    a.store(sum, noise, out, pix, inv_done);
}

// One wave a block of a masked pass, lane = block pixel. A block whose word is not `first` was
// skipped, and its pixels get what accumulate_masked_kernel (crt_device.hip) gives them: a pass from
// sample 0 zeroes sum, noise and out; a later one leaves sum and noise alone and writes out = sum *
// (1 / (double)n), n = the block's own count (0 when n = 0). A rendered block's word becomes `end`
// (lane 0 alone touches the word; its pixels are lens_accumulate_kernel's). Launched behind the list
// kernel, which reads the words as they were.
__global__ __launch_bounds__(256) void lens_skip_kernel(uint32_t* __restrict__ blocks, uint32_t nblocks, uint32_t w,
                                                        uint32_t h, uint32_t tiles_x, uint32_t first, uint32_t end,
                                                        double* __restrict__ sum, double* __restrict__ noise,
                                                        double* __restrict__ out) {
    const uint32_t blk = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (blk >= nblocks) return;  // the whole wave
    uint32_t word = 0;
    if (lane == 0) word = blocks[blk];
    word = __shfl(word, 0);
    if (word == first) {
        if (lane == 0) blocks[blk] = end;
        return;
    }
    const uint32_t col = (blk % tiles_x) * CRT_BLOCK_W + lane % CRT_BLOCK_W;
    const uint32_t row = (blk / tiles_x) * CRT_BLOCK_H + lane / CRT_BLOCK_W;
    if (col >= w || row >= h) return;
    const size_t pix = static_cast<size_t>(row) * w + col;
    if (first == 0) {
        sum[pix * 3 + 0] = 0;
        sum[pix * 3 + 1] = 0;
        sum[pix * 3 + 2] = 0;
        if (noise) {
            noise[pix * 2 + 0] = 0;
            noise[pix * 2 + 1] = 0;
        }
        if (out) {
            out[pix * 3 + 0] = 0;
            out[pix * 3 + 1] = 0;
            out[pix * 3 + 2] = 0;
        }
    } else if (out) {
        const uint32_t n = word & ~CRT_BLOCK_STOPPED;
        const double inv = 1 / static_cast<double>(n);
        out[pix * 3 + 0] = n ? sum[pix * 3 + 0] * inv : 0.0;
        out[pix * 3 + 1] = n ? sum[pix * 3 + 1] * inv : 0.0;
        out[pix * 3 + 2] = n ? sum[pix * 3 + 2] * inv : 0.0;
    }
}

// The ray through the centre of pixel p = row * w + col, no draws: PINHOLE features_kernel's ray
// (crt_device.hip: the random terms left out, not multiplied by zero), every other kind
// lens_rays_kernel's with fx = col + 0.5 and fy = row_in_face + 0.5.
template <uint32_t KIND>
__global__ __launch_bounds__(256) void lens_centre_rays_kernel(LensView V, uint32_t pixels, double* __restrict__ rays) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    const uint32_t row = p / V.w, col = p % V.w;
    double o[3], d[3];
    if constexpr (KIND == CRT_LENS_PINHOLE) {
        const double fr = static_cast<double>(row), fc = static_cast<double>(col);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double center = (V.F[k] + V.U[k] * fr) + V.R[k] * fc;
            o[k] = V.O[k];
            d[k] = center - o[k];
        }
    } else {
        uint32_t rf = row, face = 0;
        if constexpr (KIND == CRT_LENS_CUBE) {
            face = row / V.w;
            rf = row % V.w;
        }
        project<KIND>(V, face, static_cast<double>(col) + 0.5, static_cast<double>(rf) + 0.5, o, d);
    }
    double* dst = rays + 6 * static_cast<size_t>(p);
    dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
    dst[3] = d[0]; dst[4] = d[1]; dst[5] = d[2];
}

// crt_feature records from the closest hits of the centre rays: t, point, normal, prim and material
// are the hit's; albedo and the miss record are features_kernel's (crt_device.hip).
__global__ __launch_bounds__(256) void lens_feature_kernel(const crt_hit* __restrict__ hits, uint32_t pixels,
                                                           const DevMaterial* __restrict__ mats, double bg0, double bg1,
                                                           double bg2, crt_feature* __restrict__ out) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= pixels) return;
    const crt_hit h = hits[p];
    crt_feature f{};
    f.prim = -1;
    if (h.prim >= 0) {
        const DevMaterial& m = mats[h.material];
        const bool glass = m.kind == CRT_DIELECTRIC;
        for (int j = 0; j < 3; ++j) {
            f.point[j] = h.point[j];
            f.normal[j] = h.normal[j];
            f.albedo[j] = glass ? 1.0 : m.color[j];
        }
        f.t = h.t;
        f.prim = h.prim;
        f.material = h.material;
    } else {
        f.albedo[0] = bg0;
        f.albedo[1] = bg1;
        f.albedo[2] = bg2;
    }
    out[p] = f;
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

// The batch scratch of the lens renders (rays, radiance, states): a buffer of the library's own, one kept per
// device and grown on demand, not a block of the stream-ordered pass pool. A whole-frame batch is larger than what
// the pool keeps reserved; the runtime then maps more memory into the pool for the call and gives it back after
// it (reserved 32 -> 64 -> 32 MiB at every call, whatever the release threshold), and the first accesses of the
// call's kernels to such a block went wrong on the MI355X: rays the generator had written were read as what the
// memory held before, for the first 1024 batches or so of the radiance kernel. Memory from
// hipMalloc showed none of it.
// take(): the kept buffer if it is large enough and no other call holds it, after the work of its last user (an
// event, waited for on the caller's stream); else a fresh allocation. give(): records the event and keeps the
// buffer, or, for a fresh one, keeps it in place of a smaller kept one (which is freed once its last user is
// done) or frees it once the stream is done (two calls at once on one device: rare, and it blocks).
struct LensScratch {
    std::mutex mu;
    char* ptr = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool held = false;
};
static LensScratch g_lens_scratch[kMaxDevices];

static hipError_t lens_scratch_take(int device, size_t bytes, hipStream_t st, char** out) {
    LensScratch& c = g_lens_scratch[device];
    {
        std::lock_guard<std::mutex> lk(c.mu);
        if (c.ptr && c.bytes >= bytes && !c.held) {
            const hipError_t e = hipStreamWaitEvent(st, c.done, 0);
            if (e != hipSuccess) return e;
            c.held = true;
            *out = c.ptr;
            return hipSuccess;
        }
    }
    return hipMalloc(reinterpret_cast<void**>(out), bytes);
}

static void lens_scratch_give(int device, char* p, size_t bytes, hipStream_t st) {
    LensScratch& c = g_lens_scratch[device];
    std::unique_lock<std::mutex> lk(c.mu);
    if (p == c.ptr) {
        (void)hipEventRecord(c.done, st);
        c.held = false;
        return;
    }
    if (!c.held && bytes > c.bytes) {  // the fresh buffer takes the kept one's place
        char* old = c.ptr;
        hipEvent_t ev = c.done;
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
        if (ev) {
            if (old) (void)hipEventSynchronize(ev);
            (void)hipEventRecord(ev, st);
            c.ptr = p;
            c.bytes = bytes;
            c.done = ev;
            lk.unlock();
            if (old) (void)hipFree(old);
            return;
        }
    }
    lk.unlock();
    (void)hipStreamSynchronize(st);
    (void)hipFree(p);
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

int device_render_lens(const crt_scene* s, int device, const crt_camera* cam, const crt_lens* lens, const crt_env* env,
                       double* d_rgb, void* stream, const crt_env_sampler* smp, const crt_light_sampler* lights) {
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
        HIP_TRY(lens_scratch_take(device, records * (48 + 24 + 4), st, &scratch));
        double* rays = reinterpret_cast<double*>(scratch);
        double* rgb = reinterpret_cast<double*>(scratch + records * 48);
        uint32_t* states = reinterpret_cast<uint32_t*>(scratch + records * (48 + 24));
        hipError_t e = ln::launch_rays(V, lens->kind, first, static_cast<uint32_t>(records), 0, spp, rays, states, st);
        if (e == hipSuccess) rc = device_radiance(s, device, rays, records, states, &rp, env, rgb, st, smp, lights);
        if (e == hipSuccess && rc == CRT_OK) {
            const dim3 grid((count + ln::kWavesPerBlock - 1) / ln::kWavesPerBlock), block(64 * ln::kWavesPerBlock);
            hipLaunchKernelGGL(ln::lens_reduce_kernel, grid, block, 0, st, rgb, count, spp, L, inv_spp, d_rgb + first * 3);
            e = hipGetLastError();
        }
        lens_scratch_give(device, scratch, records * (48 + 24 + 4), st);
        if (e != hipSuccess) return fail(CRT_E_HIP, std::string("lens kernels: ") + hipGetErrorString(e));
        if (rc) return rc;
    }
    return CRT_OK;
}

// crt_render_lens_pass_async: samples [first, first + count) of the whole frame (d_blocks == nullptr)
// or of the pixels of the blocks whose word equals `first`, in batches of whole pixels as
// device_render_lens's: generate, trace, accumulate, free. A masked pass lists its pixels first and
// waits for `stream` once to read their number (the radiance query needs its record count on the host).
// env, smp and lights are device_radiance's (crt_render_lens_pass_lit_async); all null: none.
int device_render_lens_pass(const crt_scene* s, int device, const crt_camera* cam, const crt_lens* lens, uint32_t first,
                            uint32_t count, double* d_sum, double* d_noise, double* d_rgb, uint32_t* d_blocks,
                            void* stream, const crt_env* env, const crt_env_sampler* smp, const crt_light_sampler* lights) {
    int rc = device_check(device);
    if (rc) return rc;
    if (!s->dev[device].valid)
        return fail(CRT_E_NOT_UPLOADED, "scene not uploaded to device " + std::to_string(device));
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint64_t pixels = static_cast<uint64_t>(cam->image_w) * cam->image_h;
    void* pool_v = nullptr;
    rc = device_pass_pool(device, &pool_v);
    if (rc) return rc;
    hipMemPool_t pool = static_cast<hipMemPool_t>(pool_v);
    const uint32_t L = sample_chunk_len(cam->samples_per_pixel), end = first + count;
    const double inv_done = 1 / static_cast<double>(end);
    const bool fresh = first == 0;
    uint32_t* list = nullptr;
    uint64_t todo = pixels;
    if (d_blocks) {
        const uint32_t tiles_x = (cam->image_w + CRT_BLOCK_W - 1) / CRT_BLOCK_W;
        const uint32_t nblocks = static_cast<uint32_t>(crt_block_count(cam->image_w, cam->image_h));
        // one allocation: the count and the list, then the segments' counts / offsets
        const uint32_t nseg = static_cast<uint32_t>((pixels + ln::kListThreads - 1) / ln::kListThreads);
        HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&list), (pixels + 1 + nseg) * sizeof(uint32_t), pool, st));
        uint32_t* seg = list + pixels + 1;
        const uint32_t npx = static_cast<uint32_t>(pixels);
        hipLaunchKernelGGL(ln::lens_list_count_kernel, dim3(nseg), dim3(ln::kListThreads), 0, st, d_blocks, cam->image_w, npx,
                           tiles_x, first, seg);
        hipLaunchKernelGGL(ln::lens_list_scan_kernel, dim3(1), dim3(ln::kListThreads), 0, st, seg, nseg, list);
        hipLaunchKernelGGL(ln::lens_list_write_kernel, dim3(nseg), dim3(ln::kListThreads), 0, st, d_blocks, cam->image_w, npx,
                           tiles_x, first, seg, list);
        hipLaunchKernelGGL(ln::lens_skip_kernel, dim3((nblocks + 3) / 4), dim3(256), 0, st, d_blocks, nblocks,
                           cam->image_w, cam->image_h, tiles_x, first, end, d_sum, d_noise, d_rgb);
        hipError_t e = hipGetLastError();
        uint32_t active = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&active, list, sizeof active, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) {
            (void)hipFreeAsync(list, st);
            return fail(CRT_E_HIP, std::string("lens pass: the active pixel list: ") + hipGetErrorString(e));
        }
        todo = active;
    }
    crt_radiance_params rp{};
    rp.max_depth = cam->max_depth;
    rp.base_seed = cam->base_seed;  // unused: every path has a state
    for (int k = 0; k < 3; ++k) rp.background[k] = cam->background[k];
    rp.t_min = cam->t_min;
    rp.flags = lens->flags;
    const ln::LensView V = ln::lens_view(cam, lens);
    const bool trace = cam->max_depth != 0;  // else every path is +0 (crt_radiance_async): nothing to trace
    const uint64_t per_batch = trace ? lens_batch_size(lens, count) : std::max<uint64_t>(todo, 1);
    const uint32_t* entries = list ? list + 1 : nullptr;
    for (uint64_t at = 0; at < todo && rc == CRT_OK; at += per_batch) {
        const uint32_t n = static_cast<uint32_t>(std::min<uint64_t>(per_batch, todo - at));
        const size_t records = static_cast<size_t>(n) * count;
        char* scratch = nullptr;
        double* rgb = nullptr;
        hipError_t e = hipSuccess;
        if (trace) {  // one allocation: the rays, the radiance, then the states
            e = lens_scratch_take(device, records * (48 + 24 + 4), st, &scratch);
            if (e == hipSuccess) {
                double* rays = reinterpret_cast<double*>(scratch);
                rgb = reinterpret_cast<double*>(scratch + records * 48);
                uint32_t* states = reinterpret_cast<uint32_t*>(scratch + records * (48 + 24));
                e = ln::launch_rays(V, lens->kind, at, static_cast<uint32_t>(records), first, count, rays, states, st, entries);
                if (e == hipSuccess) rc = device_radiance(s, device, rays, records, states, &rp, env, rgb, st, smp, lights);
            }
        }
        if (e == hipSuccess && rc == CRT_OK) {
            if (count <= ln::kSerialSamples) {
                hipLaunchKernelGGL(ln::lens_accumulate_serial_kernel, dim3((n + 255) / 256), dim3(256), 0, st, rgb, entries, at,
                                   n, count, L, fresh, inv_done, d_sum, d_noise, d_rgb);
            } else {
                const dim3 grid((n + ln::kWavesPerBlock - 1) / ln::kWavesPerBlock), block(64 * ln::kWavesPerBlock);
                hipLaunchKernelGGL(ln::lens_accumulate_kernel, grid, block, 0, st, rgb, entries, at, n, count, L, fresh,
                                   inv_done, d_sum, d_noise, d_rgb);
            }
            e = hipGetLastError();
        }
        if (scratch) lens_scratch_give(device, scratch, records * (48 + 24 + 4), st);
        if (e != hipSuccess) rc = fail(CRT_E_HIP, std::string("lens pass kernels: ") + hipGetErrorString(e));
    }
    if (list) (void)hipFreeAsync(list, st);
    return rc;
}

static hipError_t launch_centre_rays(const ln::LensView& V, uint32_t kind, uint32_t pixels, double* d_rays, hipStream_t st) {
    const dim3 grid((pixels + 255) / 256), block(256);
    switch (kind) {
        case CRT_LENS_PINHOLE:
            hipLaunchKernelGGL(ln::lens_centre_rays_kernel<CRT_LENS_PINHOLE>, grid, block, 0, st, V, pixels, d_rays);
            break;
        case CRT_LENS_ORTHOGRAPHIC:
            hipLaunchKernelGGL(ln::lens_centre_rays_kernel<CRT_LENS_ORTHOGRAPHIC>, grid, block, 0, st, V, pixels, d_rays);
            break;
        case CRT_LENS_EQUIRECT:
            hipLaunchKernelGGL(ln::lens_centre_rays_kernel<CRT_LENS_EQUIRECT>, grid, block, 0, st, V, pixels, d_rays);
            break;
        case CRT_LENS_FISHEYE:
            hipLaunchKernelGGL(ln::lens_centre_rays_kernel<CRT_LENS_FISHEYE>, grid, block, 0, st, V, pixels, d_rays);
            break;
        default:
            hipLaunchKernelGGL(ln::lens_centre_rays_kernel<CRT_LENS_CUBE>, grid, block, 0, st, V, pixels, d_rays);
            break;
    }
    return hipGetLastError();
}

int device_lens_centre_rays(int device, const crt_camera* cam, const crt_lens* lens, double* d_rays, void* stream) {
    const int rc = device_check(device);
    if (rc) return rc;
    DeviceGuard g(device);
    const uint32_t pixels = cam->image_w * cam->image_h;
    const hipError_t e = launch_centre_rays(ln::lens_view(cam, lens), lens->kind, pixels, d_rays, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("lens_centre_rays_kernel launch: ") + hipGetErrorString(e));
    return CRT_OK;
}

// crt_lens_features_async: the centre rays, crt_trace_async's closest hits over (t_min, +inf), then
// the records; rays and hits (120 bytes a pixel) come from the pass pool
int device_lens_features(const crt_scene* s, int device, const crt_camera* cam, const crt_lens* lens, crt_feature* d_feat,
                         void* stream) {
    int rc = device_check(device);
    if (rc) return rc;
    if (!s->dev[device].valid)
        return fail(CRT_E_NOT_UPLOADED, "scene not uploaded to device " + std::to_string(device));
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t pixels = cam->image_w * cam->image_h;
    void* pool_v = nullptr;
    rc = device_pass_pool(device, &pool_v);
    if (rc) return rc;
    char* scratch = nullptr;
    HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&scratch), static_cast<size_t>(pixels) * (48 + sizeof(crt_hit)),
                                   static_cast<hipMemPool_t>(pool_v), st));
    double* rays = reinterpret_cast<double*>(scratch);
    crt_hit* hits = reinterpret_cast<crt_hit*>(scratch + static_cast<size_t>(pixels) * 48);
    crt_trace_params tp{};
    tp.t_min = cam->t_min;
    tp.t_max = std::numeric_limits<double>::infinity();
    hipError_t e = launch_centre_rays(ln::lens_view(cam, lens), lens->kind, pixels, rays, st);
    if (e == hipSuccess) rc = device_trace(s, device, rays, pixels, nullptr, &tp, hits, nullptr, st);
    if (e == hipSuccess && rc == CRT_OK) {
        hipLaunchKernelGGL(ln::lens_feature_kernel, dim3((pixels + 255) / 256), dim3(256), 0, st, hits, pixels,
                           s->dev[device].mats, cam->background[0], cam->background[1], cam->background[2], d_feat);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(scratch, st);
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("lens feature kernels: ") + hipGetErrorString(e));
    return rc;
}

// crt_render_lens: device_render_lens for a host array, blocking: the render on a stream of its
// own, one copy back. env (null: none) has its texels in host memory here: uploaded for the call,
// freed after it. sampled: once the texels have arrived a sampler is built on them (blocking), the
// render goes through it, and it is freed with them. lights: a light sampler of the uploaded scene
// is built for the call (crt_render_lens_lights, crt_render_lens_lit) and freed after it
int device_render_lens_host(crt_scene* s, int device, const crt_camera* cam, const crt_lens* lens, const crt_env* env,
                            double* rgb, bool sampled, bool lights) {
    int rc = device_upload(s, device);
    if (rc) return rc;
    DeviceGuard g(device);
    const size_t bytes = static_cast<size_t>(cam->image_w) * cam->image_h * 3 * sizeof(double);
    double* d_rgb = nullptr;
    double* d_texels = nullptr;
    crt_env d_env{};
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreate(&st);
    if (e == hipSuccess) e = hipMalloc(&d_rgb, bytes);
    if (e == hipSuccess && env) {
        const size_t env_bytes = size_t{6} * env->face_size * env->face_size * 3 * sizeof(double);
        d_env = *env;
        e = hipMalloc(&d_texels, env_bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(d_texels, env->texels, env_bytes, hipMemcpyHostToDevice, st);
        d_env.texels = d_texels;
    }
    crt_env_sampler* smp = nullptr;
    if (e == hipSuccess && env && sampled) {
        e = hipStreamSynchronize(st);
        if (e == hipSuccess) rc = device_env_sampler_create(device, &d_env, &smp);
    }
    crt_light_sampler* lsmp = nullptr;
    if (e == hipSuccess && rc == CRT_OK && lights) rc = device_light_sampler_create(s, device, &lsmp);
    if (e == hipSuccess && rc == CRT_OK) rc = device_render_lens(s, device, cam, lens, env ? &d_env : nullptr, d_rgb, st, smp, lsmp);
    if (e == hipSuccess && rc == CRT_OK) e = hipMemcpyAsync(rgb, d_rgb, bytes, hipMemcpyDeviceToHost, st);
    if (st) {
        const hipError_t se = hipStreamSynchronize(st);
        if (e == hipSuccess) e = se;
        (void)hipStreamDestroy(st);
    }
    (void)device_env_sampler_free(smp);
    (void)device_light_sampler_free(lsmp);
    (void)hipFree(d_rgb);
    (void)hipFree(d_texels);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("crt_render_lens: ") + hipGetErrorString(e));
    return CRT_OK;
}

}  // namespace crt
