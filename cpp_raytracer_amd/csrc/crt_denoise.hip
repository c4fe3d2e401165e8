// gfx950 denoiser: the edge-stopping a-trous filter of crt_denoise_async (include/crt_render.h
// states every expression and its order; this file evaluates exactly those, in IEEE f64 with
// -ffp-contract=off, so tests/denoise_model.py's numpy restatement gives the same bits). The
// blocking driver crt_render_denoised is in crt_drivers.hip.
//
// One iteration is one launch of filter_kernel over 32 x 8 pixel tiles, one thread per pixel.
// Before the first, pack_kernel packs the inputs into the two records the taps read: the state
// (c0, c1, c2, v; 32 bytes, ping-pong between iterations) and the guide (normal, point, t, prim;
// 64 bytes, constant), so a tap is three aligned 32-byte reads instead of reads of three arrays
// with 24-, 8- and 88-byte records. The two stages are also callable on their own
// (device_denoise_pack, device_denoise_filter): crt_render_denoised_devices packs on every device
// over its own rows and filters the gathered records on device 0.
// Two tap routes, one arithmetic (filter_pixel, instantiated over the route's reader):
//   LDS     the tile and its halo of 2 * step pixels staged in LDS as planes of doubles (a lane's
//           neighbour is the next double: ds_read_b64 without bank conflicts); for the steps whose
//           tile fits 64 KB (1 and 2: 38 and 56 KB)
//   gather  every tap read from global memory (L2 / Infinity Cache): the larger steps, whose halo
//           would be most of the tile
// CRT_DENOISE_ROUTE=gather | lds forces one route wherever it exists (tests, tools/denoise_gain.py).
#include <hip/hip_runtime.h>

#define CRT_HD __host__ __device__ __forceinline__

#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "crt_internal.h"
#include "crt_hip_util.h"

#pragma clang fp contract(off)

namespace crt {

namespace dn {

constexpr int kTileW = 32, kTileH = 8;           // pixels per block: one thread each
constexpr int kPlanes = 11;                      // c0 c1 c2 v n0 n1 n2 P0 P1 P2 prim
constexpr size_t kLdsLimit = 64 * 1024;          // the LDS route's tile (with halo) must fit this

struct alignas(16) State {  // the filtered signal of one pixel
    double c[3];
    double v;
};
struct alignas(16) Guide {  // what steers the weights: constant over the iterations
    double n[3];
    double P[3];
    double t;
    long long prim;
};
static_assert(sizeof(State) == 32 && sizeof(Guide) == 64, "tap records");

struct Params {
    int w, h, step;
    uint32_t squarings;
    double sl2;  // sigma_l * sigma_l
    double sp2;  // sigma_p * sigma_p
};

__device__ __forceinline__ bool finite(double x) {
    return (static_cast<unsigned long long>(__double_as_longlong(x)) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// state and guide are packed separately (a render's guide is constant, its state changes with every
// pass): either output may be null, and then its inputs are not read. Linear in the pixel index, so
// it packs a whole frame or a lane's packed owned rows alike.
__global__ __launch_bounds__(256) void pack_kernel(const double* __restrict__ rgb, const double* __restrict__ var,
                                                   const crt_feature* __restrict__ feat, uint32_t n,
                                                   State* __restrict__ state, Guide* __restrict__ guide) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (state) {
        State s;
        for (int j = 0; j < 3; ++j) s.c[j] = rgb[3 * static_cast<size_t>(i) + j];
        s.v = var[i];
        state[i] = s;
    }
    if (guide) {
        Guide g;
        for (int j = 0; j < 3; ++j) {
            g.n[j] = feat[i].normal[j];
            g.P[j] = feat[i].point[j];
        }
        g.t = feat[i].t;
        g.prim = feat[i].prim;
        guide[i] = g;
    }
}

// reader of the gather route: frame coordinates -> global memory
struct GlobalTaps {
    const State* state;
    const Guide* guide;
    int w;
    __device__ __forceinline__ State cv(int x, int y) const { return state[static_cast<size_t>(y) * w + x]; }
    __device__ __forceinline__ double v(int x, int y) const { return state[static_cast<size_t>(y) * w + x].v; }
    __device__ __forceinline__ long long prim(int x, int y) const { return guide[static_cast<size_t>(y) * w + x].prim; }
    __device__ __forceinline__ void geom(int x, int y, double n[3], double P[3]) const {
        const Guide& g = guide[static_cast<size_t>(y) * w + x];
        for (int j = 0; j < 3; ++j) {
            n[j] = g.n[j];
            P[j] = g.P[j];
        }
    }
};

// reader of the LDS route: frame coordinates -> the block's staged planes (x0, y0 = the frame
// coordinates of the tile's first staged pixel; lw * lh pixels per plane)
struct LdsTaps {
    const double* planes;
    int x0, y0, lw, np;
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * lw + (x - x0); }
    __device__ __forceinline__ State cv(int x, int y) const {
        const int i = at(x, y);
        State s;
        s.c[0] = planes[i];
        s.c[1] = planes[np + i];
        s.c[2] = planes[2 * np + i];
        s.v = planes[3 * np + i];
        return s;
    }
    __device__ __forceinline__ double v(int x, int y) const { return planes[3 * np + at(x, y)]; }
    __device__ __forceinline__ long long prim(int x, int y) const {
        return __double_as_longlong(planes[10 * np + at(x, y)]);
    }
    __device__ __forceinline__ void geom(int x, int y, double n[3], double P[3]) const {
        const int i = at(x, y);
        for (int j = 0; j < 3; ++j) {
            n[j] = planes[(4 + j) * np + i];
            P[j] = planes[(7 + j) * np + i];
        }
    }
};

// One pixel of one iteration: crt_denoise_async's expressions, in its order. gp = the pixel's guide.
template <typename Taps>
__device__ __forceinline__ State filter_pixel(const Taps& T, const Guide& gp, int x, int y, const Params& A) {
    const State p = T.cv(x, y);
    const double g[3] = {0.25, 0.5, 0.25};
    const double hk[5] = {1.0 / 16, 0.25, 3.0 / 8, 0.25, 1.0 / 16};
    double vbar = 0.0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = min(max(x + dx, 0), A.w - 1), qy = min(max(y + dy, 0), A.h - 1);
            vbar = vbar + (g[dy + 1] * g[dx + 1]) * T.v(qx, qy);
        }
    const double yp = (p.c[0] + p.c[1]) + p.c[2];
    const double D = A.sl2 * vbar + (1e-6 * (yp * yp) + DBL_MIN);
    const double bden = A.sp2 * (gp.t * gp.t);
    double W = 0.0, V = 0.0, C[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + A.step * dx, qy = y + A.step * dy;
            if (qx < 0 || qx >= A.w || qy < 0 || qy >= A.h) continue;
            const State q = T.cv(qx, qy);
            if (!(finite(q.c[0]) && finite(q.c[1]) && finite(q.c[2]) && finite(q.v))) continue;
            const long long pq = T.prim(qx, qy);
            if ((gp.prim < 0) != (pq < 0)) continue;
            double N = 1, b = 0;
            if (gp.prim >= 0) {
                double nq[3], Pq[3];
                T.geom(qx, qy, nq, Pq);
                const double nd = (gp.n[0] * nq[0] + gp.n[1] * nq[1]) + gp.n[2] * nq[2];
                N = nd > 0 ? nd : 0.0;
                for (uint32_t s = 0; s < A.squarings; ++s) N = N * N;
                const double e0 = Pq[0] - gp.P[0], e1 = Pq[1] - gp.P[1], e2 = Pq[2] - gp.P[2];
                const double e = (e0 * gp.n[0] + e1 * gp.n[1]) + e2 * gp.n[2];
                b = (e * e) / bden;
            }
            const double d = ((q.c[0] + q.c[1]) + q.c[2]) - yp;
            const double a = (d * d) / D;
            const double wt = (hk[dy + 2] * hk[dx + 2] * N) / ((1 + a) * (1 + b));
            W = W + wt;
            C[0] = C[0] + wt * q.c[0];
            C[1] = C[1] + wt * q.c[1];
            C[2] = C[2] + wt * q.c[2];
            V = V + (wt * wt) * q.v;
        }
    if (!(finite(p.c[0]) && finite(p.c[1]) && finite(p.c[2]) && finite(p.v)) || !(W > 0)) return p;
    State r;
    r.c[0] = C[0] / W;
    r.c[1] = C[1] / W;
    r.c[2] = C[2] / W;
    r.v = V / (W * W);
    return r;
}

// out_state: the next iteration's input, or null for the last iteration, which writes the
// caller's unpacked out_rgb / out_var (out_var may be null)
template <bool LDS>
__global__ __launch_bounds__(kTileW * kTileH) void filter_kernel(const State* __restrict__ in,
                                                                 const Guide* __restrict__ guide, Params A,
                                                                 State* __restrict__ out_state,
                                                                 double* __restrict__ out_rgb,
                                                                 double* __restrict__ out_var) {
    extern __shared__ __attribute__((aligned(16))) double planes[];
    const int tx = threadIdx.x % kTileW, ty = threadIdx.x / kTileW;
    const int x = blockIdx.x * kTileW + tx, y = blockIdx.y * kTileH + ty;
    const bool inside = x < A.w && y < A.h;
    State r;
    if constexpr (LDS) {
        const int R = 2 * A.step, lw = kTileW + 2 * R, lh = kTileH + 2 * R, np = lw * lh;
        const int x0 = static_cast<int>(blockIdx.x) * kTileW - R, y0 = static_cast<int>(blockIdx.y) * kTileH - R;
        for (int i = threadIdx.x; i < np; i += kTileW * kTileH) {
            const int gx = x0 + i % lw, gy = y0 + i / lw;
            State s{};
            Guide g{};
            if (gx >= 0 && gx < A.w && gy >= 0 && gy < A.h) {  // pixels off the frame are never read
                s = in[static_cast<size_t>(gy) * A.w + gx];
                g = guide[static_cast<size_t>(gy) * A.w + gx];
            }
            planes[i] = s.c[0];
            planes[np + i] = s.c[1];
            planes[2 * np + i] = s.c[2];
            planes[3 * np + i] = s.v;
            for (int j = 0; j < 3; ++j) {
                planes[(4 + j) * np + i] = g.n[j];
                planes[(7 + j) * np + i] = g.P[j];
            }
            planes[10 * np + i] = __longlong_as_double(g.prim);
        }
        __syncthreads();
        if (!inside) return;
        const LdsTaps T{planes, x0, y0, lw, np};
        r = filter_pixel(T, guide[static_cast<size_t>(y) * A.w + x], x, y, A);
    } else {
        if (!inside) return;
        const GlobalTaps T{in, guide, A.w};
        r = filter_pixel(T, guide[static_cast<size_t>(y) * A.w + x], x, y, A);
    }
    const size_t pix = static_cast<size_t>(y) * A.w + x;
    if (out_state) {
        out_state[pix] = r;
    } else {
        out_rgb[3 * pix + 0] = r.c[0];
        out_rgb[3 * pix + 1] = r.c[1];
        out_rgb[3 * pix + 2] = r.c[2];
        if (out_var) out_var[pix] = r.v;
    }
}

static size_t lds_bytes(int step) {
    const size_t R = 2 * static_cast<size_t>(step);
    return (kTileW + 2 * R) * (kTileH + 2 * R) * kPlanes * sizeof(double);
}

// the route of a step: LDS where the staged tile fits (CRT_DENOISE_ROUTE=gather: never)
static bool lds_route(int step) {
    const char* e = std::getenv("CRT_DENOISE_ROUTE");
    if (e && std::strcmp(e, "gather") == 0) return false;
    return lds_bytes(step) <= kLdsLimit;
}

}  // namespace dn

static_assert(sizeof(dn::State) == kDenoiseStateBytes && sizeof(dn::Guide) == kDenoiseGuideBytes, "record sizes");

static int check_frame(uint32_t w, uint32_t h) {
    const uint64_t n64 = static_cast<uint64_t>(w) * h;
    if (n64 >= 0x7fffffffull || w > 0x3fffffffu || h > 0x3fffffffu)
        return fail(CRT_E_INVALID, "crt_denoise_async: frame has more than 2^31-2 pixels");
    return CRT_OK;
}

static hipError_t launch_pack(uint32_t n, const double* d_rgb, const double* d_var, const crt_feature* d_feat,
                              dn::State* state, dn::Guide* guide, hipStream_t st) {
    hipLaunchKernelGGL(dn::pack_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d_rgb, d_var, d_feat, n, state, guide);
    return hipGetLastError();
}

static hipError_t launch_filter(uint32_t w, uint32_t h, dn::State* const state[2], const dn::Guide* guide,
                                const crt_denoise_params* prm, double* d_out, double* d_var_out, hipStream_t st) {
    hipError_t e = hipSuccess;
    const dim3 grid((w + dn::kTileW - 1) / dn::kTileW, (h + dn::kTileH - 1) / dn::kTileH);
    for (uint32_t i = 0; i < prm->iterations && e == hipSuccess; ++i) {
        const bool last = i + 1 == prm->iterations;
        dn::Params A{static_cast<int>(w), static_cast<int>(h), 1 << i, prm->normal_squarings,
                     prm->sigma_l * prm->sigma_l, prm->sigma_p * prm->sigma_p};
        dn::State* out = last ? nullptr : state[(i + 1) & 1];
        if (dn::lds_route(A.step))
            hipLaunchKernelGGL(dn::filter_kernel<true>, grid, dim3(dn::kTileW * dn::kTileH), dn::lds_bytes(A.step), st,
                               state[i & 1], guide, A, out, d_out, d_var_out);
        else
            hipLaunchKernelGGL(dn::filter_kernel<false>, grid, dim3(dn::kTileW * dn::kTileH), 0, st, state[i & 1], guide,
                               A, out, d_out, d_var_out);
        e = hipGetLastError();
    }
    return e;
}

int device_denoise_pack(int device, uint64_t pixels, const double* d_rgb, const double* d_var,
                        const crt_feature* d_feat, void* d_state, void* d_guide, void* stream) {
    const int rc = device_check(device);
    if (rc) return rc;
    if (pixels == 0 || (!d_state && !d_guide)) return CRT_OK;
    if (pixels >= 0x7fffffffull) return fail(CRT_E_INVALID, "denoise pack: more than 2^31-2 pixels");
    DeviceGuard g(device);
    const hipError_t e = launch_pack(static_cast<uint32_t>(pixels), d_rgb, d_var, d_feat, static_cast<dn::State*>(d_state),
                                     static_cast<dn::Guide*>(d_guide), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("denoise pack_kernel launch: ") + hipGetErrorString(e));
    return CRT_OK;
}

int device_denoise_filter(int device, uint32_t w, uint32_t h, void* d_state, void* d_state_tmp, const void* d_guide,
                          const crt_denoise_params* prm, double* d_out, double* d_var_out, void* stream) {
    int rc = device_check(device);
    if (rc) return rc;
    if (static_cast<uint64_t>(w) * h == 0) return CRT_OK;
    rc = check_frame(w, h);
    if (rc) return rc;
    DeviceGuard g(device);
    dn::State* const state[2] = {static_cast<dn::State*>(d_state), static_cast<dn::State*>(d_state_tmp)};
    const hipError_t e = launch_filter(w, h, state, static_cast<const dn::Guide*>(d_guide), prm, d_out, d_var_out,
                                       static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("denoise kernels: ") + hipGetErrorString(e));
    return CRT_OK;
}

// The two stages back to back over scratch of its own from the pass pool.
int device_denoise(int device, uint32_t w, uint32_t h, const double* d_rgb, const double* d_var,
                   const crt_feature* d_feat, const crt_denoise_params* prm, double* d_out, double* d_var_out,
                   void* stream) {
    int rc = device_check(device);
    if (rc) return rc;
    const uint64_t n64 = static_cast<uint64_t>(w) * h;
    if (n64 == 0) return CRT_OK;
    rc = check_frame(w, h);
    if (rc) return rc;
    const uint32_t n = static_cast<uint32_t>(n64);
    DeviceGuard g(device);
    void* pool_v = nullptr;
    rc = device_pass_pool(device, &pool_v);
    if (rc) return rc;
    hipMemPool_t pool = static_cast<hipMemPool_t>(pool_v);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one allocation: the guide, then the two states
    char* scratch = nullptr;
    const size_t guide_bytes = static_cast<size_t>(n) * sizeof(dn::Guide), state_bytes = static_cast<size_t>(n) * sizeof(dn::State);
    HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&scratch), guide_bytes + 2 * state_bytes, pool, st));
    dn::Guide* guide = reinterpret_cast<dn::Guide*>(scratch);
    dn::State* const state[2] = {reinterpret_cast<dn::State*>(scratch + guide_bytes),
                                 reinterpret_cast<dn::State*>(scratch + guide_bytes + state_bytes)};
    hipError_t e = launch_pack(n, d_rgb, d_var, d_feat, state[0], guide, st);
    if (e == hipSuccess) e = launch_filter(w, h, state, guide, prm, d_out, d_var_out, st);
    (void)hipFreeAsync(scratch, st);
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("denoise kernels: ") + hipGetErrorString(e));
    return CRT_OK;
}

}  // namespace crt
