// gfx950 render path: the reference's per-pixel/per-sample loop (camera.h:264-297), recursive
// integrator (camera.h:205-258), BVH traversal (bvh.h:585-715), primitive tests (sphere.h:45-96,
// parallelogram.h:177-240) and material scatter (material.h:64-263) as ONE kernel.
//
// Numerics: IEEE double throughout, compiled with -ffp-contract=off, every expression in the
// reference's operation order, so the geometry of each path (hit points, directions, RNG
// decisions) is bit-identical to the reference's for the same per-sample RNG stream. Radiance is
// accumulated forward (throughput) instead of by recursion; that re-association moves a
// sample's colour by a few ulps and never changes a path.
#include <hip/hip_runtime.h>

#define CRT_HD __host__ __device__ __forceinline__

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "crt_internal.h"
#include "crt_hip_util.h"
#include "crt_rows.h"
#include "crt_ray_class.h"
#include "crt_ray_gate.h"
#include "crt_schlick.h"
#include "crt_env.h"
#include "crt_env_sampler.h"
#include "crt_light_sampler.h"

#pragma clang fp contract(off)

namespace crt {

namespace dev {

#ifndef CRT_BLOCK
#define CRT_BLOCK 256
#endif
constexpr int kBlock = CRT_BLOCK;
// pixel tile of one work item's 64 units (kTileW x kTileH owned rows): 16 x 4 matches the
// multi-GPU bench's 4-row blocks, so a tile is contiguous on the image at any GPU count
// (per-rank share at 8 GPUs 13.0 vs 13.2 ms for 8 x 8; one GPU 87.5 vs 87.0)
#ifndef CRT_TILE_W
#define CRT_TILE_W 16
#endif
constexpr uint32_t kTileW = CRT_TILE_W, kTileH = 64 / CRT_TILE_W;
// waves per SIMD of the W5 instances (the "five-wave" ones)
constexpr int kManyWaves = 5;
// the HBM-scene instances' sibling-pair walk (walk_pairs; 0 builds the one-node walk for A/B)
#ifndef CRT_PAIR_WALK
#define CRT_PAIR_WALK 1
#endif
constexpr double kScale = 1 / static_cast<double>(4294967295u - 1);  // rand_util.h:110-112

typedef double Dvec2 __attribute__((ext_vector_type(2)));
typedef uint32_t Uvec4 __attribute__((ext_vector_type(4)));

struct SceneView {
    const DevNode* nodes;      // f64 nodes (HBM): trace(), the walk's EXACT variant and fallback
    const DevNodeF* fnodes;    // f32 walk nodes (HBM), refs = byte offsets
    uint32_t ntop;             // HBM-scene kernels: f32 refs below ntop are read from the LDS copy
    const uint32_t* refs;
    const DevSphere* spheres;
    const DevSpherePair* spair;  // f32 filter records (HBM)
    uint32_t spair_lds;          // LSCENE kernels: LDS byte offset of the staged copy
    const uint32_t* sphere_mat;
    const DevQuad* quads;
    const uint32_t* quad_mat;
    const DevMaterial* mats;
    const DevQuadF* quadf;       // f32 filter records of the parallelograms (HBM)
    const DevMaterial* sphere_mrec;  // per-slot material records (shade)
    const DevMaterial* quad_mrec;
    uint32_t quadf_lds;          // LSCENE kernels: LDS byte offset of the staged copy
    const DevQuadBox* quadbox;   // flat boxes of axis-aligned parallelograms (HBM)
    // LSCENE kernels: LDS byte offsets of the staged refs / f64 spheres / parallelograms, read
    // through typed LDS pointers (ds_read, not flat); spheres_lds = ~0u when the spheres stay in HBM
    uint32_t refs_lds, spheres_lds, quads_lds;
    uint32_t inv64_lds;          // flat-parallelogram LDS kernels: the lanes' 1 / d ([k][lane] doubles)
    unsigned long long* guard;   // parity guard words (DeviceCopy::guard)
    // link instances (render_kernel LINK): the miss-link table in HBM (DeviceCopy::links) and the
    // LDS byte offset of its staged copy, 16 bytes a node: the record of ref r at links_lds + (r >> 1)
    const uint16_t* links;
    uint32_t links_lds;
    uint32_t sentinel;           // link instances: the sentinel's ref, where a traversal ends (leaf_step)
};

struct CamView {
    double o[3], p00[3], pdx[3], pdy[3], ddx[3], ddy[3];
    double defocus_angle;
    double bg[3];
    double t_min;
    double inv_spp;
    uint32_t w, h, spp, max_depth, base_seed;
};

struct Work {
    uint32_t owned_rows;   // rows of this tiling
    uint32_t row_block, tile_count, tile_index;
    // one launch renders a band of the owned frame: owned rows [k0, k0 + bh) x columns
    // [col0, col0 + bw), in kTileW x kTileH pixel tiles (launch_render: a band has at most 65535
    // tiles either way, so a tile's coordinates pack into 16 bits each, and its partial sums
    // stay within the partial-sum budget)
    uint32_t col0, k0, bw, bh;
    uint32_t tiles_x, tiles_y, tiles;
    uint32_t chunks, chunk_len;        // sample chunks per pixel in this launch
    // first sample of the launch (a multiple of chunk_len; 0 for a one-shot render): chunk c of
    // the launch holds samples [s0 + c * chunk_len, min(spp, s0 + (c + 1) * chunk_len)), which is
    // chunk s0 / chunk_len + c of the whole job (crt_render_pass_async)
    uint32_t s0;
    // work queue, taken in order by the waves of a persistent grid (render_kernel): bulk items
    // (tile i / groups, chunks [(i % groups) * item_chunks, + item_chunks)), then tail items
    // (tile j / tail_chunks, chunk bulk_chunks + j % tail_chunks); 64 units per chunk
    // XCD-local queues (v12): the band's tiles (tile-major) are cut into `segments` contiguous
    // ranges, segment x = tiles [tiles * x / segments, tiles * (x + 1) / segments), each with its own
    // counter queue[x] (zeroed before the launch) over its items: its tiles' bulk items, then its
    // tiles' tail items. A wave starts on segment blockIdx % segments (blocks b and b + 8 share an
    // XCD and its L2) and moves on to the next segments when its own is dry.
    uint32_t* queue;
    uint32_t segments;      // 8, or 1 (CRT_XCD_QUEUES=0)
    uint32_t n_items, bulk_items;
    uint32_t item_chunks, groups, bulk_chunks, tail_chunks;
    uint32_t rb_shift;      // log2(row_block) when it is a power of two, else 32
    // LDS layout of the scene-staging kernels (byte offsets / 16-byte padded sizes)
    uint32_t lds_nodes, lds_refs, lds_spheres, lds_quads, lds_quadf, lds_stack;
    uint32_t bytes_nodes, bytes_refs, bytes_spheres, bytes_quads, bytes_quadf;
    uint32_t lds_sph64, bytes_sph64;  // sphere-only LDS scenes: the f64 spheres too, when they fit
    uint32_t sphere_only;   // every primitive is a sphere: refs[slot] == slot
    uint32_t exact_slab;    // the scene needs walk_step's EXACT variant for every ray
    uint32_t ntop;          // HBM-scene kernels: f32 nodes [0, ntop) bytes staged in LDS at offset 0
    uint32_t sentinel;      // the sentinel node's reference (byte offset into the f32 nodes)
    uint32_t lds_cam;       // LDS copy of the CamView (read where used: keeps it out of SGPRs)
    uint32_t lds_acc;       // five-wave instances: the lanes' pixel sums (3 x kBlock doubles)
    uint32_t lds_inv64;     // flat-parallelogram LDS instances: the lanes' 1 / d (3 x kBlock doubles)
    // link instances: the miss-link table, staged where the plan keeps the guard levels and the stack
    uint32_t lds_links, bytes_links;
    uint32_t packed;        // the output holds only the owned rows (CRT_TILING_PACKED)
    // instrumented pass only (COUNT): walk speculatively like the timed kernel (CRT_COUNT_SPEC=1),
    // count per-round lane numbers (CRT_ROUND_COUNTERS=1; their atomics shift the phase timings)
    uint32_t count_spec, round_counters;
    uint32_t f32_ok;        // node bounds fit the f32 walk's error analysis (else f64 decides)
    uint32_t pair_walk;     // HBM-scene kernels built with CRT_PAIR_WALK: walk_pairs for NaN-free rays
    uint32_t spheres_f32;   // sphere-only scene within the f32 filter's range (two-pass leaves)
    uint32_t quads_f32;     // parallelogram-only scene within its f32 filter's range (two-pass leaves)
    uint32_t quads_flat;    // ... and every parallelogram axis-aligned: pass 1 is the flat-box node test
    float tmin32;           // RN32(camera t_min)
};

struct Counters {
    unsigned long long rays, nodes, sphere_tests, quad_tests;
    unsigned long long cyc_walk, cyc_leaf, cyc_shade, cyc_total;  // wave cycles (instrumented pass)
    unsigned long long cyc_tail;  // from the wave's first idle lane (chunk done) to its end
    unsigned long long it_walk, it_leaf, it_shade;  // wave iterations (lane utilization)
    unsigned long long slow_nodes, it_slow;  // node tests decided in f64 (lanes / wave iterations)
    unsigned long long cand, it_cand;        // two-pass leaves: exact tests of candidates (lanes / wave iterations)
    // per traversal round (walk + leaf): rounds, lanes walking at its start, lanes holding a leaf
    // after the walk, lanes with a finished ray after the leaf step (CRT_DEBUG_COUNTERS)
    unsigned long long rounds, round_walkers, round_leaves, round_done, shade_rounds;
    unsigned long long cyc_draw, cyc_init;  // wave ticks drawing units / starting paths + traversal set-up
};

// one lane's counts in the instrumented pass, added to the 64-bit Counters when the lane ends, and
// before then whenever one of them passes 2^31 (flush_counts, once per shade round): a lane of the
// persistent grid traces units for the whole launch, and a small grid on a large frame would wrap
// 32-bit counts (64-bit lane counts would cost the instrumented kernel spills)
struct LaneCounters {
    uint32_t rays, nodes, sphere_tests, quad_tests;
    uint32_t it_walk, it_leaf, it_shade;
    uint32_t slow_nodes, it_slow;
    uint32_t cand, it_cand;
};

// adds a lane's counts to the launch's totals and clears them (iteration counters are incremented
// by whichever lane led that iteration)
__device__ __forceinline__ void flush_counts(LaneCounters& c, Counters* t) {
    using ull = unsigned long long;
    atomicAdd(&t->rays, static_cast<ull>(c.rays));
    atomicAdd(&t->nodes, static_cast<ull>(c.nodes));
    atomicAdd(&t->sphere_tests, static_cast<ull>(c.sphere_tests));
    atomicAdd(&t->quad_tests, static_cast<ull>(c.quad_tests));
    atomicAdd(&t->it_walk, static_cast<ull>(c.it_walk));
    atomicAdd(&t->it_leaf, static_cast<ull>(c.it_leaf));
    atomicAdd(&t->it_shade, static_cast<ull>(c.it_shade));
    atomicAdd(&t->slow_nodes, static_cast<ull>(c.slow_nodes));
    atomicAdd(&t->it_slow, static_cast<ull>(c.it_slow));
    atomicAdd(&t->cand, static_cast<ull>(c.cand));
    atomicAdd(&t->it_cand, static_cast<ull>(c.it_cand));
    c = LaneCounters{};
}

// counts one per wave: only the lowest active lane increments
__device__ __forceinline__ bool wave_leader() {
    const uint64_t m = __ballot(1);
    return (threadIdx.x & 63) == static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
}

// Debug builds only (-DCRT_WATCHDOG=1, never the library's default): every wave-level loop of
// the render kernel checks a deadline (3 s after the launch's first wave started) and, past it,
// the wave prints where it was and ends (s_endpgm), so a kernel that would spin forever finishes
// with a report instead of hanging the device (tools/gpu_watchdog.sh).
#ifndef CRT_WATCHDOG
#define CRT_WATCHDOG 0
#endif
#if CRT_WATCHDOG
__device__ unsigned long long crt_wd_deadline;
#define CRT_WD(id, a, b)                                                                                   \
    do {                                                                                                   \
        if (wall_clock64() > *(volatile unsigned long long*)&crt_wd_deadline) {                            \
            if (wave_leader())                                                                             \
                printf("crt watchdog: block %u wave %u loop %d a %u b %u\n", blockIdx.x, threadIdx.x >> 6,  \
                       (int)(id), (unsigned)(a), (unsigned)(b));                                            \
            __builtin_amdgcn_endpgm();                                                                     \
        }                                                                                                  \
    } while (0)
#else
#define CRT_WD(id, a, b) do {} while (0)
#endif

// ---- reference RNG (rand_util.h:85-117) with per-sample state ------------------------------
__device__ __forceinline__ double rnd(uint32_t& s, double lo, double hi) {
    s = 1664525u * s + 1013904223u;
    return lo + (hi - lo) * static_cast<double>(s) * kScale;
}
// rnd(s, -1, 1) and rnd(s, 0, 1) with one f64 operation fewer, bit for bit: (1 - -1) * x = 2x is
// exact (x < 2^32), and RN(2x * kScale) = RN(x * (2 kScale)) with 2 kScale exact; 0 + y = y for
// the y = RN(x * kScale) >= 0 here (+0 included)
__device__ __forceinline__ double rnd_pm1(uint32_t& s) {
    s = 1664525u * s + 1013904223u;
    return static_cast<double>(s) * (2 * kScale) + -1.0;
}
__device__ __forceinline__ double rnd_01(uint32_t& s) {
    s = 1664525u * s + 1013904223u;
    return static_cast<double>(s) * kScale;
}

__device__ __forceinline__ uint32_t sample_seed(uint32_t base, uint32_t pixel, uint32_t sample) {
    uint64_t z = (static_cast<uint64_t>(pixel) << 32) | sample;
    z += static_cast<uint64_t>(base) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return static_cast<uint32_t>(z ^ (z >> 32));
}

// sqrt(x) bit for bit for x in [2^-767, inf), given r = v_rsq_f64(x): hipcc's own gfx950
// expansion of the IEEE sqrt (Goldschmidt + two Newton corrections) without its small-x scaling
// and 0/inf fix-up, which are identities there. Outside that range: sqrt() itself.
__device__ __forceinline__ double sqrt_from_rsq(double x, double r) {
    if (__builtin_expect(!(x >= 0x1p-767 && x < __builtin_inf()), 0)) return sqrt(x);
    double g = x * r, h = r * 0.5;
    const double e = fma(-h, g, 0.5);
    g = fma(g, e, g);
    h = fma(h, e, h);
    double d = fma(-g, g, x);
    g = fma(d, h, g);
    d = fma(-g, g, x);
    return fma(d, h, g);
}

// The shading code's square roots and reciprocals (unit vectors, the Dielectric's sin and
// refraction) without the range scaling and special-case fix-ups of hipcc's IEEE expansions, in
// the five-wave sphere-only kernel instances (FAST; config 2 73.7 -> 73.1-73.4 ms); the others
// keep sqrt() and the division (config 3 90.0 -> 91.3 ms, config 4 139.1 -> 140.2 ms with them).
template <bool FAST>
__device__ __forceinline__ double sqrt_exact(double x) {
    if (FAST) return sqrt_from_rsq(x, __builtin_amdgcn_rsq(x));
    return sqrt(x);
}
// 1 / s bit for bit: hipcc's gfx950 division 1 / s is div_scale, v_rcp_f64, two Newton steps
// y = fma(y, fma(-s, y, 1), y), q = 1 * y, r = fma(-s, q, 1), div_fmas = fma(r, y, q), div_fixup.
// For |s| in [2^-500, 2^500] div_scale scales nothing (it returns its operand), div_fmas adds no
// scale and div_fixup returns its first operand (no NaN, inf, zero or denormal arises), so the
// same operations without those three are that division's result; outside the range: 1 / s.
__device__ __forceinline__ double recip_core(double s) {  // |s| in [2^-500, 2^500]
    double y = __builtin_amdgcn_rcp(s);
    y = fma(y, fma(-s, y, 1.0), y);
    y = fma(y, fma(-s, y, 1.0), y);
    return fma(fma(-s, y, 1.0), y, y);
}
template <bool FAST>
__device__ __forceinline__ double recip_exact(double s) {
    if (!FAST) return 1 / s;
    if (__builtin_expect(!(fabs(s) >= 0x1p-500 && fabs(s) <= 0x1p500), 0)) return 1 / s;
    return recip_core(s);
}

// Vec3D::random_unit_vector (vec3d.h:64-75): rejection in the cube, then * (1 / |v|)
template <bool FAST = false>
__device__ __forceinline__ void random_unit_vector(uint32_t& s, double& x, double& y, double& z) {
    double m2;
    do {
        x = rnd_pm1(s);
        y = rnd_pm1(s);
        z = rnd_pm1(s);
        m2 = x * x + y * y + z * z;
    } while (!(m2 < 1));
    double inv = recip_exact<FAST>(sqrt_exact<FAST>(x * x + y * y + z * z));
    x = x * inv;
    y = y * inv;
    z = z * inv;
}

// AABB::is_hit_by_optimized (aabb.h:132-174). The early returns of the reference are folded into
// one boolean (the tests have no side effects), so the whole node is loaded up front (four
// 16-byte loads) and the test runs without branches.
struct NodeRegs {
    double b[6];
    uint32_t index, count, axis, flags;
};

__device__ __forceinline__ NodeRegs load_node(const DevNode* nodes, uint32_t i) {
    const uint4* p = reinterpret_cast<const uint4*>(nodes + i);
    const uint4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
    NodeRegs n;
    n.b[0] = __hiloint2double(q0.y, q0.x);
    n.b[1] = __hiloint2double(q0.w, q0.z);
    n.b[2] = __hiloint2double(q1.y, q1.x);
    n.b[3] = __hiloint2double(q1.w, q1.z);
    n.b[4] = __hiloint2double(q2.y, q2.x);
    n.b[5] = __hiloint2double(q2.w, q2.z);
    n.index = q3.x;
    n.count = q3.y;
    n.axis = q3.z;
    n.flags = q3.w;
    return n;
}

__device__ __forceinline__ bool slab(const NodeRegs& n, const double o[3], const double inv[3],
                                     uint32_t neg, double tmin, double tmax) {
    // x[neg] / x[!neg]: neg bit k selects max as the entry bound on axis k
    const double bx0 = (neg & 1u) ? n.b[1] : n.b[0], bx1 = (neg & 1u) ? n.b[0] : n.b[1];
    const double by0 = (neg & 2u) ? n.b[3] : n.b[2], by1 = (neg & 2u) ? n.b[2] : n.b[3];
    const double bz0 = (neg & 4u) ? n.b[5] : n.b[4], bz1 = (neg & 4u) ? n.b[4] : n.b[5];
    double xtmin = (bx0 - o[0]) * inv[0];
    double xtmax = (bx1 - o[0]) * inv[0];
    const double ytmin = (by0 - o[1]) * inv[1];
    const double ytmax = (by1 - o[1]) * inv[1];
    const double ztmin = (bz0 - o[2]) * inv[2];
    const double ztmax = (bz1 - o[2]) * inv[2];
    const bool c1 = !(xtmin > ytmax || ytmin > xtmax);
    if (ytmin > xtmin) xtmin = ytmin;
    if (ytmax < xtmax) xtmax = ytmax;
    const bool c2 = !(xtmin > ztmax || ztmin > xtmax);
    if (ztmin > xtmin) xtmin = ztmin;
    if (ztmax < xtmax) xtmax = ztmax;
    return c1 & c2 & (xtmin < tmax) & (xtmax > tmin);
}

// Reciprocal of a ray's dot(d, d) for div_a: ia = RN(1 / a), or NaN when a is outside the range
// where div_a's corrections are exact (then div_a divides).
// (in_range: gate_recip(a), crt_ray_gate.h)
template <bool FAST = false>
__device__ __forceinline__ double recip_a(double a, bool in_range) {
    return in_range ? (FAST ? recip_core(a) : 1 / a) : __builtin_nan("");
}
template <bool FAST = false>
__device__ __forceinline__ double recip_a(double a) { return recip_a<FAST>(a, gate_recip(a)); }

// n / a correctly rounded from ia = RN(1/a): q0 = n * ia, then two residual corrections
// q += fma(-a, q, n) * ia (Markstein's theorem: with ia = RN(1/a) and q within 1 ulp, the
// corrected q is RN(n / a); the first correction makes q faithful). No over/underflow for
// |n|, a in [2^-500, 2^500]; anything else divides.
__device__ __forceinline__ double div_a(double n, double a, double ia) {
    const double an = fabs(n);
    if (__builtin_expect(!(an >= 0x1p-500 && an <= 0x1p500 && ia == ia), 0)) return n / a;
    double q = n * ia;
    q = fma(fma(-a, q, n), ia, q);
    return fma(fma(-a, q, n), ia, q);
}

// Sphere::hit_by (sphere.h:45-96) returning the accepted root through t.
// Before the exact sqrt and divisions, a coarse bound (hardware rsq, error <= 2^-23 relative;
// margins of 2^-12 on every term) proves "both roots >= t_max" or "both roots <= t_min" for
// spheres that cannot be accepted; only those are skipped, so the accepted roots are exactly the
// reference's. NaN/inf anywhere makes the bound inconclusive and falls through to the exact test.
// The sqrt and the two divisions by a are the correctly rounded ones (sqrt_from_rsq, div_a with
// ia = recip_a(a)); lo / hi are lim_tmin / lim_tmax of the current t_min / t_max.
// Coarse-reject limits of hit_sphere: t * a scaled outward by 2^-30 (tmin side: inward).
__device__ __forceinline__ double lim_tmax(double tmax, double a) { return tmax * a * (1 + 0x1p-30); }
__device__ __forceinline__ double lim_tmin(double tmin, double a) { return tmin * a * (1 - 0x1p-30); }

// COARSE = false skips the coarse reject (the candidates of two-pass leaves passed a filter).
template <bool COARSE = true>
__device__ __forceinline__ bool hit_sphere(const DevSphere& sp, const double o[3], const double d[3],
                                           double a, double ia, double tmin, double tmax, double lo,
                                           double hi, double& t) {
    double ocx = o[0] - sp.c[0], ocy = o[1] - sp.c[1], ocz = o[2] - sp.c[2];
    double b = d[0] * ocx + d[1] * ocy + d[2] * ocz;
    double c = (ocx * ocx + ocy * ocy + ocz * ocz) - sp.r * sp.r;
    double disc = b * b - a * c;
    if (disc < 0) return false;
    const double rs = __builtin_amdgcn_rsq(disc);
    if (COARSE) {
        const double sqa = disc * rs;                              // ~sqrt(disc)
        const double m = (fabs(b) + sqa) * 0x1p-12;                // covers every rounding error
        const bool beyond = (-b - sqa) - m > hi;   // r1 > tmax, so r2 too  (hi = lim_tmax)
        const bool before = (-b + sqa) + m < lo;   // r2 < tmin, so r1 too  (lo = lim_tmin)
        if (beyond || before) return false;
    }
    double sq = sqrt_from_rsq(disc, rs);
    double root = div_a(-b - sq, a, ia);
    if (!(tmin < root && root < tmax)) {
        root = div_a(-b + sq, a, ia);
        if (!(tmin < root && root < tmax)) return false;
    }
    t = root;
    return true;
}

// v_min/v_max(3)_f32 of non-NaN operands. Written out because fminf/fmaxf make the compiler
// quieten possible signalling NaNs of operands it cannot prove canonical (tmin', tmax') with an
// extra v_max each, in every walk step.
// v_cndmask_b32 with a lane mask from a ballot (scalar registers): m ? a : b per lane
__device__ __forceinline__ uint32_t vsel(uint64_t m, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(b), "v"(a), "s"(m));
    return r;
}

// The walk's step on the lanes of `on` alone (an exec-masked select: the other lanes keep
// `keep`): m ? a : top, zero-extended. A 16-bit `top` fresh from a load has its register's high
// half undefined yet; SDWA reads the low word, where a plain select would need a v_and first.
// (s_and_saveexec writes SCC: clobbered.)
__device__ __forceinline__ uint32_t vsel_top_on(uint64_t on, uint64_t m, uint32_t a, uint16_t top, uint32_t keep) {
    uint64_t save;
    asm("s_and_saveexec_b64 %[save], %[on]\n\t"
        "s_mov_b64 vcc, %[m]\n\t"
        "v_cndmask_b32_sdwa %[r], %[b], %[a], vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n\t"
        "s_mov_b64 exec, %[save]"
        : [r] "+v"(keep), [save] "=&s"(save)
        : [a] "v"(a), [b] "v"(__builtin_bit_cast(_Float16, top)), [m] "s"(m), [on] "s"(on)
        : "vcc", "scc");
    return keep;
}
__device__ __forceinline__ uint32_t vsel_top_on(uint64_t on, uint64_t m, uint32_t a, uint32_t top, uint32_t keep) {
    uint64_t save;
    asm("s_and_saveexec_b64 %[save], %[on]\n\t"
        "v_cndmask_b32_e64 %[r], %[b], %[a], %[m]\n\t"
        "s_mov_b64 exec, %[save]"
        : [r] "+v"(keep), [save] "=&s"(save)
        : [a] "v"(a), [b] "v"(top), [m] "s"(m), [on] "s"(on)
        : "scc");
    return keep;
}
__device__ __forceinline__ float vmin(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmax(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float vmin3(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// b wave-uniform, in an SGPR
__device__ __forceinline__ float vmax_s(float a, float b) { float r; asm("v_max_f32 %0, %2, %1" : "=v"(r) : "v"(a), "s"(b)); return r; }
__device__ __forceinline__ float vmax_abs(float a, float b) {
    float r;
    asm("v_max_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax3_0(float a, float b) {  // max(a, b, 0)
    float r;
    asm("v_max3_f32 %0, %1, %2, 0" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// the kernel's min / max for crt_quad_filter.h flat_box_candidate
struct DevMinMax {
    static __device__ __forceinline__ float min(float a, float b) { return vmin(a, b); }
    static __device__ __forceinline__ float max(float a, float b) { return vmax(a, b); }
    static __device__ __forceinline__ float min3(float a, float b, float c) { return vmin3(a, b, c); }
    static __device__ __forceinline__ float max3(float a, float b, float c) { return vmax3(a, b, c); }
    static __device__ __forceinline__ float max_s(float a, float b) { return vmax_s(a, b); }
    static __device__ __forceinline__ float max_abs(float a, float b) { return vmax_abs(a, b); }
};

// The candidate filter of two-pass sphere leaves, two spheres per step in packed f32
// (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32: one instruction for both spheres). It returns two
// bits, false only where the exact test (hit_sphere, i.e. Sphere::hit_by) provably rejects the
// sphere for every t_max' <= t_max. No square root: with y = -b - hi and w = b + lo,
//   no real root          <=  D < 0
//   both roots >= t_max   <=  y > 0 and y^2 > D
//   both roots <= t_min   <=  w > 0 and w^2 > D
// i.e. reject <=> max(y|y|, w|w|, 0) > D, where D bounds the exact test's discriminant from above
// with room to spare:
//   D = b'^2 - a' (q' (1 - 2^-15) - r2e - kap),  b' = d32 . X, q' = X . X, X = o32 - c32,
//   r2e = RN32(r^2 (1 + 2^-14) + 2^22 |c - c32|^2)  (per sphere, DevSpherePair),
//   kap = RN32(2^22 |o - o32|^2 + 2^-50)           (per ray),
// and hi = RN32(t_max a (1 + 2^-20)), lo = RN32(t_min a (1 - 2^-20)). Error budget: with
// S = a (|oc|^2 + r^2) >= b^2, |disc|, and Delta = |o - o32| + |c - c32| (the rounding of the
// inputs), every f32 rounding error is below 2^-19 S, and the terms in Delta are at most
// 4 a |oc| Delta + 2 a Delta^2 <= 2^-17 a |oc|^2 + 2^20 a Delta^2 (AM-GM); the slack of D,
// 2^-15 a q' + 2^-14 a r^2 + 2^22 a (|o - o32|^2 + |c - c32|^2) >= those, also covers the error of
// b' inside y and w (2 |y| |b' - b| <= 2^-18 a q + 2^18 a Delta^2), and hi / lo carry a 2^-20
// relative slack for the rounding of the exact roots (the f64 analysis: 2^-30). A sphere the
// filter rejects is rejected by the exact test for this t_max and any smaller one, so hits and
// the tie order are the sequential loop's. Valid for |o_k|, |d_k|, |c_k|, |r| <= 2^30 and
// a in [2^-60, 2^60] (leaf_step checks; W.spheres_f32 for the scene).
// tools/fuzz_sphere_filter.c checks the filter (this exact f32 sequence) against the exact test.
typedef float F2 __attribute__((ext_vector_type(2)));
// The ray in f32 for the packed filter (per entered leaf), two scalars per register pair; the
// packed instructions broadcast one half with op_sel / op_sel_hi (no splatted copies: 10 VGPRs
// instead of 20 while the leaf phase runs).
struct LeafRay32 {
    F2 oxy, ozdx, dydz, akap, hilo;  // (ox, oy) (oz, dx) (dy, dz) (a, kap) (hi, lo)
};
__device__ __forceinline__ void leaf_ray32(const double o[3], const double d[3], double a, double tmin,
                                           double tmax, LeafRay32& L) {
    float o32[3];
    double e2 = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o32[k] = static_cast<float>(o[k]);
        const double e = o[k] - static_cast<double>(o32[k]);
        e2 = e2 + e * e;
    }
    L.oxy = F2{o32[0], o32[1]};
    L.ozdx = F2{o32[2], static_cast<float>(d[0])};
    L.dydz = F2{static_cast<float>(d[1]), static_cast<float>(d[2])};
    L.akap = F2{static_cast<float>(a), static_cast<float>(e2 * 0x1p22 + 0x1p-50)};
    L.hilo = F2{static_cast<float>(tmax * a * (1 + 0x1p-20)), static_cast<float>(tmin * a * (1 - 0x1p-20))};
}
// (leaf_ray32's ranges: gate_leaf32, crt_ray_gate.h; trav_init keeps the verdict in Trav::neg)
__device__ __forceinline__ float vmul_abs(float a, float b) {  // a * |b|
    float r;
    asm("v_mul_f32 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// packed f32 with one operand broadcast from the low (_L) or high (_H) half of a ray pair p
__device__ __forceinline__ F2 sub_pL(F2 p, F2 c) {  // (p.x, p.x) - c
    F2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(p), "v"(c));
    return r;
}
__device__ __forceinline__ F2 sub_pH(F2 p, F2 c) {  // (p.y, p.y) - c
    F2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(p), "v"(c));
    return r;
}
__device__ __forceinline__ F2 add_pH(F2 p, F2 c) {  // (p.y, p.y) + c
    F2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "v"(p), "v"(c));
    return r;
}
__device__ __forceinline__ F2 mul_pL(F2 p, F2 c) {  // (p.x, p.x) * c
    F2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(r) : "v"(p), "v"(c));
    return r;
}
__device__ __forceinline__ F2 mul_pH(F2 p, F2 c) {  // (p.y, p.y) * c
    F2 r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1]" : "=v"(r) : "v"(p), "v"(c));
    return r;
}
__device__ __forceinline__ F2 fma_pL(F2 p, F2 c, F2 e) {  // fma((p.x, p.x), c, e)
    F2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(r) : "v"(p), "v"(c), "v"(e));
    return r;
}
__device__ __forceinline__ F2 fma_pH(F2 p, F2 c, F2 e) {  // fma((p.y, p.y), c, e)
    F2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "=v"(r) : "v"(p), "v"(c), "v"(e));
    return r;
}
__device__ __forceinline__ F2 nsub_pL(F2 b, F2 p) {  // -b - (p.x, p.x)
    F2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel_hi:[1,0] neg_lo:[1,1] neg_hi:[1,1]" : "=v"(r) : "v"(b), "v"(p));
    return r;
}
__device__ __forceinline__ F2 add_bH(F2 b, F2 p) {  // b + (p.y, p.y)
    F2 r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(b), "v"(p));
    return r;
}
// records read through explicitly typed LDS / global pointers (a generic pointer would make the
// compiler emit flat loads), as 16-byte vectors
typedef float Fvec4 __attribute__((ext_vector_type(4)));
struct PairLines {
    Fvec4 c;   // cx0 cx1 cy0 cy1
    Fvec4 zr;  // cz0 cz1 r2e0 r2e1
};
typedef __attribute__((address_space(3))) const PairLines LdsPair;
typedef __attribute__((address_space(1))) const PairLines GlobalPair;
template <typename P>
__device__ __forceinline__ DevSpherePair pair_at(P p) {
    const Fvec4 c = p->c, zr = p->zr;
    DevSpherePair r;
    r.cx[0] = c.x; r.cx[1] = c.y; r.cy[0] = c.z; r.cy[1] = c.w;
    r.cz[0] = zr.x; r.cz[1] = zr.y; r.r2e[0] = zr.z; r.r2e[1] = zr.w;
    return r;
}
struct SphereLines {
    Dvec2 a, b;  // (cx, cy), (cz, r)
};
typedef __attribute__((address_space(1))) const SphereLines GlobalSphere;
__device__ __forceinline__ DevSphere sphere_global(const DevSphere* p) {
    const GlobalSphere* q = (GlobalSphere*)p;
    const Dvec2 a = q->a, b = q->b;
    DevSphere r;
    r.c[0] = a.x; r.c[1] = a.y; r.c[2] = b.x; r.r = b.y;
    return r;
}
// an f32 parallelogram record in HBM through a typed global pointer (4 x 16-byte loads)
typedef __attribute__((address_space(1))) const Fvec4 GlobalFvec4;
__device__ __forceinline__ DevQuadF quadf_global(const DevQuadF* p) {
    const GlobalFvec4* q = (GlobalFvec4*)p;
    DevQuadF r;
    Fvec4* dst = reinterpret_cast<Fvec4*>(&r);
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = q[k];
    return r;
}
// a 16-byte aligned record (DevSphere, DevQuad, u32) at an LDS byte offset, read as ds_read
typedef __attribute__((address_space(3))) const Dvec2 LdsDvec2;
template <typename T>
__device__ __forceinline__ T lds_rec(uint32_t off) {
    static_assert(sizeof(T) % 16 == 0, "16-byte lines");
    T r;
    Dvec2* dst = reinterpret_cast<Dvec2*>(&r);
    const LdsDvec2* src = (LdsDvec2*)static_cast<uintptr_t>(off);
#pragma unroll
    for (uint32_t k = 0; k < sizeof(T) / 16; ++k) dst[k] = src[k];
    return r;
}
__device__ __forceinline__ uint32_t lds_u32(uint32_t off) {
    return *(__attribute__((address_space(3))) const uint32_t*)static_cast<uintptr_t>(off);
}
// the verdicts of the record's two spheres shifted into cand: bit 1 = first, bit 0 = second
// (1 = candidate); cand = cand + cand + verdict by v_addc_co_u32 with the compare's VCC as the
// carry (written out: the compiler turns the C form into a shift, two selects and an or); the
// s_nop 1 is the VALU-writes-VCC -> VALU-reads-VCC hazard the compiler pads the same way
__device__ __forceinline__ uint32_t sphere_pair_candidates(uint32_t cand, const DevSpherePair& sp, const LeafRay32& L) {
    const F2 cx = {sp.cx[0], sp.cx[1]}, cy = {sp.cy[0], sp.cy[1]}, cz = {sp.cz[0], sp.cz[1]};
    const F2 r2e = {sp.r2e[0], sp.r2e[1]};
    const F2 xx = sub_pL(L.oxy, cx), xy = sub_pH(L.oxy, cy), xz = sub_pL(L.ozdx, cz);
    const F2 b = fma_pH(L.dydz, xz, fma_pL(L.dydz, xy, mul_pH(L.ozdx, xx)));
    const F2 q = __builtin_elementwise_fma(xz, xz, __builtin_elementwise_fma(xy, xy, xx * xx));
    const F2 g = __builtin_elementwise_fma(q, F2{1 - 0x1p-15f, 1 - 0x1p-15f}, -add_pH(L.akap, r2e));
    const F2 D = __builtin_elementwise_fma(b, b, -mul_pL(L.akap, g));
    const F2 y = nsub_pL(b, L.hilo), w = add_bH(b, L.hilo);
    const float m0 = vmax3_0(vmul_abs(y.x, y.x), vmul_abs(w.x, w.x));
    const float m1 = vmax3_0(vmul_abs(y.y, y.y), vmul_abs(w.y, w.y));
    asm volatile("v_cmp_ngt_f32 vcc, %1, %2\n\ts_nop 1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
                 : "+v"(cand) : "v"(m0), "v"(D.x) : "vcc");
    asm volatile("v_cmp_ngt_f32 vcc, %1, %2\n\ts_nop 1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc"
                 : "+v"(cand) : "v"(m1), "v"(D.y) : "vcc");
    return cand;
}

// Parallelogram::hit_by (parallelogram.h:177-240)
__device__ __forceinline__ bool hit_quad(const DevQuad& q, const double o[3], const double d[3],
                                         double tmin, double tmax, double& t) {
    double den = q.n[0] * d[0] + q.n[1] * d[1] + q.n[2] * d[2];
    if (fabs(den) < 1e-9) return false;
    double vx = q.v[0] - o[0], vy = q.v[1] - o[1], vz = q.v[2] - o[2];
    double ht = (q.n[0] * vx + q.n[1] * vy + q.n[2] * vz) / den;
    if (!(tmin < ht && ht < tmax)) return false;
    double px = o[0] + d[0] * ht, py = o[1] + d[1] * ht, pz = o[2] + d[2] * ht;
    double wx = px - q.v[0], wy = py - q.v[1], wz = pz - q.v[2];
    // alpha = dot(sn, cross(w, s2)); beta = dot(sn, cross(s1, w))
    double c1x = wy * q.s2[2] - wz * q.s2[1];
    double c1y = wz * q.s2[0] - wx * q.s2[2];
    double c1z = wx * q.s2[1] - wy * q.s2[0];
    double alpha = q.sn[0] * c1x + q.sn[1] * c1y + q.sn[2] * c1z;
    double c2x = q.s1[1] * wz - q.s1[2] * wy;
    double c2y = q.s1[2] * wx - q.s1[0] * wz;
    double c2z = q.s1[0] * wy - q.s1[1] * wx;
    double beta = q.sn[0] * c2x + q.sn[1] * c2y + q.sn[2] * c2z;
    if (0 <= alpha && alpha <= 1 && 0 <= beta && beta <= 1) {
        t = ht;
        return true;
    }
    return false;
}

// sphere i: LS kernels read the LDS copy or, in the f32-filter mode, HBM through a typed pointer
template <bool LS>
__device__ __forceinline__ DevSphere sphere_at(const SceneView& S, uint32_t i) {
    if (!LS) return S.spheres[i];
    return S.spheres_lds != ~0u ? lds_rec<DevSphere>(S.spheres_lds + (i << 5)) : sphere_global(S.spheres + i);
}

// Resolve the hit record (hittable.h:46-71): hit point ray(t), outward normal, front face.
// IR: the sphere's 1/r comes in as ir (shade: the slot's material record holds RN(1/r), the
// same value the division gives); otherwise it is divided here.
template <bool LS, bool IR = false, bool SPH = false, bool QONLY = false>
__device__ __forceinline__ uint32_t hit_record(const SceneView& S, uint32_t ref, const double o[3],
                                               const double d[3], double t, double p[3],
                                               double nrm[3], bool& front, double ir_in = 0) {
    p[0] = o[0] + d[0] * t;
    p[1] = o[1] + d[1] * t;
    p[2] = o[2] + d[2] * t;
    double nx, ny, nz;
    uint32_t m;
    if (QONLY || (!SPH && (ref & kRefQuad))) {
        if constexpr (LS) {
            const DevQuad q = lds_rec<DevQuad>(S.quads_lds + ((ref & ~kRefQuad) << 7));
            nx = q.n[0]; ny = q.n[1]; nz = q.n[2];
        } else {
            const DevQuad& q = S.quads[ref & ~kRefQuad];
            nx = q.n[0]; ny = q.n[1]; nz = q.n[2];
        }
        m = S.quad_mat[ref & ~kRefQuad];
    } else {
        const auto normal = [&](const DevSphere& sp) {
            const double ir = IR ? ir_in : 1 / sp.r;  // (hit_point - center) / radius
            nx = (p[0] - sp.c[0]) * ir;
            ny = (p[1] - sp.c[1]) * ir;
            nz = (p[2] - sp.c[2]) * ir;
        };
        if constexpr (LS) normal(sphere_at<LS>(S, ref));
        else normal(S.spheres[ref]);
        m = S.sphere_mat[ref];
    }
    if (d[0] * nx + d[1] * ny + d[2] * nz > 0) {
        nrm[0] = -nx; nrm[1] = -ny; nrm[2] = -nz;
        front = false;
    } else {
        nrm[0] = nx; nrm[1] = ny; nrm[2] = nz;
        front = true;
    }
    return m;
}

// Per-lane traversal stack, interleaved [level][lane] so a wave's pushes hit distinct banks
// (LDS) or whole lines (HBM fallback for trees deeper than the LDS budget). Entries are u16 when
// the BVH has < 65536 nodes.
template <typename SE>
struct Stack {
    SE* base;
    uint32_t stride;
    __device__ __forceinline__ void put(int i, uint32_t v) { base[static_cast<size_t>(i) * stride] = static_cast<SE>(v); }
    __device__ __forceinline__ uint32_t get(int i) const { return base[static_cast<size_t>(i) * stride]; }
};

// BVH::hit_by (bvh.h:585-715): iterative DFS over the preorder nodes, near child first by the
// sign of the ray direction on the split axis, leaf primitives in order shrinking t_max.
// Control flow is "while-while" (Aila & Laine 2009): a lane walks interior nodes until it enters
// a leaf (or finishes), and the wave then tests all lanes' leaves together, so the primitive loop
// runs with most lanes active. Per lane, the sequence of node tests and primitive tests is
// exactly the reference's.
template <typename SE, bool COUNT>
__device__ __forceinline__ bool trace(const SceneView& S, Stack<SE>& st, const double o[3],
                                      const double d[3], double tmin, double& tmax,
                                      uint32_t& hit_ref, LaneCounters& ctr) {
    const double inv[3] = {1 / d[0], 1 / d[1], 1 / d[2]};
    const uint32_t neg = (d[0] < 0 ? 1u : 0u) | (d[1] < 0 ? 2u : 0u) | (d[2] < 0 ? 4u : 0u);
    const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];  // dot(ray.dir, ray.dir)
    const double ia = recip_a(a), lo = lim_tmin(tmin, a);
    double hi = lim_tmax(tmax, a);
    bool found = false;
    int sp = 0;
    uint32_t cur = 0;
    bool done = false;
    while (!done) {
        uint32_t first = 0, count = 0;
        while (true) {  // interior walk until a leaf is entered
            const NodeRegs n = load_node(S.nodes, cur);
            if (COUNT) ctr.nodes++;
            const bool enter = slab(n, o, inv, neg, tmin, tmax) | (n.count > 0 && (n.flags & kNodeAlways) != 0);
            if (enter) {
                if (n.count > 0) {
                    first = n.index;
                    count = n.count;
                    break;
                }
                if ((neg >> n.axis) & 1u) {  // children: left = flags, right = index
                    st.put(sp++, n.flags);
                    cur = n.index;
                } else {
                    st.put(sp++, n.index);
                    cur = n.flags;
                }
            } else {
                if (sp == 0) {
                    done = true;
                    break;
                }
                cur = st.get(--sp);
            }
        }
        for (uint32_t i = first; i < first + count; ++i) {  // the entered leaf's primitives
            const uint32_t ref = S.refs[i];
            double t;
            bool h;
            if (ref & kRefQuad) {
                if (COUNT) ctr.quad_tests++;
                h = hit_quad(S.quads[ref & ~kRefQuad], o, d, tmin, tmax, t);
            } else {
                if (COUNT) ctr.sphere_tests++;
                h = hit_sphere(S.spheres[ref], o, d, a, ia, tmin, tmax, lo, hi, t);
            }
            if (h) {
                tmax = t;
                hi = lim_tmax(t, a);
                hit_ref = ref;
                found = true;
            }
        }
        if (count > 0) {
            if (sp == 0) done = true;
            else cur = st.get(--sp);
        }
    }
    return found;
}

// Per-lane traversal state of the render kernel's current ray. The kernel advances it one BVH
// node per iteration (walk) and tests an entered leaf's primitives in a separate, batched phase;
// per lane the sequence of node tests and primitive tests is exactly trace()'s, i.e. the
// reference's BVH::hit_by.
enum : uint32_t { kWalk = 0, kLeaf = 1, kDone = 2, kIdle = 3 };

constexpr uint32_t kZeroDir = 8u;
// Trav::neg bits 4, 5: the ray is outside leaf_ray32's ranges (gate_leaf32) / div_a's (gate_recip).
// Clear for every ray that passes ray_gate (crt_ray_gate.h). The walks index Trav::neg by a node's
// split axis (0-2; 3 at the sentinel), so the bits are out of their way.
constexpr uint32_t kNoLeaf32 = 16u, kNoRecip = 32u;

struct Trav {
    // f32 copies for the walk's node test (walk()): inv32 = RN32(1/d), oinv32 = RN32(o * (1/d)),
    // marg = the per-ray part of the decision margin (inf: every node test is decided in f64)
    float inv32[3], oinv32[3];
    float marg;
    float tmax32;    // RN32(min(tmax, 2^100))
    double a;        // dot(d, d)
    double tmax;
    uint32_t cur, ref;
    int32_t sp;      // stack levels in use; -1 after the pop that follows the last leaf
    uint32_t first, count;  // the entered leaf's primitive range (walk -> leaf_step)
    uint32_t neg;    // bit k: d[k] < 0; kZeroDir: a slab value may be NaN (walk_step EXACT);
                     // kNoLeaf32: outside leaf_ray32's ranges (leaf_step tests every sphere
                     // exactly); kNoRecip: dot(d, d) outside div_a's range (it divides)
    uint32_t state;
    bool found;
};

__device__ __forceinline__ bool finite_nonzero(double x) { return fabs(x) < __builtin_inf() && x != 0; }
__device__ __forceinline__ bool finite(double x) { return fabs(x) < __builtin_inf(); }
__device__ __forceinline__ float tmax_f32(double t) { return static_cast<float>(fmin(t, 0x1p100)); }

// f32_ok: the scene's node bounds fit the f32 error analysis (Work::f32_ok)
__device__ __forceinline__ void trav_init(const double o[3], const double d[3], bool f32_ok, Trav& R) {
    R.a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    R.tmax = __builtin_inf();
    R.tmax32 = 0x1p100f;
    R.cur = 0;
    R.sp = 0;
    R.ref = 0;
    // The f32 walk's ray constants, in f32 (v12): inv32 = v_rcp_f32(RN32(d)) (within 1 ulp of
    // 1/RN32(d), so within 3.01u of 1/d), oinv32 = RN32(RN32(o) * inv32) (within 5.02u of o/d);
    // walk() bounds the resulting slab values for these. The analysis holds for
    // 2^-40 <= |1/d_k| <= 2^40 and |o_k| <= 2^40, here ensured by 2^-39 <= |RN32(d_k)| <= 2^39
    // (gate_walk_f32); other rays get marg = inf, i.e. every node test decided in f64.
    float d32[3], o32[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d32[k] = static_cast<float>(d[k]);
        o32[k] = static_cast<float>(o[k]);
        R.inv32[k] = __builtin_amdgcn_rcpf(d32[k]);
        R.oinv32[k] = o32[k] * R.inv32[k];
    }
    // (read only where f32 holds below: no NaN among the three then)
    const float A = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(R.oinv32[0]), __builtin_fabsf(R.oinv32[1])),
                                    __builtin_fabsf(R.oinv32[2]));
    // bit k: d[k] < 0 (not the sign bit: -0.0 is not negative)
    R.neg = (d[0] < 0 ? 1u : 0u) | (d[1] < 0 ? 2u : 0u) | (d[2] < 0 ? 4u : 0u);
    bool f32 = f32_ok;
    // The range checks of this ray, all four implied by ray_gate (the proof is in crt_ray_gate.h);
    // a wave with a lane outside the gate evaluates them one by one, as every set-up used to.
    // NaN-free slab values (the min/max and f32 walks): 1/d finite and non-zero, o finite. Rays
    // with a direction component outside [2^-1000, 2^1000] (zero, tiny, huge, NaN) take the EXACT
    // walk, which is the reference's select sequence for any ray.
    if (__builtin_expect(__ballot(!ray_gate(o32, d32)) != 0, 0)) {
        f32 = f32 && gate_walk_f32(o32, d32);
        R.neg |= (gate_walk_plain(o, d) ? 0u : kZeroDir) | (gate_leaf32(o, d, R.a) ? 0u : kNoLeaf32) |
                 (gate_recip(R.a) ? 0u : kNoRecip);
    }
    R.marg = f32 ? __builtin_fmaxf(A * 0x1p-19f, 0x1p-60f) : __builtin_inff();
    R.state = kWalk;
    R.found = false;
}

// ---- the render kernel's BVH walk ------------------------------------------------------------
// One node of the DFS (bvh.h:617-712 loop body without the leaf's primitive loop), branch-free:
// the node and the stack top are loaded in one batch, and the push / pop / leaf / done outcomes
// are selected rather than branched to (only the push is a masked store).
//
// Node test (AABB::is_hit_by_optimized, aabb.h:132-174). The reference swaps each axis' (t0, t1)
// by the sign of d and then narrows with "if (y > x) x = y"-style selects; for NaN-free slab
// values that is exactly
//   near = max_k min(t0_k, t1_k), far = min_k max(t0_k, t1_k),
//   enter = near <= far && near < tmax && far > tmin
// (c1 && c2 of the reference <=> every near_i <= far_j; +-0 ties only meet comparisons), with
// t_jk = RN(RN(b_jk - o_k) * inv_k) in f64. A slab value is NaN only for 0 * inf or inf - inf:
// rays whose 1/d is not finite and non-zero or whose origin is not finite (R.neg & kZeroDir), and
// scenes with an inverted / NaN node box (Work::exact_slab, where min/max would reorder the axis)
// take the EXACT variant: the reference's select sequence verbatim on the f64 node.
//
// The other rays decide the test in f32 first (Trav::inv32 / oinv32 / marg, DevNodeF):
//   t'_jk = fma(b32_jk, inv32_k, -oinv32_k),  b32 = RN32(b), inv32 = v_rcp_f32(RN32(d)) within
//   3.01u of inv = 1/d, oinv32 = RN32(RN32(o) * inv32) within 5.02u of o inv (trav_init; u =
//   2^-24). With A = max_k |o_k inv_k| and |b| <= |b - o| + |o|:
//   |t' - t| <= 4.01u |b||inv| + 5.02u |o||inv| + u |t'| + 2.01 u64 |t|
//            <= 5.02u |t'| + 9.04u A + 2^-85 = 2^-21.7 |t'| + 2^-20.8 A + 2^-85
// (2^-85: f32 underflow at |inv| <= 2^40). min / max are 1-Lipschitz, so lo' = max(near', tmin')
// and hi' = min(far', tmax') are within that bound of lo = max(near, tmin), hi = min(far, tmax)
// with |t'| <= M = max(|lo'|, |hi'|) (tmin', tmax' are RN32 of tmin, tmax, within u M; tmax' =
// 2^100 for larger tmax never binds, as |t'| < 2^82 here), and gap' = RN32(hi' - lo') is within
// 14.1u M + 18.1u A + 2^-84 <= 2^-20.1 M + 2^-19.8 A + 2^-84 of gap = hi - lo. So with
// th = 2^-19 M + marg, marg = max(2^-19 A', 2^-60), A' = max_k |oinv32_k| >= A (1 - 5.1u):
//   gap' >  th  =>  gap > 0: far > near, near < tmax, far > tmin  (enter)
//   gap' < -th  =>  gap < 0: far < near, far < tmin or tmax < near (no entry)
// and only lanes with |gap'| <= th (grazing rays, ties, rays with marg = inf) run the f64 test on
// the f64 node. Every decision is the f64 test's, so each ray visits the reference's node
// sequence. The f32 test is 18 single-rate instructions where the f64 one is 25 half-rate ones.
//
// Intervals of a query (query_kernel: any caller's t_min, a per-ray t_max of either sign, where the
// camera has t_min = 1e-5 and t_max = +inf shrinking to hit distances). The bound above used
// "tmin', tmax' are within u M of tmin, tmax", which takes |tmin|, |tmax| <= M for granted; it
// holds without that. Let E bound |near' - near|. RN32 is monotone and, for |tmin| <= 2^100,
// |tmin' - tmin| <= u |tmin| + 2^-150 (the second term: f32 underflow of a tiny t_min). Compare
// lo' = max(near', tmin') with lo = max(near, tmin):
//   both take the node's value: |lo' - lo| <= E; both take the bound: |lo' - lo| <= u |tmin| with
//   |tmin| <= |lo'| (1 + 2u) <= M (1 + 2u);
//   lo' = near' >= tmin' but tmin > near: then near' - E <= near < tmin <= tmin' + u |tmin| <=
//   near' + u |tmin|, so -E < lo - lo' <= u |tmin| and |tmin| <= (|near'| + E) (1 + 2u);
//   lo' = tmin' > near' but near >= tmin: then tmin' - u |tmin| <= tmin <= near <= near' + E <
//   tmin' + E, so |lo - lo'| <= max(E, u |tmin|) with |tmin| <= |lo'| (1 + 2u).
// In every case |lo' - lo| <= max(E, u (M + E)(1 + 2u)) + 2^-150: the bound's u M term, whatever
// the sign or size of t_min; hi' = min(far', tmax') likewise for -2^100 <= t_max <= 2^100. A
// larger t_max is 2^100 in f32 and never binds (|t'| < 2^82). So the call's f32 walk needs
// |t_min| <= 2^100 (device_trace clears Work::f32_ok otherwise); t_max > t_min >= -2^100 then
// holds for every traced ray, because a ray with an empty interval (t_max <= t_min) is never
// traced: it would fail the node test at the sentinel, the walks' only exit (query_kernel,
// crt_ray_class.h). The speculative and the pair walk rest on
// t_max only shrinking during a traversal and on the test being monotone in the box; neither
// depends on where the interval starts.
typedef __attribute__((address_space(3))) const unsigned char LdsByte;
struct NodeLines {
    Dvec2 b[3];  // (x.min, x.max), (y.min, y.max), (z.min, z.max)
    Uvec4 meta;  // index count axis flags
};
template <typename P>
__device__ __forceinline__ void node_lines(P p, NodeLines& n) {
    n.b[0] = p->b[0];
    n.b[1] = p->b[1];
    n.b[2] = p->b[2];
    n.meta = p->meta;
}
typedef __attribute__((address_space(1))) const NodeLines GlobalNode;
// the f64 node behind f32 ref `cur`
__device__ __forceinline__ GlobalNode* node64(const SceneView& S, uint32_t cur) {
    return (GlobalNode*)(S.nodes + (cur >> kNodeFShift));
}

// the f64 min/max test of a NaN-free ray (the f32 test's fallback)
__device__ __forceinline__ bool slab64(GlobalNode* p, const double o[3], const double d[3], double tmin,
                                       double tmax) {
    NodeLines nd;
    node_lines(p, nd);
    // divided here, in the rare branch: hoisted out of the walk loop, 1/d would hold 6 VGPRs
    double dx = d[0], dy = d[1], dz = d[2];
    asm volatile("" : "+v"(dx), "+v"(dy), "+v"(dz));
    const double inv[3] = {1 / dx, 1 / dy, 1 / dz};
    const Dvec2 bx = nd.b[0], by = nd.b[1], bz = nd.b[2];
    const double x0 = (bx.x - o[0]) * inv[0], x1 = (bx.y - o[0]) * inv[0];
    const double y0 = (by.x - o[1]) * inv[1], y1 = (by.y - o[1]) * inv[1];
    const double z0 = (bz.x - o[2]) * inv[2], z1 = (bz.y - o[2]) * inv[2];
    const double near = fmax(fmax(fmin(x0, x1), fmin(y0, y1)), fmin(z0, z1));
    const double far = fmin(fmin(fmax(x0, x1), fmax(y0, y1)), fmax(z0, z1));
    return (near <= far) & (near < tmax) & (far > tmin);
}

// the same test with the lane's 1 / d read from LDS (S.inv64_lds, written by the traversal set-up
// with the same division): the flat-parallelogram instances, whose walk decides ~28% of its
// iterations in f64 (Cornell's box faces lie on node bounds)
__device__ __forceinline__ bool slab64_inv(GlobalNode* p, const double o[3], uint32_t inv_lds, double tmin,
                                           double tmax) {
    NodeLines nd;
    node_lines(p, nd);
    typedef __attribute__((address_space(3))) const double LdsDoubleC;
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));  // recomputed here, not held live across the walk
    LdsDoubleC* q = (LdsDoubleC*)static_cast<uintptr_t>(inv_lds + t * 8);
    const double inv[3] = {q[0], q[kBlock], q[2 * kBlock]};
    const Dvec2 bx = nd.b[0], by = nd.b[1], bz = nd.b[2];
    const double x0 = (bx.x - o[0]) * inv[0], x1 = (bx.y - o[0]) * inv[0];
    const double y0 = (by.x - o[1]) * inv[1], y1 = (by.y - o[1]) * inv[1];
    const double z0 = (bz.x - o[2]) * inv[2], z1 = (bz.y - o[2]) * inv[2];
    const double near = fmax(fmax(fmin(x0, x1), fmin(y0, y1)), fmin(z0, z1));
    const double far = fmin(fmin(fmax(x0, x1), fmax(y0, y1)), fmax(z0, z1));
    return (near <= far) & (near < tmax) & (far > tmin);
}

// The 32-byte f32 node at ref `cur`: LS kernels hold all nodes in LDS at offset 0 (the LDS
// pointer is the ref itself: render_kernel checks that its dynamic LDS starts at address 0),
// TOP kernels the first S.ntop bytes of them; the rest is read from HBM, with a separate masked
// load into the same registers (no per-lane pointer select, no flat loads).
struct NodeF {
    Uvec4 q0;  // x.min x.max y.min y.max (f32 bits)
    Uvec4 q1;  // z.min z.max w0 w1
};
typedef __attribute__((address_space(3))) const NodeF LdsNodeF;
typedef __attribute__((address_space(1))) const NodeF GlobalNodeF;
template <bool TOP, bool LS>
__device__ __forceinline__ void fetch_nodef(const SceneView& S, uint32_t cur, Uvec4& q0, Uvec4& q1) {
    if (LS) {
        LdsNodeF* p = (LdsNodeF*)static_cast<uintptr_t>(cur);
        q0 = p->q0;
        q1 = p->q1;
    } else if (TOP) {
        // Lanes below the treelet read HBM, the others LDS, into the same registers. Written as C,
        // the compiler waits for the HBM loads before it issues the LDS reads (it cannot know that
        // the two exec masks are disjoint, so it orders the register writes), which puts the LDS
        // latency behind the HBM latency in every step of a wave with lanes on both sides. Here
        // both are in flight together, and the statement waits for both (its loads are outside
        // the compiler's counters).
        // A side whose mask is empty is branched over: a vector-memory instruction issued with
        // EXEC = 0 still takes its slot in the address / data units (TA / TD, config 4's
        // binding resource), and a wave whose lanes are all in the treelet (or all below it)
        // is common at the start (end) of its rays' traversals.
        const uint64_t hbm = __ballot(cur >= S.ntop);
        uint64_t save;
        asm volatile(
            "s_and_saveexec_b64 %[save], %[hbm]\n\t"
            "s_cbranch_execz 1f\n\t"
            "global_load_dwordx4 %[q0], %[cur], %[base]\n\t"
            "global_load_dwordx4 %[q1], %[cur], %[base] offset:16\n"
            "1:\n\t"
            "s_andn2_b64 exec, %[save], %[hbm]\n\t"
            "s_cbranch_execz 2f\n\t"
            "ds_read_b128 %[q0], %[cur]\n\t"
            "ds_read_b128 %[q1], %[cur] offset:16\n"
            "2:\n\t"
            "s_mov_b64 exec, %[save]\n\t"
            "s_waitcnt vmcnt(0) lgkmcnt(0)"
            : [q0] "=&v"(q0), [q1] "=&v"(q1), [save] "=&s"(save)
            : [cur] "v"(cur), [hbm] "s"(hbm), [base] "s"(S.fnodes)
            : "memory");
    } else {
        GlobalNodeF* p = (GlobalNodeF*)(reinterpret_cast<const char*>(S.fnodes) + cur);
        q0 = p->q0;
        q1 = p->q1;
    }
}

// The node's two words (w0, w1: bytes 24-31) alone, the same way
typedef uint32_t Uvec2 __attribute__((ext_vector_type(2)));
template <bool TOP, bool LS>
__device__ __forceinline__ Uvec2 fetch_nodef_words(const SceneView& S, uint32_t cur) {
    typedef __attribute__((address_space(3))) const Uvec2 LdsU2;
    typedef __attribute__((address_space(1))) const Uvec2 GlobalU2;
    if (LS) return *(LdsU2*)static_cast<uintptr_t>(cur + 24);
    if (!TOP) return *(GlobalU2*)(reinterpret_cast<const char*>(S.fnodes) + cur + 24);
    const uint64_t hbm = __ballot(cur >= S.ntop);
    uint64_t save;
    Uvec2 w;
    asm volatile(
        "s_and_saveexec_b64 %[save], %[hbm]\n\t"
        "s_cbranch_execz 1f\n\t"
        "global_load_dwordx2 %[w], %[cur], %[base] offset:24\n"
        "1:\n\t"
        "s_andn2_b64 exec, %[save], %[hbm]\n\t"
        "s_cbranch_execz 2f\n\t"
        "ds_read_b64 %[w], %[cur] offset:24\n"
        "2:\n\t"
        "s_mov_b64 exec, %[save]\n\t"
        "s_waitcnt vmcnt(0) lgkmcnt(0)"
        : [w] "=&v"(w), [save] "=&s"(save)
        : [cur] "v"(cur), [hbm] "s"(hbm), [base] "s"(S.fnodes)
        : "memory");
    return w;
}

// The lane's miss link at node ref `cur` (LINK instances): lbase = S.links_lds + 2 * octant
typedef __attribute__((address_space(3))) const uint16_t LdsU16;
__device__ __forceinline__ uint16_t link16_at(uint32_t lbase, uint32_t cur) {
    return *(LdsU16*)static_cast<uintptr_t>(lbase + (cur >> 1));
}
__device__ __forceinline__ uint32_t link_at(uint32_t lbase, uint32_t cur) { return link16_at(lbase, cur); }

// ---- the stackless form (LINK: the five-wave LDS-scene render instances) -----------------------
// BVH::hit_by (bvh.h:684-698) picks the near child by dir_is_negative[split_axis] alone, so a
// ray's DFS order is fixed by its three sign bits (the octant, R.neg & 7), whatever t_max does.
// The node a pop returns is therefore a static function of (node, octant): miss(root, o) = the
// sentinel, and for an interior node N whose near and far children under o are n and f,
// miss(n, o) = f and miss(f, o) = miss(N, o). With that table (crt_walk_links.h, staged in the
// bytes the plan keeps for the guard levels and the stack) a step is
//   cur = (enter && interior) ? near : miss[cur][o],
// an entered leaf continues at its own miss link after its primitives (the stack walk's pop after
// the leaf), and the traversal ends at the sentinel, whose links point to itself (so the "reached
// the sentinel with no leaf recorded" case re-tests the sentinel like the second guard level made
// it do, and parks). No push, no pop, no stack pointer, no guard levels, no R.sp. At every step the
// stack walk's top IS miss(cur, o): by induction, pushing f on entering N leaves the top f =
// miss(n, o) for n, and a pop below f exposes what was the top at N, miss(N, o) = miss(f, o). So
// the visited node sequence is the stack walk's, and every primitive test, tie and frame bit
// stays the same. The speculative walk's argument above (monotone node test, t_max only shrinking)
// speaks of the order of the nodes alone and never of the stack, so it holds as it stands; a
// parked lane stays on its node.
//
// The speculative link walk's loop of the sphere-only instance, written out (link_spec_steps).
// The loop is the wave's and a divergent one: a parking lane leaves it. Written in C++, the
// compiler keeps "still in the loop" as exec and re-merges every lane mask that lives across the
// loop's blocks with it (three s_andn2 / s_and / s_or each), and the exec-masked select saves and
// restores exec: 24 scalar instructions a step beside the 28 vector ones, at an issue cost of
// about one vector instruction each. The block below owns the loop, so that the compiler never
// sees exec differ from the call's mask: it saves exec on entry, restores it on every exit, and
// inside it exec IS the mask of the lanes still in the loop. A lane that has recorded its first
// leaf is then exec & ~nop, a parking lane leaves exec before the select of the next node (so it
// keeps its node with no saved exec), and the step's mask algebra is 8 scalar instructions and
// the f64 branch. The flat-parallelogram instance (G2 = false) keeps the C++ loop: it sends 28 %
// of its steps to the f64 test, and leaving and re-entering the block that often cost it more
// than the scalar instructions saved (config 3 +0.5 ms in every round).
//
// One step of a lane, from the node test's `enter` and the node's `leaf` bit (leaf: or the
// sentinel). x: either value.
//   in loop  nop  enter  leaf | in loop'  nop'  pref'  cur'
//      0      x     x     x   |    0       0    pref   cur     not in exec: nothing written
//      1      x     0     x   |    1      nop   pref   link    missed the node
//      1      x     1     0   |    1      nop   pref   near    entered an interior node
//      1      1     1     1   |    1       0    cur    link    first leaf: recorded, walks on
//      1      0     1     1   |    0       0    pref   cur     second leaf: parks
// A lane that reaches the sentinel with nothing recorded is row four: it records the sentinel,
// follows its link to itself and parks there in its next step, row five. With rm = enter & leaf:
// first = rm & nop (pref <- cur), park = rm & ~nop, nop' = nop & ~rm, exec' = exec & ~park, cur'
// on exec' = (enter & ~leaf) ? near : link.
// This is the C++ step's `rec` (= in loop & ~nop), `pm`, `on` and vsel_top_on, lane for lane
// (tests/test_walk_step_masks.py enumerates the rows against a per-lane restatement of it).
// Termination: only rm lanes park and they leave nop in the same step, so nop is a subset of
// exec at every step and the loop's test "nop != 0" never runs on an empty exec; a lane at the
// sentinel always enters it (its box is unbounded), so it gets rm, and every lane reaches the
// sentinel after finitely many links. The trip count is the C++ loop's: that one also ends when
// nop empties or the last lane parks, and a step in which the last lane parks empties nop.
//
// The rare f64 decision stays in C++: when a lane of exec is undecided (|gap| <= th) the block
// restores exec and hands back `in` = the loop's exec (never empty there) and, per lane, dec = 0
// on the undecided lanes of the loop, the f32 gap (never 0 when decided: th > 0) on its other
// lanes and 1 outside it. The caller replaces the zeros by the f64 verdict's sign and calls the
// block again, which sees in != 0, takes exec = in, reads the node's words and the link again
// (cur has not moved) and continues at the mask algebra. A finished walk returns in = 0.
// No exit leaves a load pending: the block's reads are outside the compiler's wait counters, and
// their registers are the compiler's again at once after the statement, so the loop's exit comes
// after the step's lgkmcnt(0) and the hand-back waits for the link's read (still in flight at
// the "undecided" branch) before it leaves.
// COUNT: the block counts the loop's lanes on a node other than the sentinel (nodes) and its own
// trips (steps, per wave). The node's two reads land in fixed registers, q0 = v[8:11] and q1 =
// v[4:7] (clobbered): an operand cannot name one register of a 128-bit tuple.
#define CRT_LINK_STEPS_ASM(COUNT_STEP, COUNT_CMP, COUNT_ADD)                                          \
    "s_mov_b64 %[save], exec\n\t"                                                                         \
    "s_cmp_lg_u64 %[in], 0\n\t"                                                                           \
    "s_cbranch_scc1 3f\n"                                                                                 \
    "0:\n\t"                                                                                              \
    "ds_read_b128 v[8:11], %[cur]\n\t"                                                                    \
    "ds_read_b128 v[4:7], %[cur] offset:16\n\t"                                                           \
    "v_lshrrev_b32_e32 %[top], 1, %[cur]\n\t"                                                                \
    "v_add_u32_e32 %[top], %[lbase], %[top]\n\t"                                                                \
    "ds_read_u16 %[top], %[top]\n\t"                                                                            \
    COUNT_STEP                                                                                            \
    "s_waitcnt lgkmcnt(2)\n\t"                                                                            \
    "v_fma_f32 v8, v8, %[i0], -%[o0]\n\t"                                                                 \
    "v_fma_f32 v9, v9, %[i0], -%[o0]\n\t"                                                                 \
    "v_fma_f32 v10, v10, %[i1], -%[o1]\n\t"                                                               \
    "v_fma_f32 v11, v11, %[i1], -%[o1]\n\t"                                                               \
    "v_min_f32_e32 %[dec], v8, v9\n\t"                                                                    \
    "v_max_f32_e32 v8, v8, v9\n\t"                                                                        \
    "v_min_f32_e32 v9, v10, v11\n\t"                                                                      \
    "v_max_f32_e32 v10, v10, v11\n\t"                                                                     \
    "s_waitcnt lgkmcnt(1)\n\t"                                                                            \
    COUNT_CMP                                                                                             \
    "v_fma_f32 v4, v4, %[i2], -%[o2]\n\t"                                                                 \
    "v_fma_f32 v5, v5, %[i2], -%[o2]\n\t"                                                                 \
    COUNT_ADD                                                                                             \
    "v_min_f32_e32 v11, v4, v5\n\t"                                                                       \
    "v_max_f32_e32 v4, v4, v5\n\t"                                                                        \
    "v_max_f32_e32 v11, %[tmin], v11\n\t"                                                                 \
    "v_min_f32_e32 v4, v4, %[tmax]\n\t"                                                                   \
    "v_max3_f32 v9, %[dec], v9, v11\n\t"                                                                  \
    "v_min3_f32 v8, v8, v10, v4\n\t"                                                                      \
    "v_sub_f32_e32 %[dec], v8, v9\n\t"                                                                    \
    "v_max_f32_e64 v8, |v9|, |v8|\n\t"                                                                    \
    "v_fmamk_f32 v8, v8, 0x36000000, %[marg]\n\t"                                                         \
    "v_cmp_ngt_f32_e64 vcc, |%[dec]|, v8\n\t"                                                             \
    "s_cbranch_vccnz 2f\n\t"                                                                              \
    "v_cmp_lt_f32_e32 vcc, 0, %[dec]\n"                                                                   \
    "1:\n\t"                                                                                              \
    "v_cmp_gt_i32_e64 %[lm], 0, v7\n\t"                                                                   \
    "v_bfe_u32 v8, %[neg], v6, 1\n\t"                                                                     \
    "v_lshl_or_b32 v8, v8, 5, v7\n\t"                                                                     \
    "s_and_b64 %[lm], vcc, %[lm]\n\t"                                                                     \
    "s_andn2_b64 vcc, vcc, %[lm]\n\t"                                                                     \
    "s_and_b64 %[in], %[lm], %[nop]\n\t"                                                                  \
    "v_cndmask_b32_e64 %[pref], %[pref], %[cur], %[in]\n\t"                                               \
    "s_andn2_b64 %[in], %[lm], %[nop]\n\t"                                                                \
    "s_andn2_b64 %[nop], %[nop], %[lm]\n\t"                                                               \
    "s_andn2_b64 exec, exec, %[in]\n\t"                                                                   \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                            \
    "v_cndmask_b32_sdwa %[cur], %[top], v8, vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:DWORD\n\t" \
    "s_cmp_lg_u64 %[nop], 0\n\t"                                                                          \
    "s_cbranch_scc1 0b\n\t"                                                                               \
    "s_mov_b64 exec, %[save]\n\t"                                                                         \
    "s_mov_b64 %[in], 0\n\t"                                                                              \
    "s_branch 4f\n"                                                                                       \
    "2:\n\t" /* undecided lanes in vcc: hand back, with the link's read landed */                          \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                            \
    "s_mov_b64 %[in], exec\n\t"                                                                           \
    "s_nop 1\n\t"                                                                                         \
    "v_cndmask_b32_e64 %[dec], %[dec], 0, vcc\n\t"                                                        \
    "s_andn2_b64 exec, %[save], %[in]\n\t"                                                                \
    "v_mov_b32_e32 %[dec], 1.0\n\t"                                                                       \
    "s_mov_b64 exec, %[save]\n\t"                                                                         \
    "s_branch 4f\n"                                                                                       \
    "3:\n\t" /* called again with the f64 verdicts in dec */                                              \
    "s_mov_b64 exec, %[in]\n\t"                                                                           \
    "ds_read_b64 v[6:7], %[cur] offset:24\n\t"                                                            \
    "v_lshrrev_b32_e32 %[top], 1, %[cur]\n\t"                                                                \
    "v_add_u32_e32 %[top], %[lbase], %[top]\n\t"                                                                \
    "ds_read_u16 %[top], %[top]\n\t"                                                                            \
    "v_cmp_lt_f32_e32 vcc, 0, %[dec]\n\t"                                                                 \
    "s_waitcnt lgkmcnt(0)\n\t"                                                                            \
    "s_branch 1b\n"                                                                                       \
    "4:"
// COUNT: the wave's trips; the loop's lanes off the sentinel (the carry-in two instructions after
// its compare: a VALU read of a VALU-written mask needs two wait states)
#define CRT_LINK_COUNT_STEP "s_add_u32 %[steps], %[steps], 1\n\t"
#define CRT_LINK_COUNT_CMP "v_cmp_ne_u32_e32 vcc, -1, v7\n\t"
#define CRT_LINK_COUNT_ADD "v_addc_co_u32_e32 %[nodes], vcc, 0, %[nodes], vcc\n\t"
#define CRT_LINK_STEPS_OUT [cur] "+v"(cur), [pref] "+v"(pref), [dec] "+v"(dec), [nop] "+s"(nop), [in] "+s"(in), \
                           [save] "=&s"(save), [lm] "=&s"(lm), [top] "=&v"(top)
#define CRT_LINK_STEPS_IN [lbase] "v"(lbase), [i0] "v"(R.inv32[0]), [i1] "v"(R.inv32[1]), [i2] "v"(R.inv32[2]),  \
                          [o0] "v"(R.oinv32[0]), [o1] "v"(R.oinv32[1]), [o2] "v"(R.oinv32[2]), [tmax] "v"(R.tmax32), \
                          [marg] "v"(R.marg), [neg] "v"(R.neg), [tmin] "s"(tmin32)
#define CRT_LINK_STEPS_CLOBBER "v4", "v5", "v6", "v7", "v8", "v9", "v10", "v11", "vcc", "scc"

// The loop of walk<SPEC, LINK> of the sphere-only instance: every lane of the call from R.cur to
// its first entered leaf recorded in `pref` (or the sentinel) and on to where it parks, `cur`
template <bool COUNT>
__device__ __forceinline__ void link_spec_steps(const SceneView& S, const double o[3], const double d[3], double tmin,
                                                float tmin32, const Trav& R, uint32_t lbase, uint32_t& cur, uint32_t& pref,
                                                LaneCounters& ctr) {
    uint64_t nop = __ballot(true);  // the lanes of this call
    uint64_t in = 0;                // the loop's exec at a hand-back; 0: not in the loop
    uint64_t save, lm;
    float dec;
    uint32_t top, steps = 0;
    asm volatile("" : "=v"(dec), "=v"(pref));  // written before they are read: every lane records a node
    for (;;) {
        if constexpr (COUNT) {
            asm volatile(CRT_LINK_STEPS_ASM(CRT_LINK_COUNT_STEP, CRT_LINK_COUNT_CMP, CRT_LINK_COUNT_ADD)
                         : CRT_LINK_STEPS_OUT, [nodes] "+v"(ctr.nodes), [steps] "+s"(steps)
                         : CRT_LINK_STEPS_IN
                         : CRT_LINK_STEPS_CLOBBER);
        } else {
            asm volatile(CRT_LINK_STEPS_ASM("", "", "")
                         : CRT_LINK_STEPS_OUT
                         : CRT_LINK_STEPS_IN
                         : CRT_LINK_STEPS_CLOBBER);
        }
        if (__builtin_expect(in == 0, 1)) break;
        if (COUNT && wave_leader()) ctr.it_slow++;
        if (dec == 0.f) {
            if (COUNT) ctr.slow_nodes++;
            dec = slab64(node64(S, cur), o, d, tmin, R.tmax) ? 1.f : -1.f;
        }
    }
    if (COUNT && wave_leader()) ctr.it_walk += steps;
}

template <typename SE, bool COUNT, bool EXACT, bool TOP, bool LS, bool GS, bool SPEC, bool INVL = false, bool G2 = true,
          bool LINK = false>
__device__ __forceinline__ void walk(const SceneView& S, Stack<SE>& st, const double o[3], const double d[3],
                                     double tmin, float tmin32, Trav& R, LaneCounters& ctr) {
    static_assert(!LINK || (LS && !GS && !TOP), "miss links are staged by the LDS-scene instances only");
    // Every step ends with the next node in `cur`: the near child of an entered interior node,
    // else the stack top, popped. The level below the stack holds the sentinel node, entered by
    // every ray, so popping an empty stack leads to the sentinel and the only exit is "entered a
    // node with primitives" (a leaf, or the sentinel: traversal over). An entered leaf ends the
    // walk already popped (the reference pops right after the leaf's primitive loop, which leaves
    // the stack unchanged); its primitive range goes to leaf_step in R.first / R.count. So the
    // loop body has no branch but that exit (and the rare f64 decision), and every lane makes
    // the same updates.
    // The stack is walked with a pointer to its top level (level sp - 1). The far child is stored
    // at level sp whatever the outcome (above the live stack unless it is pushed; the stack has
    // depth + 1 levels); at the sentinel that store rewrites the guard level with the sentinel's
    // own reference, and the speculative read of the top reads the level below the guard (in
    // bounds: the host keeps it inside the allocation).
    // LINK: no stack (st is never read); `top` below is the lane's miss link at `cur`, read with
    // the node like the speculative pop it replaces
    const ptrdiff_t stride = LINK ? 0 : static_cast<ptrdiff_t>(st.stride);
    SE* const empty = LINK ? nullptr : st.base - stride;
    SE* tp = LINK ? nullptr : st.base + (static_cast<ptrdiff_t>(R.sp) - 1) * stride;
    const uint32_t lbase = LINK ? S.links_lds + ((R.neg & 7u) << 1) : 0u;
    uint32_t cur = R.cur;
    uint32_t w0, w1;  // the last node's DevNodeF words (leaf / sentinel at the exit)
    bool stop;
    if (EXACT) {
        // divided here: without the barrier the compiler hoists these three divisions out of
        // the traversal rounds into every shade round, although the EXACT walk is rare
        double dx = d[0], dy = d[1], dz = d[2];
        uint32_t neg = R.neg;  // likewise the three sign masks
        asm volatile("" : "+v"(dx), "+v"(dy), "+v"(dz), "+v"(neg));
        const double inv[3] = {1 / dx, 1 / dy, 1 / dz};
        do {
            NodeLines nd;
            node_lines(node64(S, cur), nd);
            const Uvec4 meta = nd.meta;  // index count axis flags
            const uint32_t top = LINK ? link_at(lbase, cur) : *tp;  // speculative pop
            if (COUNT) {
                if (meta.y != kSentinelCount) ctr.nodes++;
                if (wave_leader()) ctr.it_walk++;
            }
            // x[neg] / x[!neg]
            const bool nx = neg & 1u, ny = (neg >> 1) & 1u, nz = (neg >> 2) & 1u;
            const double bx0 = nx ? nd.b[0].y : nd.b[0].x, bx1 = nx ? nd.b[0].x : nd.b[0].y;
            const double by0 = ny ? nd.b[1].y : nd.b[1].x, by1 = ny ? nd.b[1].x : nd.b[1].y;
            const double bz0 = nz ? nd.b[2].y : nd.b[2].x, bz1 = nz ? nd.b[2].x : nd.b[2].y;
            double xtmin = (bx0 - o[0]) * inv[0];
            double xtmax = (bx1 - o[0]) * inv[0];
            const double ytmin = (by0 - o[1]) * inv[1];
            const double ytmax = (by1 - o[1]) * inv[1];
            const double ztmin = (bz0 - o[2]) * inv[2];
            const double ztmax = (bz1 - o[2]) * inv[2];
            const bool c1 = !(xtmin > ytmax || ytmin > xtmax);
            if (ytmin > xtmin) xtmin = ytmin;
            if (ytmax < xtmax) xtmax = ytmax;
            const bool c2 = !(xtmin > ztmax || ztmin > xtmax);
            if (ztmin > xtmin) xtmin = ztmin;
            if (ztmax < xtmax) xtmax = ztmax;
            const bool enter = (c1 & c2 & (xtmin < R.tmax) & (xtmax > tmin)) |
                               (meta.y != 0 && (meta.w & kNodeAlways) != 0) | (meta.y == kSentinelCount);
            const bool inner = enter & (meta.y == 0);
            const bool far_first = (neg >> meta.z) & 1u;
            const uint32_t left = meta.w << kNodeFShift, right = meta.x << kNodeFShift;
            if (!LINK) tp[stride] = static_cast<SE>(far_first ? left : right);
            stop = enter ^ inner;  // entered, not interior: a leaf or the sentinel
            cur = inner ? (far_first ? right : left) : top;
            if (!LINK) tp += inner ? stride : -stride;
            w0 = meta.x;
            w1 = meta.y == kSentinelCount ? kSentinelW1 : (kLeafFlagF | meta.y);
        } while (!stop);
    } else if constexpr (SPEC && LINK && G2 && !CRT_WATCHDOG) {
        // the speculative walk below with its loop written out (link_spec_steps); a watchdog
        // build keeps the C++ loop, which can check its deadline in every step
        uint32_t pref;
        static_assert(!INVL, "link_spec_steps decides in f64 with slab64: no 1 / d in LDS in this instance");
        link_spec_steps<COUNT>(S, o, d, tmin, tmin32, R, lbase, cur, pref, ctr);
        const Uvec2 w = fetch_nodef_words<TOP, LS>(S, pref);
        R.state = w.y == kSentinelW1 ? kDone : kLeaf;
        R.first = w.x;
        R.count = w.y & ~kLeafFlagF;
        R.cur = cur;
        return;
    } else if (SPEC) {
        // Speculative walk (Aila & Laine's postponed leaves): a lane that enters its first leaf
        // records it and walks on, with its t_max of now, until it enters a second leaf (or
        // the sentinel), where it parks without moving: that node is the next round's first
        // step and is tested again then. The wave's loop runs while some lane still walks to
        // its first leaf, so lanes that find theirs early keep doing DFS steps instead of idling.
        // The primitive tests are the reference's, in its order: the DFS order does not depend
        // on t_max; a node entered here with the t_max of before the recorded leaf's tests is
        // either entered under the smaller t_max too, or the reference culls it, and then it
        // also culls (i) the parked node, tested again, and (ii) every far child pushed below
        // it, tested at its pop — their boxes lie inside the culled one, and the rounded slab
        // values are monotone in the bounds (near(child) >= near(parent), far(child) <=
        // far(parent)), so the test fails for them at any t_max the culled one failed at.
        // Only node visits are added. The stack stays within depth + 1 levels: it is the same DFS.
        // The loop is the wave's, and a divergent one: a parking lane leaves it (`break`), which
        // takes it out of the exec mask of every later step; the loop ends for the lanes still in
        // it when no lane of the wave is on its way to a first leaf any more. A lane parks by not
        // moving: the step's update of `cur` and of the stack pointer is made on the lanes of
        // exec & ~park alone (vsel_top_on), so the lane keeps the parked node and, in the stack
        // forms, the stack pointer of before the step (what popping, remembering the node and
        // undoing the pop after the loop gave, for a select a step and a VGPR more).
        // Whether a lane still walks to its first leaf is the lane mask `nop` (scalar registers),
        // cleared by scalar logic at that leaf (or at the sentinel when the lane entered it with
        // no leaf recorded: traversal over); the recorded node is `pref`. The loop's exit test is
        // a scalar compare of the mask, and every lane leaves the loop with a node recorded, so
        // `pref` needs no "none yet" value and no compare of its own.
        // The node sequence is unchanged: a running lane's `cur`, stack pointer and stack
        // stores are exactly those of the pop-and-undo form at every step (the parking step is
        // the lane's last, and its unconditional store at tp[stride] lands where it always did);
        // `nop` is cleared in the very step in which `pref` used to leave ~0u, so `park` and the
        // loop's trip count are the same; and a parked lane ends on the same (cur, tp) as after
        // the undo.
        // How it is written follows the compiler: masks come from ballots of fresh
        // compares only (a ballot of a lane boolean merged across blocks costs two vector
        // instructions); `nop` is updated in the loop's own body, not under an `if`, or it moves
        // to VGPRs; `park` exists as a lane boolean too, for the break, built from positive terms
        // (`rec` = a leaf is recorded, the complement of `nop`), because every negated lane
        // boolean is answered with the inverse vector compare.
        bool rec = false;
        uint64_t nop = __ballot(true);  // the lanes of this call
        uint32_t pref = 0;
        for (;;) {
            CRT_WD(4, cur, static_cast<uint32_t>(tp - empty));
            {
                Uvec4 q0, q1;
                fetch_nodef<TOP, LS>(S, cur, q0, q1);
                w0 = q1.z;
                w1 = q1.w;
                // speculative pop, in its own width (vsel_top_on)
                const auto top = [&] {
                    if constexpr (LINK) return link16_at(lbase, cur);
                    else return *tp;
                }();
                if (COUNT) {
                    if (w1 != kSentinelW1) ctr.nodes++;
                    if (wave_leader()) ctr.it_walk++;
                }
                const float x0 = __builtin_fmaf(__uint_as_float(q0.x), R.inv32[0], -R.oinv32[0]);
                const float x1 = __builtin_fmaf(__uint_as_float(q0.y), R.inv32[0], -R.oinv32[0]);
                const float y0 = __builtin_fmaf(__uint_as_float(q0.z), R.inv32[1], -R.oinv32[1]);
                const float y1 = __builtin_fmaf(__uint_as_float(q0.w), R.inv32[1], -R.oinv32[1]);
                const float z0 = __builtin_fmaf(__uint_as_float(q1.x), R.inv32[2], -R.oinv32[2]);
                const float z1 = __builtin_fmaf(__uint_as_float(q1.y), R.inv32[2], -R.oinv32[2]);
                const float lo = vmax3(vmin(x0, x1), vmin(y0, y1), vmax_s(vmin(z0, z1), tmin32));
                const float hi = vmin3(vmax(x0, x1), vmax(y0, y1), vmin(vmax(z0, z1), R.tmax32));
                const float gap = hi - lo;
                const float th = __builtin_fmaf(vmax_abs(lo, hi), 0x1p-19f, R.marg);
                // The step's outcomes as lane masks (ballots of the compares: scalar algebra, and
                // selects on the masks). The f64 decision comes back as the sign of `dec`, so that
                // "entered" is one compare after the rare branch and not a boolean merged across
                // it. Only `park` is a lane boolean as well (the loop's divergent exit), built
                // from the same two compares.
                float dec = gap;
                const bool unc = !(fabsf(gap) > th);
                if (__builtin_expect(__ballot(unc) != 0, 0)) {
                    if (COUNT && wave_leader()) ctr.it_slow++;
                    if (unc) {
                        if (COUNT) ctr.slow_nodes++;
                        dec = (INVL ? slab64_inv(node64(S, cur), o, S.inv64_lds, tmin, R.tmax)
                                    : slab64(node64(S, cur), o, d, tmin, R.tmax)) ? 1.f : -1.f;
                    }
                }
                const bool enter = dec > 0.f, leaf = w1 >= kLeafFlagF;  // leaf: or the sentinel
                const uint64_t em = __ballot(enter), lm = __ballot(leaf);
                const uint64_t im = em & ~lm;  // entered, interior
                const uint64_t rm = em & lm;   // reached: entered a leaf or the sentinel
                const uint32_t near = w1 | (__builtin_amdgcn_ubfe(R.neg, w0, 1) << kNodeFShift);
                if (!LINK) tp[stride] = static_cast<SE>(near ^ (1u << kNodeFShift));
                // a lane that reaches the sentinel with no leaf recorded records it and pops the
                // second guard level, which holds the sentinel too (LINK: follows the sentinel's
                // link to itself): it parks there, with a leaf recorded (one compare fewer a step
                // than testing for the sentinel here; G2 = false: the compare, for the
                // flat-parallelogram instances, whose five-wave register allocation spilled 14
                // VGPRs instead of 8 without it)
                const bool reached = enter && leaf;
                const bool park = reached && (rec || (!G2 && w1 == kSentinelW1));
                const uint64_t pm = rm & (G2 ? ~nop : (~nop | __ballot(w1 == kSentinelW1)));
                pref = vsel(rm & nop, cur, pref);  // the first leaf (or the sentinel)
                nop &= ~rm;
                rec = rec || reached;
                // a parking lane stays on its node, its stack pointer unmoved, and leaves the loop
                const uint64_t on = __ballot(true) & ~pm;
                cur = vsel_top_on(on, im, near, top, cur);
                if (!LINK) tp += static_cast<int32_t>(vsel(im & on, static_cast<uint32_t>(stride), vsel(on, static_cast<uint32_t>(-stride), 0u)));
                if (park) break;
            }
            if (nop == 0) break;
        }
        // the recorded node's words (a leaf's primitive range, or the sentinel: traversal over)
        {
            const Uvec2 w = fetch_nodef_words<TOP, LS>(S, pref);
            w0 = w.x;
            w1 = w.y;
        }
        R.state = w1 == kSentinelW1 ? kDone : kLeaf;
        R.first = w0;
        R.count = w1 & ~kLeafFlagF;
        R.cur = cur;
        if (!LINK) R.sp = static_cast<int32_t>(static_cast<uint32_t>(tp - empty)) / static_cast<int32_t>(st.stride);
        return;
    } else {
        do {
            CRT_WD(5, cur, static_cast<uint32_t>(tp - empty));
            Uvec4 q0, q1;
            fetch_nodef<TOP, LS>(S, cur, q0, q1);
            w0 = q1.z;
            w1 = q1.w;
            const uint32_t top = LINK ? link_at(lbase, cur) : *tp;  // speculative pop
            if (COUNT) {
                if (w1 != kSentinelW1) ctr.nodes++;
                if (wave_leader()) ctr.it_walk++;
            }
            // the sentinel and linear-mode leaves carry [-inf, inf] boxes: entered (lo' = tmin',
            // hi' = tmax')
            const float x0 = __builtin_fmaf(__uint_as_float(q0.x), R.inv32[0], -R.oinv32[0]);
            const float x1 = __builtin_fmaf(__uint_as_float(q0.y), R.inv32[0], -R.oinv32[0]);
            const float y0 = __builtin_fmaf(__uint_as_float(q0.z), R.inv32[1], -R.oinv32[1]);
            const float y1 = __builtin_fmaf(__uint_as_float(q0.w), R.inv32[1], -R.oinv32[1]);
            const float z0 = __builtin_fmaf(__uint_as_float(q1.x), R.inv32[2], -R.oinv32[2]);
            const float z1 = __builtin_fmaf(__uint_as_float(q1.y), R.inv32[2], -R.oinv32[2]);
            const float lo = vmax3(vmin(x0, x1), vmin(y0, y1), vmax_s(vmin(z0, z1), tmin32));
            const float hi = vmin3(vmax(x0, x1), vmax(y0, y1), vmin(vmax(z0, z1), R.tmax32));
            const float gap = hi - lo;
            const float th = __builtin_fmaf(vmax_abs(lo, hi), 0x1p-19f, R.marg);
            bool enter = gap > 0.f;
            const bool unc = !(fabsf(gap) > th);
            if (__builtin_expect(__ballot(unc) != 0, 0)) {
                if (COUNT && wave_leader()) ctr.it_slow++;
                if (unc) {
                    if (COUNT) ctr.slow_nodes++;
                    enter = INVL ? slab64_inv(node64(S, cur), o, S.inv64_lds, tmin, R.tmax)
                                 : slab64(node64(S, cur), o, d, tmin, R.tmax);
                }
            }
            const bool inner = enter & (w1 < kLeafFlagF);
            // siblings are side by side, the left one 64-byte aligned: near = left | 32 when the
            // right child comes first (v_bfe_u32 takes the offset from w0's low five bits: the
            // split axis), far = near ^ 32. At a leaf the store lands above the live stack; at the
            // sentinel it overwrites the guard level, which every traversal start rewrites.
            const uint32_t near = w1 | (__builtin_amdgcn_ubfe(R.neg, w0, 1) << kNodeFShift);
            if (!LINK) tp[stride] = static_cast<SE>(near ^ (1u << kNodeFShift));
            stop = enter ^ inner;  // entered, not interior: a leaf or the sentinel
            cur = inner ? near : top;
            if (!LINK) tp += inner ? stride : -stride;
        } while (!stop);
    }
    R.state = w1 == kSentinelW1 ? kDone : kLeaf;
    R.first = w0;
    R.count = w1 & ~kLeafFlagF;
    R.cur = cur;
    // levels in use after the pop; -1 when the leaf was entered with an empty stack
    if (!LINK) R.sp = static_cast<int32_t>(static_cast<uint32_t>(tp - empty)) / static_cast<int32_t>(st.stride);
}

// ---- the sibling-pair walk of the HBM-scene kernels (CRT_PAIR_WALK) ----------------------------
// A step tests BOTH children of an entered interior node: one 64-byte read (siblings are side by
// side, the left one 64-byte aligned, so a pair is one half of a 128-byte line) and two f32 node
// tests. Deep trees in HBM walk a dependent chain of node reads; testing a pair per step halves
// its length (config 4: ~38 node tests a ray, each an L1 / L2 latency).
// The lane's position is a token: the byte offset of the first node to test, | 1 when it is to be
// tested alone. Without the bit the step tests that node and its sibling (offset ^ 32: siblings
// are side by side, 64-byte aligned), the first one being the near child of their parent in the
// ray's order. An entered interior child X continues as token(X) = X.left | (the ray's sign on
// X's split axis) << 5 = X's near child (the old walk's `near`); an entered leaf that cannot be
// processed now (a far child) continues as its own offset | 1, i.e. a re-test of its box alone.
// Exactness (the primitive tests are the reference's, in its order, with its t_max):
// - the DFS order of the children does not depend on t_max, and is the reference's
//   (bvh.h:684-698: near child first by the sign of d on the parent's split axis);
// - the node test is monotone in t_max and in the box: a child box lies inside its parent's
//   (node boxes are unions of their primitives' boxes), and the rounded slab values satisfy
//   near(child) >= near(parent), far(child) <= far(parent), so "child entered at t" implies
//   "parent entered at t" and at any larger t_max;
// - so testing a node at a t_max at least the reference's (children before their elder sibling's
//   subtree has shrunk it) only adds node visits: a node the pair walk culls, the reference culls
//   too, at its own (smaller or equal) t_max;
// - and a leaf's primitives run only right after its box was entered at the current t_max: the
//   first leaf a step enters (tested at the current t_max) exits to the leaf phase at once; every
//   other leaf is re-tested (its offset | 1) when the walk comes back to it. The reference tests a
//   leaf's box iff every ancestor was entered at its (larger) t_max, which the entry of the leaf
//   at the current t_max implies, so both test the same leaves at the same t_max.
// - A popped interior token is not re-tested itself: its children are tested at the current
//   t_max, and by monotonicity they all fail where the reference would cull it.
// The speculative form (SPEC: Aila & Laine's postponed leaves, walk()): a lane that has recorded
// its first leaf walks on with the t_max of now and parks at its second leaf as a re-test token,
// so the leaf is tested again at the then-current t_max in the next round.
// Stack: tokens, the far token stored at level sp unconditionally (pushed when both children are
// entered and the near one is interior); the guard level holds the sentinel's token (its offset
// | 1: its "sibling", past the node array, is never tested). The root's token is 0 | 1 (the pad
// node beside it is never tested). tests/test_pair_walk_model.py runs this state machine against
// the reference's DFS on random trees.

constexpr uint32_t kTokAlone = 1u;  // token bit 0: the first node alone (root, sentinel, re-tests)

// The step's two f32 nodes: f (the first) and g = f ^ 32, read from the LDS treelet or from HBM
// (the treelet holds whole sibling pairs, scene_layout, so f and g are on the same side),
// both sides in flight together as in fetch_nodef.
template <bool TOP>
__device__ __forceinline__ void fetch_two(const SceneView& S, uint32_t f, uint32_t g, Uvec4& a0, Uvec4& a1, Uvec4& b0,
                                          Uvec4& b1) {
    if (TOP) {
        const uint64_t hbm = __ballot(f >= S.ntop);
        uint64_t save;
        asm volatile(
            "s_and_saveexec_b64 %[save], %[hbm]\n\t"
            "s_cbranch_execz 1f\n\t"
            "global_load_dwordx4 %[a0], %[f], %[base]\n\t"
            "global_load_dwordx4 %[a1], %[f], %[base] offset:16\n\t"
            "global_load_dwordx4 %[b0], %[g], %[base]\n\t"
            "global_load_dwordx4 %[b1], %[g], %[base] offset:16\n"
            "1:\n\t"
            "s_andn2_b64 exec, %[save], %[hbm]\n\t"
            "s_cbranch_execz 2f\n\t"
            "ds_read_b128 %[a0], %[f]\n\t"
            "ds_read_b128 %[a1], %[f] offset:16\n\t"
            "ds_read_b128 %[b0], %[g]\n\t"
            "ds_read_b128 %[b1], %[g] offset:16\n"
            "2:\n\t"
            "s_mov_b64 exec, %[save]\n\t"
            "s_waitcnt vmcnt(0) lgkmcnt(0)"
            : [a0] "=&v"(a0), [a1] "=&v"(a1), [b0] "=&v"(b0), [b1] "=&v"(b1), [save] "=&s"(save)
            : [f] "v"(f), [g] "v"(g), [hbm] "s"(hbm), [base] "s"(S.fnodes)
            : "memory");
    } else {
        GlobalNodeF* qa = (GlobalNodeF*)(reinterpret_cast<const char*>(S.fnodes) + f);
        GlobalNodeF* qb = (GlobalNodeF*)(reinterpret_cast<const char*>(S.fnodes) + g);
        a0 = qa->q0;
        a1 = qa->q1;
        b0 = qb->q0;
        b1 = qb->q1;
    }
}

// the f32 node test of walk() on one node: lo' = max(near', tmin'), hi' = min(far', tmax')
__device__ __forceinline__ void node_lohi(const Uvec4& q0, const Uvec4& q1, const Trav& R, float tmin32, float& lo,
                                          float& hi) {
    const float x0 = __builtin_fmaf(__uint_as_float(q0.x), R.inv32[0], -R.oinv32[0]);
    const float x1 = __builtin_fmaf(__uint_as_float(q0.y), R.inv32[0], -R.oinv32[0]);
    const float y0 = __builtin_fmaf(__uint_as_float(q0.z), R.inv32[1], -R.oinv32[1]);
    const float y1 = __builtin_fmaf(__uint_as_float(q0.w), R.inv32[1], -R.oinv32[1]);
    const float z0 = __builtin_fmaf(__uint_as_float(q1.x), R.inv32[2], -R.oinv32[2]);
    const float z1 = __builtin_fmaf(__uint_as_float(q1.y), R.inv32[2], -R.oinv32[2]);
    lo = vmax3(vmin(x0, x1), vmin(y0, y1), vmax_s(vmin(z0, z1), tmin32));
    hi = vmin3(vmax(x0, x1), vmax(y0, y1), vmin(vmax(z0, z1), R.tmax32));
}

template <typename SE, bool COUNT, bool TOP, bool INVL>
__device__ __forceinline__ void walk_pairs(const SceneView& S, Stack<SE>& st, const double o[3], const double d[3],
                                           double tmin, float tmin32, Trav& R, LaneCounters& ctr) {
    const ptrdiff_t stride = static_cast<ptrdiff_t>(st.stride);
    SE* const empty = st.base - stride;
    SE* tp = st.base + (static_cast<ptrdiff_t>(R.sp) - 1) * stride;
    uint32_t cur = R.cur;
    uint32_t run = 1;
    uint32_t pref = ~0u;  // the first leaf's re-test token (or the sentinel's), ~0u: none yet
    // The per-lane logic is written on lane masks (uint64_t ballots: scalar ALU) with v_cndmask
    // selects (vsel); as bools across the rare f64 branch, the compiler materialises the
    // conditions as 0 / 1 in VGPRs and spends ~40 VALU a step on them. (The loop state as masks
    // too, with a wave-uniform body and masked updates: 65 VALU a step instead of 69, but config 4
    // 128.9-129.4 vs 127.7-127.8 ms, profiles/r06_pair_tuning.)
    uint64_t nop = __ballot(true);  // lanes with no leaf recorded yet
    do {
        CRT_WD(7, cur, static_cast<uint32_t>(tp - empty));
        if (run) {
            const uint32_t f = cur & ~kTokAlone, g = f ^ 32u;  // the first node and its sibling
            Uvec4 a0, a1, b0, b1;
            fetch_two<TOP>(S, f, g, a0, a1, b0, b1);
            const uint32_t top = *tp;  // speculative pop
            float lo1, hi1, lo2, hi2;
            node_lohi(a0, a1, R, tmin32, lo1, hi1);
            node_lohi(b0, b1, R, tmin32, lo2, hi2);
            const float g1 = hi1 - lo1, g2 = hi2 - lo2;
            // each node its own threshold (walk()'s bound, M = max(|lo'|, |hi'|) of that node).
            // One shared threshold (the larger M) would save a VALU a step but leaves 16x as many
            // node tests to f64: a sibling missed on an axis the ray runs almost parallel to has
            // |lo'| ~ |inv|, and its M made the other node's gap undecidable (config 4: 1.49e9
            // f64 node tests a frame, 13% of walk iterations with one)
            const float t1 = __builtin_fmaf(vmax_abs(lo1, hi1), 0x1p-19f, R.marg);
            const float t2 = __builtin_fmaf(vmax_abs(lo2, hi2), 0x1p-19f, R.marg);
            const uint64_t two = __ballot(cur == f);  // the sibling is tested too
            uint64_t e1 = __ballot(g1 > 0.f), e2 = __ballot(g2 > 0.f) & two;
            const uint64_t u1 = __ballot(!(fabsf(g1) > t1)), u2 = two & __ballot(!(fabsf(g2) > t2));
            if (COUNT) {
                if (a1.w != kSentinelW1) ctr.nodes++;
                ctr.nodes += cur == f ? 1 : 0;
                if (wave_leader()) ctr.it_walk++;
            }
            if (__builtin_expect((u1 | u2) != 0, 0)) {  // lanes the f32 margin cannot decide: f64
                if (COUNT && wave_leader()) ctr.it_slow++;
                const uint64_t me = 1ull << (threadIdx.x & 63);
                bool f1 = false, f2 = false;
                if (u1 & me) {
                    if (COUNT) ctr.slow_nodes++;
                    f1 = INVL ? slab64_inv(node64(S, f), o, S.inv64_lds, tmin, R.tmax) : slab64(node64(S, f), o, d, tmin, R.tmax);
                }
                if (u2 & me) {
                    if (COUNT) ctr.slow_nodes++;
                    f2 = INVL ? slab64_inv(node64(S, g), o, S.inv64_lds, tmin, R.tmax) : slab64(node64(S, g), o, d, tmin, R.tmax);
                }
                e1 = (e1 & ~u1) | __ballot(f1);
                e2 = (e2 & ~u2) | __ballot(f2);
            }
            const uint64_t i1 = __ballot(a1.w < kLeafFlagF), i2 = __ballot(b1.w < kLeafFlagF);
            // X: the first entered node in the reference's order (the first one, else its sibling)
            const uint64_t both = e1 & e2, any = e1 | e2;
            const uint64_t xi = (e1 & i1) | (~e1 & i2);
            // an entered leaf: the first one is recorded and the walk goes on with its
            // continuation (the sibling's token, or the stack top); the second one parks as its
            // re-test token (the sibling's token pushed when both were entered). The sentinel is
            // recorded like a leaf and met again on the second guard level, where the lane parks.
            const uint64_t leaf = any & ~xi;
            const uint64_t park = leaf & ~nop;  // the sentinel: recorded, then met again below the guard
            const uint64_t dp = (any & xi) | park;  // cur = X's token
            // the nodes' tokens: an interior node's near child, a leaf's re-test
            const uint32_t tok1 = vsel(i1, (__builtin_amdgcn_ubfe(R.neg, a1.z, 1) << kNodeFShift) | a1.w, cur | kTokAlone);
            const uint32_t tok2 = vsel(i2, (__builtin_amdgcn_ubfe(R.neg, b1.z, 1) << kNodeFShift) | b1.w, g | kTokAlone);
            const uint32_t tx = vsel(e1, tok1, tok2);
            pref = vsel(leaf & nop, tx, pref);
            tp[stride] = static_cast<SE>(tok2);
            cur = vsel(dp, tx, vsel(both, tok2, top));
            // one level up when the walk descends with both entered, one down when it pops
            tp += static_cast<int32_t>(vsel(dp & both, 1u, vsel(~dp & ~both, ~0u, 0u))) * stride;
            run = vsel(park, 0u, 1u);
        }
        nop = __ballot(pref == ~0u);
    } while (nop != 0);
    {
        const Uvec2 w = fetch_nodef_words<TOP, false>(S, pref & ~kTokAlone);  // the recorded leaf
        R.state = w.y == kSentinelW1 ? kDone : kLeaf;
        R.first = w.x;
        R.count = w.y & ~kLeafFlagF;
    }
    R.cur = cur;
    R.sp = static_cast<int32_t>(static_cast<uint32_t>(tp - empty)) / static_cast<int32_t>(st.stride);
}

// the entered leaf's primitives in order (bvh.h:635-652), then "return" to the DFS.
// Sphere-only scenes store spheres in slot order, so the slot indexes them directly and the next
// sphere is loaded while the current one is tested.
// QONLY: every primitive is a parallelogram (the flat-parallelogram instances): the sphere paths,
// and with them the ray's sphere constants (dot(d, d), its reciprocal, the coarse-reject limits),
// are compiled out
// LINK: the walk left the leaf's miss link in R.cur; the traversal is over when that is the sentinel
template <typename SE, bool COUNT, bool TOP, bool LS, bool FAST = false, bool QONLY = false, bool LINK = false>
__device__ __forceinline__ void leaf_step(const SceneView& S, Stack<SE>& st, const double o[3],
                                              const double d[3], double tmin, float tmin32, bool sphere_only, bool pairs,
                                              bool qfilter, bool qflat, Trav& R, LaneCounters& ctr) {
    const uint2 range = make_uint2(R.first, R.count);  // index, count
    const uint32_t end = range.x + range.y;
    const double ia = recip_a<FAST>(R.a, !(R.neg & kNoRecip)), lo = lim_tmin(tmin, R.a);
    double hi = lim_tmax(R.tmax, R.a);
    if (!QONLY && pairs && range.y <= 32 && !(R.neg & kNoLeaf32)) {
        // two passes: the packed f32 candidate filter over every sphere against the leaf-entry
        // t_max, then the full test of the candidates in slot order with the shrinking t_max. A
        // sphere the first pass rejects is rejected by the full test for any smaller t_max too,
        // so the hits and the tie order are the sequential loop's; the full-test pass runs only
        // as often as the lane with most candidates needs (typically 1-3 of 6-12).
        // Pass 1 reads pair records (slots first + i, first + i + 1) and shifts both verdicts
        // into `cand`: after the pass, bit nbits - 1 - i stands for sphere i (nbits = count
        // rounded up to even; an odd count's extra verdict, for the slot after the leaf, is
        // masked off).
        LeafRay32 L;
        leaf_ray32(o, d, R.a, tmin, R.tmax, L);
        uint32_t cand = 0;
        const uint32_t nbits = (range.y + 1) & ~1u;
        if constexpr (LS) {
            for (uint32_t i = 0; i < range.y; i += 2) {
                if (COUNT) {
                    ctr.sphere_tests += i + 1 < range.y ? 2 : 1;
                    if (wave_leader()) ctr.it_leaf += 2;
                }
                cand = sphere_pair_candidates(cand, pair_at((LdsPair*)static_cast<uintptr_t>(S.spair_lds + ((range.x + i) << 5))), L);
            }
        } else {
            for (uint32_t i = 0; i < range.y; i += 2) {
                if (COUNT) {
                    ctr.sphere_tests += i + 1 < range.y ? 2 : 1;
                    if (wave_leader()) ctr.it_leaf += 2;
                }
                cand = sphere_pair_candidates(cand, pair_at((GlobalPair*)(S.spair + range.x + i)), L);
            }
        }
        cand &= ~(range.y & 1u);  // an odd count's last verdict is the slot after the leaf
        while (cand) {
            CRT_WD(6, cand, range.y);
            if (COUNT) {
                ctr.cand++;
                if (wave_leader()) ctr.it_cand++;
            }
            const uint32_t b = 31 - __builtin_clz(cand);
            cand ^= 1u << b;
            const uint32_t i = range.x + (nbits - 1 - b);
            double t;
            // the f64 spheres are in HBM (L1) in this mode
            if (hit_sphere<false>(sphere_at<LS>(S, i), o, d, R.a, ia, tmin, R.tmax, lo, hi, t)) {
                R.tmax = t;
                R.tmax32 = tmax_f32(t);
                hi = lim_tmax(t, R.a);
                R.ref = i;
                R.found = true;
            }
        }
    } else if (LS && qfilter && qflat && range.y <= 32) {
        // axis-aligned parallelograms (every Box face, the Cornell walls): pass 1 is the walk's
        // f32 node test on each one's flat box (crt_quad_filter.h: a rejection is a proven miss of
        // the reference's Parallelogram::hit_by for this t_max and any smaller one); rays outside
        // the walk's range have marg = inf and keep every parallelogram. Pass 2 as below.
        // one loop per flat axis over the leaf's records grouped by it (stage_image), each record
        // setting the bit of its slot
        uint32_t cand = 0;
        const uint32_t base = S.quadf_lds + (range.x << 5);
        const uint32_t g = lds_u32(base + 28);  // the group sizes, in the leaf's first record
        const uint32_t e0 = g & 0xffu, e1 = e0 + ((g >> 8) & 0xffu);
        uint32_t i = 0;
        const auto filter = [&](auto axis) {
            if (COUNT) {
                ctr.quad_tests++;
                if (wave_leader()) ctr.it_leaf++;
            }
            LdsNodeF* p = (LdsNodeF*)static_cast<uintptr_t>(base + (i << 5));
            const Uvec4 q0 = p->q0, q1 = p->q1;
            const float b[6] = {__uint_as_float(q0.x), __uint_as_float(q0.y), __uint_as_float(q0.z),
                                __uint_as_float(q0.w), __uint_as_float(q1.x), __uint_as_float(q1.y)};
            cand |= static_cast<uint32_t>(flat_axis_candidate<decltype(axis)::value, DevMinMax>(b, R.inv32, R.oinv32, tmin32, R.tmax32, R.marg)) << q1.z;
        };
        for (; i < e0; ++i) filter(std::integral_constant<int, 0>{});
        for (; i < e1; ++i) filter(std::integral_constant<int, 1>{});
        for (; i < range.y; ++i) filter(std::integral_constant<int, 2>{});
        while (cand) {
            CRT_WD(6, cand, range.y);
            if (COUNT) {
                ctr.cand++;
                if (wave_leader()) ctr.it_cand++;
            }
            const uint32_t i = range.x + static_cast<uint32_t>(__builtin_ctz(cand));
            cand &= cand - 1;
            double t;
            if (hit_quad(lds_rec<DevQuad>(S.quads_lds + (i << 7)), o, d, tmin, R.tmax, t)) {
                R.tmax = t;
                R.tmax32 = tmax_f32(t);
                R.ref = kRefQuad | i;
                R.found = true;
            }
        }
    } else if (LS && qfilter && !qflat && range.y <= 32 && quad_ray32_ok(o, d)) {
        // parallelogram-only scenes (a slot is its parallelogram's index): the same two passes,
        // with the f32 filter of crt_quad_filter.h (quad_candidate) in pass 1. LDS-scene kernels
        // only: in the HBM-scene kernels its registers cost spills (none of the reference's
        // parallelogram-only scenes is that large)
        QuadRay32 L;
        quad_ray32(o, d, tmin, R.tmax, L);
        uint32_t cand = 0;
        for (uint32_t i = 0; i < range.y; ++i) {
            if (COUNT) {
                ctr.quad_tests++;
                if (wave_leader()) ctr.it_leaf++;
            }
            const DevQuadF q = LS ? lds_rec<DevQuadF>(S.quadf_lds + ((range.x + i) << 6)) : quadf_global(S.quadf + range.x + i);
            cand |= static_cast<uint32_t>(quad_candidate(q, L, [](float x) { return __builtin_amdgcn_rcpf(x); })) << i;
        }
        while (cand) {
            CRT_WD(6, cand, range.y);
            if (COUNT) {
                ctr.cand++;
                if (wave_leader()) ctr.it_cand++;
            }
            const uint32_t i = range.x + static_cast<uint32_t>(__builtin_ctz(cand));
            cand &= cand - 1;
            double t;
            bool h;
            if constexpr (LS) h = hit_quad(lds_rec<DevQuad>(S.quads_lds + (i << 7)), o, d, tmin, R.tmax, t);
            else h = hit_quad(S.quads[i], o, d, tmin, R.tmax, t);
            if (h) {
                R.tmax = t;
                R.tmax32 = tmax_f32(t);
                R.ref = kRefQuad | i;
                R.found = true;
            }
        }
    } else if (!QONLY && sphere_only) {
        DevSphere cur = sphere_at<LS>(S, range.x);
        for (uint32_t i = range.x; i < end; ++i) {
            // one past the leaf's last sphere is still inside the scene copy (sphere_mat follows
            // the spheres in HBM, the parallelogram / stack regions in LDS); it is never tested
            const DevSphere nxt = sphere_at<LS>(S, i + 1);
            if (COUNT) {
                ctr.sphere_tests++;
                if (wave_leader()) ctr.it_leaf++;
            }
            double t;
            if (hit_sphere(cur, o, d, R.a, ia, tmin, R.tmax, lo, hi, t)) {
                R.tmax = t;
                R.tmax32 = tmax_f32(t);
                hi = lim_tmax(t, R.a);
                R.ref = i;
                R.found = true;
            }
            cur = nxt;
        }
    } else {
        for (uint32_t i = range.x; i < end; ++i) {
            // LS: refs, spheres and parallelograms are all staged (spheres_f32 is off here)
            const uint32_t ref = LS ? lds_u32(S.refs_lds + (i << 2)) : S.refs[i];
            double t;
            bool h;
            if (COUNT && wave_leader()) ctr.it_leaf++;
            if (QONLY || (ref & kRefQuad)) {
                if (COUNT) ctr.quad_tests++;
                if constexpr (LS) h = hit_quad(lds_rec<DevQuad>(S.quads_lds + ((ref & ~kRefQuad) << 7)), o, d, tmin, R.tmax, t);
                else h = hit_quad(S.quads[ref & ~kRefQuad], o, d, tmin, R.tmax, t);
            } else {
                if (COUNT) ctr.sphere_tests++;
                if constexpr (LS) h = hit_sphere(lds_rec<DevSphere>(S.spheres_lds + (ref << 5)), o, d, R.a, ia, tmin, R.tmax, lo, hi, t);
                else h = hit_sphere(S.spheres[ref], o, d, R.a, ia, tmin, R.tmax, lo, hi, t);
            }
            if (h) {
                R.tmax = t;
                R.tmax32 = tmax_f32(t);
                hi = lim_tmax(t, R.a);
                R.ref = ref;
                R.found = true;
            }
        }
    }
    // the pop after the leaf was made by walk (R.cur is the next node, unless the stack was empty)
    R.state = (LINK ? R.cur == S.sentinel : R.sp < 0) ? kDone : kWalk;
}

__device__ __forceinline__ uint32_t owned_row(const Work& w, uint32_t k) {
    if (w.rb_shift < 32) {  // power-of-two row blocks: no division
        const uint32_t blk = k >> w.rb_shift, in = k & ((1u << w.rb_shift) - 1);
        return ((blk * w.tile_count + w.tile_index) << w.rb_shift) | in;
    }
    const uint32_t blk = k / w.row_block, in = k % w.row_block;
    return (blk * w.tile_count + w.tile_index) * w.row_block + in;
}

// State of one lane's current path: the ray, the throughput and the bounces left (ray_color's
// depth_left, camera.h:207-213). Emission enters a path only where it ends (a DiffuseLight never
// scatters, a miss returns the background), so no running radiance is kept: the terminal
// T * (emit | background) goes straight into the pixel's sum.
struct Path {
    double o[3], d[3];
    double T[3];
    uint32_t depth;
    uint32_t rng;
};

// random_ray_through_pixel (camera.h:184-200) for a fresh sample
__device__ __forceinline__ void start_path(const CamView& C, uint32_t row, uint32_t col, uint32_t rng, Path& P) {
    if (C.defocus_angle <= 0) {
        P.o[0] = C.o[0]; P.o[1] = C.o[1]; P.o[2] = C.o[2];
    } else {  // random_point_in_defocus_disk (camera.h:160-168, vec3d.h:79-85)
        double vx, vy;
        do {
            vx = rnd_pm1(rng);
            vy = rnd_pm1(rng);
        } while (!(vx * vx + vy * vy + 0.0 * 0.0 < 1));
        P.o[0] = (C.o[0] + C.ddx[0] * vx) + C.ddy[0] * vy;
        P.o[1] = (C.o[1] + C.ddx[1] * vx) + C.ddy[1] * vy;
        P.o[2] = (C.o[2] + C.ddx[2] * vx) + C.ddy[2] * vy;
    }
    // converted here at every call: hoisted out of the kernel's loop, the two doubles would
    // stay live (and spill) across all phases
    uint32_t ir = row, ic = col;
    asm volatile("" : "+v"(ir), "+v"(ic));
    const double fr = static_cast<double>(ir), fc = static_cast<double>(ic);
    // a g++ build evaluates the second jitter draw (the pixel_delta_y one) first
    const double uy = rnd(rng, -0.5, 0.5);
    const double ux = rnd(rng, -0.5, 0.5);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double center = (C.p00[k] + C.pdy[k] * fr) + C.pdx[k] * fc;
        const double sample = (center + C.pdx[k] * ux) + C.pdy[k] * uy;
        P.d[k] = sample - P.o[k];
        P.T[k] = 1;
    }
    P.depth = C.max_depth;
    P.rng = rng;
}

// One level of ray_color (camera.h:205-258) after the closest-hit query: scatters
// (material.h:64-263) into the next ray, or ends the path adding T * (background | emission) to
// acc. Returns true when the path has ended (miss, light, absorption).
// What shade tells the NEE instances (nee_segment) about a hit that scattered: the normal facing
// the ray and the material kind. Every other instance compiles it out.
struct ShadeOut {
    double n[3];
    uint32_t kind;
};

// NEE == 2 (the lights instances, light_segment): a light hit adds nothing here; ex->kind tells the
// caller, which weights the emission itself (it needs the light's true normal: for an emitting
// sphere slot M.emit[0] is the emission, not 1 / r, so n below is not that normal).
template <bool LS, bool SPH = false, bool QONLY = false, bool FAST = false, int NEE = 0>
__device__ __forceinline__ bool shade(const SceneView& S, const CamView& C, Path& P, bool hit,
                                      uint32_t ref, double t, double acc[3], ShadeOut* ex = nullptr) {
    if (!hit) {
        acc[0] = acc[0] + P.T[0] * C.bg[0];
        acc[1] = acc[1] + P.T[1] * C.bg[1];
        acc[2] = acc[2] + P.T[2] * C.bg[2];
        return true;
    }
    // the slot's material record, loaded first (its address needs only the slot)
    const DevMaterial& M = (QONLY || (!SPH && (ref & kRefQuad))) ? S.quad_mrec[ref & ~kRefQuad] : S.sphere_mrec[ref];
    double p[3], n[3];
    bool front;
    (void)hit_record<LS, true, SPH, QONLY>(S, ref, P.o, P.d, t, p, n, front, M.emit[0]);
    const uint32_t kind = M.kind;
    const bool lam = kind == CRT_LAMBERTIAN, met = kind == CRT_METAL, die = kind == CRT_DIELECTRIC;
    if (!(lam || met || die)) {  // DiffuseLight: emits, never scatters (material.h:248-263)
        if constexpr (NEE == 2) {
            ex->kind = kind;
            return true;
        }
        acc[0] = acc[0] + P.T[0] * M.emit[0];
        acc[1] = acc[1] + P.T[1] * M.emit[1];
        acc[2] = acc[2] + P.T[2] * M.emit[2];
        return true;
    }
    // The scatter functions are interleaved by their common steps, so a wave with several
    // materials runs each step once: unit(d) (Metal material.h:120, Dielectric :191), the
    // Dielectric reflect-or-refract draw, random_unit_vector (Lambertian :70, Metal :123 — the
    // only draw of either), then the reflection (vec3d.h:144-155) shared by Metal and a
    // reflecting Dielectric. Every lane still makes its own material's draws in the reference's
    // order (no lane draws in two of these steps).
    double ux0 = 0, uy0 = 0, uz0 = 0;
    if (met || die) {
        const double il = recip_exact<FAST>(sqrt_exact<FAST>(P.d[0] * P.d[0] + P.d[1] * P.d[1] + P.d[2] * P.d[2]));
        ux0 = P.d[0] * il;
        uy0 = P.d[1] * il;
        uz0 = P.d[2] * il;
    }
    bool reflect = met;
    double cosv = 0, ratio = 0;
    if (die) {  // material.h:185-218, vec3d.h:168-200
        ratio = front ? M.color[0] : M.param;  // 1. / ri, ri / 1. (precomputed: upload)
        cosv = fmin((-ux0) * n[0] + (-uy0) * n[1] + (-uz0) * n[2], 1.);
        const double sinv = sqrt_exact<FAST>(1 - cosv * cosv);
        if (ratio * sinv > 1) {
            reflect = true;  // total internal reflection, no draw
        } else {
            const double r0 = front ? M.color[1] : M.color[2];  // reflectance's r0 (upload)
            const double pw = pow5(1 - cosv);
            const double u = rnd_01(P.rng);
            reflect = u < r0 + (1 - r0) * pw;
            // a branch a 1-ulp different pow could flip (crt_schlick.h): counted, never taken in
            // practice (probability ~2^-50 per decision)
            if (__builtin_expect(schlick_undecided(u, r0, pw), 0)) atomicAdd(S.guard, 1ull);
        }
    }
    double rx = 0, ry = 0, rz = 0;
    if (lam || met) random_unit_vector<FAST>(P.rng, rx, ry, rz);
    double nd[3];
    if (reflect) {  // Metal (material.h:116-139) or a reflecting Dielectric
        const double k2 = 2 * (ux0 * n[0] + uy0 * n[1] + uz0 * n[2]);
        nd[0] = ux0 - n[0] * k2;
        nd[1] = uy0 - n[1] * k2;
        nd[2] = uz0 - n[2] * k2;
        if (met) {
            nd[0] = nd[0] + rx * M.param;
            nd[1] = nd[1] + ry * M.param;
            nd[2] = nd[2] + rz * M.param;
            if (n[0] * nd[0] + n[1] * nd[1] + n[2] * nd[2] < 0) return true;  // absorbed; emits 0
        }
    } else if (die) {  // refraction
        const double px = (ux0 + n[0] * cosv) * ratio;
        const double py = (uy0 + n[1] * cosv) * ratio;
        const double pz = (uz0 + n[2] * cosv) * ratio;
        const double sq = -sqrt_exact<FAST>(fabs(1 - (px * px + py * py + pz * pz)));
        nd[0] = px + n[0] * sq;
        nd[1] = py + n[1] * sq;
        nd[2] = pz + n[2] * sq;
    } else {  // Lambertian (material.h:64-86)
        nd[0] = n[0] + rx; nd[1] = n[1] + ry; nd[2] = n[2] + rz;
        if (fabs(nd[0]) < 1e-8 && fabs(nd[1]) < 1e-8 && fabs(nd[2]) < 1e-8) {
            nd[0] = n[0]; nd[1] = n[1]; nd[2] = n[2];
        }
    }
    if (kind != CRT_DIELECTRIC) {  // attenuation = intrinsic colour (dielectric: 1)
        P.T[0] = P.T[0] * M.color[0];
        P.T[1] = P.T[1] * M.color[1];
        P.T[2] = P.T[2] * M.color[2];
    }
    P.o[0] = p[0]; P.o[1] = p[1]; P.o[2] = p[2];
    P.d[0] = nd[0]; P.d[1] = nd[1]; P.d[2] = nd[2];
    P.depth -= 1;
    if constexpr (NEE != 0) {
        ex->n[0] = n[0]; ex->n[1] = n[1]; ex->n[2] = n[2];
        ex->kind = kind;
    }
    return false;
}

// 16-byte cooperative copy global -> LDS (the scene staging of LSCENE kernels)
__device__ __forceinline__ void stage_lds(unsigned char* dst, const void* src, uint32_t bytes) {
    const uint4* s = static_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
    for (uint32_t i = threadIdx.x; i < bytes / 16; i += kBlock) d[i] = s[i];
}

// The render kernel: a persistent grid (as many blocks as are resident) whose waves take work
// items from a queue in HBM, one atomic per item: item = (8x8 pixel tile, sample chunk), 64
// (chunk, pixel) units, in tile-major order. A wave's lanes draw units as they finish one,
// crossing from one item into the next without waiting, so a lane idles only once the queue is
// dry, and the grid drains within about one unit.
// Persistent per-lane state machine (WALK -> LEAF -> ... -> DONE -> shade -> WALK) in traversal
// rounds: every walking lane walks the DFS to its next entered leaf (or the end of its
// traversal), then the lanes holding a leaf test it together. Lanes whose ray is finished park
// until kShadeBatch of them are finished (or nobody traverses), then shade together, and a
// finished path starts the lane's next sample at once (path regeneration). So the shading code
// runs with many lanes active, and a wave is never held by its slowest ray or path.
// A unit's samples are summed in sample order into partial[chunk][pixel].
// LSCENE: nodes, primitive refs, spheres and parallelograms are staged in LDS first.
// 4 waves per SIMD (128 VGPRs): the f32 walk / packed sphere filter state does not fit 96
// VGPRs without ~66 spills (5 waves: 3932 vs 4158 Msamples/s on config 2)
#ifndef CRT_WAVES_PER_EU
#define CRT_WAVES_PER_EU 4
#endif
// LDS-scene kernels: 5 waves per SIMD (96 VGPRs) spill 65 VGPRs with the work-queue state and
// wrote 94 GB of scratch per config-2 frame: 5262 vs 5499 Msamples/s at 4 (config 3: 1958 vs
// 1939); with v10's block pools 5 had measured +0.7%. The HBM-scene kernels lose 14% at 5.
#ifndef CRT_WAVES_PER_EU_LDS
#define CRT_WAVES_PER_EU_LDS 4
#endif
// The NEE instances of radiance_kernel carry about 16 more VGPRs a lane (Nee) than instances that
// sit at 107 to 123 of 128: three waves per SIMD (168 VGPRs) keep them out of scratch.
#ifndef CRT_WAVES_PER_EU_NEE
#define CRT_WAVES_PER_EU_NEE 3
#endif
#ifndef CRT_SHADE_BATCH
#define CRT_SHADE_BATCH 48
#endif
constexpr int kShadeBatch = CRT_SHADE_BATCH;

// HBM-scene kernels keep the top of the node array in LDS (CRT_NO_LDS_TOP=1 at run time: none)
constexpr bool kTopTreelet = true;
// The timed kernels walk speculatively (walk(): lanes that found their first leaf walk on to the
// next one). The instrumented pass (COUNT) walks like the reference by default, so its node counts
// are the reference's (the algorithmic-byte basis); with Work::count_spec (CRT_COUNT_SPEC=1 at run
// time) it walks speculatively too, for the timed kernel's phase timings and lane utilization (its
// node counts then include the speculative visits).
// Static wave priority per phase (s_setprio 0-3; the SQ issues a ready instruction of the highest
// priority wave first, then the oldest): the traversal phases are dependency chains (LDS read ->
// test -> next address), the shade and path-start phases have more independent work to fill in.
// Config 2 (ms/frame, one box): none 87.9; walk 1 86.6; walk+leaf 1 85.6; walk 2 / leaf 1 85.6;
// walk 1 / leaf 2 85.6; walk 2 / leaf 2 / start 1 85.4; walk 3 / leaf 2 / start 1 (kept) 85.3;
// walk 1 / leaf 1 / start 1 86.0.
constexpr int kPrioWalk = 3, kPrioLeaf = 2, kPrioShade = 0, kPrioInit = 1;
template <int P>
__device__ __forceinline__ void set_prio() {
    if constexpr ((kPrioWalk | kPrioLeaf | kPrioShade | kPrioInit) != 0) __builtin_amdgcn_s_setprio(P);
}

// ---- what the persistent-wave kernels (render_kernel, query_kernel, radiance_kernel) share ------
// The scene staging, without its barrier (the caller's). LSCENE: nodes, primitive refs, spheres and
// parallelograms go to LDS and S points there; else the first W.ntop bytes of f32 nodes do.
template <bool LSCENE, bool LINK>
__device__ __forceinline__ void stage_scene(unsigned char* smem, const SceneView& Sg, const Work& W, SceneView& S) {
    if (LSCENE) {  // f32 nodes at LDS offset 0 (fetch_nodef: a node's LDS address is its ref)
        if (static_cast<uint32_t>(reinterpret_cast<uintptr_t>((LdsByte*)smem)) != 0) __builtin_trap();
        stage_lds(smem, Sg.fnodes, W.bytes_nodes);
        stage_lds(smem + W.lds_quads, Sg.quads, W.bytes_quads);
        S.quads = reinterpret_cast<const DevQuad*>(smem + W.lds_quads);
        S.quads_lds = W.lds_quads;
        if (W.quads_f32) {  // the parallelogram filter's records (flat boxes when axis-aligned)
            stage_lds(smem + W.lds_quadf, W.quads_flat ? static_cast<const void*>(Sg.quadbox) : Sg.quadf, W.bytes_quadf);
            S.quadf_lds = W.lds_quadf;
        }
        S.refs_lds = W.lds_refs;
        S.spheres_lds = W.spheres_f32 ? (W.bytes_sph64 ? W.lds_sph64 : ~0u) : W.lds_spheres;
        if (W.spheres_f32) {
            // sphere-only: the filter's pair records in LDS; refs are unused (slot = sphere),
            // and the f64 spheres (candidates' exact tests, shading) stay in HBM / L1
            stage_lds(smem + W.lds_spheres, Sg.spair, W.bytes_spheres);
            if (W.bytes_sph64) stage_lds(smem + W.lds_sph64, Sg.spheres, W.bytes_sph64);
            S.spair_lds = W.lds_spheres;
        } else {
            stage_lds(smem + W.lds_refs, Sg.refs, W.bytes_refs);
            stage_lds(smem + W.lds_spheres, Sg.spheres, W.bytes_spheres);
            S.refs = reinterpret_cast<const uint32_t*>(smem + W.lds_refs);
            S.spheres = reinterpret_cast<const DevSphere*>(smem + W.lds_spheres);
        }
        if (LINK) {  // the miss links, in the bytes of the guard levels and the stack
            stage_lds(smem + W.lds_links, Sg.links, W.bytes_links);
            S.links_lds = W.lds_links;
            S.sentinel = W.sentinel;
        }
    } else if (W.ntop) {  // HBM scene: keep the first ntop bytes of f32 nodes (top levels) in LDS
        if (static_cast<uint32_t>(reinterpret_cast<uintptr_t>((LdsByte*)smem)) != 0) __builtin_trap();
        stage_lds(smem, Sg.fnodes, W.ntop);
        S.ntop = W.ntop;
    }
}

// The lane's stack: levels 0..depth above two guard levels holding the sentinel reference and one
// more level walk() may read (three levels in HBM; in LDS that one is other data). LINK: no stack,
// its bytes hold the miss links.
template <typename SE, bool GSTACK, bool LINK>
__device__ __forceinline__ Stack<SE> lane_stack(unsigned char* smem, SE* gstack, const Work& W) {
    Stack<SE> st{};
    if (LINK) return st;
    if (GSTACK) {
        st.stride = gridDim.x * kBlock;
        st.base = gstack + (static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x) + 3 * static_cast<size_t>(st.stride);
    } else {
        st.base = reinterpret_cast<SE*>(smem + W.lds_stack) + threadIdx.x;
        st.stride = kBlock;
    }
    st.base[-static_cast<ptrdiff_t>(st.stride)] = static_cast<SE>(W.sentinel);
    st.base[-2 * static_cast<ptrdiff_t>(st.stride)] = static_cast<SE>(W.sentinel);
    return st;
}

typedef __attribute__((address_space(3))) double LdsDouble;
// the sibling-pair walk (walk_pairs) of the HBM-scene instances
template <bool LSCENE>
constexpr bool kPairWalk = CRT_PAIR_WALK && !LSCENE;

// One ray's traversal set-up, for new rays and scattered ones alike. The guard levels get the
// sentinel back (the f32 walk's store at the sentinel overwrote it). pw: the pair walk's lanes hold
// tokens (walk_pairs): the root pair's left child, and the sentinel's token in the guard levels;
// rays that need the EXACT walk keep plain refs.
template <typename SE, bool LSCENE, bool GSTACK, bool kInvLds, bool LINK, bool kFlatOnly>
__device__ __forceinline__ void ray_setup(const Work& W, Stack<SE>& st, const double o[3], const double d[3], bool pw, Trav& R) {
    trav_init(o, d, W.f32_ok != 0, R);
    const bool tok = kPairWalk<LSCENE> && pw && !(R.neg & kZeroDir);
    if (!LINK) st.base[-static_cast<ptrdiff_t>(st.stride)] = static_cast<SE>(W.sentinel | (tok ? kTokAlone : 0u));
    if (!LINK && !kFlatOnly) st.base[-2 * static_cast<ptrdiff_t>(st.stride)] = static_cast<SE>(W.sentinel | (tok ? kTokAlone : 0u));
    if (tok) R.cur = kTokAlone;
    if (kInvLds) {  // the f64 node test's 1 / d, divided once per ray (slab64_inv)
        uint32_t t = threadIdx.x;
        asm volatile("" : "+v"(t));
        LdsDouble* const inv_l = (LdsDouble*)static_cast<uintptr_t>(W.lds_inv64 + t * 8);
        inv_l[0] = 1 / d[0];
        inv_l[kBlock] = 1 / d[1];
        inv_l[2 * kBlock] = 1 / d[2];
    }
}

// The walk of one traversal round: every walking lane to its next entered leaf, or to the end of
// its traversal. The instrumented pass (COUNT) walks like the reference unless W.count_spec.
template <typename SE, bool COUNT, bool LSCENE, bool GSTACK, bool kInvLds, bool kFlatOnly, bool LINK>
__device__ __forceinline__ void walk_round(const SceneView& S, const Work& W, Stack<SE>& st, const double o[3], const double d[3],
                                           double tmin, float tmin32, bool pw, Trav& R, LaneCounters& ctr) {
    constexpr bool kTop = kTopTreelet && !LSCENE;
    if (kPairWalk<LSCENE> && pw) {
        // W.pair_walk is off for scenes that need the EXACT walk (W.exact_slab); a ray
        // with a zero / tiny / huge direction component takes it, on plain refs
        if (__ballot(R.state == kWalk && (R.neg & kZeroDir)) != 0) {
            if (R.state == kWalk && (R.neg & kZeroDir))
                walk<SE, COUNT, true, kTop, LSCENE, GSTACK, false>(S, st, o, d, tmin, tmin32, R, ctr);
        }
        if (R.state == kWalk && !(R.neg & kZeroDir))
            walk_pairs<SE, COUNT, kTop, kInvLds>(S, st, o, d, tmin, tmin32, R, ctr);
    } else if (!W.exact_slab && __ballot(R.state == kWalk && (R.neg & kZeroDir)) == 0) {
        if (R.state == kWalk) {
            if (!COUNT || W.count_spec)
                walk<SE, COUNT, false, kTop, LSCENE, GSTACK, true, kInvLds, !kFlatOnly, LINK>(S, st, o, d, tmin, tmin32, R, ctr);
            else
                walk<SE, COUNT, false, kTop, LSCENE, GSTACK, false, kInvLds, true, LINK>(S, st, o, d, tmin, tmin32, R, ctr);
        }
    } else {
        if (R.state == kWalk) walk<SE, COUNT, true, kTop, LSCENE, GSTACK, false, false, true, LINK>(S, st, o, d, tmin, tmin32, R, ctr);
    }
}

// The front end of the query and radiance kernels: a wave takes 64 consecutive rays per atomic
// (`queue` counts batches), and its lanes take the batch's rays in lane order as they finish one,
// crossing into the next batch without waiting. The wave's batch (wave-uniform) is rays
// [b_base, b_base + b_cnt), b_pos of them taken. True: the lane drew `ray`.
__device__ __forceinline__ bool draw_batch(uint32_t* queue, uint32_t batches, uint32_t n, uint32_t lane, bool& need, bool& dry,
                                           uint32_t& b_base, uint32_t& b_cnt, uint32_t& b_pos, uint32_t& ray) {
    bool start = false;
    while (!dry) {
        const uint64_t m = __ballot(need);
        if (m == 0) break;
        if (b_pos >= b_cnt) {  // the batch is used up: the next one
            const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
            uint32_t v = 0;
            if (lane == leader) v = atomicAdd(queue, 1u);
            const uint32_t j = __builtin_amdgcn_readlane(v, leader);
            if (j >= batches) {
                dry = true;
                break;
            }
            b_base = j * 64u;
            b_pos = 0;
            b_cnt = min(64u, n - b_base);
        }
        const uint32_t take = min(static_cast<uint32_t>(__popcll(m)), b_cnt - b_pos);
        const uint32_t r = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                     __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
        if (need && r < take) {
            ray = b_base + b_pos + r;
            need = false;
            start = true;
        }
        b_pos += take;
    }
    if (dry) need = false;
    return start;
}

// PM (primitive mix): 0 sphere-only scenes (every parallelogram path compiled out), 1 any scene,
// 2 parallelogram-only scenes of axis-aligned parallelograms (LDS scenes: the flat-box filter
// only, no sphere paths)
// W5: 5 waves per SIMD (96 VGPRs, ~40-48 of them spilled), launched for sphere-only and
// flat-parallelogram LDS scenes whose LDS copy leaves room for five blocks per CU (scene_layout)
// MASK: the masked pass of an adaptive render (crt_render_pass_masked_async). The queues run over
// the band's active tiles only: active[0] = their number, active[1 + i] = the band tile of list
// entry i, in tile-major order (active_list_kernel). A separate instance: the unmasked instances
// keep their code.
// LINK: the stackless walk over the scene's miss links (walk(), LINK), launched for the five-wave
// sphere-only and flat-parallelogram instances when the table exists and fits the stack region
// (dispatch_render); no Stack, no guard levels, no sentinel stores in the traversal set-up.
template <typename SE, bool GSTACK, bool LSCENE, bool COUNT, int PM, bool W5, bool MASK = false, bool LINK = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(W5 ? kManyWaves : LSCENE ? CRT_WAVES_PER_EU_LDS : CRT_WAVES_PER_EU, 8))) void render_kernel(
    SceneView Sg, CamView C, Work W, double* __restrict__ partial, SE* __restrict__ gstack,
    Counters* __restrict__ counters, const uint32_t* __restrict__ active) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // the instances with PM = 0 are launched for sphere-only scenes only, PM = 2 for scenes of
    // axis-aligned parallelograms only: the other primitive's paths are compiled out of them
    constexpr bool kSphOnly = PM == 0, kFlatOnly = PM == 2;
    // sqrt / reciprocal expansions without range fix-ups (sqrt_exact, recip_exact): measured
    // faster only in the five-wave sphere-only instance
    constexpr bool kFast = kSphOnly && W5;
    SceneView S = Sg;
    stage_scene<LSCENE, LINK>(smem, Sg, W, S);
    if (LSCENE || W.ntop) __syncthreads();  // with the staging only: one barrier of its own
    // The camera constants are read from an LDS copy in start_path / shade: held in SGPRs for
    // the whole kernel they would spill (into VGPR lanes, reloaded with v_readlane per use).
    if (threadIdx.x == 0) *reinterpret_cast<CamView*>(smem + W.lds_cam) = C;
#if CRT_WATCHDOG
    if (threadIdx.x == 0) atomicCAS(&crt_wd_deadline, 0ull, wall_clock64() + 300000000ull);  // 3 s at 100 MHz
#endif
    __syncthreads();
    const CamView& CL = *reinterpret_cast<const CamView*>(smem + W.lds_cam);
    const float tmin32 = W.tmin32;  // a kernel argument (SGPR): no conversion in the walk loop
    const uint32_t lane = threadIdx.x & 63;
    LaneCounters ctr{};
    const unsigned long long t_start = COUNT ? wall_clock64() : 0;
    Stack<SE> st = lane_stack<SE, GSTACK, LINK>(smem, gstack, W);
    // The wave's current item (wave-uniform) and how many of its 64 units are drawn; lanes take
    // the next units in lane order. A unit's sum goes to partial[chunk][pixel] whichever lane
    // traced it, so frames do not depend on the schedule.
    uint32_t item_pos = 0, item_units = 0;
    // tiles in the queues: the band's, or (MASK) the true number of active ones, whatever the host
    // sized the grid and the items for
    const uint32_t q_tiles = MASK ? active[0] : W.tiles;
    uint32_t seg = blockIdx.x % W.segments, seg_tried = 0;  // the wave's queue (XCD-local first)
    uint32_t item_txy = 0, item_chunk = 0;
    // the lane's unit: tile (tx | ty << 16), chunk << 6 | tile pixel; and its current sample
    uint32_t u_txy = 0, u_cp = 0, s = 0;
    double acc[3] = {0, 0, 0};
    // the five-wave sphere-only instance: the pixel sum lives in LDS (three doubles a lane,
    // [k][lane]), not in six VGPRs live across every phase (spill stores 17 -> 9; config 2 73.1-73.4
    // -> 72.6 ms, config 3 0.4% slower with it in the flat instance); shade adds a path's
    // contribution to a zeroed local (0 + x = x) that then goes into the LDS sum: the same
    // additions as acc + x
    constexpr bool kAccLds = kFast;
    LdsDouble* const acc_l = (LdsDouble*)static_cast<uintptr_t>(W.lds_acc + threadIdx.x * 8);
    // the five-wave flat-parallelogram instance keeps each ray's f64 1 / d in LDS for the walk's f64
    // node tests (slab64_inv) instead of dividing at each one
    constexpr bool kInvLds = (kFlatOnly && LSCENE && W5) || (!LSCENE && !GSTACK);
    // the instrumented pass walks pairs only when it walks like the timed kernel (CRT_COUNT_SPEC=1)
    const bool pw = kPairWalk<LSCENE> && W.pair_walk && (!COUNT || W.count_spec);
    S.inv64_lds = W.lds_inv64;
    if (kAccLds) {
        acc_l[0] = 0;
        acc_l[kBlock] = 0;
        acc_l[2 * kBlock] = 0;
    }
    Path P;
    Trav R;
    R.state = kIdle;
    bool need = true, start = false, cont = false;
    uint32_t cw = 0, cl = 0, cs = 0;  // wall_clock64 ticks (100 MHz), differences mod 2^32
    uint32_t cd = 0, ci = 0;
    unsigned long long t_first_idle = 0;
    while (true) {
        CRT_WD(1, item_pos, item_units);
        // lanes without a unit draw until each holds a unit with samples to trace or the queue
        // is dry. A unit off the image has no pixel sum; one with max_depth == 0 sums
        // RGB::zero() (camera.h:211-213) and is written at once.
        if (COUNT) cd -= static_cast<uint32_t>(wall_clock64());
        set_prio<kPrioInit>();
        while (true) {
            CRT_WD(2, item_pos, item_units);
            const uint64_t m = __ballot(need);
            if (m == 0) break;
            if (item_pos >= item_units) {  // the item is used up: the next one from a queue
                const uint32_t leader = static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
                item_units = 0;
                item_pos = 0;
                // this wave's segment first, then the others in turn; seg == segments: all dry
                while (seg < W.segments) {
                    const uint32_t t0 = static_cast<uint32_t>(static_cast<uint64_t>(q_tiles) * seg / W.segments);
                    const uint32_t t1 = static_cast<uint32_t>(static_cast<uint64_t>(q_tiles) * (seg + 1) / W.segments);
                    const uint32_t nt = t1 - t0, bulk = nt * W.groups;
                    uint32_t v = 0;
                    if (lane == leader) v = atomicAdd(W.queue + seg, 1u);
                    const uint32_t j = __builtin_amdgcn_readlane(v, leader);
                    if (j < nt * (W.groups + W.tail_chunks)) {
                        uint32_t tile;
                        if (j < bulk) {
                            tile = j / W.groups;
                            item_chunk = (j - tile * W.groups) * W.item_chunks;
                            item_units = 64 * W.item_chunks;
                        } else {
                            const uint32_t jt = j - bulk;
                            tile = jt / W.tail_chunks;
                            item_chunk = W.bulk_chunks + (jt - tile * W.tail_chunks);
                            item_units = 64;
                        }
                        tile += t0;
                        if (MASK) tile = active[1 + tile];  // wave-uniform: a scalar load
                        item_txy = (tile % W.tiles_x) | ((tile / W.tiles_x) << 16);
                        break;
                    }
                    if (++seg_tried >= W.segments) seg = W.segments;  // every segment is dry
                    else seg = seg + 1 == W.segments ? 0 : seg + 1;
                }
            }
            if (item_units == 0) {  // the queues are dry
                need = false;
                break;
            }
            const uint32_t take = min(static_cast<uint32_t>(__popcll(m)), item_units - item_pos);
            const uint32_t r = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                         __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
            if (need && r < take) {
                const uint32_t uu = item_pos + r, pix = uu & 63, chunk = item_chunk + (uu >> 6);
                u_txy = item_txy;
                u_cp = (chunk << 6) | pix;
                // band-local column and owned row
                const uint32_t col = (item_txy & 0xffffu) * kTileW + pix % kTileW, k = (item_txy >> 16) * kTileH + pix / kTileW;
                if (chunk < W.chunks && col < W.bw && k < W.bh) {
                    s = W.s0 + chunk * W.chunk_len;
                    if (C.max_depth > 0) {
                        need = false;
                        start = true;
                    } else if (!COUNT) {
                        double* dst = partial + (static_cast<size_t>(chunk) * W.bh * W.bw +
                                                 static_cast<size_t>(k) * W.bw + col) * 3;
                        dst[0] = 0;
                        dst[1] = 0;
                        dst[2] = 0;
                    }
                }
            }
            item_pos += take;
        }
        if (COUNT) {
            const uint32_t now = static_cast<uint32_t>(wall_clock64());
            cd += now;
            ci -= now;
        }
        if (start) {
            const uint32_t pix = u_cp & 63;
            const uint32_t col = W.col0 + (u_txy & 0xffffu) * kTileW + pix % kTileW;
            const uint32_t row = owned_row(W, W.k0 + (u_txy >> 16) * kTileH + pix / kTileW);
            start_path(CL, row, col, sample_seed(C.base_seed, row * C.w + col, s), P);
        }
        // one traversal set-up for new samples and scattered rays alike (the wave runs it once)
        if (start || cont) {
            ray_setup<SE, LSCENE, GSTACK, kInvLds, LINK, kFlatOnly>(W, st, P.o, P.d, pw, R);
            if (COUNT) ctr.rays++;
        }
        start = false;
        cont = false;
        if (COUNT) ci += static_cast<uint32_t>(wall_clock64());
        // traversal rounds (walk to the next entered leaf, test it) until enough lanes hold a
        // finished ray, or none is traversing
        while (true) {
            CRT_WD(3, R.state, R.cur);
            if (COUNT && W.round_counters) {
                const unsigned long long nw = __popcll(__ballot(R.state == kWalk));
                if (wave_leader()) {
                    atomicAdd(&counters->rounds, 1ull);
                    atomicAdd(&counters->round_walkers, nw);
                }
            }
            if (COUNT) cw -= static_cast<uint32_t>(wall_clock64());
            set_prio<kPrioWalk>();
            walk_round<SE, COUNT, LSCENE, GSTACK, kInvLds, kFlatOnly, LINK>(S, W, st, P.o, P.d, C.t_min, tmin32, pw, R, ctr);
            if (COUNT) cw += static_cast<uint32_t>(wall_clock64());
            set_prio<kPrioLeaf>();
            if (COUNT && W.round_counters) {
                const unsigned long long nl = __popcll(__ballot(R.state == kLeaf));
                if (wave_leader()) atomicAdd(&counters->round_leaves, nl);
            }
            if (COUNT) cl -= static_cast<uint32_t>(wall_clock64());
            if (R.state == kLeaf) leaf_step<SE, COUNT, kTopTreelet && !LSCENE, LSCENE, kFast, kFlatOnly, LINK>(S, st, P.o, P.d, C.t_min, tmin32, kSphOnly || (!kFlatOnly && W.sphere_only != 0), !kFlatOnly && W.spheres_f32 != 0, kFlatOnly || (!kSphOnly && W.quads_f32 != 0), kFlatOnly || (!kSphOnly && W.quads_flat != 0), R, ctr);
            if (COUNT) cl += static_cast<uint32_t>(wall_clock64());
            const uint64_t pending = __ballot(R.state == kWalk);
            const uint64_t finished = __ballot(R.state == kDone);
            const int nfin = __popcll(finished);
            if (COUNT && W.round_counters && wave_leader()) atomicAdd(&counters->round_done, static_cast<unsigned long long>(nfin));
            if (pending == 0 || nfin >= kShadeBatch) break;
        }
        const uint64_t m_done = __ballot(R.state == kDone);
        if (COUNT && t_first_idle == 0 && __ballot(R.state == kIdle) != 0) t_first_idle = wall_clock64();
        if (m_done == 0) break;  // every lane idle: the queue is dry
        if (COUNT) cs -= static_cast<uint32_t>(wall_clock64());
        set_prio<kPrioShade>();
        if (COUNT && W.round_counters && wave_leader()) atomicAdd(&counters->shade_rounds, 1ull);
        if (COUNT && ((ctr.rays | ctr.nodes | ctr.sphere_tests | ctr.quad_tests | ctr.it_walk | ctr.it_leaf |
                       ctr.it_shade | ctr.slow_nodes | ctr.it_slow | ctr.cand | ctr.it_cand) & 0x80000000u))
            flush_counts(ctr, counters);
        if (R.state == kDone) {
            if (COUNT && wave_leader()) ctr.it_shade++;
            double contrib[3] = {0, 0, 0};
            bool ended = shade<LSCENE, kSphOnly, kFlatOnly, kFast>(S, CL, P, R.found, R.ref, R.tmax, kAccLds ? contrib : acc);
            if (kAccLds && ended) {
                acc_l[0] = acc_l[0] + contrib[0];
                acc_l[kBlock] = acc_l[kBlock] + contrib[1];
                acc_l[2 * kBlock] = acc_l[2 * kBlock] + contrib[2];
            }
            // a scattered ray with no bounce left returns RGB::zero() (camera.h:211-213)
            if (!ended && P.depth == 0) ended = true;
            if (!ended) {
                cont = true;  // the scattered ray: traversal set-up with the new samples' (above)
            } else {
                const uint32_t chunk = u_cp >> 6;
                if (++s < min(C.spp, W.s0 + (chunk + 1) * W.chunk_len)) {
                    start = true;  // the unit's next sample (started after the draw, with the drawers)
                } else {  // the unit is done: its sum (samples in order) to partial[chunk][pixel]
                    if (!COUNT) {
                        const uint32_t pix = u_cp & 63;
                        const uint32_t col = (u_txy & 0xffffu) * kTileW + pix % kTileW, k = (u_txy >> 16) * kTileH + pix / kTileW;
                        double* dst = partial + (static_cast<size_t>(chunk) * W.bh * W.bw +
                                                 static_cast<size_t>(k) * W.bw + col) * 3;
                        dst[0] = kAccLds ? acc_l[0] : acc[0];
                        dst[1] = kAccLds ? acc_l[kBlock] : acc[1];
                        dst[2] = kAccLds ? acc_l[2 * kBlock] : acc[2];
                    }
                    if (kAccLds) {
                        acc_l[0] = 0;
                        acc_l[kBlock] = 0;
                        acc_l[2 * kBlock] = 0;
                    }
                    acc[0] = 0;
                    acc[1] = 0;
                    acc[2] = 0;
                    need = true;
                }
                R.state = kIdle;
            }
        }
        if (COUNT) cs += static_cast<uint32_t>(wall_clock64());
    }
    if (COUNT) {
        using ull = unsigned long long;
        flush_counts(ctr, counters);
        if (lane == 0) {  // per-wave phase times (the wave executes each phase as one)
            atomicAdd(&counters->cyc_walk, static_cast<ull>(cw));
            atomicAdd(&counters->cyc_leaf, static_cast<ull>(cl));
            atomicAdd(&counters->cyc_shade, static_cast<ull>(cs));
            atomicAdd(&counters->cyc_draw, static_cast<ull>(cd));
            atomicAdd(&counters->cyc_init, static_cast<ull>(ci));
            const unsigned long long t_end = wall_clock64();
            atomicAdd(&counters->cyc_total, t_end - t_start);
            atomicAdd(&counters->cyc_tail, t_first_idle ? t_end - t_first_idle : 0ull);
        }
    }
}

// pixel_color /= spp (camera.h:290, rgb.h:76): sum the chunks in order, multiply by 1/spp.
// One thread per pixel of the launch's band.
__global__ __launch_bounds__(256) void resolve_kernel(const double* __restrict__ partial,
                                                      double* __restrict__ out, Work W, uint32_t w,
                                                      uint32_t h, double inv_spp) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint64_t band = static_cast<uint64_t>(W.bh) * W.bw;
    if (i >= band) return;
    const uint32_t k = W.k0 + static_cast<uint32_t>(i / W.bw), col = W.col0 + static_cast<uint32_t>(i % W.bw);
    const size_t pix = static_cast<size_t>(W.packed ? k : owned_row(W, k)) * w + col;
    const size_t plane = band * 3;
    double r = partial[i * 3 + 0], g = partial[i * 3 + 1], b = partial[i * 3 + 2];
    for (uint32_t c = 1; c < W.chunks; ++c) {
        r = r + partial[c * plane + i * 3 + 0];
        g = g + partial[c * plane + i * 3 + 1];
        b = b + partial[c * plane + i * 3 + 2];
    }
    out[pix * 3 + 0] = r * inv_spp;
    out[pix * 3 + 1] = g * inv_spp;
    out[pix * 3 + 2] = b * inv_spp;
}

// resolve_kernel for one pass of a progressive render (crt_render_pass_async): the pass's chunk
// sums are added in chunk order to the pixel's running sum in `sum` (the layout of the frame), with
// resolve_kernel's own additions: a pass from sample 0 starts from partial[0], a later one from the
// stored sum, so passes issued in order add exactly what the one-shot resolve adds. out (may be
// null) receives sum * inv_done, inv_done = 1 / (double)(samples done after this pass): the frame
// so far, and after the last pass resolve_kernel's frame.
// noise (may be null; 2 doubles a pixel, the frame's pixel addressing): t += y and q += y * y over
// the pass's first full_chunks chunks, y = (r + g) + b of the chunk's sum. The ragged last chunk of
// a job has fewer samples, so its sum is not distributed like the others, and is left out.
__global__ __launch_bounds__(256) void accumulate_kernel(const double* __restrict__ partial,
                                                         double* __restrict__ sum, double* __restrict__ noise,
                                                         double* __restrict__ out, Work W, uint32_t w,
                                                         uint32_t full_chunks, double inv_done) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    const uint64_t band = static_cast<uint64_t>(W.bh) * W.bw;
    if (i >= band) return;
    const uint32_t k = W.k0 + static_cast<uint32_t>(i / W.bw), col = W.col0 + static_cast<uint32_t>(i % W.bw);
    const size_t pix = static_cast<size_t>(W.packed ? k : owned_row(W, k)) * w + col;
    const size_t plane = band * 3;
    const bool fresh = W.s0 == 0;
    double r, g, b;
    if (fresh) {
        r = partial[i * 3 + 0];
        g = partial[i * 3 + 1];
        b = partial[i * 3 + 2];
    } else {
        r = sum[pix * 3 + 0];
        g = sum[pix * 3 + 1];
        b = sum[pix * 3 + 2];
    }
    double t = 0, q = 0;
    if (noise && !fresh) {
        t = noise[pix * 2 + 0];
        q = noise[pix * 2 + 1];
    }
    for (uint32_t c = 0; c < W.chunks; ++c) {
        const double pr = partial[c * plane + i * 3 + 0], pg = partial[c * plane + i * 3 + 1],
                     pb = partial[c * plane + i * 3 + 2];
        if (c > 0 || !fresh) {
            r = r + pr;
            g = g + pg;
            b = b + pb;
        }
        if (c < full_chunks) {
            const double y = (pr + pg) + pb;
            t = t + y;
            q = q + y * y;
        }
    }
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

// out[i] = sum[i] * inv_done over n doubles: the frame of a progressive render that stops between
// previews (crt_render_progressive), accumulate_kernel's last step on its own.
__global__ __launch_bounds__(256) void scale_kernel(const double* __restrict__ sum, double* __restrict__ out,
                                                    uint64_t n, double inv_done) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) out[i] = sum[i] * inv_done;
}

// ---- adaptive sampling: block state, the active-tile list, the masked accumulate, the update ----
// A block is a kTileW x kTileH tile of the owned rows; blocks[b], b = by * ceil(w / kTileW) + bx,
// holds the samples accumulated in the block's pixels, and CRT_BLOCK_STOPPED.
static_assert(kTileW == CRT_BLOCK_W && kTileH == CRT_BLOCK_H, "a block is the render kernel's tile");

// The block of band tile `tile` (tile-major in the band): the band starts at a tile boundary.
__device__ __forceinline__ uint32_t band_block(const Work& W, uint32_t tile, uint32_t frame_tiles_x) {
    const uint32_t tx = tile % W.tiles_x, ty = tile / W.tiles_x;
    return (W.k0 / kTileH + ty) * frame_tiles_x + W.col0 / kTileW + tx;
}

// The band's tiles whose block word equals `first`, in tile-major order: active[0] = their number,
// active[1 + i] = the i-th one's band tile. One block of 1024 threads takes 1024 tiles a round:
// every wave counts its tiles with a ballot, the waves' counts are prefix-summed through LDS, and
// a lane writes at (round base + its wave's offset + the set bits below it): ordered compaction,
// so adjacent list entries are adjacent tiles. It also zeroes the render kernel's queue counters.
constexpr uint32_t kListThreads = 1024;
__global__ __launch_bounds__(kListThreads) void active_list_kernel(const uint32_t* __restrict__ blocks, Work W,
                                                                   uint32_t frame_tiles_x, uint32_t first,
                                                                   uint32_t* __restrict__ active) {
    __shared__ uint32_t wave_count[kListThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t base = 0;
    for (uint32_t t0 = 0; t0 < W.tiles; t0 += kListThreads) {
        const uint32_t tile = t0 + threadIdx.x;
        const bool on = tile < W.tiles && blocks[band_block(W, tile, frame_tiles_x)] == first;
        const uint64_t m = __ballot(on);
        if (lane == 0) wave_count[wave] = static_cast<uint32_t>(__popcll(m));
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t v = 0; v < kListThreads / 64; ++v) {
            const uint32_t c = wave_count[v];
            if (v < wave) before += c;
            all += c;
        }
        if (on) {
            const uint32_t below = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                             __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
            active[1 + base + before + below] = tile;
        }
        base += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) active[0] = base;
    if (threadIdx.x < 8) W.queue[threadIdx.x] = 0;  // the draw's queue counters, one per segment
}

// accumulate_kernel for a masked pass: one wave per band tile, lane = tile pixel. A tile whose
// block word equals the pass's first sample was rendered: its pixels get accumulate_kernel's
// additions, in its order, and the word becomes `end`. Any other tile was skipped: a pass from
// sample 0 zeroes its pixels (sum, noise, out); a later one leaves sum and noise alone and writes
// out = sum * (1 / (double)n), n = the block's own count (0 when n = 0). Only lane 0 touches the
// block word. partial == nullptr (W.s0 = ~0u, which no word equals): the out of every tile only,
// the frame of an adaptive render that ends between previews.
__global__ __launch_bounds__(256) void accumulate_masked_kernel(const double* __restrict__ partial,
                                                                double* __restrict__ sum, double* __restrict__ noise,
                                                                double* __restrict__ out, uint32_t* __restrict__ blocks,
                                                                Work W, uint32_t w, uint32_t frame_tiles_x,
                                                                uint32_t full_chunks, uint32_t end, double inv_done) {
    const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= W.tiles) return;  // wave-uniform
    const uint32_t b = band_block(W, tile, frame_tiles_x);
    uint32_t word = 0;
    if (lane == 0) word = blocks[b];
    word = __shfl(word, 0);
    const uint32_t col_l = (tile % W.tiles_x) * kTileW + lane % kTileW, k_l = (tile / W.tiles_x) * kTileH + lane / kTileW;
    const bool inside = col_l < W.bw && k_l < W.bh;
    const uint32_t k = W.k0 + k_l, col = W.col0 + col_l;
    const size_t pix = inside ? static_cast<size_t>(W.packed ? k : owned_row(W, k)) * w + col : 0;
    if (word != W.s0) {  // skipped
        if (!inside) return;
        if (W.s0 == 0) {
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
        return;
    }
    if (lane == 0) blocks[b] = end;
    if (!inside) return;
    const uint64_t i = static_cast<uint64_t>(k_l) * W.bw + col_l;
    const size_t plane = static_cast<size_t>(W.bh) * W.bw * 3;
    const bool fresh = W.s0 == 0;
    double r, g, bl;
    if (fresh) {
        r = partial[i * 3 + 0];
        g = partial[i * 3 + 1];
        bl = partial[i * 3 + 2];
    } else {
        r = sum[pix * 3 + 0];
        g = sum[pix * 3 + 1];
        bl = sum[pix * 3 + 2];
    }
    double t = 0, q = 0;
    if (noise && !fresh) {
        t = noise[pix * 2 + 0];
        q = noise[pix * 2 + 1];
    }
    for (uint32_t c = 0; c < W.chunks; ++c) {
        const double pr = partial[c * plane + i * 3 + 0], pg = partial[c * plane + i * 3 + 1],
                     pb = partial[c * plane + i * 3 + 2];
        if (c > 0 || !fresh) {
            r = r + pr;
            g = g + pg;
            bl = bl + pb;
        }
        if (c < full_chunks) {
            const double y = (pr + pg) + pb;
            t = t + y;
            q = q + y * y;
        }
    }
    sum[pix * 3 + 0] = r;
    sum[pix * 3 + 1] = g;
    sum[pix * 3 + 2] = bl;
    if (noise) {
        noise[pix * 2 + 0] = t;
        noise[pix * 2 + 1] = q;
    }
    if (out) {
        out[pix * 3 + 0] = r * inv_done;
        out[pix * 3 + 1] = g * inv_done;
        out[pix * 3 + 2] = bl * inv_done;
    }
}

// crt_adaptive_update: one wave per block of the owned rows (W: owned_rows and the tiling; w: the
// image width), lane = block pixel. A block whose word equals samples_done sums its pixels' se and
// m (noise_stage1_kernel's formulas; a lane off the image adds 0) over a butterfly of the 64 lanes:
// the order of the additions depends on the lane numbers only. may_stop = K >= 2 and the sample
// floor is reached. The block stops when sum se <= threshold * sum m (no division: an all-black
// block stops, a NaN never does); else it counts as active.
__global__ __launch_bounds__(256) void adaptive_update_kernel(const double* __restrict__ noise,
                                                              uint32_t* __restrict__ blocks, Work W, uint32_t w,
                                                              uint32_t n_blocks, uint32_t samples_done, double K,
                                                              double L, double threshold, uint32_t may_stop,
                                                              uint32_t* __restrict__ n_active) {
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= n_blocks) return;  // wave-uniform
    uint32_t word = 0;
    if (lane == 0) word = blocks[b];
    word = __shfl(word, 0);
    if (word != samples_done) return;
    bool stop = false;
    if (may_stop) {
        const uint32_t tiles_x = (w + kTileW - 1) / kTileW;
        const uint32_t col = (b % tiles_x) * kTileW + lane % kTileW, k = (b / tiles_x) * kTileH + lane / kTileW;
        double se = 0, mean = 0;
        if (col < w && k < W.owned_rows) {
            const size_t pix = static_cast<size_t>(W.packed ? k : owned_row(W, k)) * w + col;
            const double t = noise[pix * 2 + 0], q = noise[pix * 2 + 1];
            const double m = t / (K * L);
            const double var = q / (L * L) - K * m * m;
            se = sqrt(fmax(0.0, var) / (K * (K - 1)));
            mean = m;
        }
        for (int d = 1; d < 64; d <<= 1) {
            se = se + __shfl_xor(se, d);
            mean = mean + __shfl_xor(mean, d);
        }
        stop = se <= threshold * mean;
    }
    if (lane == 0) {
        if (stop) blocks[b] = word | CRT_BLOCK_STOPPED;
        else atomicAdd(n_active, 1u);
    }
}

// Noise figure of a progressive render (crt_noise_estimate). A pixel's K full chunk sums y_c (L
// samples each) are independent, identically distributed estimates of L times the pixel's value
// v = r + g + b; accumulate_kernel keeps t = sum y_c and q = sum y_c^2. Then m = t / (K L)
// estimates v, and the standard error of m is se = sqrt(max(0, q / L^2 - K m^2) / (K (K - 1))):
// the sample variance of y_c / L over K. The kernels return sum se and sum m over the pixels in
// two stages, both fixed trees (no atomics): stage 1, kNoiseBlocks blocks, thread j of block b
// sums pixels b * 256 + j, + kNoiseBlocks * 256, ... in order, then the block halves its 256
// values in LDS eight times; stage 2, one block does the same over the block results. The order of
// every addition depends on the pixel count only, so repeated calls give the same bits.
constexpr uint32_t kNoiseBlocks = 256;

__device__ __forceinline__ void noise_tree(double (*sh)[256], double& a, double& b) {
    sh[0][threadIdx.x] = a;
    sh[1][threadIdx.x] = b;
    __syncthreads();
    for (uint32_t h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h) {
            sh[0][threadIdx.x] = sh[0][threadIdx.x] + sh[0][threadIdx.x + h];
            sh[1][threadIdx.x] = sh[1][threadIdx.x] + sh[1][threadIdx.x + h];
        }
        __syncthreads();
    }
    a = sh[0][0];
    b = sh[1][0];
}

__global__ __launch_bounds__(256) void noise_stage1_kernel(const double* __restrict__ noise, uint64_t pixels,
                                                           double K, double L, double* __restrict__ block_sums) {
    __shared__ double sh[2][256];
    double se = 0, mean = 0;
    for (uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; p < pixels;
         p += static_cast<uint64_t>(kNoiseBlocks) * 256) {
        const double t = noise[p * 2 + 0], q = noise[p * 2 + 1];
        const double m = t / (K * L);
        const double var = q / (L * L) - K * m * m;
        se = se + sqrt(fmax(0.0, var) / (K * (K - 1)));
        mean = mean + m;
    }
    noise_tree(sh, se, mean);
    if (threadIdx.x == 0) {
        block_sums[blockIdx.x * 2 + 0] = se;
        block_sums[blockIdx.x * 2 + 1] = mean;
    }
}

__global__ __launch_bounds__(256) void noise_stage2_kernel(const double* __restrict__ block_sums,
                                                           double* __restrict__ out) {
    __shared__ double sh[2][256];
    static_assert(kNoiseBlocks == 256, "stage 2 reads one block result per thread");
    double se = block_sums[threadIdx.x * 2 + 0], mean = block_sums[threadIdx.x * 2 + 1];
    noise_tree(sh, se, mean);
    if (threadIdx.x == 0) {
        out[0] = se;
        out[1] = mean;
    }
}

// Image::send_as_ppm's integers (image.h:38-56; RGB::as_string rgb.h:99-115 with its defaults):
// Reinhard by luminance (rgb.h:27-29), gamma 2, static_cast<int>(255.999999 * .). The reference
// takes std::pow(x, 1/2) (rgb.h:10-13), a libm pow within ~1 ulp of the correctly rounded sqrt
// used here; where the truncated integer could differ for any value within 2 ulps of sqrt(x)
// (or v is NaN / out of int range), the kernel writes kPpmRedo and the host recomputes that
// pixel with std::pow (device_ppm_values), so every integer is the reference's.
constexpr double kPpmScale = 255 + 0.999999;
constexpr int32_t kPpmRedo = INT32_MIN + 1;

__device__ __forceinline__ int32_t ppm_channel(double c, double L) {
    const double x = c / (1 + L);
    const double s = sqrt(x);
    const double v = kPpmScale * s;
    if (!(v >= 0 && v < 2147483648.0)) return kPpmRedo;
    if (s < 0x1p-1000) return 0;  // pow(x, 0.5) is below 2^-999 too
    const uint64_t bits = static_cast<uint64_t>(__double_as_longlong(s));
    const double lo = __longlong_as_double(static_cast<long long>(bits - 2));
    const double hi = __longlong_as_double(static_cast<long long>(bits + 2));
    return static_cast<int32_t>(kPpmScale * lo) == static_cast<int32_t>(kPpmScale * hi) ? static_cast<int32_t>(v)
                                                                                          : kPpmRedo;
}

__global__ __launch_bounds__(256) void ppm_kernel(const double* __restrict__ rgb, uint64_t n,
                                                  int32_t* __restrict__ out) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const double c[3] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
    const double L = 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * i + k] = ppm_channel(c[k], L);
}

// The same values as 8-bit bytes (the fused output of crt_render_ppm: 3 B a pixel cross xGMI and
// PCIe instead of 24). A pixel with a value the kernel cannot settle, or outside [0, 255] (a NaN
// pixel prints INT_MIN), is listed in redo = [count, pixel...] (at most cap) for the host.
__global__ __launch_bounds__(256) void ppm8_kernel(const double* __restrict__ rgb, uint64_t n,
                                                   uint8_t* __restrict__ out, uint32_t* __restrict__ redo,
                                                   uint32_t cap) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const double c[3] = {rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]};
    const double L = 0.2126 * c[0] + 0.7152 * c[1] + 0.0722 * c[2];
    int32_t q[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        q[k] = ppm_channel(c[k], L);
        ok = ok && q[k] >= 0 && q[k] <= 255;
    }
    if (!ok) {
        const uint32_t j = atomicAdd(redo, 1u);
        if (j < cap) redo[1 + j] = static_cast<uint32_t>(i);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * i + k] = ok ? static_cast<uint8_t>(q[k]) : 0;
}

// The f64 values of the pixels ppm8_kernel listed for the host (redo = [count, pixel...]),
// gathered into one compact buffer: the host then copies them in one transfer
__global__ __launch_bounds__(256) void redo_gather_kernel(const double* __restrict__ rgb,
                                                          const uint32_t* __restrict__ list, uint32_t n,
                                                          double* __restrict__ out) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const size_t i = list[j];
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * static_cast<size_t>(j) + k] = rgb[3 * i + k];
}

// Closest-hit queries (BVH::hit_by for an arbitrary ray batch).
__global__ __launch_bounds__(kBlock) void hits_kernel(SceneView S, const double* __restrict__ rays,
                                                      uint32_t n, double t_min, double t_max,
                                                      const uint32_t* __restrict__ ref_prim,
                                                      uint32_t num_spheres,
                                                      crt_hit* __restrict__ out,
                                                      uint32_t* __restrict__ gstack) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Stack<uint32_t> st;
    st.base = gstack + i;
    st.stride = gridDim.x * kBlock;
    double o[3] = {rays[6 * i + 0], rays[6 * i + 1], rays[6 * i + 2]};
    double d[3] = {rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]};
    double tmax = t_max;
    uint32_t ref = 0;
    LaneCounters ctr{};
    crt_hit h{};
    h.prim = -1;
    if (trace<uint32_t, false>(S, st, o, d, t_min, tmax, ref, ctr)) {
        double p[3], nrm[3];
        bool front;
        h.material = hit_record<false>(S, ref, o, d, tmax, p, nrm, front);
        h.t = tmax;
        for (int k = 0; k < 3; ++k) { h.point[k] = p[k]; h.normal[k] = nrm[k]; }
        h.front_face = front ? 1 : 0;
        // ref_prim: spheres at [0, num_spheres), parallelograms after them
        const uint32_t k = (ref & kRefQuad) ? num_spheres + (ref & ~kRefQuad) : ref;
        h.prim = static_cast<int32_t>(ref_prim[k]);
    }
    out[i] = h;
}

// crt_render_features_async: hits_kernel's query for the centre ray of every owned pixel (thread
// i = owned row i / w, column i % w), start_path's expressions with the random terms left out.
__global__ __launch_bounds__(kBlock) void features_kernel(SceneView S, CamView C, Work W, uint32_t n,
                                                          const uint32_t* __restrict__ ref_prim,
                                                          uint32_t num_spheres,
                                                          crt_feature* __restrict__ out,
                                                          uint32_t* __restrict__ gstack) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    Stack<uint32_t> st;
    st.base = gstack + i;
    st.stride = gridDim.x * kBlock;
    const uint32_t k = i / C.w, col = i % C.w, row = owned_row(W, k);
    const double fr = static_cast<double>(row), fc = static_cast<double>(col);
    double o[3], d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double center = (C.p00[j] + C.pdy[j] * fr) + C.pdx[j] * fc;
        o[j] = C.o[j];
        d[j] = center - o[j];
    }
    double tmax = std::numeric_limits<double>::infinity();
    uint32_t ref = 0;
    LaneCounters ctr{};
    crt_feature f{};
    f.prim = -1;
    if (trace<uint32_t, false>(S, st, o, d, C.t_min, tmax, ref, ctr)) {
        double p[3], nrm[3];
        bool front;
        f.material = hit_record<false>(S, ref, o, d, tmax, p, nrm, front);
        f.t = tmax;
        const DevMaterial& m = S.mats[f.material];
        const bool glass = m.kind == CRT_DIELECTRIC;
        for (int j = 0; j < 3; ++j) {
            f.point[j] = p[j];
            f.normal[j] = nrm[j];
            f.albedo[j] = glass ? 1.0 : m.color[j];
        }
        const uint32_t r = (ref & kRefQuad) ? num_spheres + (ref & ~kRefQuad) : ref;
        f.prim = static_cast<int32_t>(ref_prim[r]);
    } else {
        for (int j = 0; j < 3; ++j) f.albedo[j] = C.bg[j];
    }
    out[static_cast<size_t>(W.packed ? k : row) * C.w + col] = f;
}

// ---- ray queries on device buffers (crt_trace_async) -------------------------------------------
// What a query launch reads and writes. Closest mode writes hits[i], any-hit mode occluded[i].
struct Query {
    const double* rays;       // n x {ox, oy, oz, dx, dy, dz}
    const double* tmax;       // n per-ray upper bounds, or null: t_max
    uint32_t n, batches;      // rays; 64-ray batches (query_kernel's queue)
    double t_min, t_max;
    const uint32_t* ref_prim;
    uint32_t num_spheres;
    crt_hit* hits;
    uint32_t* occluded;
    uint32_t* queue;          // query_kernel: the batch counter, zeroed before the launch
};

// one ray's result: R.found / R.ref / R.tmax as the walks leave them, through hit_record and the
// ref -> primitive table (hits_kernel's lines)
template <bool LS, bool SPH, bool ANY>
__device__ __forceinline__ void write_result(const SceneView& S, const Query& Q, uint32_t ray, const double o[3],
                                             const double d[3], bool found, uint32_t ref, double t) {
    if (ANY) {
        Q.occluded[ray] = found ? 1u : 0u;
        return;
    }
    crt_hit h{};
    h.prim = -1;
    if (found) {
        double p[3], nrm[3];
        bool front;
        h.material = hit_record<LS, false, SPH>(S, ref, o, d, t, p, nrm, front);
        h.t = t;
        for (int k = 0; k < 3; ++k) { h.point[k] = p[k]; h.normal[k] = nrm[k]; }
        h.front_face = front ? 1 : 0;
        const uint32_t k = (!SPH && (ref & kRefQuad)) ? Q.num_spheres + (ref & ~kRefQuad) : ref;
        h.prim = static_cast<int32_t>(Q.ref_prim[k]);
    }
    Q.hits[ray] = h;
}

// CRT_TRACE_PLAIN, and the scene classes without a fast instance: hits_kernel's loop, one thread
// per ray [first, first + gridDim.x * kBlock) of the batch, with the classification in front and a
// per-ray upper bound.
template <bool ANY>
__global__ __launch_bounds__(kBlock) void plain_query_kernel(SceneView S, Query Q, uint32_t first,
                                                             uint32_t* __restrict__ gstack) {
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= Q.n - first) return;
    const uint32_t i = first + slot;
    Stack<uint32_t> st;
    st.base = gstack + slot;
    st.stride = gridDim.x * kBlock;
    const double* r = Q.rays + 6 * static_cast<size_t>(i);
    const double o[3] = {r[0], r[1], r[2]};
    const double d[3] = {r[3], r[4], r[5]};
    double tmax = Q.tmax ? Q.tmax[i] : Q.t_max;
    uint32_t ref = 0;
    LaneCounters ctr{};
    bool found = false;
    if (ray_traceable(o, d, tmax) && ray_interval_open(Q.t_min, tmax))
        found = trace<uint32_t, false>(S, st, o, d, Q.t_min, tmax, ref, ctr);
    write_result<false, false, ANY>(S, Q, i, o, d, found, ref, tmax);
}

// The render kernel's traversal as a query engine: render_kernel's rounds (walk / walk_pairs,
// leaf_step) with "load the next ray" where it starts a path and write_result where it shades.
// A persistent grid; a wave takes 64 consecutive rays per atomic (Q.queue counts batches), and its
// lanes take the batch's rays in lane order as they finish one, crossing into the next batch
// without waiting, so neighbouring rays share a wave and a lane idles only once the queue is dry.
// A ray outside the contract (ray_traceable) goes straight to kDone as a miss: no traversal state
// is set up for it.
// PM as in render_kernel (0: sphere-only scenes, 1: any scene). ANY: a lane whose leaf step found
// an accepted primitive is done (occlusion: any primitive in the interval).
// The interval: t_min is the call's (wave-uniform, tmin32 = RN32(t_min) in W.tmin32), the upper
// bound the ray's own, and only rays with t_min < t_max are traced (crt_ray_class.h): the walks
// end at the sentinel, which a ray enters because its own interval is not empty (lo' = tmin' <=
// hi' = tmax' there, so the f32 test enters it or leaves it to f64, where -inf < t_max and
// t_min < inf enter it). walk()'s f32 node test holds for any such interval with |t_min| <= 2^100
// (its comment, "Intervals of a query"); the host clears W.f32_ok for other t_min, and every node
// test is then decided in f64. The f32 leaf filters' slack is one-sided for t_min >= 0; the host
// clears their flags for a negative t_min (device_trace), and the leaves then run the sequential
// loops.
template <typename SE, bool GSTACK, bool LSCENE, int PM, bool ANY>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(LSCENE ? CRT_WAVES_PER_EU_LDS : CRT_WAVES_PER_EU, 8))) void query_kernel(
    SceneView Sg, Work W, Query Q, SE* __restrict__ gstack) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool kSphOnly = PM == 0;
    SceneView S = Sg;
    stage_scene<LSCENE, false>(smem, Sg, W, S);
    __syncthreads();
    const float tmin32 = W.tmin32;
    const double tmin = Q.t_min;
    const uint32_t lane = threadIdx.x & 63;
    LaneCounters ctr{};
    Stack<SE> st = lane_stack<SE, GSTACK, false>(smem, gstack, W);
    constexpr bool kInvLds = !LSCENE && !GSTACK;  // the rays' f64 1 / d in LDS (slab64_inv)
    const bool pw = kPairWalk<LSCENE> && W.pair_walk;
    S.inv64_lds = W.lds_inv64;
    // the wave's batch (wave-uniform): rays [b_base, b_base + b_cnt), b_pos of them taken
    uint32_t b_base = 0, b_cnt = 0, b_pos = 0;
    bool dry = false;
    uint32_t ray = 0;
    double o[3] = {0, 0, 0}, d[3] = {0, 0, 0};
    Trav R;
    R.state = kIdle;
    bool need = true;
    while (true) {
        set_prio<kPrioInit>();
        bool start = draw_batch(Q.queue, Q.batches, Q.n, lane, need, dry, b_base, b_cnt, b_pos, ray);
        if (start) {
            const double* src = Q.rays + 6 * static_cast<size_t>(ray);
            o[0] = src[0]; o[1] = src[1]; o[2] = src[2];
            d[0] = src[3]; d[1] = src[4]; d[2] = src[5];
            const double tm = Q.tmax ? Q.tmax[ray] : Q.t_max;
            if (ray_traceable(o, d, tm) && ray_interval_open(tmin, tm)) {
                ray_setup<SE, LSCENE, GSTACK, kInvLds, false, false>(W, st, o, d, pw, R);
                R.tmax = tm;  // the ray's own upper bound
                R.tmax32 = tmax_f32(tm);
            } else {  // outside the contract, or an empty interval: a miss, never traced
                R.found = false;
                R.ref = 0;
                R.tmax = 0;
                R.state = kDone;
            }
        }
        while (true) {  // traversal rounds, as in render_kernel
            set_prio<kPrioWalk>();
            walk_round<SE, false, LSCENE, GSTACK, kInvLds, false, false>(S, W, st, o, d, tmin, tmin32, pw, R, ctr);
            set_prio<kPrioLeaf>();
            if (R.state == kLeaf) {
                leaf_step<SE, false, kTopTreelet && !LSCENE, LSCENE>(S, st, o, d, tmin, tmin32, kSphOnly || W.sphere_only != 0,
                                                                     W.spheres_f32 != 0, !kSphOnly && W.quads_f32 != 0,
                                                                     !kSphOnly && W.quads_flat != 0, R, ctr);
                if (ANY && R.found) R.state = kDone;
            }
            const uint64_t pending = __ballot(R.state == kWalk);
            const int nfin = __popcll(__ballot(R.state == kDone));
            if (pending == 0 || nfin >= kShadeBatch) break;
        }
        if (__ballot(R.state == kDone) == 0) break;  // every lane idle: the queue is dry
        set_prio<kPrioShade>();
        if (R.state == kDone) {
            write_result<LSCENE, kSphOnly, ANY>(S, Q, ray, o, d, R.found, R.ref, R.tmax);
            R.state = kIdle;
            need = true;
        }
    }
}

// ---- radiance queries on device buffers (crt_radiance_async) -----------------------------------
// What a radiance launch reads and writes: path i starts on rays[i] with the LCG state states[i]
// (null: sample_seed(base_seed, i, 0)) and writes rgb[3i .. 3i + 2]. The background and the call's
// t_min travel in a CamView (shade reads C.bg), the depth here.
struct Radiance {
    const double* rays;       // n x {ox, oy, oz, dx, dy, dz}
    const uint32_t* states;   // n LCG states before ray_color's first draw, or null
    double* rgb;              // n x 3
    uint32_t n, batches;      // paths; 64-path batches (radiance_kernel's queue)
    uint32_t max_depth;       // > 0: a call with depth 0 is answered without a launch
    uint32_t base_seed;
    uint32_t* queue;          // radiance_kernel: the batch counter, zeroed before the launch
};
// The ENV instances' launch: the same, and the caller's environment (crt_radiance_env_async). It
// stays in the kernel arguments and is read where a path ends in a miss: no LDS, so scene_layout
// decides as it does without one. The instances without an environment keep their arguments.
struct RadianceEnv : Radiance {
    crt_env env;
};
// The NEE instances' launch (crt_radiance_env_sampled_async): the sampler's recorded environment
// and its tables, in the kernel arguments too, so scene_layout still decides as without one.
struct RadianceNee : RadianceEnv {
    EnvTables tb;
};
// The lights instances' launch (crt_radiance_lights_async): the light sampler's tables, in the
// kernel arguments as well (no LDS: scene_layout decides as without a sampler).
struct RadianceLights : Radiance {
    LightTables tb;
};
// The lit instances' launch (crt_radiance_lit_async: an environment and the lights together): the
// environment, its sampler's tables where it has one (ENV, NEE, LGT; unused in ENV, LGT) and the light
// sampler's tables, all in the kernel arguments (no LDS: scene_layout decides as without them).
struct RadianceLit : RadianceNee {
    LightTables ltb;
};
template <bool ENV, bool NEE = false, bool LGT = false>
using RadianceOf = std::conditional_t<LGT, std::conditional_t<ENV, RadianceLit, RadianceLights>,
                                      std::conditional_t<NEE, RadianceNee, std::conditional_t<ENV, RadianceEnv, Radiance>>>;

// A path that ends in a miss under an environment: 0 + T * E(P.d) (crt_env.h) where shade's miss
// branch gives 0 + T * bg
__device__ __forceinline__ void env_miss(const crt_env& E, const CamView& C, const Path& P, double acc[3]) {
    double e[3];
    env_lookup(E, P.d, C.bg, e);
    acc[0] = acc[0] + P.T[0] * e[0];
    acc[1] = acc[1] + P.T[1] * e[1];
    acc[2] = acc[2] + P.T[2] * e[2];
}

// What a path of the NEE instances carries besides its Path (include/crt_render.h, the estimator):
// what it gathered, the previous bounce's density, and across a shadow segment the scattered
// direction to go on with and the sample's weight.
struct Nee {
    double acc[3];
    double pb;
    double nd[3];
    double f;
    bool has_pb;  // false: pb is "none" (the path's start, after a Metal or Dielectric bounce)
    bool shadow;  // the segment being traced is a shadow segment along P.d = d_s
};

__device__ __forceinline__ void nee_start(Nee& N) {
    N.acc[0] = 0; N.acc[1] = 0; N.acc[2] = 0;
    N.has_pb = false;
    N.shadow = false;
}

__device__ __forceinline__ double dot3(const double a[3], const double b[3]) {
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

__device__ __forceinline__ void nee_add(const crt_env& E, const CamView& C, const Path& P, double f, double acc[3]) {
    double e[3];
    env_lookup(E, P.d, C.bg, e);
    acc[0] = acc[0] + (P.T[0] * e[0]) * f;
    acc[1] = acc[1] + (P.T[1] * e[1]) * f;
    acc[2] = acc[2] + (P.T[2] * e[2]) * f;
}

// One finished segment of a path of the NEE instances, the header's estimator: true when the path
// has ended (N.acc is its output), false when P holds the next segment to trace: the scattered ray,
// or first the shadow ray of a Lambertian bounce (the same origin; N keeps the scattered direction).
template <bool LS, bool SPH>
__device__ __forceinline__ bool nee_segment(const SceneView& S, const CamView& C, const RadianceNee& Q, Path& P,
                                            Nee& N, bool found, uint32_t ref, double tmax) {
    constexpr double kPi = 3.141592653589793;
    if (N.shadow) {  // any hit occludes; a free segment adds the sample
        if (!found) nee_add(Q.env, C, P, N.f, N.acc);
        P.d[0] = N.nd[0]; P.d[1] = N.nd[1]; P.d[2] = N.nd[2];
        N.shadow = false;
        return false;
    }
    if (!found) {  // escape along d, weighted against the sampler unless pb is none
        double f = 1.0;
        if (N.has_pb) {
            const double sum = env_pdf(Q.env, Q.tb, P.d) + N.pb;
            f = sum > 0 ? N.pb / sum : 0.0;
        }
        nee_add(Q.env, C, P, f, N.acc);
        return true;
    }
    ShadeOut X;
    if (shade<LS, SPH, false, false, true>(S, C, P, true, ref, tmax, N.acc, &X)) return true;  // a light, or absorbed
    if (P.depth == 0) return true;
    if (X.kind != CRT_LAMBERTIAN) {
        N.has_pb = false;
        return false;
    }
    const double xi1 = rnd_01(P.rng);
    const double xi2 = rnd_01(P.rng);
    const double xi3 = rnd_01(P.rng);
    const double xi4 = rnd_01(P.rng);
    double ds[3];
    env_sample(Q.env, Q.tb, xi1, xi2, xi3, xi4, ds);
    const double cs = dot3(X.n, ds) / sqrt(dot3(ds, ds));
    const double pbs = cs / kPi;
    const double pes = env_pdf(Q.env, Q.tb, ds);
    N.pb = (dot3(X.n, P.d) / sqrt(dot3(P.d, P.d))) / kPi;
    N.has_pb = true;
    if (cs > 0 && pes > 0) {
        N.nd[0] = P.d[0]; N.nd[1] = P.d[1]; N.nd[2] = P.d[2];
        P.d[0] = ds[0]; P.d[1] = ds[1]; P.d[2] = ds[2];
        N.f = pbs / (pes + pbs);
        N.shadow = true;
    }
    return false;
}

// What a path of the lights instances carries besides its Path (include/crt_render.h, the lights
// estimator): Nee's fields with the sample's cosine in place of its weight, and the sampled light's
// slot reference.
struct LNee {
    double acc[3];
    double pb;
    double nd[3];
    double cs;
    uint32_t lref;
    bool has_pb;
    bool shadow;
};

__device__ __forceinline__ void nee_start(LNee& N) {
    N.acc[0] = 0; N.acc[1] = 0; N.acc[2] = 0;
    N.has_pb = false;
    N.shadow = false;
}

template <bool SPH>
__device__ __forceinline__ const DevMaterial& slot_material(const SceneView& S, uint32_t ref) {
    return (!SPH && (ref & kRefQuad)) ? S.quad_mrec[ref & ~kRefQuad] : S.sphere_mrec[ref];
}

// light_pdf of the hit at t of the ray (o, d) on the light in slot ref, a shadow ray's and a bounce
// ray's alike: the hit's own record (the true normal, IR off), the slot's area, its w by search
template <bool LS, bool SPH>
__device__ __forceinline__ double light_hit_pdf(const SceneView& S, const LightTables& Tb, uint32_t ref, const double o[3],
                                                const double d[3], double t) {
    double p[3], n[3];
    bool front;
    (void)hit_record<LS, false, SPH>(S, ref, o, d, t, p, n, front);
    double A;
    bool outside = true;
    if (!SPH && (ref & kRefQuad)) {
        const uint32_t i = ref & ~kRefQuad;
        if constexpr (LS) {
            const DevQuad q = lds_rec<DevQuad>(S.quads_lds + (i << 7));
            A = light_area_quad(q.s1, q.s2);
        } else {
            A = light_area_quad(S.quads[i].s1, S.quads[i].s2);
        }
    } else {
        const double r = sphere_at<LS>(S, ref).r;
        A = light_area_sphere(r);
        outside = front == (r > 0);
    }
    return light_pdf(light_weight(Tb, ref), Tb.W, A, t, n, d, outside);
}

__device__ __forceinline__ void light_add(const DevMaterial& M, const Path& P, double f, double acc[3]) {
    acc[0] = acc[0] + (P.T[0] * M.emit[0]) * f;
    acc[1] = acc[1] + (P.T[1] * M.emit[1]) * f;
    acc[2] = acc[2] + (P.T[2] * M.emit[2]) * f;
}

// nee_segment with the scene's lights in place of the map: one finished segment of a path of the
// lights instances. A shadow segment is an ordinary closest-hit segment towards the sampled point;
// it counts only when what it found is the sampled light's own slot.
template <bool LS, bool SPH>
__device__ __forceinline__ bool light_segment(const SceneView& S, const CamView& C, const RadianceLights& Q, Path& P,
                                              LNee& N, bool found, uint32_t ref, double tmax) {
    constexpr double kPi = 3.141592653589793;
    if (N.shadow) {
        if (found && ref == N.lref) {
            const double pl = light_hit_pdf<LS, SPH>(S, Q.tb, ref, P.o, P.d, tmax);
            if (pl > 0 && pl < __builtin_inf()) {
                const double pbs = N.cs / kPi;
                light_add(slot_material<SPH>(S, ref), P, pbs / (pl + pbs), N.acc);
            }
        }
        P.d[0] = N.nd[0]; P.d[1] = N.nd[1]; P.d[2] = N.nd[2];
        N.shadow = false;
        return false;
    }
    if (!found) {  // nothing samples the background: no weight
        N.acc[0] = N.acc[0] + P.T[0] * C.bg[0];
        N.acc[1] = N.acc[1] + P.T[1] * C.bg[1];
        N.acc[2] = N.acc[2] + P.T[2] * C.bg[2];
        return true;
    }
    ShadeOut X;
    X.kind = 0;
    if (shade<LS, SPH, false, false, 2>(S, C, P, true, ref, tmax, N.acc, &X)) {
        if (X.kind == CRT_DIFFUSE_LIGHT) {  // weighted against the sampler unless pb is none
            double f = 1.0;
            if (N.has_pb) {
                const double sum = light_hit_pdf<LS, SPH>(S, Q.tb, ref, P.o, P.d, tmax) + N.pb;
                f = sum > 0 ? N.pb / sum : 0.0;
            }
            light_add(slot_material<SPH>(S, ref), P, f, N.acc);
        }
        return true;  // a light, or absorbed
    }
    if (P.depth == 0) return true;
    if (X.kind != CRT_LAMBERTIAN) {
        N.has_pb = false;
        return false;
    }
    const double xi1 = rnd_01(P.rng);
    const uint32_t lref = Q.tb.ref[light_pick(Q.tb, xi1)];
    double pt[3], u[3] = {0, 0, 0};
    const bool quad = !SPH && (lref & kRefQuad);
    if (quad) {
        const double xi2 = rnd_01(P.rng);
        const double xi3 = rnd_01(P.rng);
        const uint32_t i = lref & ~kRefQuad;
        if constexpr (LS) {
            const DevQuad q = lds_rec<DevQuad>(S.quads_lds + (i << 7));
            light_point(q.v, q.s1, q.s2, xi2, xi3, pt);
        } else {
            light_point(S.quads[i].v, S.quads[i].s1, S.quads[i].s2, xi2, xi3, pt);
        }
    } else {
        random_unit_vector<false>(P.rng, u[0], u[1], u[2]);
        const DevSphere sp = sphere_at<LS>(S, lref);
        light_point(sp.c, sp.r, u, pt);
    }
    const double ds[3] = {pt[0] - P.o[0], pt[1] - P.o[1], pt[2] - P.o[2]};
    const double cs = dot3(X.n, ds) / sqrt(dot3(ds, ds));
    N.pb = (dot3(X.n, P.d) / sqrt(dot3(P.d, P.d))) / kPi;
    N.has_pb = true;
    // a point on a sphere's far side is hidden by its near side: no ray
    if (cs > 0 && (quad || dot3(u, ds) < 0)) {
        N.nd[0] = P.d[0]; N.nd[1] = P.d[1]; N.nd[2] = P.d[2];
        P.d[0] = ds[0]; P.d[1] = ds[1]; P.d[2] = ds[2];
        N.cs = cs;
        N.lref = lref;
        N.shadow = true;
    }
    return false;
}

// What a path of the lit instances (an environment and the scene's lights together) carries besides
// its Path (include/crt_render.h, the lit estimator). The light sample's draws are made after the map
// sample's shadow segment has come back (no segment draws a number: the values are the same), so
// across that segment the lane keeps the bounce's normal and not a second direction; w is the map
// sample's weight across a map segment and the light sample's cosine across a light segment.
struct Lit {
    double acc[3];
    double pb;
    double nd[3];
    double n[3];
    double w;
    uint32_t lref;
    uint32_t shadow;  // kLitNone, or the segment being traced is a shadow segment: kLitMap, kLitLight
    bool has_pb;
};
constexpr uint32_t kLitNone = 0, kLitMap = 1, kLitLight = 2;

__device__ __forceinline__ void nee_start(Lit& N) {
    N.acc[0] = 0; N.acc[1] = 0; N.acc[2] = 0;
    N.has_pb = false;
    N.shadow = kLitNone;
}

// nee_segment and light_segment joined: one finished segment of a path of the lit instances. SMP: the
// environment has a sampler (a map sample a Lambertian bounce, escapes weighted against it); without
// one the environment is found by escapes alone, as in the ENV instances. A Lambertian bounce may
// leave the map sample's shadow ray in P, then the light sample's, then the scattered ray.
template <bool LS, bool SPH, bool SMP>
__device__ __forceinline__ bool lit_segment(const SceneView& S, const CamView& C, const RadianceLit& Q, Path& P, Lit& N,
                                            bool found, uint32_t ref, double tmax) {
    constexpr double kPi = 3.141592653589793;
    if (N.shadow == kLitLight) {  // counts only when it found the sampled light's own slot
        if (found && ref == N.lref) {
            const double pl = light_hit_pdf<LS, SPH>(S, Q.ltb, ref, P.o, P.d, tmax);
            if (pl > 0 && pl < __builtin_inf()) {
                const double pbs = N.w / kPi;
                light_add(slot_material<SPH>(S, ref), P, pbs / (pl + pbs), N.acc);
            }
        }
        P.d[0] = N.nd[0]; P.d[1] = N.nd[1]; P.d[2] = N.nd[2];
        N.shadow = kLitNone;
        return false;
    }
    if (N.shadow == kLitMap) {  // any hit occludes; a free segment adds the sample; the light sample follows
        if (!found) nee_add(Q.env, C, P, N.w, N.acc);
        N.shadow = kLitNone;
    } else {
        if (!found) {  // escape along d, weighted against the map's sampler if there is one and pb is not none
            double f = 1.0;
            if constexpr (SMP) {
                if (N.has_pb) {
                    const double sum = env_pdf(Q.env, Q.tb, P.d) + N.pb;
                    f = sum > 0 ? N.pb / sum : 0.0;
                }
                nee_add(Q.env, C, P, f, N.acc);
            } else {
                env_miss(Q.env, C, P, N.acc);
            }
            return true;
        }
        ShadeOut X;
        X.kind = 0;
        if (shade<LS, SPH, false, false, 2>(S, C, P, true, ref, tmax, N.acc, &X)) {
            if (X.kind == CRT_DIFFUSE_LIGHT) {  // weighted against the light sampler unless pb is none
                double f = 1.0;
                if (N.has_pb) {
                    const double sum = light_hit_pdf<LS, SPH>(S, Q.ltb, ref, P.o, P.d, tmax) + N.pb;
                    f = sum > 0 ? N.pb / sum : 0.0;
                }
                light_add(slot_material<SPH>(S, ref), P, f, N.acc);
            }
            return true;  // a light, or absorbed
        }
        if (P.depth == 0) return true;
        if (X.kind != CRT_LAMBERTIAN) {
            N.has_pb = false;
            return false;
        }
        N.n[0] = X.n[0]; N.n[1] = X.n[1]; N.n[2] = X.n[2];
        N.nd[0] = P.d[0]; N.nd[1] = P.d[1]; N.nd[2] = P.d[2];
        bool ray_e = false;
        if constexpr (SMP) {
            const double xi1 = rnd_01(P.rng);
            const double xi2 = rnd_01(P.rng);
            const double xi3 = rnd_01(P.rng);
            const double xi4 = rnd_01(P.rng);
            double de[3];
            env_sample(Q.env, Q.tb, xi1, xi2, xi3, xi4, de);
            const double ce = dot3(N.n, de) / sqrt(dot3(de, de));
            const double pbe = ce / kPi;
            const double pe = env_pdf(Q.env, Q.tb, de);
            ray_e = ce > 0 && pe > 0;
            if (ray_e) {
                P.d[0] = de[0]; P.d[1] = de[1]; P.d[2] = de[2];
                N.w = pbe / (pe + pbe);
            }
        }
        N.pb = (dot3(N.n, N.nd) / sqrt(dot3(N.nd, N.nd))) / kPi;
        N.has_pb = true;
        if (ray_e) {
            N.shadow = kLitMap;
            return false;
        }
    }
    // the light sample of the bounce at P.o with the normal N.n
    const double xi1 = rnd_01(P.rng);
    const uint32_t lref = Q.ltb.ref[light_pick(Q.ltb, xi1)];
    double pt[3], u[3] = {0, 0, 0};
    const bool quad = !SPH && (lref & kRefQuad);
    if (quad) {
        const double xi2 = rnd_01(P.rng);
        const double xi3 = rnd_01(P.rng);
        const uint32_t i = lref & ~kRefQuad;
        if constexpr (LS) {
            const DevQuad q = lds_rec<DevQuad>(S.quads_lds + (i << 7));
            light_point(q.v, q.s1, q.s2, xi2, xi3, pt);
        } else {
            light_point(S.quads[i].v, S.quads[i].s1, S.quads[i].s2, xi2, xi3, pt);
        }
    } else {
        random_unit_vector<false>(P.rng, u[0], u[1], u[2]);
        const DevSphere sp = sphere_at<LS>(S, lref);
        light_point(sp.c, sp.r, u, pt);
    }
    const double dl[3] = {pt[0] - P.o[0], pt[1] - P.o[1], pt[2] - P.o[2]};
    const double cl = dot3(N.n, dl) / sqrt(dot3(dl, dl));
    // a point on a sphere's far side is hidden by its near side: no ray
    if (cl > 0 && (quad || dot3(u, dl) < 0)) {
        P.d[0] = dl[0]; P.d[1] = dl[1]; P.d[2] = dl[2];
        N.w = cl;
        N.lref = lref;
        N.shadow = kLitLight;
    } else {
        P.d[0] = N.nd[0]; P.d[1] = N.nd[1]; P.d[2] = N.nd[2];
    }
    return false;
}

// path `ray` of a launch, before its first segment. False: the caller's ray is outside the query
// contract (crt_ray_class.h) and must not be traced; shade's miss branch then gives 0 + 1 * bg.
__device__ __forceinline__ bool load_path(const Radiance& Q, uint32_t ray, Path& P) {
    const double* src = Q.rays + 6 * static_cast<size_t>(ray);
    P.o[0] = src[0]; P.o[1] = src[1]; P.o[2] = src[2];
    P.d[0] = src[3]; P.d[1] = src[4]; P.d[2] = src[5];
    P.T[0] = 1; P.T[1] = 1; P.T[2] = 1;
    P.depth = Q.max_depth;
    P.rng = Q.states ? Q.states[ray] : sample_seed(Q.base_seed, ray, 0);
    return ray_traceable(P.o, P.d, __builtin_inf());
}

// CRT_RADIANCE_PLAIN: ray_color as a loop of trace() and shade, one thread per path
// [first, first + gridDim.x * kBlock) of the call. Scattered rays go to trace() as they are: it is
// the reference's sequence for any ray. ENV: a miss ends the path with env_miss instead of shade.
// NEE (on top of ENV): every finished segment goes through nee_segment, shadow segments included.
// LGT (without ENV or NEE): the same through light_segment (crt_radiance_lights_async).
// ENV and LGT, with or without NEE: the same through lit_segment (crt_radiance_lit_async).
template <bool ENV = false, bool NEE = false, bool LGT = false>
__global__ __launch_bounds__(kBlock) void plain_radiance_kernel(SceneView S, CamView C, RadianceOf<ENV, NEE, LGT> Q, uint32_t first,
                                                                uint32_t* __restrict__ gstack) {
    const uint32_t slot = blockIdx.x * kBlock + threadIdx.x;
    if (slot >= Q.n - first) return;
    const uint32_t i = first + slot;
    Stack<uint32_t> st;
    st.base = gstack + slot;
    st.stride = gridDim.x * kBlock;
    Path P;
    bool traced = load_path(Q, i, P);
    LaneCounters ctr{};
    double acc[3] = {0, 0, 0};
    [[maybe_unused]] std::conditional_t<LGT, std::conditional_t<ENV, Lit, LNee>, Nee> N;
    if constexpr (NEE || LGT) nee_start(N);
    while (true) {
        double tmax = __builtin_inf();
        uint32_t ref = 0;
        const bool found = traced && trace<uint32_t, false>(S, st, P.o, P.d, C.t_min, tmax, ref, ctr);
        traced = true;
        if constexpr (LGT && ENV) {
            if (lit_segment<false, false, NEE>(S, C, Q, P, N, found, ref, tmax)) break;
            continue;
        } else if constexpr (LGT) {
            if (light_segment<false, false>(S, C, Q, P, N, found, ref, tmax)) break;
            continue;
        } else if constexpr (NEE) {
            if (nee_segment<false, false>(S, C, Q, P, N, found, ref, tmax)) break;
            continue;
        } else if constexpr (ENV) {
            if (!found) {
                env_miss(Q.env, C, P, acc);
                break;
            }
        }
        if (shade<false>(S, C, P, found, ref, tmax, acc) || P.depth == 0) break;
    }
    if constexpr (NEE || LGT) {
        acc[0] = N.acc[0]; acc[1] = N.acc[1]; acc[2] = N.acc[2];
    }
    double* dst = Q.rgb + 3 * static_cast<size_t>(i);
    dst[0] = acc[0];
    dst[1] = acc[1];
    dst[2] = acc[2];
}

// The render kernel's integrator as a query engine: query_kernel's front end (the persistent grid,
// the batch queue, "load the next ray") joined to render_kernel's back end (shade, then continue
// the scattered ray or end the path). A lane keeps its path over all its segments; a path that
// ends stores 0 + T * (emit | background), or +0, and the lane asks for the next ray.
// The caller's ray is classified before any traversal state exists (load_path); one outside the
// contract goes to kDone as a miss and is shaded as one. Scattered rays are render_kernel's: set up
// by ray_setup, which rewrites both guard levels (the f32 walk's store at the sentinel overwrote
// one). Every segment runs over (t_min, +inf) with t_min >= 0 (the ABI's rule), so the leaf filters
// hold as in a render. The camera copy in LDS is render_kernel's (shade reads the background from
// it). ENV: a lane in kDone without a hit ends its path with env_miss instead of shade.
// NEE (on top of ENV): a lane in kDone hands its finished segment to nee_segment. A Lambertian
// bounce may leave a shadow ray in P; it runs through the same ray_setup, walk_round and leaf_step
// rounds as any segment (closest hit: only "any hit" enters), and nee_segment then puts the saved
// scattered direction back. The lane's Nee stays in registers across all of it.
// LGT (without ENV or NEE): the same with light_segment and its LNee (crt_radiance_lights_async); the
// shadow ray ends on the sampled light or on what hides it, a closest hit either way.
// ENV and LGT, with or without NEE: lit_segment and its Lit (crt_radiance_lit_async); a bounce may run
// two shadow segments through these rounds before the saved scattered direction comes back.
template <typename SE, bool GSTACK, bool LSCENE, int PM, bool ENV = false, bool NEE = false, bool LGT = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu((NEE || LGT) ? CRT_WAVES_PER_EU_NEE : LSCENE ? CRT_WAVES_PER_EU_LDS : CRT_WAVES_PER_EU, 8))) void radiance_kernel(
    SceneView Sg, CamView C, Work W, RadianceOf<ENV, NEE, LGT> Q, SE* __restrict__ gstack) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool kSphOnly = PM == 0;
    SceneView S = Sg;
    stage_scene<LSCENE, false>(smem, Sg, W, S);
    if (threadIdx.x == 0) *reinterpret_cast<CamView*>(smem + W.lds_cam) = C;
    __syncthreads();
    const CamView& CL = *reinterpret_cast<const CamView*>(smem + W.lds_cam);
    const float tmin32 = W.tmin32;
    const double tmin = C.t_min;
    const uint32_t lane = threadIdx.x & 63;
    LaneCounters ctr{};
    Stack<SE> st = lane_stack<SE, GSTACK, false>(smem, gstack, W);
    constexpr bool kInvLds = !LSCENE && !GSTACK;  // the rays' f64 1 / d in LDS (slab64_inv)
    const bool pw = kPairWalk<LSCENE> && W.pair_walk;
    S.inv64_lds = W.lds_inv64;
    // the wave's batch (wave-uniform): paths [b_base, b_base + b_cnt), b_pos of them taken
    uint32_t b_base = 0, b_cnt = 0, b_pos = 0;
    bool dry = false;
    uint32_t ray = 0;
    Path P;
    Trav R;
    R.state = kIdle;
    [[maybe_unused]] std::conditional_t<LGT, std::conditional_t<ENV, Lit, LNee>, Nee> N;
    bool need = true, cont = false;
    while (true) {
        set_prio<kPrioInit>();
        bool start = draw_batch(Q.queue, Q.batches, Q.n, lane, need, dry, b_base, b_cnt, b_pos, ray);
        if constexpr (NEE || LGT) {
            if (start) nee_start(N);
        }
        if (start && !load_path(Q, ray, P)) {  // outside the contract: a miss, never traced
            start = false;
            R.found = false;
            R.ref = 0;
            R.tmax = 0;
            R.state = kDone;
        }
        // one traversal set-up for new paths and scattered rays alike
        if (start || cont) ray_setup<SE, LSCENE, GSTACK, kInvLds, false, false>(W, st, P.o, P.d, pw, R);
        cont = false;
        while (true) {  // traversal rounds, as in render_kernel
            set_prio<kPrioWalk>();
            walk_round<SE, false, LSCENE, GSTACK, kInvLds, false, false>(S, W, st, P.o, P.d, tmin, tmin32, pw, R, ctr);
            set_prio<kPrioLeaf>();
            if (R.state == kLeaf)
                leaf_step<SE, false, kTopTreelet && !LSCENE, LSCENE>(S, st, P.o, P.d, tmin, tmin32, kSphOnly || W.sphere_only != 0,
                                                                     W.spheres_f32 != 0, !kSphOnly && W.quads_f32 != 0,
                                                                     !kSphOnly && W.quads_flat != 0, R, ctr);
            const uint64_t pending = __ballot(R.state == kWalk);
            const int nfin = __popcll(__ballot(R.state == kDone));
            if (pending == 0 || nfin >= kShadeBatch) break;
        }
        if (__ballot(R.state == kDone) == 0) break;  // every lane idle: the queue is dry
        set_prio<kPrioShade>();
        if (R.state == kDone) {
            double acc[3] = {0, 0, 0};
            bool ended = true;
            if constexpr (LGT && ENV) {
                ended = lit_segment<LSCENE, kSphOnly, NEE>(S, CL, Q, P, N, R.found, R.ref, R.tmax);
                acc[0] = N.acc[0]; acc[1] = N.acc[1]; acc[2] = N.acc[2];
            } else if constexpr (LGT) {
                ended = light_segment<LSCENE, kSphOnly>(S, CL, Q, P, N, R.found, R.ref, R.tmax);
                acc[0] = N.acc[0]; acc[1] = N.acc[1]; acc[2] = N.acc[2];
            } else if constexpr (NEE) {
                ended = nee_segment<LSCENE, kSphOnly>(S, CL, Q, P, N, R.found, R.ref, R.tmax);
                acc[0] = N.acc[0]; acc[1] = N.acc[1]; acc[2] = N.acc[2];
            } else if constexpr (ENV) {
                if (!R.found) env_miss(Q.env, CL, P, acc);
                else ended = shade<LSCENE, kSphOnly>(S, CL, P, R.found, R.ref, R.tmax, acc);
            } else {
                ended = shade<LSCENE, kSphOnly>(S, CL, P, R.found, R.ref, R.tmax, acc);
            }
            // a scattered ray with no bounce left returns RGB::zero() (camera.h:211-213)
            if (!ended && P.depth == 0) ended = true;
            if (!ended) {
                cont = true;
            } else {
                double* dst = Q.rgb + 3 * static_cast<size_t>(ray);
                dst[0] = acc[0];
                dst[1] = acc[1];
                dst[2] = acc[2];
                R.state = kIdle;
                need = true;
            }
        }
    }
}

// crt_camera_rays_async: start_path as a kernel of its own, one thread per record. Record
// j * ns + (s - s0) holds owned pixel j's (owned rows in order, packed) sample s: the ray and the
// LCG state after its draws.
__global__ __launch_bounds__(256) void camera_rays_kernel(CamView C, Work W, uint32_t n, uint32_t s0, uint32_t ns,
                                                          double* __restrict__ rays, uint32_t* __restrict__ states) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = i / ns, s = s0 + i % ns;
    const uint32_t col = j % C.w, row = owned_row(W, j / C.w);
    Path P;
    start_path(C, row, col, sample_seed(C.base_seed, row * C.w + col, s), P);
    double* dst = rays + 6 * static_cast<size_t>(i);
    dst[0] = P.o[0]; dst[1] = P.o[1]; dst[2] = P.o[2];
    dst[3] = P.d[0]; dst[4] = P.d[1]; dst[5] = P.d[2];
    states[i] = P.rng;
}

// crt_pixel_variance_async: thread i = owned row i / w, column i % w. n = samples_done, or the
// pixel's block word (adaptive_update_kernel's block numbering) without the stopped bit;
// noise_stage1_kernel's expressions for m and the variance of the mean, without its sqrt.
__global__ __launch_bounds__(256) void pixel_variance_kernel(const double* __restrict__ noise,
                                                             const uint32_t* __restrict__ blocks, Work W, uint32_t w,
                                                             uint32_t n_pixels, uint32_t samples_done, uint32_t L_,
                                                             double* __restrict__ var_out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pixels) return;
    const uint32_t k = i / w, col = i % w;
    const size_t pix = static_cast<size_t>(W.packed ? k : owned_row(W, k)) * w + col;
    uint32_t n = samples_done;
    if (blocks) {
        const uint32_t tiles_x = (w + kTileW - 1) / kTileW;
        n = blocks[(k / kTileH) * tiles_x + col / kTileW] & ~CRT_BLOCK_STOPPED;
    }
    const uint32_t Ki = n / L_;
    const double K = static_cast<double>(Ki), L = static_cast<double>(L_);
    double v = 0;
    if (Ki >= 1) {
        const double t = noise[pix * 2 + 0], q = noise[pix * 2 + 1];
        const double m = t / (K * L);
        if (Ki == 1) {
            v = m * m;
        } else {
            const double var = q / (L * L) - K * m * m;
            v = (var > 0 ? var : 0.0) / (K * (K - 1));
        }
    }
    var_out[pix] = v;
}

}  // namespace dev

// =============================================================================================
// host launch plumbing

static dev::SceneView view_of(const DeviceCopy& c) {
    dev::SceneView v{c.nodes, c.fnodes, 0, c.refs, c.spheres, c.spair, 0, c.sphere_mat, c.quads, c.quad_mat,
                     c.mats, c.quadf, c.sphere_mrec, c.quad_mrec, 0, c.quadbox};
    v.guard = c.guard;
    v.links = c.links;
    return v;
}

int device_count(int* n) {
    hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) {
        *n = 0;
        return fail(CRT_E_NODEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    return CRT_OK;
}

static int check_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(CRT_E_NODEVICE, "no HIP device visible (the render path has no CPU fallback)");
    if (device < 0 || device >= n || device >= kMaxDevices)
        return fail(CRT_E_NODEVICE, "device " + std::to_string(device) + " out of range");
    return CRT_OK;
}

static size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// The device image of a scene: every array of device_layout() at its offset in one host buffer,
// built once per scene (the first upload) and copied whole to each device. The derived arrays
// (f32 nodes, filter records, per-slot material records) are written straight into the image,
// per element in parallel (parallel_for); the image is not zero-filled first, only the guard words
// (and the padding, which nothing reads) are cleared.
static void stage_image(crt_scene* s) {
    const size_t n_nodes = s->num_dnodes, n_refs = s->num_prims;
    const size_t n_sp = s->num_spheres, n_q = s->num_quads, n_m = s->num_dmats;
    size_t off[kArrCount + 1];
    const size_t total = device_layout(s, off);
    BigVec<char>& img = s->image;
    img.resize(total);
    auto at = [&](int arr) { return img.data() + off[arr]; };
    // padding between the arrays (and the guard words): zero
    for (int a = 0; a < kArrCount; ++a) {
        static const size_t kElem[kArrCount] = {sizeof(DevNode), sizeof(DevNodeF), 4, sizeof(DevSphere), sizeof(DevSpherePair),
                                                4, sizeof(DevQuad), sizeof(DevQuadF), sizeof(DevQuadBox), 4,
                                                sizeof(DevMaterial), sizeof(DevMaterial), sizeof(DevMaterial), 1};
        const size_t cnt[kArrCount] = {n_nodes, n_nodes, n_refs, n_sp, n_sp, n_sp, n_q, n_q, n_q, n_q, n_m, n_sp, n_q, 64};
        const size_t used = a == kArrGuard ? 0 : cnt[a] * kElem[a];
        std::memset(img.data() + off[a] + used, 0, off[a + 1] - off[a] - used);
    }
    // plain copies, in parallel chunks
    auto put = [&](int arr, const void* src, size_t bytes) {
        char* dst = at(arr);
        const char* sp = static_cast<const char*>(src);
        parallel_for(bytes, size_t{1} << 22, [&](size_t a, size_t b) { std::memcpy(dst + a, sp + a, b - a); });
    };
    put(kArrNodes, s->dnodes.data(), n_nodes * sizeof(DevNode));
    put(kArrRefs, s->refs.data(), n_refs * 4);
    put(kArrSpheres, s->spheres.data(), n_sp * sizeof(DevSphere));
    put(kArrSphereMat, s->sphere_mat.data(), n_sp * 4);
    put(kArrQuads, s->quads.data(), n_q * sizeof(DevQuad));
    put(kArrQuadMat, s->quad_mat.data(), n_q * 4);
    put(kArrMats, s->dmats.data(), n_m * sizeof(DevMaterial));
    // f32 refs are byte offsets (index << 5) and interior w1 must stay below kLeafFlagF
    DevNodeF* fnodes = reinterpret_cast<DevNodeF*>(at(kArrFNodes));
    std::atomic<bool> f32_bad{false};
    parallel_for(n_nodes, 4096, [&](size_t a, size_t b) {
        bool bad = false;
        for (size_t i = a; i < b; ++i) bad = node_record(s->dnodes[i], static_cast<uint32_t>(i), fnodes[i]) || bad;
        if (bad) f32_bad = true;
    });
    // sphere pair records of the f32 candidate filter (slots i, i + 1): half i of record i from
    // sphere i, the other half from sphere i + 1 (the last record's second half zero)
    DevSpherePair* spair = reinterpret_cast<DevSpherePair*>(at(kArrSpherePairs));
    std::atomic<bool> sph_bad{false};
    parallel_for(n_sp, 4096, [&](size_t a, size_t b) {
        bool bad = false;
        for (size_t i = a; i < b; ++i) {
            DevSpherePair& r = spair[i];
            bad = sphere_pair_half(s->spheres[i], r.cx[0], r.cy[0], r.cz[0], r.r2e[0]) || bad;
            if (i + 1 < n_sp) (void)sphere_pair_half(s->spheres[i + 1], r.cx[1], r.cy[1], r.cz[1], r.r2e[1]);
            else r.cx[1] = r.cy[1] = r.cz[1] = r.r2e[1] = 0;
        }
        if (bad) sph_bad = true;
    });
    // parallelogram filter records (crt_quad_filter.h quad_record, quad_flat_box)
    DevQuadF* quadf = reinterpret_cast<DevQuadF*>(at(kArrQuadF));
    DevQuadBox* quadbox = reinterpret_cast<DevQuadBox*>(at(kArrQuadBox));
    std::atomic<bool> quads_bad{false}, flat_bad{false};
    parallel_for(n_q, 4096, [&](size_t a, size_t b) {
        bool qb = false, fb = false;
        for (size_t i = a; i < b; ++i) {
            const DevQuad& q = s->quads[i];
            if (!quad_record(q.v, q.s1, q.s2, q.sn, quadf[i])) qb = true;
            quadbox[i] = DevQuadBox{};  // a record quad_flat_box rejects stays zero
            if (!quad_flat_box(q.v, q.s1, q.s2, quadbox[i])) fb = true;
        }
        if (qb) quads_bad = true;
        if (fb) flat_bad = true;
    });
    // parallelogram-only scenes of axis-aligned parallelograms: each leaf's flat boxes grouped by
    // their flat axis (regroup_leaf)
    std::atomic<bool> regroup_bad{false};
    if (!flat_bad && n_sp == 0 && n_q > 0) {
        parallel_for(n_nodes, 1 << 12, [&](size_t a, size_t b) {
            bool bad = false;
            for (size_t k = a; k < b; ++k) bad = regroup_leaf(s->dnodes[k], k, quadbox) || bad;
            if (bad) regroup_bad = true;
        });
    }
    // shading constants per slot (shading_consts)
    DevMaterial* smrec = reinterpret_cast<DevMaterial*>(at(kArrSphereMrec));
    DevMaterial* qmrec = reinterpret_cast<DevMaterial*>(at(kArrQuadMrec));
    parallel_for(n_sp, 4096, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; ++i) {
            smrec[i] = s->dmats[s->sphere_mat[i]];
            shading_consts(smrec[i], &s->spheres[i]);
        }
    });
    parallel_for(n_q, 4096, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; ++i) {
            qmrec[i] = s->dmats[s->quad_mat[i]];
            shading_consts(qmrec[i], nullptr);
        }
    });
    s->image_f32_ok = !f32_bad;
    s->image_spheres_f32_ok = !sph_bad;
    s->image_quads_f32_ok = !quads_bad;
    s->image_quads_flat_ok = !flat_bad && !regroup_bad;
    s->staged = true;
}

// The f32 flags of a scene copy: the staged image's, less what the switches turn off (read when the
// copy is bound, device_bind_copy, and by crt_launch_plan when it is asked)
struct CopyFlags {
    bool f32_ok, spheres_f32_ok, quads_f32_ok, quads_flat_ok;
};
static CopyFlags copy_flags(const crt_scene* s) {
    CopyFlags f;
    f.f32_ok = s->image_f32_ok && std::getenv("CRT_F64_NODES") == nullptr;
    f.spheres_f32_ok = s->image_spheres_f32_ok && std::getenv("CRT_F64_SPHERES") == nullptr;
    f.quads_f32_ok = s->image_quads_f32_ok && std::getenv("CRT_F64_QUADS") == nullptr;
    // CRT_GENERIC_QUADS=1: the generic parallelogram filter even for axis-aligned ones
    f.quads_flat_ok = s->image_quads_flat_ok && std::getenv("CRT_GENERIC_QUADS") == nullptr;
    return f;
}
static CopyFlags flags_of(const DeviceCopy& c) {
    return CopyFlags{c.f32_ok, c.spheres_f32_ok, c.quads_f32_ok, c.quads_flat_ok};
}

static bool u16_entries(const crt_scene* s);
static void bind_links(crt_scene* s, DeviceCopy& c);

// The pointers of a scene copy at `base` (device_layout's arrays at their offsets).
void device_bind_copy(crt_scene* s, int device, void* base, size_t total) {
    size_t off[kArrCount + 1];
    (void)device_layout(s, off);
    DeviceCopy& c = s->dev[device];
    const CopyFlags f = copy_flags(s);
    char* b = static_cast<char*>(base);
    c.base = base;
    c.bytes = total;
    c.nodes = reinterpret_cast<DevNode*>(b + off[kArrNodes]);
    c.fnodes = reinterpret_cast<DevNodeF*>(b + off[kArrFNodes]);
    c.f32_ok = f.f32_ok;
    c.refs = reinterpret_cast<uint32_t*>(b + off[kArrRefs]);
    c.spheres = reinterpret_cast<DevSphere*>(b + off[kArrSpheres]);
    c.spair = reinterpret_cast<DevSpherePair*>(b + off[kArrSpherePairs]);
    c.spheres_f32_ok = f.spheres_f32_ok;
    c.sphere_mat = reinterpret_cast<uint32_t*>(b + off[kArrSphereMat]);
    c.quads = reinterpret_cast<DevQuad*>(b + off[kArrQuads]);
    c.quadf = reinterpret_cast<DevQuadF*>(b + off[kArrQuadF]);
    c.quads_f32_ok = f.quads_f32_ok;
    c.quadbox = reinterpret_cast<DevQuadBox*>(b + off[kArrQuadBox]);
    c.quads_flat_ok = f.quads_flat_ok;
    c.quad_mat = reinterpret_cast<uint32_t*>(b + off[kArrQuadMat]);
    c.mats = reinterpret_cast<DevMaterial*>(b + off[kArrMats]);
    c.sphere_mrec = reinterpret_cast<DevMaterial*>(b + off[kArrSphereMrec]);
    c.quad_mrec = reinterpret_cast<DevMaterial*>(b + off[kArrQuadMrec]);
    c.guard = reinterpret_cast<unsigned long long*>(b + off[kArrGuard]);
    c.valid = true;
    bind_links(s, c);
}

// the nodes of the copy at `c` (device order), read back: 64 bytes a node, LDS-size trees only
static bool copy_nodes_host(const crt_scene* s, const DeviceCopy& c, std::vector<DevNode>& out) {
    out.resize(s->num_dnodes);
    return hipMemcpy(out.data(), c.nodes, out.size() * sizeof(DevNode), hipMemcpyDeviceToHost) == hipSuccess;
}

// The scene's miss-link table (crt_walk_links.h), built and checked on the host once per scene
// (scene_walk_links: a wrong link would be an endless loop of a wave) and kept in crt_scene::links:
// for trees whose refs fit u16 entries, the only ones an LDS-scene launch can take. From the host
// staging's nodes, or for a scene set up on a device (no host arrays) from the nodes of the copy
// `from`, read back. Without a table (too large, failed its check) the scene keeps the stack walk;
// that is no error.
static const std::vector<uint16_t>& scene_links(crt_scene* s, const DeviceCopy* from) {
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->links_built) return s->links;
    if (u16_entries(s) && s->num_dnodes >= 2) {
        if (s->image_device < 0) {
            std::vector<DevNode> nodes(s->dnodes.begin(), s->dnodes.end());
            (void)scene_walk_links(nodes.data(), nodes.size(), s->links);
        } else if (from) {
            std::vector<DevNode> nodes;
            if (copy_nodes_host(s, *from, nodes)) (void)scene_walk_links(nodes.data(), nodes.size(), s->links);
            else (void)hipGetLastError();
        } else {
            return s->links;  // a device-built scene whose copy is not bound yet: nothing to build from
        }
    }
    s->links_built = true;
    return s->links;
}

const std::vector<uint16_t>& device_walk_links(crt_scene* s) { return scene_links(s, nullptr); }

// The table beside the image after either staging route (the image itself stays as it is), in a
// small allocation of its own: the scene's stored bytes, padded to whole 16-byte rows for stage_lds.
// A copy that cannot get one (no table, no memory) keeps the stack walk.
static void bind_links(crt_scene* s, DeviceCopy& c) {
    c.links = nullptr;
    c.links_bytes = 0;
    std::vector<uint16_t> table = scene_links(s, &c);
    if (table.empty()) return;
    const size_t bytes = (table.size() * sizeof(uint16_t) + 15) & ~size_t(15);
    table.resize(bytes / sizeof(uint16_t), 0);
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess || hipMemcpy(d, table.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        if (d) (void)hipFree(d);
        return;
    }
    c.links = static_cast<uint16_t*>(d);
    c.links_bytes = static_cast<uint32_t>(bytes);
}

int device_nodes_host(crt_scene* s, std::vector<DevNode>& out) {
    out.clear();
    if (!u16_entries(s)) return CRT_OK;  // beyond any table: none
    if (s->image_device < 0) {  // host-built: the staging arrays
        out.assign(s->dnodes.begin(), s->dnodes.end());
        return CRT_OK;
    }
    std::lock_guard<std::mutex> lk(s->dev_mu[s->image_device]);
    const DeviceCopy& c = s->dev[s->image_device];
    if (!c.valid) return fail(CRT_E_NOT_UPLOADED, "the scene's device copy is gone");
    DeviceGuard g(s->image_device);
    if (!copy_nodes_host(s, c, out)) {
        (void)hipGetLastError();
        return fail(CRT_E_HIP, "reading the scene's nodes back failed");
    }
    return CRT_OK;
}

// Copy the scene into HBM of `device`: the staged image in one transfer. Uploads to different
// devices run concurrently (crt_drivers.hip upload_all: one thread per device); the image is
// staged once, under the scene's lock. A scene set up on a device (crt_stage_gpu.hip) is copied
// from that device's HBM instead (its copy there is already in place).
int device_upload(crt_scene* s, int device) {
    int rc = check_device(device);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(s->dev_mu[device]);
    DeviceCopy& c = s->dev[device];
    if (c.valid) return CRT_OK;
    if (s->num_dnodes >= (size_t{1} << (31 - kNodeFShift)))
        return fail(CRT_E_INVALID, "BVH too large for the device node layout");
    if (s->image_device < 0) {
        std::lock_guard<std::mutex> ls(s->mu);
        if (!s->staged) stage_image(s);
    }
    size_t off[kArrCount + 1];
    const size_t total = device_layout(s, off);
    DeviceGuard g(device);
    void* base = nullptr;
    HIP_TRY(hipMalloc(&base, total));
    hipError_t e = s->image_device >= 0
                       ? hipMemcpyPeer(base, device, s->dev[s->image_device].base, s->image_device, total)
                       : hipMemcpy(base, s->image.data(), total, hipMemcpyHostToDevice);
    // a peer copy also carries the source copy's guard words (its running Schlick count, counted
    // into by renders on that device): a new copy starts at zero, as a host-staged one does
    if (e == hipSuccess && s->image_device >= 0)
        e = hipMemset(static_cast<char*>(base) + off[kArrGuard], 0, total - off[kArrGuard]);
    if (e != hipSuccess) {
        (void)hipFree(base);
        return fail(CRT_E_HIP, std::string("scene upload: ") + hipGetErrorString(e));
    }
    device_bind_copy(s, device, base, total);
    return CRT_OK;
}

// the guard words of the scene's copy on `device` (after the renders that count into them have
// completed: synchronizes the device)
int device_guard(crt_scene* s, int device, uint64_t* schlick_undecided, bool reset) {
    int rc = check_device(device);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(s->dev_mu[device]);
    DeviceCopy& c = s->dev[device];
    if (!c.valid) return fail(CRT_E_NOT_UPLOADED, "crt_render_guard: scene not uploaded to this device");
    DeviceGuard g(device);
    HIP_TRY(hipDeviceSynchronize());
    unsigned long long v = 0;
    HIP_TRY(hipMemcpy(&v, c.guard, sizeof v, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(c.guard, 0, sizeof v));
    *schlick_undecided = v;
    return CRT_OK;
}

int device_image(crt_scene* s, int device, void* host, size_t bytes) {
    int rc = device_upload(s, device);
    if (rc) return rc;
    const DeviceCopy& c = s->dev[device];
    if (bytes != c.bytes)
        return fail(CRT_E_INVALID, "crt_scene_image: bytes must be " + std::to_string(c.bytes));
    DeviceGuard g(device);
    HIP_TRY(hipMemcpy(host, c.base, c.bytes, hipMemcpyDeviceToHost));
    return CRT_OK;
}

void device_release(crt_scene* s) {
    for (int d = 0; d < kMaxDevices; ++d) {
        DeviceCopy& c = s->dev[d];
        if (!c.valid) continue;
        DeviceGuard g(d);
        (void)hipFree(c.base);
        if (c.ref_prim) (void)hipFree(c.ref_prim);
        if (c.links) (void)hipFree(c.links);
        c = DeviceCopy{};
    }
}

static dev::CamView cam_view(const crt_camera* cam) {
    dev::CamView v{};
    for (int k = 0; k < 3; ++k) {
        v.o[k] = cam->origin[k];
        v.p00[k] = cam->pixel00[k];
        v.pdx[k] = cam->pixel_delta_x[k];
        v.pdy[k] = cam->pixel_delta_y[k];
        v.ddx[k] = cam->defocus_disk_x[k];
        v.ddy[k] = cam->defocus_disk_y[k];
        v.bg[k] = cam->background[k];
    }
    v.defocus_angle = cam->defocus_angle;
    v.t_min = cam->t_min;
    v.inv_spp = 1 / static_cast<double>(cam->samples_per_pixel);
    v.w = cam->image_w;
    v.h = cam->image_h;
    v.spp = cam->samples_per_pixel;
    v.max_depth = cam->max_depth;
    v.base_seed = cam->base_seed;
    return v;
}

static size_t align16(size_t x) { return (x + 15) & ~size_t(15); }
// scene_layout's `extra`: nothing for a trace, the camera copy for a render or a radiance query
constexpr size_t kTraceExtra = 0;
static size_t camera_extra() { return align16(sizeof(dev::CamView)); }

constexpr size_t kAccBytes = 3 * dev::kBlock * sizeof(double);  // five-wave sphere-only pixel sums
constexpr size_t kInvBytes = 3 * dev::kBlock * sizeof(double);  // flat-parallelogram instances' 1 / d
constexpr size_t kLdsSceneBudget = 40 * 1024 * dev::kBlock / 256;  // scene + stack per block (4 blocks of 256 a CU)
// sphere-only LDS scenes also stage the f64 spheres (pass 2's exact tests, shading) when the block
// still fits 40 KB: rtow 40.6 KB, 84.7 vs 85.4 ms with them in HBM / L1 (v12; round 1's layout,
// with even-aligned filter records to make room, had measured the opposite)
constexpr size_t kLdsStackBudget = 32 * 1024 * dev::kBlock / 256;
constexpr size_t kLdsBudget5 = 160 * 1024 * dev::kBlock / (64 * dev::kManyWaves * 4);  // LDS a block at five waves a SIMD
constexpr size_t kLdsPerBlock = 160 * 1024 * dev::kBlock / (256 * CRT_WAVES_PER_EU);  // LDS per block at the VGPR occupancy

// The class of a launch and what its layout step decided (scene_layout); the launch
// steps (dispatch_*) and crt_launch_plan read it.
enum QueryClass { kQueryLdsScene, kQueryLdsStack, kQueryHbmStack };
struct Layout {
    QueryClass cls = kQueryLdsScene;
    bool w5 = false;         // render: five waves per SIMD
    size_t lds = 0;          // bytes laid out so far (the launchers add theirs: lds_tail)
    size_t stack_bytes = 0;  // levels 0..depth
    size_t level = 0;        // one stack level
    size_t all_nodes = 0;    // the f32 node array
    size_t budget = 0;       // the budget the class was admitted under
};

// the instance's primitive mode: sphere-only, general, or (render, LDS scenes) flat parallelograms
static int render_prim_mode(const dev::Work& W, QueryClass cls) {
    return W.sphere_only ? 0 : (cls == kQueryLdsScene && W.quads_flat) ? 2 : 1;
}
static int query_prim_mode(const dev::Work& W) { return W.sphere_only ? 0 : 1; }

// What a launcher keeps behind the layout's `lds` bytes, for its instance: which regions (Tail),
// and where they go (lds_tail, which returns the dynamic LDS the launch requests).
struct Tail {
    bool cam;          // the camera copy after the rest (render_kernel, radiance_kernel: CL)
    bool acc;          // then the pixel sums (render_kernel: kAccLds)
    bool inv;          // or the rays' f64 1 / d (kInvLds)
    bool sibling_pad;  // a treelet alone (HBM stack) with nothing behind it
};
static Tail render_tail(bool gstack, bool lscene, int pm, bool w5) {
    return {true, w5 && pm == 0, (lscene && pm == 2 && w5) || (!lscene && !gstack), false};
}
static Tail trace_tail(bool gstack, bool lscene) { return {false, false, !lscene && !gstack, gstack}; }
static Tail radiance_tail(bool gstack, bool lscene) { return {true, false, !lscene && !gstack, false}; }
static size_t lds_tail(dev::Work& W, size_t lds, const Tail& t) {
    // a treelet alone that holds the whole node array ends with the sentinel, whose sibling slot
    // fetch_two reads too (and never tests): keep it inside the request. A cut treelet is whole
    // pairs, and every other instance has a region behind the nodes.
    if (t.sibling_pad && lds % (2 * sizeof(DevNodeF))) lds += sizeof(DevNodeF);
    if (t.cam) {
        W.lds_cam = static_cast<uint32_t>(align16(lds));
        lds = W.lds_cam + camera_extra();
    }
    if (t.acc) {
        W.lds_acc = static_cast<uint32_t>(align16(lds));
        lds = W.lds_acc + kAccBytes;
    }
    if (t.inv) {
        W.lds_inv64 = static_cast<uint32_t>(align16(lds));
        lds = W.lds_inv64 + kInvBytes;
    }
    return lds;
}
// an HBM stack's levels: 0..depth, two guard levels and the level below them
static size_t gstack_levels(const crt_scene* s) { return static_cast<size_t>(s->depth) + 4; }

// Which instance family a scene gets, from its copy's f32 flags: `f32_ok` = the walk decides in f32,
// `filters` = the two-pass leaf filters' interval rule holds (t_min >= 0)
static void class_flags(const crt_scene* s, const CopyFlags& c, bool f32_ok, bool filters, dev::Work& W) {
    W.f32_ok = f32_ok ? 1u : 0u;
    W.sphere_only = (s->num_quads == 0 && s->num_spheres != 0) ? 1u : 0u;
    W.spheres_f32 = (W.sphere_only && c.spheres_f32_ok && filters) ? 1u : 0u;
    W.quads_f32 = (s->num_spheres == 0 && s->num_quads != 0 && c.quads_f32_ok && filters) ? 1u : 0u;
    // the flat-box filter is the walk's f32 node test: it needs the walk's f32 range (f32_ok)
    W.quads_flat = (W.quads_f32 && c.quads_flat_ok && W.f32_ok) ? 1u : 0u;
    W.exact_slab = (s->exact_slab || std::getenv("CRT_EXACT_SLAB") != nullptr) ? 1u : 0u;
    W.pair_walk = (CRT_PAIR_WALK && !W.exact_slab && std::getenv("CRT_NO_PAIR_WALK") == nullptr) ? 1u : 0u;
}
// every ref fits a u16 stack entry
static bool u16_entries(const crt_scene* s) { return (s->num_dnodes << kNodeFShift) <= 65536; }

// Partial-sum budget per launch (bytes): the owned frame is rendered in bands whose partial sums
// fit it (CRT_PARTIAL_MB overrides; tests force many small bands). 4 GiB holds a whole config-2
// frame (2.9 GB) in one band; config 5 on one GPU (37.6 GB of partial sums) takes 10.
static size_t partial_budget() {
    if (const char* e = std::getenv("CRT_PARTIAL_MB"))
        return static_cast<size_t>(std::max(1, std::atoi(e))) << 20;
    return size_t{4} << 30;
}

// Samples per chunk: a function of spp only (launch_render; crt_sample_chunk_len)
#ifndef CRT_CHUNK_MIN
#define CRT_CHUNK_MIN 4
#endif
uint32_t sample_chunk_len(uint32_t spp) {
    return std::max<uint32_t>(CRT_CHUNK_MIN, (spp + 191) / 192);
}

// Scratch of pass renders (partial sums, queue, active list, the update's counter) comes from a
// memory pool of the library's own, one per device, that never gives memory back: the process's
// default pool is left alone. The default pool releases unused memory at every synchronization
// (release threshold 0), and a render in passes synchronizes between passes, so every pass drew
// its scratch from memory released and mapped again. In a C++ process on the ROCm 7.0 runtime (not
// under PyTorch's bundled runtime) whole tiles of a later pass then came out as zeros:
// crt_render_progressive in three passes of four samples lost one pass in most tiles from the
// second render of a process on (tests/cpp/passes_e2e.cpp), with every kernel serialized too; why
// was not found. With scratch that stays mapped no pass is lost, whatever the host does with the
// default pool. The pool holds the largest scratch any pass needed (at most the partial-sum
// budget) until the process ends. One-shot renders allocate as before. A pool that cannot be
// created is an error: pass renders do not fall back to the default pool.
static int pass_pool(int device, hipMemPool_t* out) {
    static std::mutex mu;
    static hipMemPool_t pools[kMaxDevices] = {};
    std::lock_guard<std::mutex> lk(mu);
    if (device < 0 || device >= kMaxDevices) return fail(CRT_E_NODEVICE, "pass scratch pool: device out of range");
    if (!pools[device]) {
        hipMemPoolProps props{};
        props.allocType = hipMemAllocationTypePinned;
        props.handleTypes = hipMemHandleTypeNone;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = device;
        hipMemPool_t pool = nullptr;
        uint64_t keep = UINT64_MAX;
        hipError_t e = hipMemPoolCreate(&pool, &props);
        if (e == hipSuccess) {
            e = hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
            if (e != hipSuccess) (void)hipMemPoolDestroy(pool);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(CRT_E_HIP, std::string("pass scratch pool on device ") + std::to_string(device) + ": " +
                                       hipGetErrorString(e));
        }
        pools[device] = pool;
    }
    *out = pools[device];
    return CRT_OK;
}

// The grid of a persistent kernel: every resident block (more would only wait); CRT_GRID_BLOCKS:
// fewer (schedule tests: a smaller grid, same results)
static int resident_blocks(int device, const void* kfn, size_t lds, uint64_t& resident) {
    int cus = 0, per_cu = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, dev::kBlock, lds));
    resident = static_cast<uint64_t>(std::max(1, cus)) * std::max(1, per_cu);
    if (const char* e = std::getenv("CRT_GRID_BLOCKS"))
        resident = std::max<uint64_t>(1, std::min<uint64_t>(resident, static_cast<uint64_t>(std::max(1, std::atoi(e)))));
    return CRT_OK;
}

// The grid and scratch of a query launch (launch_trace, launch_radiance): the resident blocks, or as
// many as the 64-ray batches fill; stream-ordered from the pass pool, an HBM stack of levels
// 0..depth, two guard levels and the level below them (lane_stack), and the zeroed batch counter.
// The caller frees both after its launch.
template <typename SE>
static int persistent_grid(const crt_scene* s, int device, const void* kfn, size_t lds, uint32_t batches, bool hbm_stack,
                           hipMemPool_t pool, hipStream_t stream, uint32_t& blocks, SE*& gstack, uint32_t*& queue) {
    uint64_t resident = 0;
    const int rc = resident_blocks(device, kfn, lds, resident);
    if (rc) return rc;
    constexpr uint32_t kWavesPerBlock = dev::kBlock / 64;
    blocks = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(resident, (batches + kWavesPerBlock - 1) / kWavesPerBlock)));
    if (hbm_stack)
        HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&gstack),
                                       gstack_levels(s) * blocks * dev::kBlock * sizeof(SE), pool, stream));
    HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&queue), 256, pool, stream));
    HIP_TRY(hipMemsetAsync(queue, 0, sizeof(uint32_t), stream));
    return CRT_OK;
}

// The plain routes (one thread per ray, trace()'s loop): launches of at most 2^20 rays that share
// one set of stacks, [level][thread] (stream order keeps them apart). launch(blocks, first, stacks):
// the same grid for every launch (the stacks' stride is its thread count); the kernel bounds itself
// by the rays left.
template <typename F>
static int plain_launches(const crt_scene* s, uint32_t n, hipMemPool_t pool, hipStream_t st, const char* what, F launch) {
    constexpr uint32_t kPlainRays = 1u << 20;
    const uint32_t max_blocks = (std::min<uint32_t>(n, kPlainRays) + dev::kBlock - 1) / dev::kBlock;
    uint32_t* d_stack = nullptr;
    HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&d_stack),
                                   static_cast<size_t>(s->depth + 1) * max_blocks * dev::kBlock * 4, pool, st));
    hipError_t e = hipSuccess;
    for (uint64_t first = 0; first < n && e == hipSuccess; first += kPlainRays) {
        launch(max_blocks, static_cast<uint32_t>(first), d_stack);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(d_stack, st);
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    return CRT_OK;
}

// The class x primitive-mode switch of the query launchers: go(GSTACK, LSCENE, PM), as constants
template <typename F>
static int by_class(QueryClass cls, bool sphere_only, F go) {
    auto mode = [&](auto gstack, auto lscene) {
        return sphere_only ? go(gstack, lscene, std::integral_constant<int, 0>{}) : go(gstack, lscene, std::integral_constant<int, 1>{});
    };
    switch (cls) {
    case kQueryLdsScene: return mode(std::false_type{}, std::true_type{});
    case kQueryLdsStack: return mode(std::false_type{}, std::false_type{});
    default: return mode(std::true_type{}, std::false_type{});
    }
}

template <typename SE, bool GSTACK, bool LSCENE, int PM, bool W5 = false, bool LINK = false>
static int launch_render(const crt_scene* s, int device, const crt_camera* cam, const dev::Work& w0,
                         size_t lds, double* d_rgb, hipStream_t stream, crt_render_stats* count_stats,
                         const RenderPass* pass) {
    const DeviceCopy& c = s->dev[device];
    dev::Work W = w0;
    lds = lds_tail(W, lds, render_tail(GSTACK, LSCENE, PM, W5));
    constexpr int kThreads = dev::kBlock;
    // a masked pass (adaptive sampling) launches the MASK instance over the active tiles' list
    const bool masked = pass && pass->blocks;
    const void* kfn = masked ? reinterpret_cast<const void*>(dev::render_kernel<SE, GSTACK, LSCENE, false, PM, W5, true, LINK>)
                             : reinterpret_cast<const void*>(dev::render_kernel<SE, GSTACK, LSCENE, false, PM, W5, false, LINK>);
    const uint64_t pixels = static_cast<uint64_t>(W.owned_rows) * cam->image_w;
    // Sample chunks: a function of spp ONLY, so every pixel's sum is grouped identically whatever
    // the tiling / number of GPUs / lane schedule / band split (bit-identical frames for 1..N
    // devices): 4 samples, or spp / 192 above 768 spp. A unit is the grain the grid drains on:
    // per-rank share at 8 GPUs 12.2 ms with 4-sample chunks vs 13.0 with 8 (one GPU 87.4 vs 87.5;
    // the partial sums double to 2.9 GB per config-2 frame). The persistent grid's waves take
    // (tile, chunk) items from a queue in tile-major order (render_kernel).
    const uint32_t spp = cam->samples_per_pixel;
    W.chunk_len = sample_chunk_len(spp);
    W.chunks = (spp + W.chunk_len - 1) / W.chunk_len;
    // A pass of a progressive render launches its own chunks only (chunk s0 / chunk_len onwards,
    // numbered from 0 in the launch and in `partial`), so its bands are sized by the pass; the
    // chunks that hold chunk_len samples (all but a job's ragged last one) feed the noise state.
    uint32_t full_chunks = 0;
    double inv_done = 0;
    hipMemPool_t pool = nullptr;  // pass renders: the library's own pool (pass_pool)
    if (pass) {
        const int rc = pass_pool(device, &pool);
        if (rc) return rc;
    }
    auto scratch = [&](void** p, size_t bytes) {
        return pool ? hipMallocFromPoolAsync(p, bytes, pool, stream) : hipMallocAsync(p, bytes, stream);
    };
    if (pass) {
        const uint32_t end = pass->first + pass->count;
        W.s0 = pass->first;
        W.chunks = (end + W.chunk_len - 1) / W.chunk_len - pass->first / W.chunk_len;
        full_chunks = end / W.chunk_len - pass->first / W.chunk_len;
        inv_done = 1 / static_cast<double>(end);
    }
    // Bands: rectangles of bx x by tiles over the owned rows x width, each one launch (render +
    // resolve). bx, by <= 65535 (a unit packs its tile as tx | ty << 16), and a band's partial
    // sums (64 pixels x 3 x chunks doubles per tile) fit the budget. A pixel's chunks are summed
    // in the same order in any band, so the split does not change frames.
    constexpr uint64_t kMaxTiles = 65535;
    const uint64_t tiles_x_all = (static_cast<uint64_t>(cam->image_w) + dev::kTileW - 1) / dev::kTileW;
    const uint64_t tiles_y_all = (static_cast<uint64_t>(W.owned_rows) + dev::kTileH - 1) / dev::kTileH;
    const uint64_t tile_bytes = 64ull * 3 * sizeof(double) * W.chunks;
    const uint64_t cap = std::max<uint64_t>(1, partial_budget() / tile_bytes);
    const uint32_t bx = static_cast<uint32_t>(std::min({tiles_x_all, kMaxTiles, cap}));
    const uint32_t by = static_cast<uint32_t>(std::min({tiles_y_all, kMaxTiles, std::max<uint64_t>(1, cap / bx)}));
    // the grid: every resident block (more would only wait), fewer when a band's items are fewer
    constexpr uint32_t kWavesPerBlock = kThreads / 64;
    uint64_t resident = 0;
    if (const int rc = resident_blocks(device, kfn, lds, resident)) return rc;
    auto knob = [](const char* name, uint32_t dflt) {
        const char* e = std::getenv(name);
        return e ? static_cast<uint32_t>(std::max(0, std::min(4096, std::atoi(e)))) : dflt;
    };

    double* partial = nullptr;
    SE* gstack = nullptr;
    dev::Counters* ctr = nullptr;
    const bool count = count_stats != nullptr;
    const uint64_t band_px = std::min<uint64_t>(static_cast<uint64_t>(bx) * dev::kTileW, cam->image_w) *
                             std::min<uint64_t>(static_cast<uint64_t>(by) * dev::kTileH, W.owned_rows);
    if (!count)
        HIP_TRY(scratch(reinterpret_cast<void**>(&partial), band_px * 3 * W.chunks * sizeof(double)));
    if (GSTACK) {
        size_t bytes = gstack_levels(s) * resident * dev::kBlock * sizeof(SE);  // + 3 levels below
        HIP_TRY(scratch(reinterpret_cast<void**>(&gstack), bytes));
    }
    if (count) {
        HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&ctr), sizeof(dev::Counters), stream));
        HIP_TRY(hipMemsetAsync(ctr, 0, sizeof(dev::Counters), stream));
    }
    uint32_t* queue = nullptr;
    HIP_TRY(scratch(reinterpret_cast<void**>(&queue), 256));
    W.queue = queue;
    uint32_t* active = nullptr;  // masked pass: a band's active tiles (active_list_kernel)
    if (masked)
        HIP_TRY(scratch(reinterpret_cast<void**>(&active), (static_cast<size_t>(bx) * by + 1) * sizeof(uint32_t)));
    dev::SceneView S = view_of(c);
    dev::CamView C = cam_view(cam);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (count) {
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        HIP_TRY(hipEventRecord(e0, stream));
    }
    for (uint64_t ty0 = 0; ty0 < tiles_y_all; ty0 += by) {
        for (uint64_t tx0 = 0; tx0 < tiles_x_all; tx0 += bx) {
            W.col0 = static_cast<uint32_t>(tx0 * dev::kTileW);
            W.k0 = static_cast<uint32_t>(ty0 * dev::kTileH);
            W.bw = static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(bx) * dev::kTileW, cam->image_w - W.col0));
            W.bh = static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(by) * dev::kTileH, W.owned_rows - W.k0));
            W.tiles_x = (W.bw + dev::kTileW - 1) / dev::kTileW;
            W.tiles_y = (W.bh + dev::kTileH - 1) / dev::kTileH;
            W.tiles = W.tiles_x * W.tiles_y;
            // the tiles the grid and the items are sized for: the band's, or what the caller of a
            // masked pass expects to be active (the kernel bounds itself by the true number)
            const uint64_t q_tiles = masked && pass->hint ? std::min<uint64_t>(pass->hint, W.tiles) : W.tiles;
            const uint64_t blocks = std::max<uint64_t>(
                1, std::min<uint64_t>(resident, (q_tiles * W.chunks + kWavesPerBlock - 1) / kWavesPerBlock));
            // Items: bulk items of K chunks for the first part of each tile's chunks, then the
            // rest in one-chunk items at the end of the queue (CRT_TAIL_CHUNKS), so the grid
            // drains on small items; a wave's lanes cross from item to item without waiting
            // either way. Large items keep a wave's lanes on one tile (coherent rays: config 2 on
            // one GPU takes 72.5 ms with K = 7, 77.1 with K = 1), small ones balance the drain
            // against a ~10x spread of tile costs. With p = (tile, chunk) pairs per wave: K =
            // min(7, p / 15) for p >= 60, else 3, and the tail takes max(1/9, 30 / p) of the
            // chunks (all of them for p <= 30). Config 2, the slowest rank's share
            // (tools/item_sweep.py, tools/grid_sweep.py, profiles/r03_schedule): N = 2 (p = 183)
            // 36.9 -> 36.7 ms, N = 4 (p = 92) 19.7 -> 19.0, N = 8 (p = 46, K = 3 with an 81-chunk
            // tail) 10.34-10.49 -> 10.17-10.31 against the earlier K = p / 30 with a 1/9 tail;
            // N = 1 (7, 13 of 125 chunks) unchanged. (CRT_ITEM_CHUNKS, CRT_TAIL_CHUNKS override.)
            const uint64_t per_lane = q_tiles * W.chunks / (blocks * kWavesPerBlock);
            const uint32_t k_auto = per_lane >= 60 ? static_cast<uint32_t>(std::min<uint64_t>(7, per_lane / 15)) : 3u;
            W.item_chunks = std::max<uint32_t>(1, knob("CRT_ITEM_CHUNKS", k_auto));
            const uint32_t tail_auto = static_cast<uint32_t>(std::max<uint64_t>(
                W.chunks / 9, std::min<uint64_t>(W.chunks, static_cast<uint64_t>(W.chunks) * 30 / std::max<uint64_t>(1, per_lane))));
            const uint32_t tail_want = std::min(W.chunks, knob("CRT_TAIL_CHUNKS", W.item_chunks > 1 ? tail_auto : 0));
            W.groups = (W.chunks - tail_want) / W.item_chunks;
            W.bulk_chunks = W.groups * W.item_chunks;
            W.tail_chunks = W.chunks - W.bulk_chunks;
            const uint64_t bulk_items = static_cast<uint64_t>(W.tiles) * W.groups;
            const uint64_t items = bulk_items + static_cast<uint64_t>(W.tiles) * W.tail_chunks;
            if (items >= 0xffffffffull) return fail(CRT_E_INVALID, "band too large for one launch");
            W.n_items = static_cast<uint32_t>(items);
            W.bulk_items = static_cast<uint32_t>(bulk_items);
            // HBM-resident scenes: one queue per XCD (blocks b and b + 8 share one), so an XCD's L2
            // serves the rays of one region of the band (config 4: 163.5 vs 166.2 ms); LDS scenes
            // keep one queue (config 2: 88.5 vs 89.0 ms with eight). CRT_XCD_QUEUES=0/1 forces.
            W.segments = knob("CRT_XCD_QUEUES", LSCENE ? 0 : 1) ? 8u : 1u;
            // a masked pass has no memset: active_list_kernel zeroes W.queue[0..7] (W is set up to here)
            if (!masked) HIP_TRY(hipMemsetAsync(queue, 0, 8 * sizeof(uint32_t), stream));
#if CRT_WATCHDOG
            {
                void* wd = nullptr;
                HIP_TRY(hipGetSymbolAddress(&wd, HIP_SYMBOL(dev::crt_wd_deadline)));
                HIP_TRY(hipMemsetAsync(wd, 0, sizeof(unsigned long long), stream));
            }
#endif
            if (count) {
                hipLaunchKernelGGL((dev::render_kernel<SE, GSTACK, LSCENE, true, PM, W5, false, LINK>), dim3(static_cast<uint32_t>(blocks)),
                                   dim3(dev::kBlock), lds, stream, S, C, W, partial, gstack, ctr, nullptr);
                HIP_TRY(hipGetLastError());
            } else if (masked) {
                const uint32_t ftx = static_cast<uint32_t>(tiles_x_all);
                hipLaunchKernelGGL(dev::active_list_kernel, dim3(1), dim3(dev::kListThreads), 0, stream, pass->blocks, W, ftx,
                                   pass->first, active);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL((dev::render_kernel<SE, GSTACK, LSCENE, false, PM, W5, true, LINK>), dim3(static_cast<uint32_t>(blocks)),
                                   dim3(dev::kBlock), lds, stream, S, C, W, partial, gstack, ctr, active);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(dev::accumulate_masked_kernel, dim3((W.tiles + 3) / 4), dim3(256), 0, stream, partial,
                                   pass->sum, pass->noise, d_rgb, pass->blocks, W, cam->image_w, ftx, full_chunks,
                                   pass->first + pass->count, inv_done);
                HIP_TRY(hipGetLastError());
            } else {
                hipLaunchKernelGGL((dev::render_kernel<SE, GSTACK, LSCENE, false, PM, W5, false, LINK>), dim3(static_cast<uint32_t>(blocks)),
                                   dim3(dev::kBlock), lds, stream, S, C, W, partial, gstack, ctr, nullptr);
                HIP_TRY(hipGetLastError());
                const uint64_t rb = (static_cast<uint64_t>(W.bw) * W.bh + 255) / 256;
                if (pass)
                    hipLaunchKernelGGL(dev::accumulate_kernel, dim3(static_cast<uint32_t>(rb)), dim3(256), 0, stream, partial,
                                       pass->sum, pass->noise, d_rgb, W, cam->image_w, full_chunks, inv_done);
                else
                    hipLaunchKernelGGL(dev::resolve_kernel, dim3(static_cast<uint32_t>(rb)), dim3(256), 0, stream, partial,
                                       d_rgb, W, cam->image_w, cam->image_h, C.inv_spp);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    c.last_walk = LINK ? CRT_WALK_LINKS : CRT_WALK_STACK;  // every band's launches were accepted
    if (count) HIP_TRY(hipEventRecord(e1, stream));
    if (partial) HIP_TRY(hipFreeAsync(partial, stream));
    HIP_TRY(hipFreeAsync(queue, stream));
    if (active) HIP_TRY(hipFreeAsync(active, stream));
    if (gstack) HIP_TRY(hipFreeAsync(gstack, stream));
    if (count) {
        dev::Counters h{};
        HIP_TRY(hipMemcpyAsync(&h, ctr, sizeof h, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipFreeAsync(ctr, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        count_stats->samples = pixels * cam->samples_per_pixel;
        count_stats->rays = h.rays;
        count_stats->nodes_visited = h.nodes;
        count_stats->sphere_tests = h.sphere_tests;
        count_stats->parallelogram_tests = h.quad_tests;
        count_stats->kernel_ms = ms;
        count_stats->ticks_walk = h.cyc_walk;
        count_stats->ticks_leaf = h.cyc_leaf;
        count_stats->ticks_shade = h.cyc_shade;
        count_stats->ticks_total = h.cyc_total;
        count_stats->wave_iters_walk = h.it_walk;
        count_stats->wave_iters_leaf = h.it_leaf;
        count_stats->wave_iters_shade = h.it_shade;
        count_stats->ticks_tail = h.cyc_tail;
        count_stats->slow_node_tests = h.slow_nodes;
        count_stats->wave_iters_slow = h.it_slow;
        count_stats->candidate_tests = h.cand;
        count_stats->wave_iters_candidates = h.it_cand;
        if (std::getenv("CRT_DEBUG_COUNTERS"))
            std::fprintf(stderr, "crt counters: rays %llu nodes %llu sphere_tests %llu quad_tests %llu it_walk %llu "
                         "it_leaf %llu it_shade %llu rounds %llu walkers/round %.2f leaves/round %.2f done/round %.2f "
"shade_rounds %llu; wave time: walk %.3f leaf %.3f shade %.3f draw %.3f init %.3f\n", h.rays, h.nodes, h.sphere_tests, h.quad_tests, h.it_walk,
                         h.it_leaf, h.it_shade, h.rounds, double(h.round_walkers) / double(h.rounds ? h.rounds : 1),
                         double(h.round_leaves) / double(h.rounds ? h.rounds : 1),
                         double(h.round_done) / double(h.rounds ? h.rounds : 1), h.shade_rounds,
                         double(h.cyc_walk) / double(h.cyc_total), double(h.cyc_leaf) / double(h.cyc_total),
                         double(h.cyc_shade) / double(h.cyc_total), double(h.cyc_draw) / double(h.cyc_total),
                         double(h.cyc_init) / double(h.cyc_total));
    }
    return CRT_OK;
}

// Kernel variant per scene: u16 stack entries below 65536 nodes; the scene itself in LDS when it
// and the stack fit the LDS budget, else the stack alone in LDS, else everything in HBM.
// scene_layout fills W's LDS layout for the class it returns (W's class flags and tmin32 are the
// caller's: class_flags), with the bytes laid out so far; the launchers add what their instance
// keeps behind that (lds_tail). `extra`: those bytes besides the rays' 1 / d, which the treelet leaves
// free: the camera copy of a render or a radiance query (camera_extra), nothing for a trace. The
// five-wave and flat-parallelogram-only instances are the render kernel's alone (five_wave_ok):
// queries run four waves per SIMD throughout, and a scene of axis-aligned parallelograms runs its
// flat-box filter in their general instance. dispatch_render, dispatch_trace and dispatch_radiance
// launch the class's instance.
template <typename SE>
static Layout scene_layout(const crt_scene* s, dev::Work& W, size_t extra, bool five_wave_ok) {
    Layout L;
    // depth + 1 levels: walk_step stores the far child at level sp unconditionally
    const size_t stack_bytes = align16(static_cast<size_t>(s->depth + 1) * dev::kBlock * sizeof(SE));
    W.bytes_nodes = static_cast<uint32_t>(align16(s->num_dnodes * sizeof(DevNodeF)));
    // sphere-only scenes in f32 range stage the filter's pair records instead of refs + spheres
    W.bytes_refs = W.spheres_f32 ? 0u : static_cast<uint32_t>(align16(s->num_prims * 4));
    W.bytes_spheres = static_cast<uint32_t>(align16(s->num_spheres * (W.spheres_f32 ? sizeof(DevSpherePair)
                                                                                         : sizeof(DevSphere))));
    W.bytes_quads = static_cast<uint32_t>(align16(s->num_quads * sizeof(DevQuad)));
    W.bytes_quadf = W.quads_f32 ? static_cast<uint32_t>(s->num_quads * (W.quads_flat ? sizeof(DevQuadBox) : sizeof(DevQuadF)))
                                : 0u;
    const size_t scene_bytes = static_cast<size_t>(W.bytes_nodes) + W.bytes_refs + W.bytes_spheres + W.bytes_quads +
                               W.bytes_quadf;
    const uint32_t level = static_cast<uint32_t>(dev::kBlock * sizeof(SE));  // one stack level
    // the sentinel is the last node; refs are byte offsets into the f32 node array
    W.sentinel = static_cast<uint32_t>(s->num_dnodes - 1) << kNodeFShift;
    L.stack_bytes = stack_bytes;
    L.level = level;
    L.all_nodes = s->num_dnodes * sizeof(DevNodeF);
    const bool force_global = std::getenv("CRT_NO_LDS_SCENE") != nullptr;
    // LDS stacks: [data][second guard: sentinel][guard level: sentinel][levels 0..depth]. A lane
    // that reaches the sentinel with no leaf recorded pops the second guard (round 6: it holds the
    // sentinel too, so the walks need no sentinel compare), and the speculative read reaches one
    // level below it: the guard starts at least three levels into the allocation and the second
    // guard lies past the data, so every level the pointer reaches has a non-negative LDS address. (With one
    // level, a 640-thread block on a small scene put that pointer at a negative address; the
    // level count derived from it then wrapped, and the flat-parallelogram instance walked a
    // garbage stack forever: the round-4 hang, found with -DCRT_WATCHDOG=1. Power-of-two blocks
    // had wrapped back onto the right level by the modular arithmetic alone.)
    auto stack_at = [&](size_t data_bytes) { return static_cast<uint32_t>(std::max<size_t>(data_bytes, 2 * level) + 2 * level); };
    // every admission counts what the launcher keeps behind the layout too (lds_tail): a
    // request above the class's budget costs a resident block
    if (!force_global && stack_at(scene_bytes) + stack_bytes + extra <= kLdsSceneBudget) {
        W.lds_nodes = 0;
        W.lds_refs = W.lds_nodes + W.bytes_nodes;
        W.lds_spheres = W.lds_refs + W.bytes_refs;
        W.lds_quads = W.lds_spheres + W.bytes_spheres;
        W.lds_quadf = W.lds_quads + W.bytes_quads;
        W.lds_sph64 = W.lds_quadf + W.bytes_quadf;
        // Sphere-only scenes and scenes of axis-aligned parallelograms run five waves per SIMD when
        // five blocks fit a CU's LDS (32 KB each), staging the f64 spheres only if they fit that
        // too (config 2: 73.7 ms at five waves without them vs 75.8 at four with them; config 3:
        // 89.8 vs 92.6); the others four, with up to 40 KB (the general instance at five: config
        // 3 116.5 vs 100.6 ms).
        const size_t budget5 = kLdsBudget5;
        const bool w5 = five_wave_ok && (64 * dev::kManyWaves * 4) % dev::kBlock == 0 && (W.sphere_only || W.quads_flat) && std::getenv("CRT_FOUR_WAVES") == nullptr &&
                        stack_at(scene_bytes) + stack_bytes + extra + (W.sphere_only ? kAccBytes : 0) +
                            (W.quads_flat ? kInvBytes : 0) <= budget5;
        const size_t budget = w5 ? budget5 : kLdsSceneBudget;
        const uint32_t sph64 = static_cast<uint32_t>(s->num_spheres * sizeof(DevSphere));
        if (W.spheres_f32 && stack_at(scene_bytes + sph64) + stack_bytes + extra + (w5 ? kAccBytes : 0) <= budget)
            W.bytes_sph64 = sph64;
        W.lds_stack = stack_at(scene_bytes + W.bytes_sph64);
        L.cls = kQueryLdsScene;
        L.w5 = w5;
        L.lds = W.lds_stack + stack_bytes;
        L.budget = budget;
        return L;
    }
    // HBM scene: the top of the (breadth-first) node array goes to LDS as far as it fits beside
    // the stack without costing resident blocks (CRT_WAVES_PER_EU blocks of 4 waves, the VGPR
    // limit); W.ntop counts bytes of f32 nodes
    const size_t per_block = kLdsPerBlock;
    L.budget = per_block;
    const bool no_top = std::getenv("CRT_NO_LDS_TOP") != nullptr;
    const size_t all_nodes = L.all_nodes;
    auto top_bytes = [&](size_t room) {
        // whole 64-byte sibling pairs (walk_pairs reads a pair from LDS or from HBM, not both)
        return no_top ? 0u : static_cast<uint32_t>(std::min(all_nodes, room / (2 * sizeof(DevNodeF)) * (2 * sizeof(DevNodeF))));
    };
    // An LDS stack needs the levels stack_at keeps below it (four without a treelet), the rays' 1 / d
    // and `extra` beside it: a stack within kLdsStackBudget that does not fit per_block with
    // them (u16 entries: 64 levels; u32: 30 and more) goes to HBM like a larger one.
    if (stack_bytes <= kLdsStackBudget && stack_at(0) + stack_bytes + kInvBytes + extra <= per_block &&
        std::getenv("CRT_FORCE_GSTACK") == nullptr) {
        // beside the treelet: the stack, the two guard levels stack_at puts above the data, the rays'
        // 1 / d and `extra` (the admission leaves at least two levels of room)
        const size_t taken = stack_bytes + 2 * level + kInvBytes + extra;
        W.ntop = top_bytes(per_block - taken);
        W.lds_nodes = 0;
        W.lds_stack = stack_at(align16(W.ntop));
        L.cls = kQueryLdsStack;
        L.lds = W.lds_stack + stack_bytes;
        return L;
    }
    W.ntop = top_bytes(per_block - extra);
    W.lds_nodes = 0;
    L.cls = kQueryHbmStack;
    L.lds = W.ntop;
    return L;
}

template <typename SE>
static int dispatch_render(const crt_scene* s, int device, const crt_camera* cam, dev::Work W,
                           double* d_rgb, hipStream_t st, crt_render_stats* count_stats, const RenderPass* pass) {
    const Layout L = scene_layout<SE>(s, W, camera_extra(), true);
    const int pm = render_prim_mode(W, L.cls);
    // The stackless walk (walk(), LINK): the timed five-wave sphere-only and flat-parallelogram
    // instances, when the copy has a validated miss-link table (u16 entries) that fits the bytes the
    // plan keeps for the guard levels and the stack, where it is staged; the plan itself is unchanged.
    // Their instrumented pass (COUNT) walks the same way, so its counters are the link walk's (the
    // stack walk's, node for node). Everything else walks with the stack. CRT_NO_LINK_WALK=1
    // (read here, at the call) keeps the stack walk: the A/B switch of tests/test_gpu_link_walk.py.
    if constexpr (std::is_same_v<SE, uint16_t>) {
        const DeviceCopy& c = s->dev[device];
        const size_t table = s->num_dnodes * 16;
        if (L.cls == kQueryLdsScene && L.w5 && (pm == 0 || pm == 2) && c.links &&
            c.links_bytes >= align16(table) && table <= 2 * L.level + L.stack_bytes &&
            std::getenv("CRT_NO_LINK_WALK") == nullptr) {
            W.lds_links = static_cast<uint32_t>(W.lds_stack - 2 * L.level);
            W.bytes_links = static_cast<uint32_t>(align16(table));
            return pm == 0 ? launch_render<SE, false, true, 0, true, true>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass)
                           : launch_render<SE, false, true, 2, true, true>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass);
        }
    }
    switch (L.cls) {
    case kQueryLdsScene:
        if (pm == 0)
            return L.w5 ? launch_render<SE, false, true, 0, true>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass)
                        : launch_render<SE, false, true, 0, false>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass);
        if (pm == 2)
            return L.w5 ? launch_render<SE, false, true, 2, true>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass)
                        : launch_render<SE, false, true, 2, false>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass);
        return launch_render<SE, false, true, 1>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass);
    case kQueryLdsStack:
        if (pm == 0) return launch_render<SE, false, false, 0>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass);
        return launch_render<SE, false, false, 1>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass);
    default:
        if (pm == 0) return launch_render<SE, true, false, 0>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass);
        return launch_render<SE, true, false, 1>(s, device, cam, W, L.lds, d_rgb, st, count_stats, pass);
    }
}

// The tiling checked (null: the whole frame as one tile) and W cleared but for its tiling part:
// which rows the tile owns, how the buffers hold them (packed), the row block's shift.
static int tiling_work(const crt_camera* cam, const crt_tiling* t, dev::Work& W) {
    crt_tiling tl{1, 1, 0, 0};
    if (t) tl = *t;
    if (tl.flags & ~CRT_TILING_PACKED) return fail(CRT_E_INVALID, "unknown tiling flags");
    if (tl.row_block == 0 || tl.tile_count == 0 || tl.tile_index >= tl.tile_count)
        return fail(CRT_E_INVALID, "bad tiling");
    W = dev::Work{};
    W.row_block = tl.row_block;
    W.tile_count = tl.tile_count;
    W.tile_index = tl.tile_index;
    W.owned_rows = count_owned(cam->image_h, tl.row_block, tl.tile_count, tl.tile_index);
    W.packed = (tl.flags & CRT_TILING_PACKED) ? 1u : 0u;
    W.rb_shift = 32;
    for (uint32_t sh = 0; sh < 31; ++sh)
        if ((1u << sh) == W.row_block) W.rb_shift = sh;
    return CRT_OK;
}

int device_render(const crt_scene* s, int device, const crt_camera* cam, const crt_tiling* t,
                  double* d_rgb, void* stream, crt_render_stats* count_stats, const RenderPass* pass) {
    int rc = check_device(device);
    if (rc) return rc;
    if (!s->dev[device].valid)
        return fail(CRT_E_NOT_UPLOADED, "scene not uploaded to device " + std::to_string(device));
    if (cam->image_w == 0 || cam->image_h == 0) return fail(CRT_E_INVALID, "empty image");
    if (static_cast<uint64_t>(cam->image_w) * cam->image_h >= 0xffffffffull)
        return fail(CRT_E_INVALID, "image has more than 2^32-1 pixels");
    dev::Work W;
    rc = tiling_work(cam, t, W);
    if (rc) return rc;
    DeviceGuard g(device);
    if (W.owned_rows == 0 || cam->samples_per_pixel == 0) {
        if (count_stats) *count_stats = crt_render_stats{};
        if (cam->samples_per_pixel == 0 && d_rgb && W.owned_rows) {
            // 0 spp: the reference multiplies a zero sum by 1/0 -> NaN (0 * inf)
            std::vector<double> nanrow(static_cast<size_t>(cam->image_w) * 3,
                                       std::numeric_limits<double>::quiet_NaN());
            for (uint32_t k = 0; k < W.owned_rows; ++k) {
                const size_t row = owned_to_frame_row(k, W.row_block, W.tile_count, W.tile_index, W.packed != 0);
                HIP_TRY(hipMemcpyAsync(d_rgb + row * cam->image_w * 3, nanrow.data(),
                                       nanrow.size() * 8, hipMemcpyHostToDevice,
                                       static_cast<hipStream_t>(stream)));
            }
            HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
        }
        return CRT_OK;
    }
    class_flags(s, flags_of(s->dev[device]), s->dev[device].f32_ok, true, W);
    W.tmin32 = static_cast<float>(cam->t_min);
    W.count_spec = std::getenv("CRT_COUNT_SPEC") != nullptr ? 1u : 0u;
    W.round_counters = std::getenv("CRT_ROUND_COUNTERS") != nullptr ? 1u : 0u;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (count_stats) HIP_TRY(hipStreamCreate(&st));
    int r;
    if (u16_entries(s))
        r = dispatch_render<uint16_t>(s, device, cam, W, d_rgb, st, count_stats, pass);
    else
        r = dispatch_render<uint32_t>(s, device, cam, W, d_rgb, st, count_stats, pass);
    if (count_stats) (void)hipStreamDestroy(st);
    return r;
}

static int ref_prim_table(const crt_scene* cs, int device, const uint32_t** out);

int device_closest_hits(crt_scene* s, int device, const double* rays, size_t n, double t_min,
                        double t_max, crt_hit* out) {
    int rc = device_upload(s, device);
    if (rc) return rc;
    if (n == 0) return CRT_OK;
    if (n > 0x7fffffffu) return fail(CRT_E_INVALID, "too many rays");
    DeviceGuard g(device);
    const DeviceCopy& c = s->dev[device];
    const uint32_t blocks = static_cast<uint32_t>((n + dev::kBlock - 1) / dev::kBlock);
    // ref -> primitive index: the table cached beside the device copy (ref_prim_table)
    const size_t nsp = s->num_spheres;
    const uint32_t* d_sp = nullptr;
    rc = ref_prim_table(s, device, &d_sp);
    if (rc) return rc;
    double* d_rays = nullptr;
    crt_hit* d_out = nullptr;
    uint32_t* d_stack = nullptr;
    HIP_TRY(hipMalloc(&d_rays, n * 6 * sizeof(double)));
    HIP_TRY(hipMalloc(&d_out, n * sizeof(crt_hit)));
    HIP_TRY(hipMalloc(&d_stack, static_cast<size_t>(s->depth + 1) * blocks * dev::kBlock * 4));
    HIP_TRY(hipMemcpy(d_rays, rays, n * 6 * sizeof(double), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(dev::hits_kernel, dim3(blocks), dim3(dev::kBlock), 0, 0, view_of(c), d_rays,
                       static_cast<uint32_t>(n), t_min, t_max, d_sp, static_cast<uint32_t>(nsp), d_out, d_stack);
    hipError_t le = hipGetLastError();
    hipError_t se = hipDeviceSynchronize();
    if (le == hipSuccess && se == hipSuccess)
        se = hipMemcpy(out, d_out, n * sizeof(crt_hit), hipMemcpyDeviceToHost);
    (void)hipFree(d_rays);
    (void)hipFree(d_out);
    (void)hipFree(d_stack);
    if (le != hipSuccess) return fail(CRT_E_HIP, std::string("hits_kernel launch: ") + hipGetErrorString(le));
    if (se != hipSuccess) return fail(CRT_E_HIP, std::string("hits_kernel: ") + hipGetErrorString(se));
    return CRT_OK;
}

int device_ppm_values(int device, const double* d_rgb, size_t n, int32_t* h_values, void* stream) {
    int rc = check_device(device);
    if (rc) return rc;
    if (n == 0) return CRT_OK;
    if (n > (1ull << 40)) return fail(CRT_E_INVALID, "crt_ppm_values: frame too large");
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t* d_out = nullptr;
    HIP_TRY(hipMallocAsync(reinterpret_cast<void**>(&d_out), n * 3 * sizeof(int32_t), st));
    hipLaunchKernelGGL(dev::ppm_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, st,
                       d_rgb, static_cast<uint64_t>(n), d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_values, d_out, n * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    (void)hipFreeAsync(d_out, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("ppm_kernel: ") + hipGetErrorString(e));
    // pixels the kernel could not settle: recompute on the host with std::pow
    std::vector<size_t> redo;
    for (size_t p = 0; p < n; ++p)
        if (h_values[3 * p] == dev::kPpmRedo || h_values[3 * p + 1] == dev::kPpmRedo ||
            h_values[3 * p + 2] == dev::kPpmRedo)
            redo.push_back(p);
    if (redo.empty()) return CRT_OK;
    // their f64 values: the whole frame when many, else gathered on the device (one upload of the
    // list, one copy back)
    const bool whole = redo.size() > 4096;
    std::vector<double> px(whole ? n * 3 : redo.size() * 3);
    if (whole) {
        HIP_TRY(hipMemcpy(px.data(), d_rgb, n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        std::vector<uint32_t> list(redo.begin(), redo.end());
        uint32_t* d_list = nullptr;
        double* d_px = nullptr;
        HIP_TRY(hipMalloc(&d_list, list.size() * sizeof(uint32_t)));
        hipError_t ge = hipMalloc(&d_px, px.size() * sizeof(double));
        if (ge == hipSuccess) ge = hipMemcpy(d_list, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (ge == hipSuccess) {
            hipLaunchKernelGGL(dev::redo_gather_kernel, dim3(static_cast<uint32_t>((list.size() + 255) / 256)), dim3(256), 0,
                               st, d_rgb, d_list, static_cast<uint32_t>(list.size()), d_px);
            ge = hipGetLastError();
        }
        if (ge == hipSuccess) ge = hipStreamSynchronize(st);
        if (ge == hipSuccess) ge = hipMemcpy(px.data(), d_px, px.size() * sizeof(double), hipMemcpyDeviceToHost);
        (void)hipFree(d_list);
        if (d_px) (void)hipFree(d_px);
        if (ge != hipSuccess) return fail(CRT_E_HIP, std::string("ppm redo gather: ") + hipGetErrorString(ge));
    }
    for (size_t j = 0; j < redo.size(); ++j)
        ppm_pixel_host(px.data() + 3 * (whole ? redo[j] : j), h_values + 3 * redo[j]);
    return CRT_OK;
}

// ---- launchers of the kernels the blocking drivers (crt_drivers.hip) run themselves: one launch
// on `stream` of the current device each; false when the launch failed
bool device_ppm8(const double* d_rgb, uint64_t px, uint8_t* d_out, uint32_t* d_redo, uint32_t redo_cap, void* stream) {
    hipLaunchKernelGGL(dev::ppm8_kernel, dim3(static_cast<uint32_t>((px + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_rgb, px, d_out, d_redo, redo_cap);
    return hipGetLastError() == hipSuccess;
}
bool device_redo_gather(const double* d_rgb, const uint32_t* d_list, uint32_t n, double* d_out, void* stream) {
    hipLaunchKernelGGL(dev::redo_gather_kernel, dim3(static_cast<uint32_t>((static_cast<uint64_t>(n) + 255) / 256)),
                       dim3(256), 0, static_cast<hipStream_t>(stream), d_rgb, d_list, n, d_out);
    return hipGetLastError() == hipSuccess;
}
bool device_scale(const double* d_sum, double* d_out, uint64_t count, double factor, void* stream) {
    hipLaunchKernelGGL(dev::scale_kernel, dim3(static_cast<uint32_t>((count + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_sum, d_out, count, factor);
    return hipGetLastError() == hipSuccess;
}

// crt_noise_estimate: sum se and sum m over `pixels` noise records (noise_stage1_kernel). K = the
// full chunks among the first samples_done samples; fewer than two give no variance: both NaN.
int device_noise_estimate(int device, const double* d_noise, size_t pixels, uint32_t spp, uint32_t samples_done,
                          double* sum_se, double* sum_mean, void* stream) {
    int rc = check_device(device);
    if (rc) return rc;
    const uint32_t L = sample_chunk_len(spp);
    const uint32_t K = samples_done / L;
    *sum_se = *sum_mean = std::numeric_limits<double>::quiet_NaN();
    if (K < 2 || pixels == 0) return CRT_OK;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipMemPool_t pool = nullptr;  // a pass render's companion: the same scratch pool (pass_pool)
    rc = pass_pool(device, &pool);
    if (rc) return rc;
    double* d_tmp = nullptr;  // kNoiseBlocks block results, then the two sums
    HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&d_tmp), (dev::kNoiseBlocks + 1) * 2 * sizeof(double), pool, st));
    double h[2] = {0, 0};
    hipLaunchKernelGGL(dev::noise_stage1_kernel, dim3(dev::kNoiseBlocks), dim3(256), 0, st, d_noise,
                       static_cast<uint64_t>(pixels), static_cast<double>(K), static_cast<double>(L), d_tmp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(dev::noise_stage2_kernel, dim3(1), dim3(256), 0, st, d_tmp, d_tmp + 2 * dev::kNoiseBlocks);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, d_tmp + 2 * dev::kNoiseBlocks, sizeof h, hipMemcpyDeviceToHost, st);
    (void)hipFreeAsync(d_tmp, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("noise kernels: ") + hipGetErrorString(e));
    *sum_se = h[0];
    *sum_mean = h[1];
    return CRT_OK;
}

// ---- adaptive sampling (host side) ---------------------------------------------------------
bool adaptive_tiling_ok(const crt_tiling* t) {
    return !t || t->tile_count == 1 || (t->row_block != 0 && t->row_block % dev::kTileH == 0);
}

static uint32_t block_count(uint32_t w, uint32_t rows) {
    return ((w + dev::kTileW - 1) / dev::kTileW) * ((rows + dev::kTileH - 1) / dev::kTileH);
}

int device_adaptive_update(int device, const crt_camera* cam, const crt_tiling* t, const double* d_noise,
                           uint32_t* d_blocks, uint32_t samples_done, double threshold, uint32_t min_samples,
                           uint32_t* active_blocks, void* stream) {
    int rc = check_device(device);
    if (rc) return rc;
    dev::Work W;
    rc = tiling_work(cam, t, W);
    if (rc) return rc;
    *active_blocks = 0;
    const uint32_t nb = block_count(cam->image_w, W.owned_rows);
    if (nb == 0) return CRT_OK;
    const uint32_t N = cam->samples_per_pixel, L = sample_chunk_len(N), K = samples_done / L;
    const uint32_t may_stop = (K >= 2 && samples_done >= min_samples && min_samples < N) ? 1u : 0u;
    DeviceGuard g(device);
    hipMemPool_t pool = nullptr;
    rc = pass_pool(device, &pool);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint32_t* d_n = nullptr;
    HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&d_n), sizeof(uint32_t), pool, st));
    hipError_t e = hipMemsetAsync(d_n, 0, sizeof(uint32_t), st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(dev::adaptive_update_kernel, dim3((nb + 3) / 4), dim3(256), 0, st, d_noise, d_blocks, W,
                           cam->image_w, nb, samples_done, static_cast<double>(K), static_cast<double>(L), threshold,
                           may_stop, d_n);
        e = hipGetLastError();
    }
    uint32_t h = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&h, d_n, sizeof h, hipMemcpyDeviceToHost, st);
    (void)hipFreeAsync(d_n, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("adaptive update: ") + hipGetErrorString(e));
    *active_blocks = h;
    return CRT_OK;
}

// The frame of an adaptive render from its running sums, on `stream` of the current device: every
// block's sum times 1 / its own count (accumulate_masked_kernel without partial sums).
int device_frame_from_sums(const crt_camera* cam, const crt_tiling* t, double* d_sum, uint32_t* d_blocks,
                           double* d_rgb, void* stream) {
    dev::Work W;
    const int rc = tiling_work(cam, t, W);
    if (rc) return rc;
    const uint32_t tiles_x = (cam->image_w + dev::kTileW - 1) / dev::kTileW;
    W.bw = cam->image_w;
    W.bh = W.owned_rows;
    W.tiles_x = tiles_x;
    W.tiles_y = (W.owned_rows + dev::kTileH - 1) / dev::kTileH;
    W.tiles = block_count(cam->image_w, W.owned_rows);
    W.s0 = ~0u;  // no block word equals it: every tile takes the skipped branch
    hipLaunchKernelGGL(dev::accumulate_masked_kernel, dim3((W.tiles + 3) / 4), dim3(256), 0,
                       static_cast<hipStream_t>(stream), nullptr, d_sum, nullptr, d_rgb, d_blocks, W, cam->image_w,
                       tiles_x, 0u, 0u, 0.0);
    if (hipGetLastError() != hipSuccess) return fail(CRT_E_HIP, "adaptive render: frame kernel launch");
    return CRT_OK;
}

// ---- denoising inputs (host side): first-hit features and the per-pixel variance -------------
int device_check(int device) { return check_device(device); }

int device_pass_pool(int device, void** pool) {
    hipMemPool_t p = nullptr;
    const int rc = pass_pool(device, &p);
    *pool = p;
    return rc;
}

// the scene's ref -> primitive number table on `device` (hits_kernel's ref_prim), built and
// uploaded once per device copy, blocking; the scene's device lock orders the first callers
static int ref_prim_table(const crt_scene* cs, int device, const uint32_t** out) {
    crt_scene* s = const_cast<crt_scene*>(cs);  // the table is a cache beside the device copy
    std::lock_guard<std::mutex> lk(s->dev_mu[device]);
    DeviceCopy& c = s->dev[device];
    if (!c.ref_prim) {
        const size_t nsp = s->num_spheres, nq = s->num_quads;
        std::vector<uint32_t> ref_prim(std::max<size_t>(1, nsp + nq));
        std::vector<uint32_t> dev_refs;  // a scene set up on the device has no host refs
        const uint32_t* refs = s->refs.data();
        if (s->refs.size() != s->num_prims) {
            dev_refs.resize(s->num_prims);
            HIP_TRY(hipMemcpy(dev_refs.data(), c.refs, s->num_prims * 4, hipMemcpyDeviceToHost));
            refs = dev_refs.data();
        }
        for (size_t slot = 0; slot < s->num_prims; ++slot) {
            const uint32_t r = refs[slot];
            ref_prim[(r & kRefQuad) ? nsp + (r & ~kRefQuad) : r] = s->order[slot];
        }
        uint32_t* d = nullptr;
        HIP_TRY(hipMalloc(&d, ref_prim.size() * 4));
        const hipError_t e = hipMemcpy(d, ref_prim.data(), ref_prim.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail(CRT_E_HIP, std::string("feature pass: primitive table upload: ") + hipGetErrorString(e));
        }
        c.ref_prim = d;
    }
    *out = c.ref_prim;
    return CRT_OK;
}

int device_render_features(const crt_scene* s, int device, const crt_camera* cam, const crt_tiling* t,
                           crt_feature* d_feat, void* stream) {
    int rc = check_device(device);
    if (rc) return rc;
    if (!s->dev[device].valid)
        return fail(CRT_E_NOT_UPLOADED, "scene not uploaded to device " + std::to_string(device));
    if (static_cast<uint64_t>(cam->image_w) * cam->image_h >= 0x7fffffffull)
        return fail(CRT_E_INVALID, "crt_render_features_async: image has more than 2^31-2 pixels");
    dev::Work W;
    rc = tiling_work(cam, t, W);
    if (rc) return rc;
    const uint64_t n = static_cast<uint64_t>(W.owned_rows) * cam->image_w;
    if (n == 0) return CRT_OK;
    DeviceGuard g(device);
    const uint32_t* d_ref_prim = nullptr;
    rc = ref_prim_table(s, device, &d_ref_prim);
    if (rc) return rc;
    hipMemPool_t pool = nullptr;
    rc = pass_pool(device, &pool);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t blocks = static_cast<uint32_t>((n + dev::kBlock - 1) / dev::kBlock);
    uint32_t* d_stack = nullptr;  // trace()'s stacks, [level][thread], as device_closest_hits sizes them
    HIP_TRY(hipMallocFromPoolAsync(reinterpret_cast<void**>(&d_stack),
                                   static_cast<size_t>(s->depth + 1) * blocks * dev::kBlock * 4, pool, st));
    hipLaunchKernelGGL(dev::features_kernel, dim3(blocks), dim3(dev::kBlock), 0, st, view_of(s->dev[device]),
                       cam_view(cam), W, static_cast<uint32_t>(n), d_ref_prim, static_cast<uint32_t>(s->num_spheres),
                       d_feat, d_stack);
    const hipError_t e = hipGetLastError();
    (void)hipFreeAsync(d_stack, st);
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("features_kernel launch: ") + hipGetErrorString(e));
    return CRT_OK;
}

// ---- ray queries (crt_trace_async) -------------------------------------------------------------
// One query_kernel launch (persistent_grid: its grid and scratch)
template <typename SE, bool GSTACK, bool LSCENE, int PM>
static int launch_trace(const crt_scene* s, int device, dev::Work W, size_t lds, dev::Query Q, bool any,
                        hipMemPool_t pool, hipStream_t stream) {
    lds = lds_tail(W, lds, trace_tail(GSTACK, LSCENE));
    const void* kfn = any ? reinterpret_cast<const void*>(dev::query_kernel<SE, GSTACK, LSCENE, PM, true>)
                          : reinterpret_cast<const void*>(dev::query_kernel<SE, GSTACK, LSCENE, PM, false>);
    uint32_t blocks = 0;
    SE* gstack = nullptr;
    if (const int rc = persistent_grid(s, device, kfn, lds, Q.batches, GSTACK, pool, stream, blocks, gstack, Q.queue)) return rc;
    const dev::SceneView S = view_of(s->dev[device]);
    if (any)
        hipLaunchKernelGGL((dev::query_kernel<SE, GSTACK, LSCENE, PM, true>), dim3(blocks), dim3(dev::kBlock), lds, stream,
                           S, W, Q, gstack);
    else
        hipLaunchKernelGGL((dev::query_kernel<SE, GSTACK, LSCENE, PM, false>), dim3(blocks), dim3(dev::kBlock), lds, stream,
                           S, W, Q, gstack);
    const hipError_t e = hipGetLastError();
    (void)hipFreeAsync(Q.queue, stream);
    if (gstack) (void)hipFreeAsync(gstack, stream);
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("query_kernel launch: ") + hipGetErrorString(e));
    return CRT_OK;
}

static int launch_plain(const crt_scene* s, int device, const dev::Query& Q, bool any, hipMemPool_t pool,
                        hipStream_t st);

template <typename SE>
static int dispatch_trace(const crt_scene* s, int device, dev::Work W, const dev::Query& Q, bool any,
                          hipMemPool_t pool, hipStream_t st) {
    const Layout L = scene_layout<SE>(s, W, kTraceExtra, false);
    // Scenes small enough for LDS are traced faster by the plain loop (rays of a few node tests each:
    // the persistent grid's per-ray costs dominate; DESIGN section 6d has the figures), so that is
    // their route; CRT_TRACE_FAST=1 takes the LDS-scene instances (tests, tools/ray_query_rate.py)
    if (L.cls == kQueryLdsScene && std::getenv("CRT_TRACE_FAST") == nullptr) return launch_plain(s, device, Q, any, pool, st);
    return by_class(L.cls, W.sphere_only != 0, [&](auto gstack, auto lscene, auto pm) {
        return launch_trace<SE, decltype(gstack)::value, decltype(lscene)::value, decltype(pm)::value>(s, device, W, L.lds, Q, any, pool, st);
    });
}

// CRT_TRACE_PLAIN, and trace's default route for LDS scenes: plain_query_kernel (plain_launches)
static int launch_plain(const crt_scene* s, int device, const dev::Query& Q, bool any, hipMemPool_t pool,
                        hipStream_t st) {
    const dev::SceneView S = view_of(s->dev[device]);
    return plain_launches(s, Q.n, pool, st, "plain_query_kernel", [&](uint32_t blocks, uint32_t first, uint32_t* stacks) {
        if (any)
            hipLaunchKernelGGL(dev::plain_query_kernel<true>, dim3(blocks), dim3(dev::kBlock), 0, st, S, Q, first, stacks);
        else
            hipLaunchKernelGGL(dev::plain_query_kernel<false>, dim3(blocks), dim3(dev::kBlock), 0, st, S, Q, first, stacks);
    });
}

int device_trace(const crt_scene* s, int device, const double* d_rays, size_t n, const double* d_tmax,
                 const crt_trace_params* prm, crt_hit* d_hits, uint32_t* d_occluded, void* stream) {
    int rc = check_device(device);
    if (rc) return rc;
    if (!s->dev[device].valid)
        return fail(CRT_E_NOT_UPLOADED, "scene not uploaded to device " + std::to_string(device));
    if (n == 0) return CRT_OK;
    DeviceGuard g(device);
    const bool any = (prm->flags & CRT_TRACE_ANY) != 0;
    dev::Query Q{};
    Q.rays = d_rays;
    Q.tmax = d_tmax;
    Q.n = static_cast<uint32_t>(n);
    Q.batches = static_cast<uint32_t>((n + 63) / 64);
    Q.t_min = prm->t_min;
    Q.t_max = prm->t_max;
    Q.num_spheres = static_cast<uint32_t>(s->num_spheres);
    Q.hits = d_hits;
    Q.occluded = d_occluded;
    if (!any) {  // the first call builds and uploads the table, blocking
        rc = ref_prim_table(s, device, &Q.ref_prim);
        if (rc) return rc;
    }
    hipMemPool_t pool = nullptr;
    rc = pass_pool(device, &pool);
    if (rc) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (prm->flags & CRT_TRACE_PLAIN) return launch_plain(s, device, Q, any, pool, st);
    // device_render's scene classes; the walk's and the filters' interval rules (walk(), query_kernel)
    const DeviceCopy& c = s->dev[device];
    dev::Work W{};
    const bool filters = prm->t_min >= 0;
    class_flags(s, flags_of(c), c.f32_ok && std::fabs(prm->t_min) <= 0x1p100, filters, W);
    W.tmin32 = static_cast<float>(prm->t_min);
    if (u16_entries(s)) return dispatch_trace<uint16_t>(s, device, W, Q, any, pool, st);
    return dispatch_trace<uint32_t>(s, device, W, Q, any, pool, st);
}

// crt_trace: device_trace for host arrays, blocking: one upload of the rays (and bounds), one query,
// one copy back, on a stream of its own
int device_trace_host(crt_scene* s, int device, const double* rays, size_t n, const double* tmax,
                      const crt_trace_params* prm, crt_hit* hits, uint32_t* occluded) {
    int rc = device_upload(s, device);
    if (rc) return rc;
    DeviceGuard g(device);
    const bool any = (prm->flags & CRT_TRACE_ANY) != 0;
    const size_t out_bytes = n * (any ? sizeof(uint32_t) : sizeof(crt_hit));
    void* host_out = any ? static_cast<void*>(occluded) : static_cast<void*>(hits);
    double *d_rays = nullptr, *d_tmax = nullptr;
    void* d_out = nullptr;
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreate(&st);
    if (e == hipSuccess) e = hipMalloc(&d_rays, n * 6 * sizeof(double));
    if (e == hipSuccess && tmax) e = hipMalloc(&d_tmax, n * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&d_out, out_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays, rays, n * 6 * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && tmax) e = hipMemcpyAsync(d_tmax, tmax, n * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        rc = device_trace(s, device, d_rays, n, d_tmax, prm, any ? nullptr : static_cast<crt_hit*>(d_out),
                          any ? static_cast<uint32_t*>(d_out) : nullptr, st);
    if (e == hipSuccess && rc == CRT_OK) e = hipMemcpyAsync(host_out, d_out, out_bytes, hipMemcpyDeviceToHost, st);
    if (st) {
        const hipError_t se = hipStreamSynchronize(st);
        if (e == hipSuccess) e = se;
        (void)hipStreamDestroy(st);
    }
    (void)hipFree(d_rays);
    (void)hipFree(d_tmax);
    (void)hipFree(d_out);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("crt_trace: ") + hipGetErrorString(e));
    return CRT_OK;
}

// ---- radiance queries (crt_radiance_async) -----------------------------------------------------
// One radiance_kernel launch (persistent_grid: its grid and scratch)
template <typename SE, bool GSTACK, bool LSCENE, int PM, bool ENV, bool NEE, bool LGT>
static int launch_radiance(const crt_scene* s, int device, dev::Work W, size_t lds, const dev::CamView& C,
                           dev::RadianceOf<ENV, NEE, LGT> Q, hipMemPool_t pool, hipStream_t stream) {
    lds = lds_tail(W, lds, radiance_tail(GSTACK, LSCENE));
    const void* kfn = reinterpret_cast<const void*>(dev::radiance_kernel<SE, GSTACK, LSCENE, PM, ENV, NEE, LGT>);
    uint32_t blocks = 0;
    SE* gstack = nullptr;
    if (const int rc = persistent_grid(s, device, kfn, lds, Q.batches, GSTACK, pool, stream, blocks, gstack, Q.queue)) return rc;
    hipLaunchKernelGGL((dev::radiance_kernel<SE, GSTACK, LSCENE, PM, ENV, NEE, LGT>), dim3(blocks), dim3(dev::kBlock), lds, stream,
                       view_of(s->dev[device]), C, W, Q, gstack);
    const hipError_t e = hipGetLastError();
    (void)hipFreeAsync(Q.queue, stream);
    if (gstack) (void)hipFreeAsync(gstack, stream);
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("radiance_kernel launch: ") + hipGetErrorString(e));
    return CRT_OK;
}

// CRT_RADIANCE_PLAIN: plain_radiance_kernel (plain_launches)
template <bool ENV, bool NEE, bool LGT>
static int launch_plain_radiance(const crt_scene* s, int device, const dev::CamView& C, const dev::RadianceOf<ENV, NEE, LGT>& Q,
                                 hipMemPool_t pool, hipStream_t st) {
    const dev::SceneView S = view_of(s->dev[device]);
    return plain_launches(s, Q.n, pool, st, "plain_radiance_kernel", [&](uint32_t blocks, uint32_t first, uint32_t* stacks) {
        hipLaunchKernelGGL((dev::plain_radiance_kernel<ENV, NEE, LGT>), dim3(blocks), dim3(dev::kBlock), 0, st, S, C, Q, first, stacks);
    });
}

// dispatch_trace's classes; every class takes the fast route (a path is many segments per queue
// visit, unlike a single ray: DESIGN section 6e)
template <typename SE, bool ENV, bool NEE, bool LGT>
static int dispatch_radiance(const crt_scene* s, int device, dev::Work W, const dev::CamView& C,
                             const dev::RadianceOf<ENV, NEE, LGT>& Q, hipMemPool_t pool, hipStream_t st) {
    const Layout L = scene_layout<SE>(s, W, camera_extra(), false);
    return by_class(L.cls, W.sphere_only != 0, [&](auto gstack, auto lscene, auto pm) {
        return launch_radiance<SE, decltype(gstack)::value, decltype(lscene)::value, decltype(pm)::value, ENV, NEE, LGT>(s, device, W, L.lds, C, Q, pool, st);
    });
}

// the route of one call: the plain kernel, or the fast one for the scene's class and entry width
template <bool ENV, bool NEE = false, bool LGT = false>
static int route_radiance(const crt_scene* s, int device, const crt_radiance_params* prm, const dev::CamView& C,
                          const dev::RadianceOf<ENV, NEE, LGT>& Q, hipMemPool_t pool, hipStream_t st) {
    if (prm->flags & CRT_RADIANCE_PLAIN) return launch_plain_radiance<ENV, NEE, LGT>(s, device, C, Q, pool, st);
    // device_trace's scene classes and interval rules; 0 <= t_min <= 2^100 here (crt_radiance_async)
    const DeviceCopy& c = s->dev[device];
    dev::Work W{};
    class_flags(s, flags_of(c), c.f32_ok, true, W);
    W.tmin32 = static_cast<float>(prm->t_min);
    if (u16_entries(s)) return dispatch_radiance<uint16_t, ENV, NEE, LGT>(s, device, W, C, Q, pool, st);
    return dispatch_radiance<uint32_t, ENV, NEE, LGT>(s, device, W, C, Q, pool, st);
}

// env: null, or the call's environment (checked by crt_host.cpp; its texels on `device`): the ENV
// instances. Without one the launch is the instances' without ENV, as before environments existed.
// smp: null, or the sampler (built on `device`; crt_host.cpp checks it) whose recorded environment
// and tables the NEE instances read; env is not used then.
int device_radiance(const crt_scene* s, int device, const double* d_rays, size_t n, const uint32_t* d_states,
                    const crt_radiance_params* prm, const crt_env* env, double* d_rgb, void* stream,
                    const crt_env_sampler* smp, const crt_light_sampler* lights) {
    int rc = check_device(device);
    if (rc) return rc;
    if (!s->dev[device].valid)
        return fail(CRT_E_NOT_UPLOADED, "scene not uploaded to device " + std::to_string(device));
    if (n == 0) return CRT_OK;
    DeviceGuard g(device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (prm->max_depth == 0) {  // ray_color returns RGB::zero() before any query (camera.h:211-213)
        HIP_TRY(hipMemsetAsync(d_rgb, 0, n * 3 * sizeof(double), st));
        return CRT_OK;
    }
    dev::CamView C{};
    for (int k = 0; k < 3; ++k) C.bg[k] = prm->background[k];
    C.t_min = prm->t_min;
    C.max_depth = prm->max_depth;
    C.base_seed = prm->base_seed;
    dev::RadianceNee Q{};
    Q.rays = d_rays;
    Q.states = d_states;
    Q.rgb = d_rgb;
    Q.n = static_cast<uint32_t>(n);
    Q.batches = static_cast<uint32_t>((n + 63) / 64);
    Q.max_depth = prm->max_depth;
    Q.base_seed = prm->base_seed;
    hipMemPool_t pool = nullptr;
    rc = pass_pool(device, &pool);
    if (rc) return rc;
    if (lights && (env || smp)) {  // the lit instances; with smp, env is its recorded copy
        dev::RadianceLit QT{};
        static_cast<dev::Radiance&>(QT) = Q;
        QT.ltb = LightTables{lights->ref, lights->cdf, lights->sref, lights->sw, lights->W, lights->L};
        if (smp) {
            QT.env = smp->env;
            QT.tb = EnvTables{smp->w, smp->c, smp->m, smp->W};
            return route_radiance<true, true, true>(s, device, prm, C, QT, pool, st);
        }
        QT.env = *env;
        return route_radiance<true, false, true>(s, device, prm, C, QT, pool, st);
    }
    if (lights) {  // of this scene on `device` (crt_host.cpp checks it)
        dev::RadianceLights QL{};
        static_cast<dev::Radiance&>(QL) = Q;
        QL.tb = LightTables{lights->ref, lights->cdf, lights->sref, lights->sw, lights->W, lights->L};
        return route_radiance<false, false, true>(s, device, prm, C, QL, pool, st);
    }
    if (smp) {
        Q.env = smp->env;
        Q.tb = EnvTables{smp->w, smp->c, smp->m, smp->W};
        return route_radiance<true, true>(s, device, prm, C, Q, pool, st);
    }
    if (!env) return route_radiance<false>(s, device, prm, C, Q, pool, st);
    Q.env = *env;
    return route_radiance<true>(s, device, prm, C, Q, pool, st);
}

// ---- launch plans (crt_launch_plan) ------------------------------------------------------------
// The plan of one kernel: device_render's, device_trace's or device_radiance's class flags, that
// kernel's layout step and its launcher's additions, for the instance its dispatch step picks.
template <typename SE>
static void plan_of(const crt_scene* s, uint32_t kernel, const CopyFlags& c, crt_launch_plan_info& p) {
    dev::Work W{};
    W.lds_cam = W.lds_acc = W.lds_inv64 = CRT_PLAN_ABSENT;
    class_flags(s, c, c.f32_ok, true, W);
    Layout L;
    size_t total;
    int pm;
    if (kernel == CRT_PLAN_RENDER) {
        L = scene_layout<SE>(s, W, camera_extra(), true);
        pm = render_prim_mode(W, L.cls);
        total = lds_tail(W, L.lds, render_tail(L.cls == kQueryHbmStack, L.cls == kQueryLdsScene, pm, L.w5));
    } else if (kernel == CRT_PLAN_TRACE) {
        L = scene_layout<SE>(s, W, kTraceExtra, false);
        pm = query_prim_mode(W);
        total = lds_tail(W, L.lds, trace_tail(L.cls == kQueryHbmStack, L.cls == kQueryLdsScene));
        p.plain_route = (L.cls == kQueryLdsScene && std::getenv("CRT_TRACE_FAST") == nullptr) ? 1u : 0u;
    } else {
        L = scene_layout<SE>(s, W, camera_extra(), false);
        pm = query_prim_mode(W);
        total = lds_tail(W, L.lds, radiance_tail(L.cls == kQueryHbmStack, L.cls == kQueryLdsScene));
    }
    p.kernel = kernel;
    p.klass = L.cls == kQueryLdsScene ? CRT_PLAN_LDS_SCENE : L.cls == kQueryLdsStack ? CRT_PLAN_LDS_STACK : CRT_PLAN_HBM_STACK;
    p.entry_bytes = sizeof(SE);
    p.five_waves = L.w5 ? 1u : 0u;
    p.prim_mode = static_cast<uint32_t>(pm);
    p.depth = s->depth;
    p.block = dev::kBlock;
    p.num_nodes = s->num_dnodes;
    p.stack_bytes = static_cast<uint32_t>(L.stack_bytes);
    p.level = static_cast<uint32_t>(L.level);
    p.sentinel = W.sentinel;
    p.hbm_stack_levels = L.cls == kQueryHbmStack ? static_cast<uint32_t>(gstack_levels(s)) : 0u;
    p.lds_nodes = W.lds_nodes;
    p.lds_refs = W.lds_refs;
    p.lds_spheres = W.lds_spheres;
    p.lds_quads = W.lds_quads;
    p.lds_quadf = W.lds_quadf;
    p.lds_sph64 = W.lds_sph64;
    p.lds_stack = W.lds_stack;
    p.bytes_nodes = W.bytes_nodes;
    p.bytes_refs = W.bytes_refs;
    p.bytes_spheres = W.bytes_spheres;
    p.bytes_quads = W.bytes_quads;
    p.bytes_quadf = W.bytes_quadf;
    p.bytes_sph64 = W.bytes_sph64;
    p.ntop = W.ntop;
    p.all_nodes = static_cast<uint32_t>(L.all_nodes);
    p.lds_cam = W.lds_cam;
    p.lds_acc = W.lds_acc;
    p.lds_inv64 = W.lds_inv64;
    p.bytes_cam = static_cast<uint32_t>(camera_extra());
    p.bytes_acc = static_cast<uint32_t>(kAccBytes);
    p.bytes_inv64 = static_cast<uint32_t>(kInvBytes);
    p.total_lds = static_cast<uint32_t>(total);
    p.budget = static_cast<uint32_t>(L.budget);
    p.spheres_f32 = W.spheres_f32;
    p.quads_f32 = W.quads_f32;
    p.quads_flat = W.quads_flat;
    p.f32_ok = W.f32_ok;
}

int device_launch_plan(crt_scene* s, uint32_t kernel, crt_launch_plan_info* out) {
    if (s->num_dnodes == 0 || s->num_dnodes >= (size_t{1} << (31 - kNodeFShift)))
        return fail(CRT_E_INVALID, "crt_launch_plan: no device node layout for this BVH");
    if (s->image_device < 0) {  // device_upload's staging
        std::lock_guard<std::mutex> ls(s->mu);
        if (!s->staged) stage_image(s);
    }
    crt_launch_plan_info p{};
    const CopyFlags c = copy_flags(s);
    if (u16_entries(s))
        plan_of<uint16_t>(s, kernel, c, p);
    else
        plan_of<uint32_t>(s, kernel, c, p);
    *out = p;
    return CRT_OK;
}

// crt_radiance: device_radiance for host arrays, blocking: one upload of the rays (and states), one
// query, one copy back, on a stream of its own
int device_radiance_host(crt_scene* s, int device, const double* rays, size_t n, const uint32_t* states,
                         const crt_radiance_params* prm, double* rgb) {
    int rc = device_upload(s, device);
    if (rc) return rc;
    DeviceGuard g(device);
    double *d_rays = nullptr, *d_rgb = nullptr;
    uint32_t* d_states = nullptr;
    hipStream_t st = nullptr;
    hipError_t e = hipStreamCreate(&st);
    if (e == hipSuccess) e = hipMalloc(&d_rays, n * 6 * sizeof(double));
    if (e == hipSuccess && states) e = hipMalloc(&d_states, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d_rgb, n * 3 * sizeof(double));
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays, rays, n * 6 * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && states) e = hipMemcpyAsync(d_states, states, n * sizeof(uint32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) rc = device_radiance(s, device, d_rays, n, d_states, prm, nullptr, d_rgb, st);
    if (e == hipSuccess && rc == CRT_OK) e = hipMemcpyAsync(rgb, d_rgb, n * 3 * sizeof(double), hipMemcpyDeviceToHost, st);
    if (st) {
        const hipError_t se = hipStreamSynchronize(st);
        if (e == hipSuccess) e = se;
        (void)hipStreamDestroy(st);
    }
    (void)hipFree(d_rays);
    (void)hipFree(d_states);
    (void)hipFree(d_rgb);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("crt_radiance: ") + hipGetErrorString(e));
    return CRT_OK;
}

int device_camera_rays(int device, const crt_camera* cam, const crt_tiling* t, uint32_t first_sample,
                       uint32_t num_samples, double* d_rays, uint32_t* d_states, void* stream) {
    int rc = check_device(device);
    if (rc) return rc;
    dev::Work W;
    rc = tiling_work(cam, t, W);
    if (rc) return rc;
    const uint64_t pixels = static_cast<uint64_t>(W.owned_rows) * cam->image_w;
    if (pixels == 0 || num_samples == 0) return CRT_OK;
    if (pixels > 0x7fffffffull / num_samples)
        return fail(CRT_E_INVALID, "crt_camera_rays_async: more than 2^31-1 records");
    const uint32_t n = static_cast<uint32_t>(pixels * num_samples);
    DeviceGuard g(device);
    hipLaunchKernelGGL(dev::camera_rays_kernel, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       cam_view(cam), W, n, first_sample, num_samples, d_rays, d_states);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("camera_rays_kernel launch: ") + hipGetErrorString(e));
    return CRT_OK;
}

int device_pixel_variance(int device, const crt_camera* cam, const crt_tiling* t, const double* d_noise,
                          const uint32_t* d_blocks, uint32_t samples_done, double* d_var, void* stream) {
    int rc = check_device(device);
    if (rc) return rc;
    if (static_cast<uint64_t>(cam->image_w) * cam->image_h >= 0xffffffffull)
        return fail(CRT_E_INVALID, "crt_pixel_variance_async: image has more than 2^32-1 pixels");
    dev::Work W;
    rc = tiling_work(cam, t, W);
    if (rc) return rc;
    const uint64_t n = static_cast<uint64_t>(W.owned_rows) * cam->image_w;
    if (n == 0) return CRT_OK;
    DeviceGuard g(device);
    hipLaunchKernelGGL(dev::pixel_variance_kernel, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), d_noise, d_blocks, W, cam->image_w, static_cast<uint32_t>(n),
                       samples_done, sample_chunk_len(cam->samples_per_pixel), d_var);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(CRT_E_HIP, std::string("pixel_variance_kernel launch: ") + hipGetErrorString(e));
    return CRT_OK;
}

// The compile-time switches this library was built with (bench.py hashes them with the kernel
// sources, so a PMC summary is only used for the exact build it was collected on).
#ifndef CRT_ARCH
#define CRT_ARCH "unknown"
#endif
#define CRT_STR2(x) #x
#define CRT_STR(x) CRT_STR2(x)
const char* device_build_info() {
    // every compile-time parameter of the kernels (the numeric tuning knobs; the library has no
    // other build switches), and the offload target the Makefile compiled for
    return "arch=" CRT_ARCH " CRT_BLOCK=" CRT_STR(CRT_BLOCK) " CRT_TILE_W=" CRT_STR(CRT_TILE_W)
           " CRT_WAVES_PER_EU=" CRT_STR(CRT_WAVES_PER_EU) " CRT_WAVES_PER_EU_LDS=" CRT_STR(CRT_WAVES_PER_EU_LDS)
           " CRT_SHADE_BATCH=" CRT_STR(CRT_SHADE_BATCH) " CRT_CHUNK_MIN=" CRT_STR(CRT_CHUNK_MIN)
           " CRT_WATCHDOG=" CRT_STR(CRT_WATCHDOG) " CRT_PAIR_WALK=" CRT_STR(CRT_PAIR_WALK);
}

}  // namespace crt
