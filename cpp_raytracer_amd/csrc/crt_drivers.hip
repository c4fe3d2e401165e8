// The blocking render drivers: crt_render / crt_render_ppm (render_multi_impl),
// crt_render_progressive, crt_render_adaptive, crt_render_denoised,
// crt_render_denoised_devices and crt_render_lens_passes. Host code only: no kernel
// is defined here; the drivers go through the device_* functions of crt_device.hip and
// crt_denoise.hip. What the drivers share is defined once, above them: the device set with its
// concurrent upload, the per-device lane, the gather, the adaptive step and the block counts.
//
// CONSTRAINT: every driver keeps its sequence of HIP runtime calls per device and per stream: the
// order and sizes of its allocations (the max(1, ...) floors included; hipMalloc, not a pool), its
// memsets, event records, waits, copies, synchronizations and frees. The lost passes of DESIGN
// section 6b and the pass-render fault of section 6c depended on allocation and synchronization
// patterns and their cause is not known: a change here must not move them, and none claims to fix
// them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "crt_internal.h"
#include "crt_hip_util.h"
#include "crt_rows.h"

namespace crt {
namespace {

// ---- the devices of a render ----------------------------------------------------------------
// Logical devices [0, n): rows are dealt to them in 4-row blocks (row r on device (r / 4) % n,
// crt_tiling{4, n, d}). CRT_EMULATE_DEVICES=k (tests; read at every call): k logical devices, all
// on physical device 0, through the same tiling and gather code.
struct DeviceSet {
    int n = 0, n_phys = 0;
    bool emulate = false;
    static constexpr uint32_t rb = 4;  // 4-row blocks: 800 rows split exactly over 1, 2, 4, 8 devices
    int phys(int d) const { return emulate ? 0 : d; }
    crt_tiling tiling(int d, bool packed = true) const {
        return crt_tiling{rb, static_cast<uint32_t>(n), static_cast<uint32_t>(d), packed ? CRT_TILING_PACKED : 0u};
    }
};

// The devices of a call, and the scene uploaded to every physical one concurrently: one host thread
// per device, one copy of the staged image each. A worker's error message is taken from its own
// thread (crt_last_error is per thread) and raised again on this one.
int open_devices(crt_scene* s, int num_devices, DeviceSet& ds) {
    int avail = 0;
    if (hipGetDeviceCount(&avail) != hipSuccess || avail == 0)
        return fail(CRT_E_NODEVICE, "no HIP device visible (the render path has no CPU fallback)");
    if (num_devices <= 0) num_devices = avail;
    ds.n = std::min(num_devices, std::min(avail, kMaxDevices));
    if (const char* e = std::getenv("CRT_EMULATE_DEVICES")) {
        ds.n = std::max(1, std::min(std::atoi(e), 64));
        ds.emulate = true;
    }
    ds.n_phys = ds.emulate ? 1 : ds.n;
    std::vector<int> urc(ds.n_phys, CRT_OK);
    std::vector<std::string> umsg(ds.n_phys);
    {
        std::vector<std::thread> th;
        for (int d = 0; d < ds.n_phys; ++d)
            th.emplace_back([&, d] {
                urc[d] = device_upload(s, d);
                if (urc[d]) umsg[d] = crt_last_error();
            });
        for (auto& t : th) t.join();
    }
    for (int d = 0; d < ds.n_phys; ++d)
        if (urc[d]) return fail(urc[d], "device " + std::to_string(d) + ": " + umsg[d]);
    return CRT_OK;
}

// ---- one logical device's stream, events and buffers ------------------------------------------
// Set up by open / alloc / event in the driver's order with the device current; the first failure
// clears `ok` and the calls after it do nothing. close() (the destructor) synchronizes the stream
// and frees on the lane's device: the buffers in allocation order, the stream, the events.
struct Lane {
    int device = 0;  // physical
    hipStream_t stream = nullptr;
    hipEvent_t start = nullptr, done = nullptr;
    std::vector<void*> owned;
    bool ok = true;
    // the lane's rows of the frame, and its state over the passes (packed owned rows)
    crt_tiling tiling{1, 1, 0, 0};
    uint32_t rows = 0, nblk = 0, hint = 0;
    size_t px = 0;
    double *sum = nullptr, *noise = nullptr, *rgb = nullptr;
    uint32_t* blocks = nullptr;
    const void* out = nullptr;  // the rows gather_frame copies

    Lane() = default;
    Lane(const Lane&) = delete;
    Lane& operator=(const Lane&) = delete;
    ~Lane() { close(); }
    void open(int phys) { device = phys; ok = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess; }
    template <typename T>
    void alloc(T*& p, size_t bytes) {
        void* v = nullptr;
        ok = ok && hipMalloc(&v, bytes) == hipSuccess;
        if (!ok) return;
        owned.push_back(v);
        p = static_cast<T*>(v);
    }
    void event(hipEvent_t& e) { ok = ok && hipEventCreate(&e) == hipSuccess; }
    void close() {
        if (!stream && !start && !done && owned.empty()) return;
        DeviceGuard g(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (void* p : owned) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
        if (start) (void)hipEventDestroy(start);
        if (done) (void)hipEventDestroy(done);
        owned.clear();
        stream = nullptr;
        start = done = nullptr;
    }
};

// A render's lanes, closed in device order, and the frame buffer on device 0, which is allocated
// after the lanes are set up (alloc_frame) and freed after them. who: the driver, for error texts.
struct Lanes {
    const std::string who;
    DeviceSet ds;
    std::vector<Lane> lane;
    Lane frame;  // no stream: owns the frame buffer only
    Lanes(const char* who, const DeviceSet& ds) : who(who), ds(ds), lane(ds.n) {}
    ~Lanes() {
        for (Lane& l : lane) l.close();
        frame.close();
    }
};

int setup_failed(const std::string& who, const Lane& l) {
    (void)hipGetLastError();
    return fail(CRT_E_HIP, who + ": per-device setup failed on device " + std::to_string(l.device));
}

template <typename T>
int alloc_frame(Lanes& L, T*& frame, size_t bytes) {
    DeviceGuard g(0);
    L.frame.alloc(frame, bytes);
    if (L.frame.ok) return CRT_OK;
    (void)hipGetLastError();
    return fail(CRT_E_HIP, L.who + ": frame buffer");
}

// The lanes of a render in passes: per device its stream, the packed running sums and frame rows,
// the noise state and the zeroed block words as asked for, the event; then the frame on device 0.
int open_pass_lanes(Lanes& L, const crt_camera* cam, bool noise, bool blocks, double*& frame) {
    for (int d = 0; d < L.ds.n; ++d) {
        Lane& l = L.lane[d];
        DeviceGuard g(L.ds.phys(d));
        l.tiling = L.ds.tiling(d);
        l.rows = count_owned(cam->image_h, l.tiling.row_block, l.tiling.tile_count, l.tiling.tile_index);
        l.nblk = static_cast<uint32_t>(crt_block_count(cam->image_w, l.rows));
        l.px = static_cast<size_t>(l.rows) * cam->image_w;
        const size_t px = std::max<size_t>(1, l.px), bb = std::max<size_t>(1, l.nblk) * sizeof(uint32_t);
        l.open(L.ds.phys(d));
        l.alloc(l.sum, px * 3 * sizeof(double));
        l.alloc(l.rgb, px * 3 * sizeof(double));
        if (noise) l.alloc(l.noise, px * 2 * sizeof(double));
        if (blocks) l.alloc(l.blocks, bb);
        if (blocks) l.ok = l.ok && hipMemsetAsync(l.blocks, 0, bb, l.stream) == hipSuccess;
        l.event(l.done);
        l.out = l.rgb;
        if (!l.ok) return setup_failed(L.who, l);
    }
    return alloc_frame(L, frame, std::max<size_t>(1, static_cast<size_t>(cam->image_h) * cam->image_w) * 3 * sizeof(double));
}

int sync_lane(const Lane& l) {
    DeviceGuard g(l.device);
    const hipError_t e = hipStreamSynchronize(l.stream);
    if (e == hipSuccess) return CRT_OK;
    return fail(CRT_E_HIP, std::string("render on device ") + std::to_string(l.device) + ": " + hipGetErrorString(e));
}

// ---- the gather -------------------------------------------------------------------------------
// Peer access from device `to` to device `from`'s memory, enabled once per pair per process
// (hipDeviceEnablePeerAccess fails with AlreadyEnabled on a repeat call; HIP keeps such an error as
// the thread's last error, so it is read off here, not left for a later hipGetLastError).
void enable_peer_once(int to, int from) {
    static std::mutex mu;
    static bool done[kMaxDevices][kMaxDevices] = {};
    std::lock_guard<std::mutex> lk(mu);
    if (done[to][from]) return;
    done[to][from] = true;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, to, from) != hipSuccess || !can) {
        (void)hipGetLastError();
        return;  // the copies still work, staged by the runtime
    }
    DeviceGuard g(to);
    if (hipDeviceEnablePeerAccess(from, 0) != hipSuccess) (void)hipGetLastError();
}

// Device d's owned rows (crt_tiling{rb, n, d}) are packed in its buffer; copy them to their frame
// rows in `dst` (on device 0): full rb-row blocks with one strided copy (rb rows apart in the
// source, n x rb rows apart in the frame), a short last block on its own (row_spans).
// bytes_per_row: one row.
hipError_t gather_packed(char* dst, const char* src, size_t H, size_t rb, int n, int d, size_t bytes_per_row,
                         hipStream_t st) {
    const RowSpans r = row_spans(H, rb, static_cast<size_t>(n), static_cast<size_t>(d));
    hipError_t e = hipSuccess;
    if (r.full)
        e = hipMemcpy2DAsync(dst + r.first * bytes_per_row, r.step * bytes_per_row, src, rb * bytes_per_row,
                             rb * bytes_per_row, r.full, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && r.full < r.blocks)
        e = hipMemcpyAsync(dst + r.last * bytes_per_row, src + r.full * rb * bytes_per_row, (H - r.last) * bytes_per_row,
                           hipMemcpyDeviceToDevice, st);
    return e;
}

// The lanes' rows (Lane::out, row_bytes a row) from lane `first` on into `frame` on device 0: lane
// 0's stream waits for each lane and pulls its row blocks with one strided peer copy; then the
// frame goes to host_dst in one copy. Blocking. first = 1: lane 0 rendered into the frame itself.
// recorded: the lanes' `done` events were recorded behind their renders (render_multi_impl, which
// also times with them); else they are recorded here, and lane 0, whose stream does the copies, is
// not waited for.
int gather_frame(Lanes& L, void* frame, void* host_dst, size_t H, size_t row_bytes, int first = 0, bool recorded = false) {
    DeviceGuard g(0);
    hipStream_t s0 = L.lane[0].stream;
    for (int d = first; d < L.ds.n; ++d) {
        Lane& l = L.lane[d];
        if (!L.ds.emulate && d > 0) enable_peer_once(0, d);
        if (!recorded) {
            DeviceGuard gd(l.device);
            if (hipEventRecord(l.done, l.stream) != hipSuccess) return fail(CRT_E_HIP, L.who + ": event");
        }
        if ((recorded || d > 0) && hipStreamWaitEvent(s0, l.done, 0) != hipSuccess)
            return fail(CRT_E_HIP, L.who + ": gather wait failed");
        const hipError_t e = gather_packed(static_cast<char*>(frame), static_cast<const char*>(l.out), H, L.ds.rb, L.ds.n,
                                           d, row_bytes, s0);
        if (e != hipSuccess)
            return fail(CRT_E_HIP, L.who + ": gather from device " + std::to_string(d) + ": " + hipGetErrorString(e));
    }
    hipError_t e = hipMemcpyAsync(host_dst, frame, H * row_bytes, hipMemcpyDeviceToHost, s0);
    if (e == hipSuccess) e = hipStreamSynchronize(s0);
    if (e != hipSuccess) return fail(CRT_E_HIP, L.who + ": " + hipGetErrorString(e));
    return CRT_OK;
}

// ---- adaptive sampling over lanes ---------------------------------------------------------------
// One step of an adaptive render over n lanes, *done samples in: a masked pass of the next samples on
// every lane that owns rows (with_frame: writing the lanes' frame rows too), then the update on
// every such lane, which synchronizes the lane's stream. A lane's active count is its next pass's
// hint; *active gets the blocks still active on all lanes, *done the samples after the step.
int adaptive_step(const crt_scene* s, const crt_camera* cam, const crt_adaptive_params* prm, Lane* lanes, int n,
                  bool with_frame, uint32_t* done, uint32_t* active) {
    const uint32_t N = cam->samples_per_pixel;
    const uint64_t per_pass = pass_len(N, sample_chunk_len(N), prm->samples_per_pass);
    const uint32_t count = static_cast<uint32_t>(std::min<uint64_t>(per_pass, N - *done));
    int rc = CRT_OK;
    for (int d = 0; d < n && rc == CRT_OK; ++d) {
        Lane& l = lanes[d];
        const RenderPass pass{*done, count, l.sum, l.noise, l.blocks, l.hint};
        if (l.rows) rc = device_render(s, l.device, cam, &l.tiling, with_frame ? l.rgb : nullptr, l.stream, nullptr, &pass);
    }
    if (rc != CRT_OK) return rc;
    *done += count;
    *active = 0;
    for (int d = 0; d < n && rc == CRT_OK; ++d) {
        Lane& l = lanes[d];
        if (!l.rows) continue;
        uint32_t a = 0;
        rc = device_adaptive_update(l.device, cam, &l.tiling, l.noise, l.blocks, *done, prm->threshold, prm->min_samples, &a,
                                    l.stream);
        l.hint = std::max(1u, a);
        *active += a;
    }
    return rc;
}

// The lanes' block words read back: h_block_samples (may be null) gets the frame's block counts in
// frame order (owned_to_frame_block_row), *rendered the samples they stand for. A lane's words come
// by a blocking copy, or with on_stream by a copy on the lane's stream, which is then synchronized.
int block_samples(const std::string& who, Lane* lanes, int n, size_t W, bool on_stream, uint32_t* h_block_samples,
                  uint64_t* rendered) {
    const size_t tiles_x = (W + CRT_BLOCK_W - 1) / CRT_BLOCK_W;
    std::vector<uint32_t> hb;
    *rendered = 0;
    for (int d = 0; d < n; ++d) {
        const Lane& l = lanes[d];
        if (!l.nblk) continue;
        DeviceGuard g(l.device);
        hb.resize(l.nblk);
        const size_t bytes = l.nblk * sizeof(uint32_t);
        hipError_t e = on_stream ? hipMemcpyAsync(hb.data(), l.blocks, bytes, hipMemcpyDeviceToHost, l.stream)
                                 : hipMemcpy(hb.data(), l.blocks, bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess && on_stream) e = hipStreamSynchronize(l.stream);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(CRT_E_HIP, who + ": block state copy");
        }
        const crt_tiling& t = l.tiling;
        for (size_t j = 0; j * CRT_BLOCK_H < l.rows; ++j) {
            const size_t fy = owned_to_frame_block_row(j, CRT_BLOCK_H, t.row_block, t.tile_count, t.tile_index);
            const uint64_t bh = std::min<uint64_t>(CRT_BLOCK_H, l.rows - j * CRT_BLOCK_H);
            for (size_t bx = 0; bx < tiles_x; ++bx) {
                const uint32_t cnt = hb[j * tiles_x + bx] & ~CRT_BLOCK_STOPPED;
                if (h_block_samples) h_block_samples[fy * tiles_x + bx] = cnt;
                *rendered += cnt * bh * std::min<uint64_t>(CRT_BLOCK_W, W - bx * CRT_BLOCK_W);
            }
        }
    }
    return CRT_OK;
}

// ---- crt_render / crt_render_ppm ------------------------------------------------------------------
// The whole frame over devices [0, n): the scene is uploaded to every device concurrently
// (open_devices); each device renders its own rows only, packed (CRT_TILING_PACKED: a device holds
// its share of the frame, 1/n of it) on its own stream; device 0's stream then waits for each
// device and pulls that device's row blocks into the frame with ONE strided peer copy
// (hipMemcpy2DAsync over xGMI), and the assembled frame crosses PCIe once (gather_frame). Frames
// are bit-identical for any n (per-sample RNG, spp-only sample chunks).
//   h_rgb (f64 frame, crt_render): 24 B a pixel cross xGMI and PCIe; device 0 renders straight
//     into the frame.
//   h_ppm (int32 PPM values, crt_render_ppm; image.h:38-56, rgb.h:90-115): every device converts
//     its rows to 8-bit PPM values before the gather (device_ppm8), so 3 B a pixel cross xGMI and
//     PCIe; the few pixels the kernel leaves to the host (NaN, out of range, or within 2 ulps of
//     an integer step) are recomputed from their f64 values with std::pow (ppm_pixel_host).
int render_multi_impl(crt_scene* s, const crt_camera* cam, int num_devices, double* h_rgb, int32_t* h_ppm,
                      crt_render_stats* stats) {
    DeviceSet ds;
    int rc = open_devices(s, num_devices, ds);
    if (rc) return rc;
    const int n = ds.n;
    const bool ppm = h_ppm != nullptr;
    const size_t W = cam->image_w, H = cam->image_h;
    // render: each logical device its own rows on its own stream (f64 mode: device 0 into the
    // whole frame, the others packed; ppm mode: every device packed, then to 8-bit values)
    Lanes L("render", ds);
    std::vector<uint8_t*> b8(n, nullptr);
    std::vector<uint32_t*> redo(n, nullptr);  // [count, indices...] per device (ppm mode)
    constexpr uint32_t kRedoCap = 1u << 16;
    for (int d = 0; d < n && rc == CRT_OK; ++d) {
        Lane& l = L.lane[d];
        DeviceGuard g(ds.phys(d));
        const bool packed = ppm || d > 0;
        l.tiling = ds.tiling(d, packed);
        l.rows = count_owned(cam->image_h, ds.rb, static_cast<uint32_t>(n), static_cast<uint32_t>(d));
        l.px = (packed ? l.rows : H) * W;
        l.open(ds.phys(d));
        l.alloc(l.rgb, std::max<size_t>(1, l.px) * 3 * sizeof(double));
        if (ppm) l.alloc(b8[d], std::max<size_t>(1, l.px) * 3);
        if (ppm) l.alloc(redo[d], (1 + kRedoCap) * sizeof(uint32_t));
        l.event(l.start);
        l.event(l.done);
        if (!l.ok) return setup_failed(L.who, l);
        l.out = ppm ? static_cast<const void*>(b8[d]) : l.rgb;
        (void)hipEventRecord(l.start, l.stream);
        rc = device_render(s, l.device, cam, &l.tiling, l.rgb, l.stream, nullptr);
        if (rc == CRT_OK && ppm && l.px) {
            if (hipMemsetAsync(redo[d], 0, sizeof(uint32_t), l.stream) != hipSuccess)
                return fail(CRT_E_HIP, "render: redo counter");
            if (!device_ppm8(l.rgb, l.px, b8[d], redo[d], kRedoCap, l.stream))
                rc = fail(CRT_E_HIP, "render: ppm8_kernel launch");
        }
        (void)hipEventRecord(l.done, l.stream);
    }
    // gather into device 0 (the events are recorded), then one device-to-host copy
    std::vector<uint8_t> h8(ppm ? H * W * 3 : 0);
    uint8_t* frame8 = nullptr;
    if (rc == CRT_OK && ppm) rc = alloc_frame(L, frame8, std::max<size_t>(1, H * W * 3));
    if (rc == CRT_OK)
        rc = ppm ? gather_frame(L, frame8, h8.data(), H, W * 3, 0, true)
                 : gather_frame(L, L.lane[0].rgb, h_rgb, H, W * 3 * sizeof(double), 1, true);
    float max_ms = 0;
    for (Lane& l : L.lane) {
        if (!l.stream) continue;
        const int src = sync_lane(l);
        if (rc == CRT_OK) rc = src;
        float ms = 0;
        if (rc == CRT_OK && hipEventElapsedTime(&ms, l.start, l.done) == hipSuccess) max_ms = std::max(max_ms, ms);
    }
    // ppm mode: 8-bit values to int32, and the pixels each device left to the host
    if (rc == CRT_OK && ppm) {
        for (size_t i = 0; i < H * W * 3; ++i) h_ppm[i] = h8[i];
        for (int d = 0; d < n && rc == CRT_OK; ++d) {
            const Lane& l = L.lane[d];
            if (!l.rows) continue;
            DeviceGuard g(l.device);
            uint32_t cnt = 0;
            if (hipMemcpy(&cnt, redo[d], sizeof cnt, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(CRT_E_HIP, "render: redo count");
            if (!cnt) continue;
            const bool whole = cnt > kRedoCap;  // more than the list holds: every pixel of the device
            const size_t m = whole ? l.px : cnt;
            std::vector<uint32_t> idx(whole ? 0 : cnt);
            std::vector<double> rgb(3 * m);
            double* packed = nullptr;
            // the listed pixels are gathered on the device, then come in one copy (not one per pixel)
            const bool ok =
                whole ? hipMemcpy(rgb.data(), l.rgb, 3 * m * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess
                      : hipMemcpy(idx.data(), redo[d] + 1, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess &&
                            hipMalloc(&packed, 3 * m * sizeof(double)) == hipSuccess &&
                            device_redo_gather(l.rgb, redo[d] + 1, cnt, packed, nullptr) &&
                            hipMemcpy(rgb.data(), packed, 3 * m * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
            if (packed) (void)hipFree(packed);
            if (!ok) rc = fail(CRT_E_HIP, "render: redo pixels");
            for (size_t j = 0; j < m && ok; ++j) {
                const size_t k = whole ? j : idx[j];  // packed pixel index on device d
                const size_t row = owned_to_frame_row(k / W, ds.rb, n, d), col = k % W;
                ppm_pixel_host(rgb.data() + 3 * j, h_ppm + 3 * (row * W + col));
            }
        }
    }
    if (stats && rc == CRT_OK) {
        *stats = crt_render_stats{};
        stats->samples = static_cast<uint64_t>(cam->image_w) * cam->image_h * cam->samples_per_pixel;
        stats->kernel_ms = max_ms;
    }
    return rc;
}

}  // namespace

int render_multi(crt_scene* s, const crt_camera* cam, int num_devices, double* h_rgb, crt_render_stats* stats) {
    return render_multi_impl(s, cam, num_devices, h_rgb, nullptr, stats);
}

int render_multi_ppm(crt_scene* s, const crt_camera* cam, int num_devices, int32_t* h_values, crt_render_stats* stats) {
    return render_multi_impl(s, cam, num_devices, nullptr, h_values, stats);
}

// crt_render_progressive: render_multi_impl's layout (rows dealt in 4-row blocks, one stream per
// logical device, the gather into device 0, CRT_EMULATE_DEVICES) with the samples cut into passes.
// Every device keeps its packed running sums (and noise state) for the whole job and renders each
// pass into them (device_render with a RenderPass); a frame is resolved and gathered only when
// somebody looks at it: after every pass with CRT_PROGRESS_PREVIEW, else once at the end or when
// the callback stops the job. A pixel's samples stay on one device, in order, so the final frame
// is crt_render's bit for bit.
int render_progressive(crt_scene* s, const crt_camera* cam, int num_devices, uint32_t samples_per_pass,
                       uint32_t flags, crt_progress_fn fn, void* user, double* h_rgb, uint32_t* samples_done) {
    DeviceSet ds;
    int rc = open_devices(s, num_devices, ds);
    if (rc) return rc;
    const uint32_t N = cam->samples_per_pixel;
    const size_t H = cam->image_h, row_bytes = static_cast<size_t>(cam->image_w) * 3 * sizeof(double);
    const bool want_noise = (flags & CRT_PROGRESS_NOISE) != 0, want_preview = (flags & CRT_PROGRESS_PREVIEW) != 0;
    const uint64_t per_pass = pass_len(N, sample_chunk_len(N), samples_per_pass);
    Lanes L("progressive render", ds);
    double* frame = nullptr;
    rc = open_pass_lanes(L, cam, want_noise, false, frame);
    uint32_t done = 0;
    bool have_frame = false;
    while (rc == CRT_OK && done < N) {
        const uint32_t count = static_cast<uint32_t>(std::min<uint64_t>(per_pass, N - done));
        have_frame = done + count == N || (want_preview && fn);  // the last pass, or a preview
        for (Lane& l : L.lane) {
            const RenderPass pass{done, count, l.sum, l.noise};
            if (rc == CRT_OK) rc = device_render(s, l.device, cam, &l.tiling, have_frame ? l.rgb : nullptr, l.stream, nullptr, &pass);
        }
        if (rc != CRT_OK) break;
        done += count;
        double figure = std::numeric_limits<double>::quiet_NaN();
        if (want_noise && fn) {  // sum se / sum m over the devices' pixels, in device order
            double se = 0, mean = 0;
            bool any = false;
            for (const Lane& l : L.lane) {
                if (!l.px || rc != CRT_OK) continue;
                double a = 0, b = 0;
                rc = device_noise_estimate(l.device, l.noise, l.px, N, done, &a, &b, l.stream);
                se += a;
                mean += b;
                any = true;
            }
            if (rc != CRT_OK) break;
            if (any) figure = se / mean;
        }
        if (have_frame) {
            rc = gather_frame(L, frame, h_rgb, H, row_bytes);
        } else {
            for (const Lane& l : L.lane)
                if (rc == CRT_OK) rc = sync_lane(l);
        }
        if (rc != CRT_OK) break;
        if (fn && fn(user, done, N, figure, want_preview ? h_rgb : nullptr) != 0) break;
    }
    // stopped between previews: the mean of the samples so far from the running sums
    if (rc == CRT_OK && !have_frame && done > 0) {
        for (const Lane& l : L.lane) {
            if (!l.px || rc != CRT_OK) continue;
            DeviceGuard g(l.device);
            if (!device_scale(l.sum, l.rgb, static_cast<uint64_t>(l.px) * 3, 1 / static_cast<double>(done), l.stream))
                rc = fail(CRT_E_HIP, "progressive render: scale_kernel launch");
        }
        if (rc == CRT_OK) rc = gather_frame(L, frame, h_rgb, H, row_bytes);
    }
    if (samples_done) *samples_done = done;
    return rc;
}

// crt_render_adaptive: render_progressive's layout (rows dealt in 4-row blocks, so a device's
// blocks are blocks of the frame; packed running sums and noise state per device; the gather into
// device 0; CRT_EMULATE_DEVICES) with a block state per device: every step is one masked pass and
// one update on every device (adaptive_step). The frame is each block's sum times 1 / its own
// count: written by the masked passes with CRT_PROGRESS_PREVIEW, else once at the end
// (device_frame_from_sums).
int render_adaptive(crt_scene* s, const crt_camera* cam, int num_devices, const crt_adaptive_params* prm,
                    crt_adaptive_fn fn, void* user, double* h_rgb, uint32_t* h_block_samples,
                    uint64_t* samples_rendered) {
    DeviceSet ds;
    int rc = open_devices(s, num_devices, ds);
    if (rc) return rc;
    const uint32_t N = cam->samples_per_pixel;
    const size_t H = cam->image_h, row_bytes = static_cast<size_t>(cam->image_w) * 3 * sizeof(double);
    const bool want_preview = (prm->flags & CRT_PROGRESS_PREVIEW) != 0;
    const uint32_t total_blocks = static_cast<uint32_t>(crt_block_count(cam->image_w, cam->image_h));
    Lanes L("adaptive render", ds);
    double* frame = nullptr;
    rc = open_pass_lanes(L, cam, true, true, frame);
    uint32_t done = 0;
    bool have_frame = false;
    while (rc == CRT_OK && done < N) {
        have_frame = want_preview && fn;
        uint32_t active = 0;
        rc = adaptive_step(s, cam, prm, L.lane.data(), ds.n, have_frame, &done, &active);
        if (rc == CRT_OK && have_frame) rc = gather_frame(L, frame, h_rgb, H, row_bytes);
        if (rc != CRT_OK) break;
        if (fn && fn(user, done, N, active, total_blocks, want_preview ? h_rgb : nullptr) != 0) break;
        if (active == 0) break;
    }
    // ended between previews: every block's sum times 1 / its own count
    if (rc == CRT_OK && !have_frame) {
        for (const Lane& l : L.lane) {
            if (!l.rows || rc != CRT_OK) continue;
            DeviceGuard g(l.device);
            rc = device_frame_from_sums(cam, &l.tiling, l.sum, l.blocks, l.rgb, l.stream);
        }
        if (rc == CRT_OK) rc = gather_frame(L, frame, h_rgb, H, row_bytes);
    }
    uint64_t rendered = 0;
    if (rc == CRT_OK) rc = block_samples(L.who, L.lane.data(), ds.n, cam->image_w, false, h_block_samples, &rendered);
    if (samples_rendered) *samples_rendered = rendered;
    return rc;
}

// crt_render_denoised: one device, one stream. The passes (one plain pass of all samples, or
// render_adaptive's steps over one lane, the frame written by every masked pass), then features,
// variance and filter behind them on the same stream, and the two frames copied back.
int render_denoised(crt_scene* s, int device, const crt_camera* cam, const crt_adaptive_params* adaptive,
                    const crt_denoise_params* denoise, double* h_noisy, double* h_rgb, uint64_t* samples_rendered) {
    const std::string who = "denoised render";
    int rc = device_upload(s, device);
    if (rc) return rc;
    DeviceGuard g(device);
    const uint32_t N = cam->samples_per_pixel;
    Lane l;  // the whole frame: no tiling
    l.rows = cam->image_h;
    l.nblk = static_cast<uint32_t>(crt_block_count(cam->image_w, cam->image_h));
    const size_t px = l.px = static_cast<size_t>(cam->image_w) * cam->image_h;
    double *var = nullptr, *out = nullptr;
    crt_feature* feat = nullptr;
    l.open(device);
    l.alloc(l.sum, px * 3 * sizeof(double));
    l.alloc(l.noise, px * 2 * sizeof(double));
    l.alloc(l.rgb, px * 3 * sizeof(double));
    l.alloc(var, px * sizeof(double));
    l.alloc(out, px * 3 * sizeof(double));
    l.alloc(feat, px * sizeof(crt_feature));
    l.alloc(l.blocks, l.nblk * sizeof(uint32_t));
    l.ok = l.ok && hipMemsetAsync(l.blocks, 0, l.nblk * sizeof(uint32_t), l.stream) == hipSuccess;
    if (!l.ok) return setup_failed(who, l);
    uint32_t done = adaptive ? 0 : N, active = 1;
    if (!adaptive) {
        const RenderPass pass{0, N, l.sum, l.noise};
        rc = device_render(s, device, cam, nullptr, l.rgb, l.stream, nullptr, &pass);
    }
    while (rc == CRT_OK && active && done < N) rc = adaptive_step(s, cam, adaptive, &l, 1, true, &done, &active);
    if (rc == CRT_OK) rc = device_render_features(s, device, cam, nullptr, feat, l.stream);
    if (rc == CRT_OK) rc = device_pixel_variance(device, cam, nullptr, l.noise, adaptive ? l.blocks : nullptr, done, var, l.stream);
    if (rc == CRT_OK) rc = device_denoise(device, cam->image_w, cam->image_h, l.rgb, var, feat, denoise, out, nullptr, l.stream);
    uint64_t rendered = 0;
    if (rc == CRT_OK) {
        hipError_t e = hipMemcpyAsync(h_rgb, out, px * 3 * sizeof(double), hipMemcpyDeviceToHost, l.stream);
        if (e == hipSuccess && h_noisy) e = hipMemcpyAsync(h_noisy, l.rgb, px * 3 * sizeof(double), hipMemcpyDeviceToHost, l.stream);
        if (e == hipSuccess && !adaptive) e = hipStreamSynchronize(l.stream);
        if (e != hipSuccess) rc = fail(CRT_E_HIP, who + ": " + hipGetErrorString(e));
        // the block words' copy goes behind the frames' and synchronizes the stream for all three
        else if (adaptive) rc = block_samples(who, &l, 1, cam->image_w, true, nullptr, &rendered);
        else rendered = static_cast<uint64_t>(done) * px;
    }
    if (samples_rendered) *samples_rendered = rendered;
    return rc;
}

// crt_render_denoised_devices: render_adaptive's layout and steps (or one plain pass) over the
// lanes, and the denoiser behind them. Every lane keeps, beside its pass buffers, the variance of
// its pixels and their filter records (crt_denoise.hip: state 32 B, guide 64 B a pixel), packed
// over its owned rows: the guide once per render (features depend on camera and scene only), the
// state per denoised frame. Device 0 holds the whole-frame records, the unfiltered frame and the
// output: lane 0's stream waits for each lane (gather_frame's event scheme), pulls record and frame
// rows to their frame rows (gather_packed), runs the filter stage and copies both frames back.
// Everything is allocated with hipMalloc before the first pass; the calls take their scratch from
// the pass pool. CRT_DENOISE_TIMING=1 (tools/denoise_gain.py) prints every denoised frame's cost to
// stderr: host clock from the end of the pass to both frames on the host, and its split by events
// on lane 0's stream.
int render_denoised_devices(crt_scene* s, const crt_camera* cam, int num_devices, const crt_adaptive_params* adaptive,
                            const crt_denoise_params* denoise, crt_denoised_fn fn, void* user, double* h_noisy,
                            double* h_rgb, uint32_t* h_block_samples, uint64_t* samples_rendered) {
    DeviceSet ds;
    int rc = open_devices(s, num_devices, ds);
    if (rc) return rc;
    const uint32_t N = cam->samples_per_pixel;
    const size_t W = cam->image_w, H = cam->image_h, px = W * H;
    const bool want_preview = adaptive && (adaptive->flags & CRT_PROGRESS_PREVIEW) != 0 && fn;
    const uint32_t total_blocks = static_cast<uint32_t>(crt_block_count(cam->image_w, cam->image_h));
    Lanes L("denoised render", ds);
    double* frame = nullptr;
    rc = open_pass_lanes(L, cam, true, adaptive != nullptr, frame);
    if (rc) return rc;
    // the denoiser's buffers: a lane's share on its device, the whole frame's on device 0
    struct Share {
        double* var = nullptr;
        crt_feature* feat = nullptr;
        char *state = nullptr, *guide = nullptr;
    };
    std::vector<Share> share(ds.n);
    for (int d = 0; d < ds.n; ++d) {
        Lane& l = L.lane[d];
        if (!l.rows) continue;
        DeviceGuard g(l.device);
        l.alloc(share[d].var, l.px * sizeof(double));
        l.alloc(share[d].feat, l.px * sizeof(crt_feature));
        l.alloc(share[d].state, l.px * kDenoiseStateBytes);
        l.alloc(share[d].guide, l.px * kDenoiseGuideBytes);
        if (!l.ok) return setup_failed(L.who, l);
    }
    char *guide = nullptr, *state = nullptr, *state_tmp = nullptr;
    double* out = nullptr;
    rc = alloc_frame(L, guide, px * kDenoiseGuideBytes);
    if (rc == CRT_OK) rc = alloc_frame(L, state, px * kDenoiseStateBytes);
    if (rc == CRT_OK) rc = alloc_frame(L, state_tmp, px * kDenoiseStateBytes);
    if (rc == CRT_OK) rc = alloc_frame(L, out, px * 3 * sizeof(double));
    if (rc) return rc;
    hipStream_t s0 = L.lane[0].stream;
    const bool timing = std::getenv("CRT_DENOISE_TIMING") != nullptr;
    hipEvent_t ev[5] = {};
    struct EventsGuard {
        hipEvent_t* ev;
        ~EventsGuard() {
            DeviceGuard g(0);
            for (int i = 0; i < 5; ++i)
                if (ev[i]) (void)hipEventDestroy(ev[i]);
        }
    } events_guard{ev};
    if (timing) {
        DeviceGuard g(0);
        for (hipEvent_t& e : ev)
            if (hipEventCreate(&e) != hipSuccess) return fail(CRT_E_HIP, L.who + ": timing events");
    }
    // the guide records of every lane's rows, once (the first call of the feature pass for a scene
    // and device allocates its primitive table: before the first pass, as every allocation here)
    for (int d = 0; d < ds.n && rc == CRT_OK; ++d) {
        Lane& l = L.lane[d];
        if (!l.rows) continue;
        rc = device_render_features(s, l.device, cam, &l.tiling, share[d].feat, l.stream);
        if (rc == CRT_OK)
            rc = device_denoise_pack(l.device, l.px, nullptr, nullptr, share[d].feat, nullptr, share[d].guide, l.stream);
    }
    bool have_guide = false;
    // The denoised frame of the state after `done` samples, the lanes' frame rows being up to date:
    // both frames on the host when it returns.
    auto denoised_frame = [&](uint32_t done) -> int {
        const auto t0 = std::chrono::steady_clock::now();
        DeviceGuard g0(0);
        auto mark = [&](int i) { return !timing || hipEventRecord(ev[i], s0) == hipSuccess; };
        if (!mark(0)) return fail(CRT_E_HIP, L.who + ": event");
        for (int d = 0; d < ds.n; ++d) {
            Lane& l = L.lane[d];
            if (!l.rows) continue;
            int r = device_pixel_variance(l.device, cam, &l.tiling, l.noise, adaptive ? l.blocks : nullptr, done,
                                          share[d].var, l.stream);
            if (r == CRT_OK)
                r = device_denoise_pack(l.device, l.px, l.rgb, share[d].var, nullptr, share[d].state, nullptr, l.stream);
            if (r) return r;
            if (!ds.emulate && d > 0) enable_peer_once(0, d);
            {
                DeviceGuard gd(l.device);
                if (hipEventRecord(l.done, l.stream) != hipSuccess) return fail(CRT_E_HIP, L.who + ": event");
            }
            if (d > 0 && hipStreamWaitEvent(s0, l.done, 0) != hipSuccess)
                return fail(CRT_E_HIP, L.who + ": gather wait failed");
        }
        if (!mark(1)) return fail(CRT_E_HIP, L.who + ": event");
        for (int d = 0; d < ds.n; ++d) {
            const Lane& l = L.lane[d];
            if (!l.rows) continue;
            hipError_t e = gather_packed(state, share[d].state, H, ds.rb, ds.n, d, W * kDenoiseStateBytes, s0);
            if (e == hipSuccess && !have_guide)
                e = gather_packed(guide, share[d].guide, H, ds.rb, ds.n, d, W * kDenoiseGuideBytes, s0);
            if (e == hipSuccess)
                e = gather_packed(reinterpret_cast<char*>(frame), reinterpret_cast<const char*>(l.rgb), H, ds.rb, ds.n, d,
                                  W * 3 * sizeof(double), s0);
            if (e != hipSuccess)
                return fail(CRT_E_HIP, L.who + ": gather from device " + std::to_string(d) + ": " + hipGetErrorString(e));
        }
        have_guide = true;
        if (!mark(2)) return fail(CRT_E_HIP, L.who + ": event");
        const int r = device_denoise_filter(0, cam->image_w, cam->image_h, state, state_tmp, guide, denoise, out, nullptr, s0);
        if (r) return r;
        if (!mark(3)) return fail(CRT_E_HIP, L.who + ": event");
        hipError_t e = hipMemcpyAsync(h_rgb, out, px * 3 * sizeof(double), hipMemcpyDeviceToHost, s0);
        if (e == hipSuccess && h_noisy) e = hipMemcpyAsync(h_noisy, frame, px * 3 * sizeof(double), hipMemcpyDeviceToHost, s0);
        if (e == hipSuccess && !mark(4)) e = hipErrorUnknown;
        if (e == hipSuccess) e = hipStreamSynchronize(s0);
        if (e != hipSuccess) return fail(CRT_E_HIP, L.who + ": " + hipGetErrorString(e));
        if (timing) {
            const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            float ms[4] = {};
            for (int i = 0; i < 4; ++i) (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]);
            std::fprintf(stderr,
                         "crt_denoise_timing devices=%d emulated=%d done=%u host_ms=%.4f lanes_ms=%.4f gather_ms=%.4f "
                         "filter_ms=%.4f d2h_ms=%.4f\n",
                         ds.n, ds.emulate ? 1 : 0, done, host_ms, ms[0], ms[1], ms[2], ms[3]);
        }
        return CRT_OK;
    };
    uint32_t done = 0, active = 0;
    bool have_frame = false;
    if (!adaptive && rc == CRT_OK) {  // one plain pass, the lanes' frame rows written
        for (Lane& l : L.lane) {
            const RenderPass pass{0, N, l.sum, l.noise};
            if (l.rows && rc == CRT_OK) rc = device_render(s, l.device, cam, &l.tiling, l.rgb, l.stream, nullptr, &pass);
        }
        done = N;
        if (rc == CRT_OK) rc = denoised_frame(done);
        have_frame = true;
        if (rc == CRT_OK && fn) (void)fn(user, done, N, 0, total_blocks, nullptr, nullptr);
    }
    while (adaptive && rc == CRT_OK && done < N) {  // render_adaptive's loop
        have_frame = want_preview;
        rc = adaptive_step(s, cam, adaptive, L.lane.data(), ds.n, have_frame, &done, &active);
        if (rc == CRT_OK && have_frame) rc = denoised_frame(done);
        if (rc != CRT_OK) break;
        if (fn && fn(user, done, N, active, total_blocks, have_frame ? h_noisy : nullptr, have_frame ? h_rgb : nullptr) != 0)
            break;
        if (active == 0) break;
    }
    // ended between previews: every block's sum times 1 / its own count, then the denoiser
    if (rc == CRT_OK && !have_frame) {
        for (const Lane& l : L.lane) {
            if (!l.rows || rc != CRT_OK) continue;
            DeviceGuard g(l.device);
            rc = device_frame_from_sums(cam, &l.tiling, l.sum, l.blocks, l.rgb, l.stream);
        }
        if (rc == CRT_OK) rc = denoised_frame(done);
    }
    uint64_t rendered = 0;
    if (rc == CRT_OK && adaptive) {
        rc = block_samples(L.who, L.lane.data(), ds.n, cam->image_w, false, h_block_samples, &rendered);
    } else if (rc == CRT_OK) {
        rendered = static_cast<uint64_t>(done) * px;
        if (h_block_samples) std::fill(h_block_samples, h_block_samples + total_blocks, done);
    }
    if (samples_rendered) *samples_rendered = rendered;
    return rc;
}

// crt_render_lens_passes: render_adaptive's loop on one device and one stream, over the whole frame,
// with the lens pass (crt_lens.hip) in place of the masked pass; the update, the variance and the
// filter are the reference camera's, unchanged. Every pass writes the lane's frame (a skipped block's
// pixels included), so the frame is current whenever the loop ends. With `denoise` the features are
// taken once, before the first pass, and a CUBE frame is filtered one face at a time.
// The lighting of crt_render_lens_passes_lit, made once before the first pass and freed with the
// call: the environment's texels uploaded (blocking), a sampler on them, a sampler of the lights.
namespace {
struct CallLighting {
    double* texels = nullptr;
    crt_env env{};
    bool have_env = false;
    crt_env_sampler* smp = nullptr;
    crt_light_sampler* lights = nullptr;
    int make(crt_scene* s, int device, const crt_env* host_env, bool importance, bool want_lights) {
        if (host_env) {
            const size_t bytes = size_t{6} * host_env->face_size * host_env->face_size * 3 * sizeof(double);
            env = *host_env;
            HIP_TRY(hipMalloc(&texels, bytes));
            HIP_TRY(hipMemcpy(texels, host_env->texels, bytes, hipMemcpyHostToDevice));
            env.texels = texels;
            have_env = true;
            if (importance) {
                const int rc = device_env_sampler_create(device, &env, &smp);
                if (rc) return rc;
            }
        }
        return want_lights ? device_light_sampler_create(s, device, &lights) : CRT_OK;
    }
    ~CallLighting() {
        (void)device_env_sampler_free(smp);
        (void)device_light_sampler_free(lights);
        (void)hipFree(texels);
    }
};
}  // namespace

int render_lens_passes(crt_scene* s, int device, const crt_camera* cam, const crt_lens* lens,
                       const crt_adaptive_params* adaptive, const crt_denoise_params* denoise, crt_denoised_fn fn,
                       void* user, double* h_noisy, double* h_rgb, uint32_t* h_block_samples, uint64_t* samples_rendered,
                       const crt_env* env, bool importance, bool lights) {
    const std::string who = "lens passes";
    int rc = device_upload(s, device);
    if (rc) return rc;
    DeviceGuard g(device);
    CallLighting lit;  // declared before the lane: freed after the lane's stream has been drained
    rc = lit.make(s, device, env, importance, lights);
    if (rc) return rc;
    const uint32_t N = cam->samples_per_pixel, W = cam->image_w, H = cam->image_h;
    const uint64_t per_pass = pass_len(N, sample_chunk_len(N), adaptive ? adaptive->samples_per_pass : 0);
    const bool want_preview = adaptive && (adaptive->flags & CRT_PROGRESS_PREVIEW) != 0 && fn;
    Lane l;  // the whole frame: no tiling
    l.rows = H;
    l.nblk = static_cast<uint32_t>(crt_block_count(W, H));
    const size_t px = l.px = static_cast<size_t>(W) * H;
    double *var = nullptr, *out = nullptr;
    crt_feature* feat = nullptr;
    l.open(device);
    l.alloc(l.sum, px * 3 * sizeof(double));
    l.alloc(l.noise, px * 2 * sizeof(double));
    l.alloc(l.rgb, px * 3 * sizeof(double));
    if (denoise) {
        l.alloc(var, px * sizeof(double));
        l.alloc(out, px * 3 * sizeof(double));
        l.alloc(feat, px * sizeof(crt_feature));
    }
    if (adaptive) {
        l.alloc(l.blocks, l.nblk * sizeof(uint32_t));
        l.ok = l.ok && hipMemsetAsync(l.blocks, 0, l.nblk * sizeof(uint32_t), l.stream) == hipSuccess;
    }
    if (!l.ok) return setup_failed(who, l);
    if (denoise) rc = device_lens_features(s, device, cam, lens, feat, l.stream);
    // the frames of the state after `done` samples on the host when it returns
    auto frames = [&](uint32_t done) -> int {
        const double* final_rgb = l.rgb;
        if (denoise) {
            int r = device_pixel_variance(device, cam, nullptr, l.noise, l.blocks, done, var, l.stream);
            const uint32_t faces = lens->kind == CRT_LENS_CUBE ? 6 : 1, fh = H / faces;
            const size_t fpx = static_cast<size_t>(W) * fh;
            for (uint32_t f = 0; f < faces && r == CRT_OK; ++f)
                r = device_denoise(device, W, fh, l.rgb + f * fpx * 3, var + f * fpx, feat + f * fpx, denoise,
                                   out + f * fpx * 3, nullptr, l.stream);
            if (r) return r;
            final_rgb = out;
        }
        hipError_t e = hipMemcpyAsync(h_rgb, final_rgb, px * 3 * sizeof(double), hipMemcpyDeviceToHost, l.stream);
        if (e == hipSuccess && h_noisy) e = hipMemcpyAsync(h_noisy, l.rgb, px * 3 * sizeof(double), hipMemcpyDeviceToHost, l.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(l.stream);
        if (e != hipSuccess) return fail(CRT_E_HIP, who + ": " + hipGetErrorString(e));
        return CRT_OK;
    };
    uint32_t done = 0, active = l.nblk;
    bool have_frames = false;
    while (rc == CRT_OK && done < N) {
        const uint32_t count = static_cast<uint32_t>(std::min<uint64_t>(per_pass, N - done));
        rc = device_render_lens_pass(s, device, cam, lens, done, count, l.sum, l.noise, l.rgb, l.blocks, l.stream,
                                     lit.have_env ? &lit.env : nullptr, lit.smp, lit.lights);
        if (rc != CRT_OK) break;
        done += count;
        if (adaptive)
            rc = device_adaptive_update(device, cam, nullptr, l.noise, l.blocks, done, adaptive->threshold,
                                        adaptive->min_samples, &active, l.stream);
        else
            active = done < N ? l.nblk : 0;
        have_frames = want_preview;
        if (rc == CRT_OK) rc = have_frames ? frames(done) : sync_lane(l);
        if (rc != CRT_OK) break;
        if (fn && fn(user, done, N, active, l.nblk, have_frames ? h_noisy : nullptr, have_frames ? h_rgb : nullptr) != 0) break;
        if (active == 0) break;
    }
    if (rc == CRT_OK && !have_frames) rc = frames(done);
    uint64_t rendered = 0;
    if (rc == CRT_OK && adaptive) {
        rc = block_samples(who, &l, 1, W, true, h_block_samples, &rendered);
    } else if (rc == CRT_OK) {
        rendered = static_cast<uint64_t>(done) * px;
        if (h_block_samples) std::fill(h_block_samples, h_block_samples + l.nblk, done);
    }
    if (samples_rendered) *samples_rendered = rendered;
    return rc;
}

}  // namespace crt
