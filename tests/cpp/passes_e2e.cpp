// Renders in passes from a C++ process (no Python, the system's HIP runtime) against crt_render:
// the named scene "config1" at 100 x 56 and 12 spp, three passes of 4, through
// crt_render_progressive and through crt_render_adaptive with min_samples = samples_per_pixel (no
// block stops), four scenes in one process, crt_render before or after the passes. Every frame
// must equal crt_render's bit for bit. From the second render of a process on, passes whose
// scratch came from the default memory pool lost one pass in most tiles here
// (tests/test_gpu_passes_cpp.py).
//   passes_e2e        exit status 0: every frame equal
#include <cstdio>
#include <vector>

#include "crt_render.h"

static int fail(const char* what) {
    std::printf("%s: %s\n", what, crt_last_error());
    return 2;
}

int main() {
    const size_t n = 100 * 56 * 3;
    int bad_frames = 0;
    for (int rep = 0; rep < 4; ++rep) {
        crt_material* m = nullptr;
        crt_object* o = nullptr;
        size_t nm = 0, no = 0;
        crt_camera_settings cs;
        crt_camera cam;
        if (crt_scene_build_named("config1", 0, 0, &m, &nm, &o, &no, &cs)) return fail("crt_scene_build_named");
        cs.image_w = 100;
        cs.image_h = 56;
        cs.samples_per_pixel = 12;
        crt_scene* s = nullptr;
        if (crt_scene_create(m, nm, o, no, nullptr, &s)) return fail("crt_scene_create");
        if (crt_camera_resolve(&cs, &cam)) return fail("crt_camera_resolve");
        cam.base_seed = 7;
        std::vector<double> want(n), prog(n), ad(n);
        if ((rep & 1) && crt_render(s, &cam, 1, want.data(), nullptr)) return fail("crt_render");
        uint32_t done = 0;
        if (crt_render_progressive(s, &cam, 1, 4, 0, nullptr, nullptr, prog.data(), &done)) return fail("crt_render_progressive");
        crt_adaptive_params p{};
        p.min_samples = 12;
        p.samples_per_pass = 4;
        uint64_t rendered = 0;
        if (crt_render_adaptive(s, &cam, 1, &p, nullptr, nullptr, ad.data(), nullptr, &rendered)) return fail("crt_render_adaptive");
        if (!(rep & 1) && crt_render(s, &cam, 1, want.data(), nullptr)) return fail("crt_render");
        size_t bad_p = 0, bad_a = 0;
        for (size_t i = 0; i < n; ++i) {
            bad_p += prog[i] != want[i];
            bad_a += ad[i] != want[i];
        }
        std::printf("scene %d: progressive %u of 12 spp, %zu of %zu values differ from crt_render; adaptive %llu samples, %zu differ\n",
                    rep, done, bad_p, n, static_cast<unsigned long long>(rendered), bad_a);
        bad_frames += (bad_p != 0) + (bad_a != 0) + (done != 12) + (rendered != 12ull * 100 * 56);
        crt_scene_destroy(s);
        crt_free(m);
        crt_free(o);
    }
    return bad_frames ? 1 : 0;
}
