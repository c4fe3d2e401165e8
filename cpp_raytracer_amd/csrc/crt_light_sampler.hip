// Build of a crt_light_sampler's tables (include/crt_render.h states every expression and its order;
// crt_light_sampler.h holds the per-light ones). Not a hot path: the device copy's own records (slot
// references, spheres, parallelograms and per-slot materials, the bits the kernels read) come to the
// host, the sequential sums run there, and the tables go up in one allocation.
#include <hip/hip_runtime.h>

#define CRT_HD __host__ __device__ __forceinline__

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "crt_internal.h"
#include "crt_hip_util.h"
#include "crt_light_sampler.h"

#pragma clang fp contract(off)

namespace crt {

int device_light_sampler_free(crt_light_sampler* smp) {
    if (!smp) return CRT_OK;
    if (smp->w) {
        DeviceGuard g(smp->device);
        (void)hipFree(smp->w);  // the six tables are one allocation
    }
    delete smp;
    return CRT_OK;
}

int device_light_sampler_create(const crt_scene* s, int device, crt_light_sampler** out) {
    const std::string who = "crt_light_sampler_create: ";
    const int rc = device_check(device);
    if (rc) return rc;
    const DeviceCopy& c = s->dev[device];
    if (!c.valid) return fail(CRT_E_INVALID, who + "the scene is not resident on device " + std::to_string(device));
    DeviceGuard g(device);
    const size_t np = s->num_prims, nsp = s->num_spheres, nq = s->num_quads;
    std::vector<uint32_t> refs(np);
    std::vector<DevSphere> spheres(nsp);
    std::vector<DevQuad> quads(nq);
    std::vector<DevMaterial> smat(nsp), qmat(nq);
    if (np) HIP_TRY(hipMemcpy(refs.data(), c.refs, np * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (nsp) {
        HIP_TRY(hipMemcpy(spheres.data(), c.spheres, nsp * sizeof(DevSphere), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(smat.data(), c.sphere_mrec, nsp * sizeof(DevMaterial), hipMemcpyDeviceToHost));
    }
    if (nq) {
        HIP_TRY(hipMemcpy(quads.data(), c.quads, nq * sizeof(DevQuad), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(qmat.data(), c.quad_mrec, nq * sizeof(DevMaterial), hipMemcpyDeviceToHost));
    }
    struct Light {
        uint32_t prim, ref;
        double w;
    };
    std::vector<Light> lights;
    for (size_t slot = 0; slot < np; ++slot) {
        const uint32_t r = refs[slot], k = r & ~kRefQuad;
        const bool quad = (r & kRefQuad) != 0;
        if (k >= (quad ? nq : nsp)) return fail(CRT_E_INVALID, who + "the device copy holds a slot reference out of range");
        const DevMaterial& m = quad ? qmat[k] : smat[k];
        if (m.kind != CRT_DIFFUSE_LIGHT) continue;
        const double A = quad ? light_area_quad(quads[k].s1, quads[k].s2) : light_area_sphere(spheres[k].r);
        lights.push_back({s->order[slot], r, light_luminance(m.emit) * A});
    }
    if (lights.empty()) return fail(CRT_E_INVALID, who + "the scene has no light (no primitive with a CRT_DIFFUSE_LIGHT material)");
    const size_t L = lights.size();
    std::sort(lights.begin(), lights.end(), [](const Light& a, const Light& b) { return a.prim < b.prim; });
    // one block: w, cdf, sw (doubles), then prim, ref, sref
    std::vector<unsigned char> host(L * (3 * sizeof(double) + 3 * sizeof(uint32_t)));
    double* w = reinterpret_cast<double*>(host.data());
    double *cdf = w + L, *sw = w + 2 * L;
    uint32_t* prim = reinterpret_cast<uint32_t*>(w + 3 * L);
    uint32_t *ref = prim + L, *sref = prim + 2 * L;
    double sum = 0.0;
    for (size_t i = 0; i < L; ++i) {
        prim[i] = lights[i].prim;
        ref[i] = lights[i].ref;
        w[i] = lights[i].w;
        sum = sum + w[i];
        cdf[i] = sum;
    }
    if (!(sum > 0 && sum < INFINITY))
        return fail(CRT_E_INVALID, who + "the lights' total weight W must be positive and finite");
    std::sort(lights.begin(), lights.end(), [](const Light& a, const Light& b) { return a.ref < b.ref; });
    for (size_t i = 0; i < L; ++i) {
        sref[i] = lights[i].ref;
        sw[i] = lights[i].w;
    }
    unsigned char* base = nullptr;
    HIP_TRY(hipMalloc(&base, host.size()));
    const hipError_t e = hipMemcpy(base, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(base);
        return fail(CRT_E_HIP, who + hipGetErrorString(e));
    }
    crt_light_sampler* smp = new crt_light_sampler{};
    smp->scene = s;
    smp->device = device;
    smp->L = static_cast<uint32_t>(L);
    smp->w = reinterpret_cast<double*>(base);
    smp->cdf = smp->w + L;
    smp->sw = smp->w + 2 * L;
    smp->prim = reinterpret_cast<uint32_t*>(smp->w + 3 * L);
    smp->ref = smp->prim + L;
    smp->sref = smp->prim + 2 * L;
    smp->W = sum;
    *out = smp;
    return CRT_OK;
}

}  // namespace crt
