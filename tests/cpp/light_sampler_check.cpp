// csrc/crt_light_sampler.h's weights, light_pick, light_weight, light_point and light_pdf, the lines the
// sampler's build and the lights instances of the radiance kernels run, built for the host
// (-ffp-contract=off) behind C functions: tests/test_light_nee_model.py holds them to
// tests/light_nee_model.py's restatement bit for bit. The tables' sum here is the build's loop:
// sequential, from 0.0; e = color * param is material_record's expression.
#include "crt_light_sampler.h"

// per light: kind (1 sphere, 2 parallelogram), geom 9 doubles (sphere: c, r; parallelogram: v, s1, s2),
// colour 3 doubles, param
extern "C" void light_tables_host(const uint32_t* kind, const double* geom, const double* color, const double* param,
                                  uint32_t L, double* w, double* cdf) {
    double sum = 0.0;
    for (uint32_t i = 0; i < L; ++i) {
        const double* g = geom + 9 * i;
        const double e[3] = {color[3 * i] * param[i], color[3 * i + 1] * param[i], color[3 * i + 2] * param[i]};
        const double A = kind[i] == 2 ? crt::light_area_quad(g + 3, g + 6) : crt::light_area_sphere(g[3]);
        w[i] = crt::light_luminance(e) * A;
        sum = sum + w[i];
        cdf[i] = sum;
    }
}

extern "C" void light_pick_many(const double* cdf, uint32_t L, double W, const double* xi, size_t count, uint32_t* out) {
    const crt::LightTables tb{nullptr, cdf, nullptr, nullptr, W, L};
    for (size_t i = 0; i < count; ++i) out[i] = crt::light_pick(tb, xi[i]);
}

extern "C" void light_weight_many(const uint32_t* sref, const double* sw, uint32_t L, const uint32_t* refs, size_t count,
                                  double* out) {
    const crt::LightTables tb{nullptr, nullptr, sref, sw, 0.0, L};
    for (size_t i = 0; i < count; ++i) out[i] = crt::light_weight(tb, refs[i]);
}

extern "C" void light_point_quad_many(const double* geom, const double* xi, size_t count, double* out) {
    for (size_t i = 0; i < count; ++i) crt::light_point(geom, geom + 3, geom + 6, xi[2 * i], xi[2 * i + 1], out + 3 * i);
}

extern "C" void light_point_sphere_many(const double* geom, const double* u, size_t count, double* out) {
    for (size_t i = 0; i < count; ++i) crt::light_point(geom, geom[3], u + 3 * i, out + 3 * i);
}

// per hit: t, n (3), d (3), outside
extern "C" void light_pdf_many(double w, double W, double A, const double* t, const double* n, const double* d,
                               const uint8_t* outside, size_t count, double* out) {
    for (size_t i = 0; i < count; ++i) out[i] = crt::light_pdf(w, W, A, t[i], n + 3 * i, d + 3 * i, outside[i] != 0);
}
