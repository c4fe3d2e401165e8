"""ctypes binding of the C ABI in include/crt_render.h (libcrt_hip.so, built in-tree).

The library is the product: there is no Python or CPU fallback for the render path. Loading
fails loudly if the in-tree .so is missing; rendering fails loudly if no GPU is visible.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
# CRT_LIB selects an alternative in-tree build (benchmarking variants); default is the product.
LIB_PATH = Path(os.environ.get("CRT_LIB", PKG_DIR / "lib" / "libcrt_hip.so"))

CRT_LAMBERTIAN, CRT_METAL, CRT_DIELECTRIC, CRT_DIFFUSE_LIGHT = 1, 2, 3, 4
CRT_SPHERE, CRT_PARALLELOGRAM, CRT_BOX = 1, 2, 3

D3 = C.c_double * 3


class Material(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("reserved", C.c_uint32), ("color", D3), ("param", C.c_double)]


class Object(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("material", C.c_uint32), ("v", C.c_double * 9)]


class BVHParams(C.Structure):
    _fields_ = [("num_buckets", C.c_uint32), ("max_prims_in_node", C.c_uint32),
                ("linear", C.c_uint32), ("build_device", C.c_uint32)]


class CameraSettings(C.Structure):
    _fields_ = [("image_w", C.c_uint32), ("image_h", C.c_uint32),
                ("samples_per_pixel", C.c_uint32), ("max_depth", C.c_uint32),
                ("center", D3), ("direction", D3), ("lookat", D3), ("up", D3),
                ("focus_dist", C.c_double), ("fov", C.c_double), ("defocus_angle", C.c_double),
                ("background", D3),
                ("has_lookat", C.c_uint32), ("has_focus_dist", C.c_uint32),
                ("fov_is_vertical", C.c_uint32), ("reserved", C.c_uint32)]


class Camera(C.Structure):
    _fields_ = [("image_w", C.c_uint32), ("image_h", C.c_uint32),
                ("samples_per_pixel", C.c_uint32), ("max_depth", C.c_uint32),
                ("origin", D3), ("pixel00", D3), ("pixel_delta_x", D3), ("pixel_delta_y", D3),
                ("defocus_disk_x", D3), ("defocus_disk_y", D3),
                ("defocus_angle", C.c_double), ("background", D3), ("t_min", C.c_double),
                ("base_seed", C.c_uint32), ("reserved", C.c_uint32)]


class Tiling(C.Structure):
    _fields_ = [("row_block", C.c_uint32), ("tile_count", C.c_uint32),
                ("tile_index", C.c_uint32), ("flags", C.c_uint32)]


class SceneInfo(C.Structure):
    _fields_ = [("num_objects", C.c_uint64), ("num_materials", C.c_uint64),
                ("num_primitives", C.c_uint64), ("num_spheres", C.c_uint64),
                ("num_parallelograms", C.c_uint64), ("num_nodes", C.c_uint64),
                ("depth", C.c_uint32), ("max_leaf_size", C.c_uint32),
                ("device_bytes", C.c_uint64), ("build_ms", C.c_double)]


class BVHNode(C.Structure):
    _fields_ = [("bounds", C.c_double * 6), ("index", C.c_uint32), ("count", C.c_uint32),
                ("axis", C.c_uint32), ("flags", C.c_uint32)]


class Hit(C.Structure):
    _fields_ = [("t", C.c_double), ("point", D3), ("normal", D3), ("prim", C.c_int32),
                ("front_face", C.c_int32), ("material", C.c_uint32), ("reserved", C.c_uint32)]


class RenderStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays", C.c_uint64), ("nodes_visited", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("parallelogram_tests", C.c_uint64),
                ("kernel_ms", C.c_double), ("ticks_walk", C.c_uint64), ("ticks_leaf", C.c_uint64),
                ("ticks_shade", C.c_uint64), ("ticks_total", C.c_uint64),
                ("wave_iters_walk", C.c_uint64), ("wave_iters_leaf", C.c_uint64),
                ("wave_iters_shade", C.c_uint64), ("ticks_tail", C.c_uint64),
                ("slow_node_tests", C.c_uint64), ("wave_iters_slow", C.c_uint64),
                ("candidate_tests", C.c_uint64), ("wave_iters_candidates", C.c_uint64)]


class AdaptiveParams(C.Structure):
    _fields_ = [("threshold", C.c_double), ("min_samples", C.c_uint32), ("samples_per_pass", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class Feature(C.Structure):
    _fields_ = [("albedo", D3), ("normal", D3), ("point", D3), ("t", C.c_double), ("prim", C.c_int32),
                ("material", C.c_uint32)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("normal_squarings", C.c_uint32), ("sigma_l", C.c_double),
                ("sigma_p", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class TraceParams(C.Structure):
    _fields_ = [("t_min", C.c_double), ("t_max", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


CRT_TRACE_ANY, CRT_TRACE_PLAIN = 1, 2


class RadianceParams(C.Structure):
    _fields_ = [("max_depth", C.c_uint32), ("base_seed", C.c_uint32), ("background", D3), ("t_min", C.c_double),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


CRT_RADIANCE_PLAIN = 1
assert C.sizeof(RadianceParams) == 48


class ProbeParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("max_depth", C.c_uint32), ("base_seed", C.c_uint32), ("mode", C.c_uint32),
                ("background", D3), ("t_min", C.c_double), ("batch_probes", C.c_uint32), ("flags", C.c_uint32)]


CRT_PROBE_SPHERE, CRT_PROBE_HEMISPHERE = 0, 1
CRT_SH_RADIANCE, CRT_SH_IRRADIANCE = 0, 1
assert C.sizeof(ProbeParams) == 56


class Lens(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("flags", C.c_uint32), ("origin", D3), ("right", D3), ("up", D3),
                ("forward", D3), ("extent_x", C.c_double), ("extent_y", C.c_double), ("batch_pixels", C.c_uint64)]


CRT_LENS_PINHOLE, CRT_LENS_ORTHOGRAPHIC, CRT_LENS_EQUIRECT, CRT_LENS_FISHEYE, CRT_LENS_CUBE = 0, 1, 2, 3, 4
assert C.sizeof(Lens) == 128


class EnvView(C.Structure):
    """crt_env: the 88-byte view a call reads (the package's Env keeps the tensor behind it alive)."""
    _fields_ = [("texels", C.c_void_p), ("face_size", C.c_uint32), ("filter", C.c_uint32), ("right", D3), ("up", D3),
                ("forward", D3)]


CRT_ENV_NEAREST, CRT_ENV_BILINEAR = 0, 1
assert C.sizeof(EnvView) == 88


class EnvSamplerView(C.Structure):
    """struct crt_env_sampler_view: the recorded crt_env, the device pointers of the tables and W."""
    _fields_ = [("env", EnvView), ("w", C.c_void_p), ("c", C.c_void_p), ("m", C.c_void_p), ("W", C.c_double)]


assert C.sizeof(EnvSamplerView) == 120


class LightSamplerView(C.Structure):
    """struct crt_light_sampler_view: L, the device pointers of the tables and W."""
    _fields_ = [("num_lights", C.c_uint32), ("device", C.c_int32), ("prim", C.c_void_p), ("ref", C.c_void_p),
                ("sorted_ref", C.c_void_p), ("w", C.c_void_p), ("cdf", C.c_void_p), ("sorted_w", C.c_void_p),
                ("W", C.c_double)]


assert C.sizeof(LightSamplerView) == 64


class LightingView(C.Structure):
    """crt_lighting: a plain environment or a sampler's handle, and a light sampler's handle."""
    _fields_ = [("env", C.POINTER(EnvView)), ("sampler", C.c_void_p), ("lights", C.c_void_p), ("reserved", C.c_uint64)]


assert C.sizeof(LightingView) == 32


class LaunchPlan(C.Structure):
    _fields_ = ([(n, C.c_uint32) for n in ("kernel", "klass", "entry_bytes", "five_waves", "prim_mode", "plain_route",
                                           "depth", "block")] + [("num_nodes", C.c_uint64)] +
                [(n, C.c_uint32) for n in (
                    "stack_bytes", "level", "sentinel", "hbm_stack_levels",
                    "lds_nodes", "lds_refs", "lds_spheres", "lds_quads", "lds_quadf", "lds_sph64", "lds_stack",
                    "bytes_nodes", "bytes_refs", "bytes_spheres", "bytes_quads", "bytes_quadf", "bytes_sph64",
                    "ntop", "all_nodes", "lds_cam", "lds_acc", "lds_inv64", "bytes_cam", "bytes_acc", "bytes_inv64",
                    "total_lds", "budget", "spheres_f32", "quads_f32", "quads_flat", "f32_ok")] +
                [("reserved", C.c_uint32 * 9)])


CRT_PLAN_RENDER, CRT_PLAN_TRACE, CRT_PLAN_RADIANCE = 0, 1, 2
CRT_PLAN_LDS_SCENE, CRT_PLAN_LDS_STACK, CRT_PLAN_HBM_STACK = 0, 1, 2
CRT_PLAN_ABSENT = 0xFFFFFFFF
assert C.sizeof(LaunchPlan) == 200

# numpy views of the same records (for bulk scene I/O)
MATERIAL_DTYPE = np.dtype([("kind", "<u4"), ("reserved", "<u4"), ("color", "<f8", 3), ("param", "<f8")])
OBJECT_DTYPE = np.dtype([("kind", "<u4"), ("material", "<u4"), ("v", "<f8", 9)])
NODE_DTYPE = np.dtype([("bounds", "<f8", 6), ("index", "<u4"), ("count", "<u4"), ("axis", "<u4"),
                       ("flags", "<u4")])
HIT_DTYPE = np.dtype([("t", "<f8"), ("point", "<f8", 3), ("normal", "<f8", 3), ("prim", "<i4"),
                      ("front_face", "<i4"), ("material", "<u4"), ("reserved", "<u4")])
assert MATERIAL_DTYPE.itemsize == C.sizeof(Material) == 40
assert OBJECT_DTYPE.itemsize == C.sizeof(Object) == 80
assert NODE_DTYPE.itemsize == C.sizeof(BVHNode) == 64
assert HIT_DTYPE.itemsize == C.sizeof(Hit)
FEATURE_DTYPE = np.dtype([("albedo", "<f8", 3), ("normal", "<f8", 3), ("point", "<f8", 3), ("t", "<f8"),
                          ("prim", "<i4"), ("material", "<u4")])
assert FEATURE_DTYPE.itemsize == C.sizeof(Feature) == 88

P = C.POINTER
# crt_progress_fn(user, samples_done, samples_total, noise, h_rgb) -> non-zero stops the render
CRT_PROGRESS_NOISE, CRT_PROGRESS_PREVIEW = 1, 2
PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_double, C.c_void_p)
# crt_adaptive_fn(user, samples_done, samples_total, active_blocks, total_blocks, h_rgb)
ADAPTIVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
# crt_denoised_fn(user, samples_done, samples_total, active_blocks, total_blocks, h_noisy, h_rgb)
DENOISED_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
CRT_BLOCK_W, CRT_BLOCK_H, CRT_BLOCK_STOPPED = 16, 4, 0x80000000
EXPORTS = {
    "crt_abi_version": (C.c_int, []),
    "crt_last_error": (C.c_char_p, []),
    "crt_build_info": (C.c_char_p, []),
    "crt_device_count": (C.c_int, [P(C.c_int)]),
    "crt_free": (None, [C.c_void_p]),
    "crt_sample_seed": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "crt_rand_double": (C.c_double, [P(C.c_uint32), C.c_double, C.c_double]),
    "crt_scene_build_named": (C.c_int, [C.c_char_p, C.c_uint32, C.c_int, P(P(Material)), P(C.c_size_t),
                                        P(P(Object)), P(C.c_size_t), P(CameraSettings)]),
    "crt_scene_create": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, P(BVHParams),
                                   P(C.c_void_p)]),
    "crt_scene_info_get": (C.c_int, [C.c_void_p, P(SceneInfo)]),
    "crt_scene_export_bvh": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "crt_scene_upload": (C.c_int, [C.c_void_p, C.c_int]),
    "crt_scene_image": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "crt_scene_destroy": (None, [C.c_void_p]),
    "crt_camera_resolve": (C.c_int, [P(CameraSettings), P(Camera)]),
    "crt_render_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Tiling), C.c_void_p, C.c_void_p]),
    "crt_sample_chunk_len": (C.c_uint32, [C.c_uint32]),
    "crt_render_pass_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Tiling), C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "crt_noise_estimate": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32,
                                     P(C.c_double), P(C.c_double), C.c_void_p]),
    "crt_render_progressive": (C.c_int, [C.c_void_p, P(Camera), C.c_int, C.c_uint32, C.c_uint32, PROGRESS_FN,
                                         C.c_void_p, C.c_void_p, P(C.c_uint32)]),
    "crt_block_count": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "crt_render_pass_masked_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Tiling), C.c_uint32, C.c_uint32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                               C.c_void_p]),
    "crt_adaptive_update": (C.c_int, [C.c_int, P(Camera), P(Tiling), C.c_void_p, C.c_void_p, C.c_uint32,
                                      C.c_double, C.c_uint32, P(C.c_uint32), C.c_void_p]),
    "crt_render_adaptive": (C.c_int, [C.c_void_p, P(Camera), C.c_int, P(AdaptiveParams), ADAPTIVE_FN, C.c_void_p,
                                      C.c_void_p, C.c_void_p, P(C.c_uint64)]),
    "crt_render_features_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Tiling), C.c_void_p, C.c_void_p]),
    "crt_pixel_variance_async": (C.c_int, [C.c_int, P(Camera), P(Tiling), C.c_void_p, C.c_void_p, C.c_uint32,
                                           C.c_void_p, C.c_void_p]),
    "crt_denoise_async": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    P(DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "crt_render_denoised": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(AdaptiveParams), P(DenoiseParams),
                                      C.c_void_p, C.c_void_p, P(C.c_uint64)]),
    "crt_render_denoised_devices": (C.c_int, [C.c_void_p, P(Camera), C.c_int, P(AdaptiveParams), P(DenoiseParams),
                                              DENOISED_FN, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              P(C.c_uint64)]),
    "crt_render_count": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Tiling), P(RenderStats)]),
    "crt_render": (C.c_int, [C.c_void_p, P(Camera), C.c_int, C.c_void_p, P(RenderStats)]),
    "crt_render_ppm": (C.c_int, [C.c_void_p, P(Camera), C.c_int, C.c_void_p, P(RenderStats)]),
    "crt_closest_hits": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_double, C.c_double,
                                   C.c_void_p]),
    "crt_trace_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, P(TraceParams),
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "crt_trace": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, P(TraceParams), C.c_void_p,
                            C.c_void_p]),
    "crt_radiance_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, P(RadianceParams),
                                     C.c_void_p, C.c_void_p]),
    "crt_radiance": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, P(RadianceParams),
                               C.c_void_p]),
    "crt_camera_rays_async": (C.c_int, [C.c_int, P(Camera), P(Tiling), C.c_uint32, C.c_uint32, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "crt_probe_rays_async": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, P(ProbeParams), C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "crt_probes_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, P(ProbeParams),
                                   C.c_void_p, C.c_void_p]),
    "crt_probes": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, P(ProbeParams), C.c_void_p]),
    "crt_sh_eval_async": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32,
                                    C.c_void_p, C.c_void_p]),
    "crt_lens_rays_async": (C.c_int, [C.c_int, P(Camera), P(Lens), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "crt_render_lens_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), C.c_void_p, C.c_void_p]),
    "crt_render_lens": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), C.c_void_p]),
    "crt_radiance_env_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, P(RadianceParams),
                                         P(EnvView), C.c_void_p, C.c_void_p]),
    "crt_probes_env_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, P(ProbeParams),
                                       P(EnvView), C.c_void_p, C.c_void_p]),
    "crt_render_lens_env_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), P(EnvView), C.c_void_p,
                                            C.c_void_p]),
    "crt_render_lens_env": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), P(EnvView), C.c_void_p]),
    "crt_env_sampler_create": (C.c_int, [C.c_int, P(EnvView), P(C.c_void_p)]),
    "crt_env_sampler_free": (C.c_int, [C.c_void_p]),
    "crt_env_sampler_view": (C.c_int, [C.c_void_p, P(EnvSamplerView)]),
    "crt_radiance_env_sampled_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                                 P(RadianceParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "crt_probes_env_sampled_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                               P(ProbeParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "crt_render_lens_env_sampled_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), C.c_void_p, C.c_void_p,
                                                    C.c_void_p]),
    "crt_render_lens_env_sampled": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), P(EnvView), C.c_void_p]),
    "crt_light_sampler_create": (C.c_int, [C.c_void_p, C.c_int, P(C.c_void_p)]),
    "crt_light_sampler_free": (C.c_int, [C.c_void_p]),
    "crt_light_sampler_view": (C.c_int, [C.c_void_p, P(LightSamplerView)]),
    "crt_radiance_lights_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                            P(RadianceParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "crt_probes_lights_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                          P(ProbeParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "crt_render_lens_lights_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    "crt_render_lens_lights": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), C.c_void_p]),
    "crt_render_lens_pass_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), C.c_uint32, C.c_uint32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "crt_lens_centre_rays_async": (C.c_int, [C.c_int, P(Camera), P(Lens), C.c_void_p, C.c_void_p]),
    "crt_lens_features_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), C.c_void_p, C.c_void_p]),
    "crt_render_lens_passes": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), P(AdaptiveParams), P(DenoiseParams),
                                         DENOISED_FN, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_uint64)]),
    "crt_radiance_lit_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                         P(RadianceParams), P(LightingView), C.c_void_p, C.c_void_p]),
    "crt_probes_lit_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                       P(ProbeParams), P(LightingView), C.c_void_p, C.c_void_p]),
    "crt_render_lens_lit_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), P(LightingView), C.c_void_p,
                                            C.c_void_p]),
    "crt_render_lens_pass_lit_async": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), P(LightingView), C.c_uint32,
                                                 C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_uint32, C.c_void_p]),
    "crt_render_lens_lit": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), P(EnvView), C.c_int, C.c_int,
                                      C.c_void_p]),
    "crt_render_lens_passes_lit": (C.c_int, [C.c_void_p, C.c_int, P(Camera), P(Lens), P(EnvView), C.c_int, C.c_int,
                                             P(AdaptiveParams), P(DenoiseParams), DENOISED_FN, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, P(C.c_uint64)]),
    "crt_ppm_values": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "crt_ppm_write": (C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "crt_render_guard": (C.c_int, [C.c_void_p, C.c_int, P(C.c_uint64), C.c_int]),
    "crt_launch_plan": (C.c_int, [C.c_void_p, C.c_uint32, P(LaunchPlan)]),
    "crt_walk_links": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, P(C.c_size_t)]),
    "crt_walk_links_validate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, P(C.c_int)]),
    "crt_last_walk": (C.c_int, [C.c_void_p, C.c_int, P(C.c_uint32)]),
}


class CrtError(RuntimeError):
    pass


_lib = None


def lib() -> C.CDLL:
    """Load the in-tree library (once). Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise CrtError(f"{LIB_PATH} is missing: run __graft_entry__.build() "
                           "(make -C cpp_raytracer_amd); there is no fallback path")
        h = C.CDLL(str(LIB_PATH), mode=os.RTLD_NOW | C.RTLD_GLOBAL)
        for name, (res, args) in EXPORTS.items():
            f = getattr(h, name)
            f.restype = res
            f.argtypes = args
        _lib = h
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().crt_last_error().decode(errors="replace")
        raise CrtError(f"{what or 'crt'} failed ({rc}): {msg}")
