"""MI355X-native render path for DeltaPavonis/cpp_raytracer.

The hot path (Camera::render -> BVH traversal -> primitive hits -> material scatter) runs as a
gfx950 HIP kernel in lib/libcrt_hip.so behind the C ABI of include/crt_render.h. This module is
the Python host side of that ABI: scene description I/O, the reference's named scenes, camera
resolution, scene upload and render launches. It never computes a pixel itself.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np

from . import _capi
from ._capi import (CRT_BOX, CRT_DIELECTRIC, CRT_DIFFUSE_LIGHT, CRT_LAMBERTIAN, CRT_METAL,
                    CRT_PARALLELOGRAM, CRT_SPHERE, HIT_DTYPE, MATERIAL_DTYPE, NODE_DTYPE,
                    OBJECT_DTYPE, CRT_BLOCK_STOPPED, FEATURE_DTYPE, BVHParams, Camera, CameraSettings, CrtError,
                    DenoiseParams, RenderStats, SceneInfo, Tiling, TraceParams, CRT_TRACE_ANY, CRT_TRACE_PLAIN,
                    RadianceParams, CRT_RADIANCE_PLAIN, ProbeParams, CRT_PROBE_SPHERE, CRT_PROBE_HEMISPHERE,
                    CRT_SH_RADIANCE, CRT_SH_IRRADIANCE, Lens, CRT_LENS_PINHOLE, CRT_LENS_ORTHOGRAPHIC,
                    CRT_LENS_EQUIRECT, CRT_LENS_FISHEYE, CRT_LENS_CUBE, EnvView, EnvSamplerView, LightSamplerView, LightingView, CRT_ENV_NEAREST, CRT_ENV_BILINEAR,
                    check, lib)

__all__ = [
    "SceneData", "GpuScene", "CameraSettings", "Camera", "Tiling", "RenderStats", "CrtError",
    "resolve_camera", "sample_seed", "rand_double", "device_count", "lib", "ppm_values", "write_ppm",
    "sample_chunk_len", "noise_estimate", "block_count", "adaptive_update", "CRT_BLOCK_STOPPED",
    "DenoiseParams", "FEATURE_DTYPE", "denoise_params", "pixel_variance", "denoise",
    "TraceParams", "CRT_TRACE_ANY", "CRT_TRACE_PLAIN", "HIT_DTYPE",
    "RadianceParams", "CRT_RADIANCE_PLAIN",
    "ProbeParams", "CRT_PROBE_SPHERE", "CRT_PROBE_HEMISPHERE", "CRT_SH_RADIANCE", "CRT_SH_IRRADIANCE", "sh_eval",
    "Lens", "make_lens", "CRT_LENS_PINHOLE", "CRT_LENS_ORTHOGRAPHIC", "CRT_LENS_EQUIRECT", "CRT_LENS_FISHEYE",
    "CRT_LENS_CUBE", "LensRender",
    "Env", "EnvView", "EnvSamplerView", "EnvTables", "make_env", "CRT_ENV_NEAREST", "CRT_ENV_BILINEAR",
    "LightSampler", "LightSamplerView", "LightTables", "Lighting", "LightingView",
    "CRT_LAMBERTIAN", "CRT_METAL", "CRT_DIELECTRIC", "CRT_DIFFUSE_LIGHT",
    "CRT_SPHERE", "CRT_PARALLELOGRAM", "CRT_BOX",
]

SCENE_MAGIC = b"CRTS"
SCENE_VERSION = 1


def sample_seed(base: int, pixel: int, sample: int) -> int:
    return int(lib().crt_sample_seed(base & 0xFFFFFFFF, pixel & 0xFFFFFFFF, sample & 0xFFFFFFFF))


def rand_double(state: int, lo: float = 0.0, hi: float = 1.0) -> tuple[int, float]:
    """One draw of the reference LCG (rand_util.h:85-117); returns (new_state, value)."""
    s = C.c_uint32(state & 0xFFFFFFFF)
    v = lib().crt_rand_double(C.byref(s), lo, hi)
    return s.value, v


def sample_chunk_len(spp: int) -> int:
    """Samples per chunk of an spp-sample render (crt_sample_chunk_len): the boundaries of
    progressive passes are multiples of it."""
    return int(lib().crt_sample_chunk_len(spp & 0xFFFFFFFF))


def noise_estimate(device: int, noise_ptr: int, pixels: int, spp: int, samples_done: int,
                   stream: int = 0) -> tuple[float, float]:
    """(sum of the pixels' standard errors, sum of their means) from the noise state a progressive
    render keeps (crt_noise_estimate); their ratio is the frame's relative noise. NaN before two
    chunks are done."""
    se, mean = C.c_double(0), C.c_double(0)
    check(lib().crt_noise_estimate(device, C.c_void_p(noise_ptr), pixels, spp, samples_done,
                                   C.byref(se), C.byref(mean), C.c_void_p(stream)), "crt_noise_estimate")
    return se.value, mean.value


def block_count(image_w: int, owned_rows: int) -> int:
    """Blocks (16 columns x 4 owned rows, the render kernel's tile) of owned_rows rows of an
    image_w wide frame (crt_block_count): the words of an adaptive render's block state."""
    return int(lib().crt_block_count(image_w, owned_rows))


def adaptive_update(device: int, cam: Camera, noise_ptr: int, blocks_ptr: int, samples_done: int,
                    threshold: float, min_samples: int = 0, stream: int = 0,
                    tiling: Optional[Tiling] = None) -> int:
    """The stopping rule of an adaptive render (crt_adaptive_update): every block at samples_done
    whose summed standard error is at most threshold times its summed mean, and that has
    min_samples samples and two chunks, gets CRT_BLOCK_STOPPED. Returns the number of blocks still
    active. Waits for the stream."""
    t = C.byref(tiling) if tiling is not None else None
    n = C.c_uint32(0)
    check(lib().crt_adaptive_update(device, C.byref(cam), t, C.c_void_p(noise_ptr), C.c_void_p(blocks_ptr),
                                    samples_done, threshold, min_samples, C.byref(n), C.c_void_p(stream)),
          "crt_adaptive_update")
    return int(n.value)


def denoise_params(iterations: int = 5, normal_squarings: int = 7, sigma_l: float = 1.0,
                   sigma_p: float = 0.05) -> DenoiseParams:
    """crt_denoise_params: a-trous iterations (steps 1, 2, 4, ...), the normal weight's exponent
    2^normal_squarings, the colour tolerance in standard errors and the plane-distance tolerance as
    a fraction of the hit distance. The defaults are DESIGN section 6c's."""
    return DenoiseParams(iterations, normal_squarings, sigma_l, sigma_p, 0, 0)


def pixel_variance(device: int, cam: Camera, noise_ptr: int, var_ptr: int, samples_done: int,
                   blocks_ptr: int = 0, stream: int = 0, tiling: Optional[Tiling] = None) -> None:
    """Enqueue the per-pixel variance of the mean (crt_pixel_variance_async) from the noise state
    at noise_ptr into var_ptr (1 double a pixel). Every pixel has samples_done samples, or with
    blocks_ptr (an adaptive render's block state) its block's own count."""
    t = C.byref(tiling) if tiling is not None else None
    check(lib().crt_pixel_variance_async(device, C.byref(cam), t, C.c_void_p(noise_ptr or None),
                                         C.c_void_p(blocks_ptr or None), samples_done, C.c_void_p(var_ptr or None),
                                         C.c_void_p(stream)), "crt_pixel_variance_async")


def denoise(device: int, width: int, height: int, rgb_ptr: int, var_ptr: int, feat_ptr: int,
            params: DenoiseParams, out_ptr: int, var_out_ptr: int = 0, stream: int = 0) -> None:
    """Enqueue the feature-guided a-trous filter (crt_denoise_async) of the whole frame at rgb_ptr
    (h*w*3 doubles) with its variance map and feature records into out_ptr (and the filtered
    variance into var_out_ptr, 0 = not wanted). The outputs may not overlap the inputs."""
    check(lib().crt_denoise_async(device, width, height, C.c_void_p(rgb_ptr or None), C.c_void_p(var_ptr or None),
                                  C.c_void_p(feat_ptr or None), C.byref(params) if params is not None else None,
                                  C.c_void_p(out_ptr or None), C.c_void_p(var_out_ptr or None), C.c_void_p(stream)),
          "crt_denoise_async")


def sh_eval(coeff, index, dirs, irradiance: bool = False):
    """Evaluates the spherical-harmonic coefficients of GpuScene.probes(mode="sphere") on torch tensors
    of a GPU (crt_sh_eval_async): coeff (num_probes, 9, 3) float64, index (m,) int32 (the probe of
    each query, its bits a uint32) and dirs (m, 3) float64 unit directions on coeff's device. Returns
    an (m, 3) float64 tensor: the band-limited radiance from dirs[i], or with irradiance=True the
    irradiance of a surface whose normal is dirs[i]. A query whose index is not a probe gives zeros.
    Runs on coeff's device and its current stream and does not synchronise."""
    import torch
    if not (coeff.is_cuda and coeff.dtype == torch.float64 and coeff.dim() == 3 and tuple(coeff.shape[1:]) == (9, 3)):
        raise CrtError("sh_eval: coeff must be a (num_probes, 9, 3) float64 tensor on a GPU")
    m = index.shape[0] if index.dim() == 1 else -1
    if not (index.is_cuda and index.device == coeff.device and index.dtype == torch.int32 and m >= 0):
        raise CrtError("sh_eval: index must be an (m,) int32 tensor on coeff's device")
    if not (dirs.is_cuda and dirs.device == coeff.device and dirs.dtype == torch.float64 and tuple(dirs.shape) == (m, 3)):
        raise CrtError("sh_eval: dirs must be an (m, 3) float64 tensor on coeff's device")
    coeff, index, dirs = coeff.contiguous(), index.contiguous(), dirs.contiguous()
    device = coeff.device.index
    with torch.cuda.device(device):
        out = torch.empty((m, 3), dtype=torch.float64, device=coeff.device)
        if m:
            check(lib().crt_sh_eval_async(device, C.c_void_p(coeff.data_ptr() or None), coeff.shape[0],
                                          C.c_void_p(index.data_ptr()), C.c_void_p(dirs.data_ptr()), m,
                                          CRT_SH_IRRADIANCE if irradiance else CRT_SH_RADIANCE,
                                          C.c_void_p(out.data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "crt_sh_eval_async")
        return out


def _basis(who, forward, up):
    """(right, up, forward) of make_lens and make_env: forward normalised, right = normalise(forward x
    up), up = right x forward, in numpy."""
    f = np.asarray(forward, np.float64).reshape(3)
    u = np.asarray(up, np.float64).reshape(3)
    f = f / np.sqrt(f.dot(f))
    r = np.cross(f, u)
    r = r / np.sqrt(r.dot(r))
    u = np.cross(r, f)
    if not (np.isfinite(f).all() and np.isfinite(r).all()):
        raise CrtError(f"{who}: forward and up must be finite, non-zero and not parallel")
    return r, u, f


_LENS_KINDS = {"pinhole": CRT_LENS_PINHOLE, "orthographic": CRT_LENS_ORTHOGRAPHIC, "equirect": CRT_LENS_EQUIRECT,
               "fisheye": CRT_LENS_FISHEYE, "cube": CRT_LENS_CUBE}


def make_lens(kind, origin=(0.0, 0.0, 0.0), forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), extent_x: float = 0.0,
              extent_y: float = 0.0, batch_pixels: int = 0, plain: bool = False) -> Lens:
    """A crt_lens for GpuScene.render_lens / lens_rays: kind is a CRT_LENS_* constant or "pinhole",
    "orthographic", "equirect", "fisheye", "cube". The basis is orthonormalised here, in numpy (the
    library uses it as given): forward is normalised, right = normalise(forward x up), then up = right x
    forward. With both extents 0, EQUIRECT gets the full sphere (pi, pi / 2) and FISHEYE a half-angle of
    pi / 2 each way; ORTHOGRAPHIC needs its half width and half height. batch_pixels sizes the internal
    batches only; plain=True passes CRT_RADIANCE_PLAIN to the radiance query: the same bits either way."""
    if isinstance(kind, str):
        if kind not in _LENS_KINDS:
            raise CrtError(f"make_lens: kind must be one of {sorted(_LENS_KINDS)}")
        kind = _LENS_KINDS[kind]
    r, u, f = _basis("make_lens", forward, up)
    if extent_x == 0 and extent_y == 0:
        if kind == CRT_LENS_EQUIRECT:
            extent_x, extent_y = float(np.pi), float(np.pi) / 2
        elif kind == CRT_LENS_FISHEYE:
            extent_x = extent_y = float(np.pi) / 2
    D3 = _capi.D3
    return Lens(kind, CRT_RADIANCE_PLAIN if plain else 0, D3(*[float(v) for v in origin]), D3(*r.tolist()),
                D3(*u.tolist()), D3(*f.tolist()), float(extent_x), float(extent_y), int(batch_pixels))


_ENV_FILTERS = {"nearest": CRT_ENV_NEAREST, "bilinear": CRT_ENV_BILINEAR}


class _DevicePtr:
    """A device allocation of `count` doubles as torch.as_tensor reads it."""

    def __init__(self, ptr: int, shape, typestr: str = "<f8"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 2}


class EnvTables:
    """A sampler's tables (crt_env_sampler_view), copied: w and c (6n, n), m (6n,) float64 tensors on
    the sampler's device, and the total W."""

    def __init__(self, w, c, m, W: float):
        self.w, self.c, self.m, self.W = w, c, m, W


class Env:
    """A cube-map environment for GpuScene.radiance / probes / render_lens (make_env): the (6n, n, 3)
    float64 tensor on a GPU, kept alive here, and the crt_env view of it that the calls read. With
    make_env(importance=True) it owns a crt_env_sampler (freed with it) and the calls take the
    *_env_sampled entries: next-event estimation of the map with MIS."""

    def __init__(self, texels, view: EnvView, sampler: Optional[int] = None):
        self.texels = texels
        self.view = view
        self.sampler = sampler  # the crt_env_sampler handle, or None

    @property
    def face_size(self) -> int:
        return int(self.view.face_size)

    @property
    def tables(self) -> EnvTables:
        """The sampler's tables as the device holds them (CrtError without importance=True)."""
        import torch
        if self.sampler is None:
            raise CrtError("Env.tables: the Env has no sampler (make_env(..., importance=True))")
        v = EnvSamplerView()
        check(lib().crt_env_sampler_view(C.c_void_p(self.sampler), C.byref(v)), "crt_env_sampler_view")
        n, dev = int(v.env.face_size), self.texels.device
        with torch.cuda.device(dev):
            torch.cuda.synchronize(dev)
            w, c, m = (torch.as_tensor(_DevicePtr(p, shape), device=dev).clone()
                       for p, shape in ((v.w, (6 * n, n)), (v.c, (6 * n, n)), (v.m, (6 * n,))))
            torch.cuda.synchronize(dev)
        return EnvTables(w, c, m, float(v.W))

    def __del__(self):
        h, self.sampler = getattr(self, "sampler", None), None
        if h is not None and _capi._lib is not None:
            _capi._lib.crt_env_sampler_free(C.c_void_p(h))


class LightTables:
    """A light sampler's tables (crt_light_sampler_view), copied to the host: prim (L,) uint32, the
    lights' flattened primitive indices in pick order, w and cdf (L,) float64, and the total W."""

    def __init__(self, prim, w, cdf, W: float):
        self.prim, self.w, self.cdf, self.W = prim, w, cdf, W


class LightSampler:
    """A sampler of a scene's own lights on one device (GpuScene.light_sampler): it owns the
    crt_light_sampler handle, freed with it, and keeps the scene alive. radiance, probes and
    render_lens take it as lights=: next-event estimation of the DiffuseLight primitives with MIS."""

    def __init__(self, scene, device: int, handle: int):
        self.scene, self.device, self.handle = scene, device, handle

    @property
    def tables(self) -> LightTables:
        import torch
        v = LightSamplerView()
        check(lib().crt_light_sampler_view(C.c_void_p(self.handle), C.byref(v)), "crt_light_sampler_view")
        L, dev = int(v.num_lights), torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            torch.cuda.synchronize(dev)
            w, cdf = (torch.as_tensor(_DevicePtr(p, (L,)), device=dev).cpu().numpy().copy() for p in (v.w, v.cdf))
            # uint32 through int32: the bits are the indices' (below 2^31)
            prim = torch.as_tensor(_DevicePtr(v.prim, (L,), "<i4"), device=dev).cpu().numpy().astype(np.uint32)
        return LightTables(prim, w, cdf, float(v.W))

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h is not None and _capi is not None and _capi._lib is not None:  # _capi is gone at interpreter exit
            _capi._lib.crt_light_sampler_free(C.c_void_p(h))


def _lights_on(who: str, lights, env, scene, device: int) -> int:
    """The handle of lights= for a call of `scene` on `device` (0 without one), after the front end's rules."""
    if lights is None:
        return 0
    if env is not None:
        raise ValueError(f"{who}: lights= and env= cannot be combined")
    if not isinstance(lights, LightSampler):
        raise CrtError(f"{who}: lights must be a LightSampler (GpuScene.light_sampler)")
    if lights.scene is not scene or lights.device != device:
        raise CrtError(f"{who}: the LightSampler belongs to another scene or device (it is on device {lights.device})")
    return lights.handle


class Lighting:
    """What lights a radiance, probe or lens call (lighting=): two independent choices. env: None (the
    constant background) or an Env (make_env), whose importance decides between the sampled and the
    plain map. lights: None or a LightSampler (GpuScene.light_sampler). With both, every Lambertian
    bounce samples the map and the lights, each weighted against the bounce (include/crt_render.h,
    crt_lighting). The object keeps both alive; Lighting() with nothing set is the unlit call."""

    def __init__(self, env: Optional["Env"] = None, lights: Optional["LightSampler"] = None):
        if env is not None and not isinstance(env, Env):
            raise CrtError("Lighting: env must be an Env (make_env)")
        if lights is not None and not isinstance(lights, LightSampler):
            raise CrtError("Lighting: lights must be a LightSampler (GpuScene.light_sampler)")
        self.env, self.lights = env, lights


def _lighting_on(who: str, lighting, env, lights, scene, device: int) -> Optional[LightingView]:
    """The crt_lighting of lighting= for a call of `scene` on `device` (None without one), after the
    front end's rules: not with env= or lights=; the members' own rules as env= and lights= have them."""
    if lighting is None:
        return None
    if env is not None or lights is not None:
        raise ValueError(f"{who}: lighting= cannot be combined with env= or lights=")
    if not isinstance(lighting, Lighting):
        raise CrtError(f"{who}: lighting must be a Lighting")
    view = LightingView()
    if lighting.env is not None:
        ev = _env_on(who, lighting.env, device)
        if lighting.env.sampler:
            view.sampler = lighting.env.sampler
        else:
            view.env = C.pointer(ev)  # the structure keeps ev alive
    if lighting.lights is not None:
        view.lights = _lights_on(who, lighting.lights, None, scene, device)
    return view


def _env_texels_ok(t) -> bool:
    import torch
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.dim() == 3 and
            t.shape[2] == 3 and t.shape[1] >= 1 and t.shape[0] == 6 * t.shape[1] and t.is_contiguous())


def make_env(texels, forward=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), filter="bilinear", importance: bool = False) -> Env:
    """An environment from a cube frame: texels is a contiguous (6n, n, 3) float64 torch tensor on a
    GPU in render_lens's "cube" layout (a render_lens(cam, make_lens("cube")) frame as it is; it is
    not copied, and the Env keeps it alive). The basis is built as make_lens builds it; filter is
    "nearest" or "bilinear" (or a CRT_ENV_* constant). Paths that leave the scene then see the map
    in place of the constant background (include/crt_render.h, crt_env). importance=True builds a
    luminance sampler of the map on the texels' device (crt_env_sampler_create: it waits for that
    device, and the texels must then stay unchanged): radiance, probes and render_lens sample the map
    at every Lambertian bounce and weight it against the bounce's own escape (MIS), so a small bright
    region no longer has to be found by chance. The face size is then at most 2048."""
    if isinstance(filter, str):
        if filter not in _ENV_FILTERS:
            raise CrtError(f"make_env: filter must be one of {sorted(_ENV_FILTERS)}")
        filter = _ENV_FILTERS[filter]
    if not _env_texels_ok(texels):
        raise CrtError("make_env: texels must be a contiguous (6n, n, 3) float64 tensor on a GPU")
    if texels.shape[1] > 16384:
        raise CrtError("make_env: the face size must be at most 16384")
    r, u, f = _basis("make_env", forward, up)
    D3 = _capi.D3
    view = EnvView(texels.data_ptr(), texels.shape[1], int(filter), D3(*r.tolist()), D3(*u.tolist()), D3(*f.tolist()))
    if not importance:
        return Env(texels, view)
    import torch
    handle = C.c_void_p()
    with torch.cuda.device(texels.device):
        torch.cuda.synchronize(texels.device)  # the build reads the texels on the device's null stream
        check(lib().crt_env_sampler_create(texels.device.index, C.byref(view), C.byref(handle)), "crt_env_sampler_create")
    return Env(texels, view, handle.value)


def _env_on(who: str, env, device: int) -> EnvView:
    """The view of `env` for a call on `device`; CrtError unless it is an Env whose tensor is still a
    contiguous float64 cube frame on that device."""
    if not isinstance(env, Env):
        raise CrtError(f"{who}: env must be an Env (make_env)")
    t = env.texels
    if not _env_texels_ok(t) or t.data_ptr() != env.view.texels or t.shape[1] != env.view.face_size:
        raise CrtError(f"{who}: env's texels must be the contiguous (6n, n, 3) float64 tensor it was made from")
    if t.device.index != device:
        raise CrtError(f"{who}: env's texels are on cuda:{t.device.index}, the call runs on cuda:{device}")
    return env.view


def device_count() -> int:
    n = C.c_int(0)
    rc = lib().crt_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def ppm_values(device: int, frame_ptr: int, height: int, width: int, stream: int = 0) -> np.ndarray:
    """Image::send_as_ppm's integers (h, w, 3 int32) for a device frame of h*w RGB f64 pixels
    (crt_ppm_values: computed on the GPU)."""
    out = np.zeros((height, width, 3), np.int32)
    check(lib().crt_ppm_values(device, C.c_void_p(frame_ptr), height * width, out.ctypes.data,
                               C.c_void_p(stream)), "crt_ppm_values")
    return out


def write_ppm(path, values: np.ndarray) -> None:
    """Writes (h, w, 3) integers as Image::send_as_ppm does (crt_ppm_write)."""
    v = np.ascontiguousarray(values, np.int32)
    h, w, _ = v.shape
    check(lib().crt_ppm_write(str(path).encode(), w, h, v.ctypes.data), "crt_ppm_write")


def _settings_bytes(cs: CameraSettings) -> bytes:
    return C.string_at(C.addressof(cs), C.sizeof(cs))


@dataclass
class SceneData:
    """Host description of a world: materials + objects (+ the scene's camera settings)."""
    materials: np.ndarray
    objects: np.ndarray
    camera: CameraSettings

    @classmethod
    def named(cls, name: str, seed: Optional[int] = None) -> "SceneData":
        """A scene of the reference's src/main.cpp, built with the reference's RNG semantics."""
        mp = C.POINTER(_capi.Material)()
        op = C.POINTER(_capi.Object)()
        nm, no = C.c_size_t(0), C.c_size_t(0)
        cs = CameraSettings()
        rc = lib().crt_scene_build_named(name.encode(), (seed or 0) & 0xFFFFFFFF, int(seed is not None),
                                         C.byref(mp), C.byref(nm), C.byref(op), C.byref(no),
                                         C.byref(cs))
        check(rc, f"crt_scene_build_named({name!r})")
        try:
            mats = np.frombuffer(C.string_at(mp, nm.value * MATERIAL_DTYPE.itemsize),
                                 dtype=MATERIAL_DTYPE).copy()
            objs = np.frombuffer(C.string_at(op, no.value * OBJECT_DTYPE.itemsize),
                                 dtype=OBJECT_DTYPE).copy()
        finally:
            lib().crt_free(C.cast(mp, C.c_void_p))
            lib().crt_free(C.cast(op, C.c_void_p))
        return cls(mats, objs, cs)

    # --- the CRTS serialization format (header, camera settings, materials, objects) ---
    def to_bytes(self) -> bytes:
        head = SCENE_MAGIC + struct.pack("<IQQ", SCENE_VERSION, len(self.materials), len(self.objects))
        return (head + _settings_bytes(self.camera) + self.materials.astype(MATERIAL_DTYPE).tobytes()
                + self.objects.astype(OBJECT_DTYPE).tobytes())

    def save(self, path) -> None:
        Path(path).write_bytes(self.to_bytes())

    @classmethod
    def from_bytes(cls, b: bytes) -> "SceneData":
        if b[:4] != SCENE_MAGIC:
            raise CrtError("not a CRTS scene file")
        ver, nm, no = struct.unpack_from("<IQQ", b, 4)
        if ver != SCENE_VERSION:
            raise CrtError(f"CRTS version {ver} unsupported")
        off = 4 + struct.calcsize("<IQQ")
        cs = CameraSettings.from_buffer_copy(b[off:off + C.sizeof(CameraSettings)])
        off += C.sizeof(CameraSettings)
        mats = np.frombuffer(b, MATERIAL_DTYPE, nm, off).copy()
        off += nm * MATERIAL_DTYPE.itemsize
        objs = np.frombuffer(b, OBJECT_DTYPE, no, off).copy()
        return cls(mats, objs, cs)

    @classmethod
    def load(cls, path) -> "SceneData":
        return cls.from_bytes(Path(path).read_bytes())


def resolve_camera(settings: CameraSettings, base_seed: int = 0) -> Camera:
    """Camera::init (camera.h:87-157) -> the per-sample loop's constants."""
    cam = Camera()
    check(lib().crt_camera_resolve(C.byref(settings), C.byref(cam)), "crt_camera_resolve")
    cam.base_seed = base_seed & 0xFFFFFFFF
    return cam


def camera_with(settings: CameraSettings, **kw) -> CameraSettings:
    """A copy of `settings` with fields replaced (image_w=..., samples_per_pixel=..., ...)."""
    cs = CameraSettings.from_buffer_copy(_settings_bytes(settings))
    for k, v in kw.items():
        setattr(cs, k, v)
    return cs


class GpuScene:
    """A flattened scene + reference-order BVH with per-device HBM copies. The BVH is built on
    the host, or on GPU `build_device` (the same tree, crt_bvh_params.build_device)."""

    def __init__(self, data: SceneData, num_buckets: int = 32, max_prims_in_node: int = 12,
                 linear: bool = False, build_device: Optional[int] = None):
        self.data = data
        self._h = C.c_void_p()
        mats = np.ascontiguousarray(data.materials, dtype=MATERIAL_DTYPE)
        objs = np.ascontiguousarray(data.objects, dtype=OBJECT_DTYPE)
        prm = BVHParams(num_buckets, max_prims_in_node, int(linear),
                        0 if build_device is None else build_device + 1)
        check(lib().crt_scene_create(mats.ctypes.data, len(mats), objs.ctypes.data, len(objs),
                                     C.byref(prm), C.byref(self._h)), "crt_scene_create")

    def close(self) -> None:
        if self._h:
            lib().crt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    def info(self) -> SceneInfo:
        si = SceneInfo()
        check(lib().crt_scene_info_get(self._h, C.byref(si)), "crt_scene_info_get")
        return si

    def export_bvh(self) -> tuple[np.ndarray, np.ndarray]:
        si = self.info()
        nodes = np.zeros(si.num_nodes, NODE_DTYPE)
        order = np.zeros(si.num_primitives, np.uint32)
        check(lib().crt_scene_export_bvh(self._h, nodes.ctypes.data, order.ctypes.data),
              "crt_scene_export_bvh")
        return nodes, order

    def launch_plan(self, kernel="render") -> _capi.LaunchPlan:
        """What a launch of `kernel` ("render", "trace", "radiance") would decide for this scene: class,
        entry width, instance and LDS layout (crt_launch_plan). Host only; reads the CRT_* switches now."""
        k = {"render": _capi.CRT_PLAN_RENDER, "trace": _capi.CRT_PLAN_TRACE, "radiance": _capi.CRT_PLAN_RADIANCE}.get(kernel, kernel)
        p = _capi.LaunchPlan()
        check(lib().crt_launch_plan(self._h, int(k), C.byref(p)), "crt_launch_plan")
        return p

    def walk_links(self) -> Optional[np.ndarray]:
        """The miss links of the stackless walk (crt_walk_links): a (device nodes, 8) uint16 array,
        entry [node, octant] = the reference (node index * 32) of the node the walk continues at when
        it does not descend from `node`; None when the scene has no table."""
        n = C.c_size_t(0)
        check(lib().crt_walk_links(self._h, None, 0, C.byref(n)), "crt_walk_links")
        if n.value == 0:
            return None
        out = np.zeros((n.value, 8), np.uint16)
        check(lib().crt_walk_links(self._h, out.ctypes.data, out.size, C.byref(n)), "crt_walk_links")
        return out

    def walk_links_valid(self, links: np.ndarray) -> bool:
        """The check every upload runs on its table, for a caller's one (crt_walk_links_validate)."""
        t = np.ascontiguousarray(links, np.uint16)
        ok = C.c_int(0)
        check(lib().crt_walk_links_validate(self._h, t.ctypes.data, t.size, C.byref(ok)), "crt_walk_links_validate")
        return bool(ok.value)

    def last_walk(self, device: int = 0) -> str:
        """The walk of the last render launch on `device`: "none", "stack" or "links" (crt_last_walk)."""
        w = C.c_uint32(0)
        check(lib().crt_last_walk(self._h, device, C.byref(w)), "crt_last_walk")
        return ("none", "stack", "links")[w.value]

    def upload(self, device: int = 0) -> None:
        check(lib().crt_scene_upload(self._h, device), f"crt_scene_upload(device={device})")

    def light_sampler(self, device: int = 0) -> LightSampler:
        """A sampler of the scene's DiffuseLight primitives on `device` (crt_light_sampler_create; it
        uploads the scene there if needed and blocks). CrtError for a scene without a light."""
        self.upload(device)
        h = C.c_void_p()
        check(lib().crt_light_sampler_create(self._h, device, C.byref(h)), "crt_light_sampler_create")
        return LightSampler(self, device, h.value)

    def device_image(self, device: int = 0) -> np.ndarray:
        """The bytes of the scene's copy in HBM of `device` (crt_scene_image)."""
        out = np.zeros(self.info().device_bytes, np.uint8)
        check(lib().crt_scene_image(self._h, device, out.ctypes.data, out.nbytes),
              f"crt_scene_image(device={device})")
        return out

    def render_async(self, device: int, cam: Camera, out_ptr: int, stream: int = 0,
                     tiling: Optional[Tiling] = None) -> None:
        """Enqueue a render of the owned rows into the device buffer at out_ptr."""
        t = C.byref(tiling) if tiling is not None else None
        check(lib().crt_render_async(self._h, device, C.byref(cam), t, C.c_void_p(out_ptr),
                                     C.c_void_p(stream)), "crt_render_async")

    def render_pass(self, device: int, cam: Camera, first: int, count: int, sum_ptr: int,
                    noise_ptr: int = 0, out_ptr: int = 0, stream: int = 0,
                    tiling: Optional[Tiling] = None) -> None:
        """Enqueue samples [first, first + count) of a cam.samples_per_pixel job into the running
        sums at sum_ptr (crt_render_pass_async; boundaries are multiples of sample_chunk_len).
        noise_ptr: 2 doubles a pixel of noise state; out_ptr: the frame so far. 0 = not wanted."""
        t = C.byref(tiling) if tiling is not None else None
        check(lib().crt_render_pass_async(self._h, device, C.byref(cam), t, first, count,
                                          C.c_void_p(sum_ptr), C.c_void_p(noise_ptr or None),
                                          C.c_void_p(out_ptr or None), C.c_void_p(stream)),
              "crt_render_pass_async")

    def render_pass_masked(self, device: int, cam: Camera, first: int, count: int, sum_ptr: int,
                           noise_ptr: int, out_ptr: int, blocks_ptr: int, active_hint: int = 0,
                           stream: int = 0, tiling: Optional[Tiling] = None) -> None:
        """render_pass for the blocks whose word at blocks_ptr equals `first` only
        (crt_render_pass_masked_async); their words become first + count. active_hint: how many
        blocks the caller expects to be rendered (0: unknown); it never changes the result."""
        t = C.byref(tiling) if tiling is not None else None
        check(lib().crt_render_pass_masked_async(self._h, device, C.byref(cam), t, first, count,
                                                 C.c_void_p(sum_ptr), C.c_void_p(noise_ptr or None),
                                                 C.c_void_p(out_ptr or None), C.c_void_p(blocks_ptr or None),
                                                 min(active_hint, 0xFFFFFFFF), C.c_void_p(stream)),
              "crt_render_pass_masked_async")

    def render_adaptive(self, cam: Camera, threshold: float, min_samples: int = 0, samples_per_pass: int = 0,
                        callback=None, num_devices: int = 1,
                        preview: bool = False) -> tuple[np.ndarray, np.ndarray, int]:
        """Blocking adaptive render (crt_render_adaptive): blocks of 16 x 4 pixels stop between
        passes once their noise is at most `threshold`. callback(samples_done, samples_total,
        active_blocks, total_blocks, frame) runs after every pass (frame as render_progressive's);
        a true return stops the render. Returns (frame, the blocks' sample counts as a
        (ceil(h / 4), ceil(w / 16)) uint32 array, the samples rendered over all pixels)."""
        out = np.empty((cam.image_h, cam.image_w, 3), np.float64)
        counts = np.zeros(((cam.image_h + 3) // 4, (cam.image_w + 15) // 16), np.uint32)
        raised = []

        def trampoline(_user, done, total, active, blocks, h_rgb):
            try:
                return 1 if callback(done, total, active, blocks, out if h_rgb else None) else 0
            except BaseException as e:  # not through the C frames: stop, raise after the call
                raised.append(e)
                return 1

        fn = _capi.ADAPTIVE_FN(trampoline) if callback is not None else _capi.ADAPTIVE_FN()
        prm = _capi.AdaptiveParams(threshold, min_samples, samples_per_pass,
                                   _capi.CRT_PROGRESS_PREVIEW if preview else 0, 0)
        rendered = C.c_uint64(0)
        rc = lib().crt_render_adaptive(self._h, C.byref(cam), num_devices, C.byref(prm), fn, None,
                                       out.ctypes.data, counts.ctypes.data, C.byref(rendered))
        if raised:
            raise raised[0]
        check(rc, "crt_render_adaptive")
        return out, counts, int(rendered.value)

    # the module functions, beside the passes they go with
    adaptive_update = staticmethod(adaptive_update)
    block_count = staticmethod(block_count)
    pixel_variance = staticmethod(pixel_variance)
    denoise = staticmethod(denoise)

    def render_features(self, device: int, cam: Camera, feat_ptr: int, stream: int = 0,
                        tiling: Optional[Tiling] = None) -> None:
        """Enqueue the first-hit features of the owned pixels (crt_render_features_async) into the
        device buffer at feat_ptr: one 88-byte crt_feature (FEATURE_DTYPE) per pixel, at
        render_async's pixel addresses."""
        t = C.byref(tiling) if tiling is not None else None
        check(lib().crt_render_features_async(self._h, device, C.byref(cam), t, C.c_void_p(feat_ptr or None),
                                              C.c_void_p(stream)), "crt_render_features_async")

    def render_denoised(self, cam: Camera, params: Optional[DenoiseParams] = None, threshold: Optional[float] = None,
                        min_samples: int = 0, samples_per_pass: int = 0, device: int = 0,
                        noisy: bool = False, *, num_devices: int = 1, callback=None, preview: bool = False,
                        counts: bool = False):
        """Blocking denoised render: every sample, or with `threshold` an adaptive render
        (render_adaptive's rule), then features, variance and the filter. Returns (denoised frame,
        unfiltered frame or None, samples rendered over all pixels).
        With the keyword arguments at their defaults: on `device` (crt_render_denoised). Otherwise
        over devices [0, num_devices) with the filter on device 0 (crt_render_denoised_devices; 0 =
        all visible devices; `device` must be 0): the same frames bit for bit.
        callback(samples_done, samples_total, active_blocks, total_blocks, noisy, denoised) runs
        after every pass; a true return stops the render. With preview=True (needs `threshold`;
        min_samples >= the job's samples never stops a block) every call gets the denoised frame of
        the state so far and, with noisy=True, the unfiltered one (views of the returned arrays:
        copy them to keep them); else both are None. counts=True appends the blocks' sample counts
        (render_adaptive's array) to the result."""
        out = np.empty((cam.image_h, cam.image_w, 3), np.float64)
        raw = np.empty_like(out) if noisy else None
        prm = params if params is not None else denoise_params()
        rendered = C.c_uint64(0)
        if num_devices == 1 and callback is None and not preview and not counts:
            ad = _capi.AdaptiveParams(threshold, min_samples, samples_per_pass, 0, 0) if threshold is not None else None
            check(lib().crt_render_denoised(self._h, device, C.byref(cam), C.byref(ad) if ad is not None else None,
                                            C.byref(prm), raw.ctypes.data if noisy else None, out.ctypes.data,
                                            C.byref(rendered)), "crt_render_denoised")
            return out, raw, int(rendered.value)
        if device != 0:
            raise CrtError("render_denoised: device must be 0 with num_devices, callback, preview or counts "
                           "(the render runs on devices [0, num_devices))")
        if preview and threshold is None:
            raise CrtError("render_denoised: preview needs an adaptive render (threshold; min_samples >= the job's "
                           "samples renders plain passes)")
        ad = None
        if threshold is not None:
            ad = _capi.AdaptiveParams(threshold, min_samples, samples_per_pass,
                                      _capi.CRT_PROGRESS_PREVIEW if preview else 0, 0)
        blocks = np.zeros(((cam.image_h + 3) // 4, (cam.image_w + 15) // 16), np.uint32)
        raised = []

        def trampoline(_user, done, total, active, nblocks, h_noisy, h_rgb):
            try:
                return 1 if callback(done, total, active, nblocks, raw if h_noisy else None, out if h_rgb else None) else 0
            except BaseException as e:  # not through the C frames: stop, raise after the call
                raised.append(e)
                return 1

        fn = _capi.DENOISED_FN(trampoline) if callback is not None else _capi.DENOISED_FN()
        rc = lib().crt_render_denoised_devices(self._h, C.byref(cam), num_devices, C.byref(ad) if ad is not None else None,
                                               C.byref(prm), fn, None, raw.ctypes.data if noisy else None,
                                               out.ctypes.data, blocks.ctypes.data, C.byref(rendered))
        if raised:
            raise raised[0]
        check(rc, "crt_render_denoised_devices")
        return (out, raw, int(rendered.value), blocks) if counts else (out, raw, int(rendered.value))

    def render_progressive(self, cam: Camera, samples_per_pass: int = 0, callback=None, num_devices: int = 1,
                           preview: bool = False, noise: bool = False) -> tuple[np.ndarray, int]:
        """Blocking whole-frame render in passes (crt_render_progressive). After every pass
        callback(samples_done, samples_total, noise, frame) is called: noise is the frame's
        relative noise with noise=True (else NaN), frame the (h, w, 3) picture so far with
        preview=True (else None; a view of the returned array: copy it to keep it). A true return
        stops the render. Returns (frame, samples_done): the mean of the samples rendered."""
        out = np.empty((cam.image_h, cam.image_w, 3), np.float64)
        raised = []

        def trampoline(_user, done, total, figure, h_rgb):
            try:
                return 1 if callback(done, total, figure, out if h_rgb else None) else 0
            except BaseException as e:  # not through the C frames: stop, raise after the call
                raised.append(e)
                return 1

        fn = _capi.PROGRESS_FN(trampoline) if callback is not None else _capi.PROGRESS_FN()
        flags = (_capi.CRT_PROGRESS_NOISE if noise else 0) | (_capi.CRT_PROGRESS_PREVIEW if preview else 0)
        done = C.c_uint32(0)
        rc = lib().crt_render_progressive(self._h, C.byref(cam), num_devices, samples_per_pass, flags, fn,
                                          None, out.ctypes.data, C.byref(done))
        if raised:
            raise raised[0]
        check(rc, "crt_render_progressive")
        return out, int(done.value)

    def render_count(self, device: int, cam: Camera, tiling: Optional[Tiling] = None) -> RenderStats:
        st = RenderStats()
        t = C.byref(tiling) if tiling is not None else None
        check(lib().crt_render_count(self._h, device, C.byref(cam), t, C.byref(st)), "crt_render_count")
        return st

    def render(self, cam: Camera, num_devices: int = 1) -> tuple[np.ndarray, RenderStats]:
        """Blocking whole-frame render gathered into host memory: (h, w, 3) float64."""
        out = np.empty((cam.image_h, cam.image_w, 3), np.float64)
        st = RenderStats()
        check(lib().crt_render(self._h, C.byref(cam), num_devices, out.ctypes.data, C.byref(st)),
              "crt_render")
        return out, st

    def render_ppm(self, cam: Camera, num_devices: int = 1) -> tuple[np.ndarray, RenderStats]:
        """Blocking whole-frame render fused with Image::send_as_ppm's integers (crt_render_ppm:
        each device tone-maps its rows to 8-bit values before the gather): (h, w, 3) int32."""
        out = np.empty((cam.image_h, cam.image_w, 3), np.int32)
        st = RenderStats()
        check(lib().crt_render_ppm(self._h, C.byref(cam), num_devices, out.ctypes.data, C.byref(st)),
              "crt_render_ppm")
        return out, st

    def guard(self, device: int = 0, reset: bool = False) -> int:
        """Dielectric decisions since upload (or the last reset) that a one-ulp different
        pow(1 - cos, 5) could have flipped (crt_render_guard; 0 = every branch as the reference's)."""
        v = C.c_uint64()
        check(lib().crt_render_guard(self._h, device, C.byref(v), int(reset)), "crt_render_guard")
        return int(v.value)

    def closest_hits(self, rays: np.ndarray, t_min: float = 1e-5, t_max: float = float("inf"),
                     device: int = 0) -> np.ndarray:
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
        out = np.zeros(len(rays), HIT_DTYPE)
        check(lib().crt_closest_hits(self._h, device, rays.ctypes.data, len(rays), t_min, t_max,
                                     out.ctypes.data), "crt_closest_hits")
        return out

    def trace_async(self, device: int, rays_ptr: int, n: int, hits_ptr: int = 0, occluded_ptr: int = 0,
                    t_min: float = 1e-5, t_max: float = float("inf"), tmax_ptr: int = 0, flags: int = 0,
                    stream: int = 0) -> None:
        """Enqueue a ray query on device buffers (crt_trace_async): n rays of 6 doubles at rays_ptr
        over (t_min, t_max), or up to tmax_ptr[i] for ray i. Closest hits (72-byte crt_hit records,
        HIT_DTYPE) go to hits_ptr; with CRT_TRACE_ANY in flags, one uint32 a ray (1 = something is
        hit) to occluded_ptr. CRT_TRACE_PLAIN takes crt_closest_hits' kernel instead of the render
        kernel's traversal: the same results. The scene must be uploaded to `device`."""
        prm = TraceParams(t_min, t_max, flags, 0)
        check(lib().crt_trace_async(self._h, device, C.c_void_p(rays_ptr or None), n, C.c_void_p(tmax_ptr or None),
                                    C.byref(prm), C.c_void_p(hits_ptr or None), C.c_void_p(occluded_ptr or None),
                                    C.c_void_p(stream)), "crt_trace_async")

    def trace(self, rays, t_min: float = 1e-5, t_max: float = float("inf"), tmax=None, any_hit: bool = False,
              plain: bool = False):
        """Ray query on torch tensors of a GPU: rays (n, 6) float64, tmax None or (n,) float64 of
        per-ray upper bounds, on the rays' device. Runs on that device's current stream and does
        not synchronise; the scene is uploaded there first if it is not yet (that, and the first
        closest-hit call, block). Returns an (n, 72) uint8 tensor (after .cpu().numpy(),
        .view(HIT_DTYPE) gives the records), or with any_hit an (n,) bool tensor."""
        import torch
        if not (rays.is_cuda and rays.dtype == torch.float64 and rays.dim() == 2 and rays.shape[1] == 6):
            raise CrtError("trace: rays must be an (n, 6) float64 tensor on a GPU")
        rays = rays.contiguous()
        n, device = rays.shape[0], rays.device.index
        if tmax is not None:
            if not (tmax.is_cuda and tmax.device == rays.device and tmax.dtype == torch.float64 and tmax.shape == (n,)):
                raise CrtError("trace: tmax must be an (n,) float64 tensor on the rays' device")
            tmax = tmax.contiguous()
        flags = (CRT_TRACE_ANY if any_hit else 0) | (CRT_TRACE_PLAIN if plain else 0)
        with torch.cuda.device(device):
            out = torch.empty((n,), dtype=torch.int32, device=rays.device) if any_hit else \
                torch.empty((n, HIT_DTYPE.itemsize), dtype=torch.uint8, device=rays.device)
            if n:
                self.upload(device)
                self.trace_async(device, rays.data_ptr(), n, 0 if any_hit else out.data_ptr(),
                                 out.data_ptr() if any_hit else 0, t_min, t_max,
                                 tmax.data_ptr() if tmax is not None else 0, flags,
                                 torch.cuda.current_stream(device).cuda_stream)
            return out != 0 if any_hit else out

    def radiance_async(self, device: int, rays_ptr: int, n: int, out_ptr: int, states_ptr: int = 0, *,
                       max_depth: int, background, t_min: float = 1e-5, base_seed: int = 0, flags: int = 0,
                       stream: int = 0, env: Optional[EnvView] = None, sampler: int = 0, lights: int = 0,
                       lighting: Optional[LightingView] = None) -> None:
        """Enqueue a radiance query on device buffers (crt_radiance_async): n rays of 6 doubles at
        rays_ptr, each the first segment of one path of ray_color with `max_depth` bounces over
        (t_min, inf). Path i's LCG state is the uint32 states_ptr[i], or sample_seed(base_seed, i, 0)
        with states_ptr = 0. Three doubles a path go to out_ptr: what the sample adds to a pixel's
        sum in a render. CRT_RADIANCE_PLAIN takes one thread a path: the same bits. The scene must be
        uploaded to `device`. env: an EnvView (crt_env) whose texels are on `device`: paths that end in
        a miss see it in place of `background` (crt_radiance_env_async). sampler: a crt_env_sampler
        handle built on `device` (Env.sampler) in place of env (crt_radiance_env_sampled_async). lights: a
        crt_light_sampler handle of this scene on `device` (LightSampler.handle), without env or sampler
        (crt_radiance_lights_async). lighting: a LightingView (crt_lighting) in place of all three: an
        environment and the lights together (crt_radiance_lit_async)."""
        prm = RadianceParams(max_depth, base_seed & 0xFFFFFFFF, _capi.D3(*[float(v) for v in background]), t_min,
                             flags, 0)
        if lighting is not None:
            if env is not None or sampler or lights:
                raise ValueError("radiance_async: lighting= cannot be combined with env=, sampler= or lights=")
            check(lib().crt_radiance_lit_async(self._h, device, C.c_void_p(rays_ptr or None), n,
                                               C.c_void_p(states_ptr or None), C.byref(prm), C.byref(lighting),
                                               C.c_void_p(out_ptr or None), C.c_void_p(stream)),
                  "crt_radiance_lit_async")
            return
        if lights:
            check(lib().crt_radiance_lights_async(self._h, device, C.c_void_p(rays_ptr or None), n,
                                                  C.c_void_p(states_ptr or None), C.byref(prm), C.c_void_p(lights),
                                                  C.c_void_p(out_ptr or None), C.c_void_p(stream)),
                  "crt_radiance_lights_async")
            return
        if sampler:
            check(lib().crt_radiance_env_sampled_async(self._h, device, C.c_void_p(rays_ptr or None), n,
                                                       C.c_void_p(states_ptr or None), C.byref(prm), C.c_void_p(sampler),
                                                       C.c_void_p(out_ptr or None), C.c_void_p(stream)),
                  "crt_radiance_env_sampled_async")
            return
        if env is not None:
            check(lib().crt_radiance_env_async(self._h, device, C.c_void_p(rays_ptr or None), n,
                                               C.c_void_p(states_ptr or None), C.byref(prm), C.byref(env),
                                               C.c_void_p(out_ptr or None), C.c_void_p(stream)),
                  "crt_radiance_env_async")
            return
        check(lib().crt_radiance_async(self._h, device, C.c_void_p(rays_ptr or None), n, C.c_void_p(states_ptr or None),
                                       C.byref(prm), C.c_void_p(out_ptr or None), C.c_void_p(stream)),
              "crt_radiance_async")

    def radiance(self, rays, states=None, max_depth: int = 50, background=(0.7, 0.8, 1.0), t_min: float = 1e-5,
                 base_seed: int = 0, plain: bool = False, env: Optional[Env] = None,
                 lights: Optional[LightSampler] = None, lighting: Optional[Lighting] = None):
        """Path-traced radiance of the caller's rays on torch tensors of a GPU: rays (n, 6) float64,
        states None or an (n,) int32 tensor on the rays' device whose bits are the paths' LCG states
        (None: sample_seed(base_seed, i, 0)). Runs on the rays' device and its current stream and
        does not synchronise; the scene is uploaded there first if it is not yet (that blocks).
        Returns an (n, 3) float64 tensor. env (make_env, on the rays' device): the environment that
        paths leaving the scene see in place of `background`. lights (light_sampler, of the
        rays' device; not with env): every Lambertian bounce also samples the scene's lights (MIS).
        lighting (a Lighting; not with env or lights): an environment and the lights together."""
        import torch
        if env is not None and not isinstance(env, Env):
            raise CrtError("radiance: env must be an Env (make_env)")
        if not (rays.is_cuda and rays.dtype == torch.float64 and rays.dim() == 2 and rays.shape[1] == 6):
            raise CrtError("radiance: rays must be an (n, 6) float64 tensor on a GPU")
        rays = rays.contiguous()
        n, device = rays.shape[0], rays.device.index
        lit = _lighting_on("radiance", lighting, env, lights, self, device)
        lh = _lights_on("radiance", lights, env, self, device)
        view = _env_on("radiance", env, device) if env is not None else None
        if states is not None:
            if not (states.is_cuda and states.device == rays.device and states.dtype == torch.int32 and
                    states.shape == (n,)):
                raise CrtError("radiance: states must be an (n,) int32 tensor on the rays' device")
            states = states.contiguous()
        with torch.cuda.device(device):
            out = torch.empty((n, 3), dtype=torch.float64, device=rays.device)
            if n:
                self.upload(device)
                self.radiance_async(device, rays.data_ptr(), n, out.data_ptr(),
                                    states.data_ptr() if states is not None else 0, max_depth=max_depth,
                                    background=background, t_min=t_min, base_seed=base_seed,
                                    flags=CRT_RADIANCE_PLAIN if plain else 0,
                                    stream=torch.cuda.current_stream(device).cuda_stream, env=view,
                                    sampler=(env.sampler or 0) if env is not None else 0, lights=lh, lighting=lit)
            return out

    @staticmethod
    def _probe_params(samples, mode, max_depth, background, t_min, base_seed, batch_probes, flags) -> ProbeParams:
        if isinstance(mode, str):
            if mode not in ("sphere", "hemisphere"):
                raise CrtError('probes: mode must be "sphere" or "hemisphere"')
            mode = CRT_PROBE_HEMISPHERE if mode == "hemisphere" else CRT_PROBE_SPHERE
        return ProbeParams(samples, max_depth, base_seed & 0xFFFFFFFF, mode, _capi.D3(*[float(v) for v in background]),
                           t_min, batch_probes, flags)

    def probes_async(self, device: int, points_ptr: int, normals_ptr: int, n: int, out_ptr: int, *, samples: int,
                     mode=CRT_PROBE_SPHERE, max_depth: int, background, t_min: float = 1e-5, base_seed: int = 0,
                     batch_probes: int = 0, flags: int = 0, stream: int = 0, env: Optional[EnvView] = None,
                     sampler: int = 0, lights: int = 0, lighting: Optional[LightingView] = None) -> None:
        """Enqueue a probe bake on device buffers (crt_probes_async): n points of 3 doubles at
        points_ptr, with CRT_PROBE_HEMISPHERE their unit normals at normals_ptr (0 with
        CRT_PROBE_SPHERE). `samples` directions a probe are drawn on the device, path-traced as
        radiance_async traces them and reduced in a fixed order: n x 9 x 3 doubles (SH coefficients of
        bands 0..2 per channel) or n x 1 x 3 (irradiance) go to out_ptr. batch_probes sizes the
        internal batches only; flags may hold CRT_RADIANCE_PLAIN: the same bits either way. The scene
        must be uploaded to `device`. env, sampler: as radiance_async's (crt_probes_env_async,
        crt_probes_env_sampled_async). lights: as radiance_async's (crt_probes_lights_async). lighting: as
        radiance_async's (crt_probes_lit_async)."""
        prm = self._probe_params(samples, mode, max_depth, background, t_min, base_seed, batch_probes, flags)
        if lighting is not None:
            if env is not None or sampler or lights:
                raise ValueError("probes_async: lighting= cannot be combined with env=, sampler= or lights=")
            check(lib().crt_probes_lit_async(self._h, device, C.c_void_p(points_ptr or None),
                                             C.c_void_p(normals_ptr or None), n, C.byref(prm), C.byref(lighting),
                                             C.c_void_p(out_ptr or None), C.c_void_p(stream)), "crt_probes_lit_async")
            return
        if lights:
            check(lib().crt_probes_lights_async(self._h, device, C.c_void_p(points_ptr or None),
                                                C.c_void_p(normals_ptr or None), n, C.byref(prm), C.c_void_p(lights),
                                                C.c_void_p(out_ptr or None), C.c_void_p(stream)), "crt_probes_lights_async")
            return
        if sampler:
            check(lib().crt_probes_env_sampled_async(self._h, device, C.c_void_p(points_ptr or None),
                                                     C.c_void_p(normals_ptr or None), n, C.byref(prm),
                                                     C.c_void_p(sampler), C.c_void_p(out_ptr or None),
                                                     C.c_void_p(stream)), "crt_probes_env_sampled_async")
            return
        if env is not None:
            check(lib().crt_probes_env_async(self._h, device, C.c_void_p(points_ptr or None),
                                             C.c_void_p(normals_ptr or None), n, C.byref(prm), C.byref(env),
                                             C.c_void_p(out_ptr or None), C.c_void_p(stream)), "crt_probes_env_async")
            return
        check(lib().crt_probes_async(self._h, device, C.c_void_p(points_ptr or None), C.c_void_p(normals_ptr or None), n,
                                     C.byref(prm), C.c_void_p(out_ptr or None), C.c_void_p(stream)), "crt_probes_async")

    @staticmethod
    def _probe_inputs(who, points, normals, mode):
        import torch
        if mode not in ("sphere", "hemisphere"):
            raise CrtError(f'{who}: mode must be "sphere" or "hemisphere"')
        if not (points.is_cuda and points.dtype == torch.float64 and points.dim() == 2 and points.shape[1] == 3):
            raise CrtError(f"{who}: points must be an (n, 3) float64 tensor on a GPU")
        if (normals is not None) != (mode == "hemisphere"):
            raise CrtError(f'{who}: normals are required with mode="hemisphere" and must be None with mode="sphere"')
        if normals is not None:
            if not (normals.is_cuda and normals.device == points.device and normals.dtype == torch.float64 and
                    normals.shape == points.shape):
                raise CrtError(f"{who}: normals must be an (n, 3) float64 tensor on the points' device")
            normals = normals.contiguous()
        return points.contiguous(), normals

    def probes(self, points, normals=None, samples: int = 1024, mode: str = "sphere", max_depth: int = 50,
               background=(0.7, 0.8, 1.0), t_min: float = 1e-5, base_seed: int = 0, batch_probes: int = 0,
               plain: bool = False, env: Optional[Env] = None, lights: Optional[LightSampler] = None,
               lighting: Optional[Lighting] = None):
        """Probe bake on torch tensors of a GPU: points (n, 3) float64; with mode="hemisphere", normals
        (n, 3) float64 unit vectors on the points' device (None with mode="sphere"). Runs on the
        points' device and its current stream and does not synchronise; the scene is uploaded there
        first if it is not yet (that blocks). Returns an (n, 9, 3) float64 tensor of SH coefficients
        (sphere; sh_eval evaluates them) or (n, 1, 3) of irradiance (hemisphere). env (make_env, on the
        points' device): the environment in place of `background`, as in radiance. lights, lighting: as in
        radiance."""
        import torch
        if env is not None and not isinstance(env, Env):
            raise CrtError("probes: env must be an Env (make_env)")
        points, normals = self._probe_inputs("probes", points, normals, mode)
        n, device = points.shape[0], points.device.index
        lit = _lighting_on("probes", lighting, env, lights, self, device)
        lh = _lights_on("probes", lights, env, self, device)
        view = _env_on("probes", env, device) if env is not None else None
        with torch.cuda.device(device):
            out = torch.empty((n, 9 if mode == "sphere" else 1, 3), dtype=torch.float64, device=points.device)
            if n:
                self.upload(device)
                self.probes_async(device, points.data_ptr(), normals.data_ptr() if normals is not None else 0, n,
                                  out.data_ptr(), samples=samples, mode=mode, max_depth=max_depth, background=background,
                                  t_min=t_min, base_seed=base_seed, batch_probes=batch_probes,
                                  flags=CRT_RADIANCE_PLAIN if plain else 0,
                                  stream=torch.cuda.current_stream(device).cuda_stream, env=view,
                                  sampler=(env.sampler or 0) if env is not None else 0, lights=lh, lighting=lit)
            return out

    def probe_rays(self, points, normals=None, samples: int = 1024, mode: str = "sphere", base_seed: int = 0):
        """The rays and LCG states a bake of these probes traces (crt_probe_rays_async), on the points'
        device and its current stream, without synchronising: (rays (n * samples, 6) float64, states
        (n * samples,) int32), record probe * samples + sample. radiance(rays, states, ...) is the
        per-sample radiance that probes(...) reduces."""
        import torch
        points, normals = self._probe_inputs("probe_rays", points, normals, mode)
        n, device = points.shape[0], points.device.index
        prm = self._probe_params(samples, mode, 1, (0.0, 0.0, 0.0), 1e-5, base_seed, 0, 0)
        with torch.cuda.device(device):
            records = n * samples if n else 0
            rays = torch.empty((records, 6), dtype=torch.float64, device=points.device)
            states = torch.empty((records,), dtype=torch.int32, device=points.device)
            if n:
                check(lib().crt_probe_rays_async(device, C.c_void_p(points.data_ptr()),
                                                 C.c_void_p(normals.data_ptr() if normals is not None else None), n,
                                                 C.byref(prm), C.c_void_p(rays.data_ptr() or None),
                                                 C.c_void_p(states.data_ptr() or None),
                                                 C.c_void_p(torch.cuda.current_stream(device).cuda_stream)),
                      "crt_probe_rays_async")
            return rays, states

    def camera_rays(self, cam: Camera, first_sample: int = 0, num_samples: Optional[int] = None,
                    tiling: Optional[Tiling] = None, device: int = 0):
        """The camera's own rays and the LCG states after their draws (crt_camera_rays_async), on
        `device` and its current stream, without synchronising: (rays (n, 6) float64, states (n,)
        int32) for the tiling's owned pixels (None: the whole frame; owned rows in order, packed) and
        samples [first_sample, first_sample + num_samples) (None: up to cam.samples_per_pixel), record
        pixel * num_samples + (sample - first_sample). radiance(rays, states, cam.max_depth,
        cam.background, cam.t_min) is then the per-sample radiance of a render with cam."""
        import torch
        from .tiles import owned_rows
        if not isinstance(cam, Camera):
            raise CrtError("camera_rays: cam must be a resolved Camera (resolve_camera)")
        if num_samples is None:
            num_samples = cam.samples_per_pixel - first_sample
        if first_sample < 0 or num_samples < 0:
            raise CrtError("camera_rays: first_sample and num_samples must not be negative")
        if first_sample + num_samples > 0xFFFFFFFF:
            raise CrtError("camera_rays: first_sample + num_samples exceeds 2^32-1")
        rows = cam.image_h
        if tiling is not None:
            if not isinstance(tiling, Tiling) or tiling.row_block == 0 or tiling.tile_index >= tiling.tile_count:
                raise CrtError("camera_rays: bad tiling")
            rows = len(owned_rows(cam.image_h, tiling.row_block, tiling.tile_count, tiling.tile_index))
        n = rows * cam.image_w * num_samples
        with torch.cuda.device(device):
            dev = torch.device("cuda", device)
            rays = torch.empty((n, 6), dtype=torch.float64, device=dev)
            states = torch.empty((n,), dtype=torch.int32, device=dev)
            if n:
                check(lib().crt_camera_rays_async(device, C.byref(cam), C.byref(tiling) if tiling is not None else None,
                                                  first_sample, num_samples, C.c_void_p(rays.data_ptr()),
                                                  C.c_void_p(states.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream(device).cuda_stream)),
                      "crt_camera_rays_async")
            return rays, states

    def lens_rays(self, cam: Camera, lens: Lens, first_sample: int = 0, num_samples: Optional[int] = None,
                  device: int = 0):
        """The rays a lens render of the whole frame traces and the LCG states after their draws
        (crt_lens_rays_async), on `device` and its current stream, without synchronising: (rays (n, 6)
        float64, states (n,) int32) for samples [first_sample, first_sample + num_samples) (None: up to
        cam.samples_per_pixel), record (row * image_w + col) * num_samples + (sample - first_sample).
        radiance(rays, states, cam.max_depth, cam.background, cam.t_min) is the per-sample radiance
        that render_lens reduces."""
        import torch
        if not isinstance(cam, Camera) or not isinstance(lens, Lens):
            raise CrtError("lens_rays: cam must be a resolved Camera (resolve_camera) and lens a Lens (make_lens)")
        if num_samples is None:
            num_samples = cam.samples_per_pixel - first_sample
        if first_sample < 0 or num_samples < 0:
            raise CrtError("lens_rays: first_sample and num_samples must not be negative")
        if first_sample + num_samples > 0xFFFFFFFF:
            raise CrtError("lens_rays: first_sample + num_samples exceeds 2^32-1")
        n = cam.image_h * cam.image_w * num_samples
        if n > 0x7FFFFFFF:
            raise CrtError("lens_rays: more than 2^31-1 records")
        with torch.cuda.device(device):
            dev = torch.device("cuda", device)
            rays = torch.empty((n, 6), dtype=torch.float64, device=dev)
            states = torch.empty((n,), dtype=torch.int32, device=dev)
            if n:
                check(lib().crt_lens_rays_async(device, C.byref(cam), C.byref(lens), first_sample, num_samples,
                                                C.c_void_p(rays.data_ptr()), C.c_void_p(states.data_ptr()),
                                                C.c_void_p(torch.cuda.current_stream(device).cuda_stream)),
                      "crt_lens_rays_async")
            return rays, states

    def render_lens_async(self, device: int, cam: Camera, lens: Lens, out_ptr: int, stream: int = 0,
                          env: Optional[EnvView] = None, sampler: int = 0, lights: int = 0,
                          lighting: Optional[LightingView] = None) -> None:
        """Enqueue a whole-frame render through `lens` (crt_render_lens_async) into the device buffer
        at out_ptr (image_h * image_w * 3 doubles): the rays of lens_rays, traced as radiance_async
        traces them and summed per pixel in render_async's order. The scene must be uploaded to
        `device`. env, sampler: as radiance_async's (crt_render_lens_env_async,
        crt_render_lens_env_sampled_async). lights: as radiance_async's (crt_render_lens_lights_async).
        lighting: as radiance_async's (crt_render_lens_lit_async)."""
        if lighting is not None:
            if env is not None or sampler or lights:
                raise ValueError("render_lens_async: lighting= cannot be combined with env=, sampler= or lights=")
            check(lib().crt_render_lens_lit_async(self._h, device, C.byref(cam), C.byref(lens), C.byref(lighting),
                                                  C.c_void_p(out_ptr or None), C.c_void_p(stream)),
                  "crt_render_lens_lit_async")
            return
        if lights:
            check(lib().crt_render_lens_lights_async(self._h, device, C.byref(cam), C.byref(lens), C.c_void_p(lights),
                                                     C.c_void_p(out_ptr or None), C.c_void_p(stream)),
                  "crt_render_lens_lights_async")
            return
        if sampler:
            check(lib().crt_render_lens_env_sampled_async(self._h, device, C.byref(cam), C.byref(lens),
                                                          C.c_void_p(sampler), C.c_void_p(out_ptr or None),
                                                          C.c_void_p(stream)), "crt_render_lens_env_sampled_async")
            return
        if env is not None:
            check(lib().crt_render_lens_env_async(self._h, device, C.byref(cam), C.byref(lens), C.byref(env),
                                                  C.c_void_p(out_ptr or None), C.c_void_p(stream)),
                  "crt_render_lens_env_async")
            return
        check(lib().crt_render_lens_async(self._h, device, C.byref(cam), C.byref(lens), C.c_void_p(out_ptr or None),
                                          C.c_void_p(stream)), "crt_render_lens_async")

    def render_lens(self, cam: Camera, lens: Lens, device: int = 0, env: Optional[Env] = None,
                    lights: Optional[LightSampler] = None, lighting: Optional[Lighting] = None):
        """Whole-frame render through `lens` (make_lens) into an (h, w, 3) float64 torch tensor on
        `device`. Runs on that device's current stream and does not synchronise; the scene is uploaded
        there first if it is not yet (that blocks). With kind "pinhole" the frame is render_async's,
        bit for bit. env (make_env, on `device`): the environment in place of cam.background, as in
        radiance. lights, lighting: as in radiance."""
        import torch
        if not isinstance(cam, Camera) or not isinstance(lens, Lens):
            raise CrtError("render_lens: cam must be a resolved Camera (resolve_camera) and lens a Lens (make_lens)")
        lit = _lighting_on("render_lens", lighting, env, lights, self, device)
        lh = _lights_on("render_lens", lights, env, self, device)
        view = _env_on("render_lens", env, device) if env is not None else None
        with torch.cuda.device(device):
            out = torch.empty((cam.image_h, cam.image_w, 3), dtype=torch.float64, device=torch.device("cuda", device))
            self.upload(device)
            self.render_lens_async(device, cam, lens, out.data_ptr(), torch.cuda.current_stream(device).cuda_stream,
                                   env=view, sampler=(env.sampler or 0) if env is not None else 0, lights=lh,
                                   lighting=lit)
            return out

    def render_lens_pass(self, device: int, cam: Camera, lens: Lens, first: int, count: int, sum_ptr: int,
                         noise_ptr: int = 0, out_ptr: int = 0, blocks_ptr: int = 0, active_hint: int = 0,
                         stream: int = 0, lighting=None) -> None:
        """Samples [first, first + count) of a cam.samples_per_pixel lens render of the whole frame into
        the running sums at sum_ptr (crt_render_lens_pass_async; render_pass's buffers and boundaries).
        With blocks_ptr (one uint32 per 16 x 4 block of the frame) only the blocks whose word equals
        `first` are generated and traced, and the call waits for the stream once to read how many
        pixels that is; without it the call only enqueues. active_hint never changes the result.
        lighting: a Lighting (or a LightingView) of this scene on `device`: the samples are lit by it
        (crt_render_lens_pass_lit_async); Lighting() with nothing set gives the unlit pass's bytes."""
        if lighting is not None:
            lit = lighting if isinstance(lighting, LightingView) else _lighting_on("render_lens_pass", lighting, None,
                                                                                   None, self, device)
            check(lib().crt_render_lens_pass_lit_async(self._h, device, C.byref(cam), C.byref(lens), C.byref(lit), first,
                                                       count, C.c_void_p(sum_ptr or None), C.c_void_p(noise_ptr or None),
                                                       C.c_void_p(out_ptr or None), C.c_void_p(blocks_ptr or None),
                                                       min(active_hint, 0xFFFFFFFF), C.c_void_p(stream)),
                  "crt_render_lens_pass_lit_async")
            return
        check(lib().crt_render_lens_pass_async(self._h, device, C.byref(cam), C.byref(lens), first, count,
                                               C.c_void_p(sum_ptr or None), C.c_void_p(noise_ptr or None),
                                               C.c_void_p(out_ptr or None), C.c_void_p(blocks_ptr or None),
                                               min(active_hint, 0xFFFFFFFF), C.c_void_p(stream)),
              "crt_render_lens_pass_async")

    def lens_centre_rays(self, cam: Camera, lens: Lens, device: int = 0):
        """The rays through the pixel centres of a lens frame (crt_lens_centre_rays_async), the rays
        lens_features traces: an (h * w, 6) float64 torch tensor on `device`, record row * w + col.
        Runs on the device's current stream and does not synchronise."""
        import torch
        if not isinstance(cam, Camera) or not isinstance(lens, Lens):
            raise CrtError("lens_centre_rays: cam must be a resolved Camera (resolve_camera) and lens a Lens (make_lens)")
        with torch.cuda.device(device):
            rays = torch.empty((cam.image_h * cam.image_w, 6), dtype=torch.float64, device=torch.device("cuda", device))
            check(lib().crt_lens_centre_rays_async(device, C.byref(cam), C.byref(lens), C.c_void_p(rays.data_ptr() or None),
                                                   C.c_void_p(torch.cuda.current_stream(device).cuda_stream)),
                  "crt_lens_centre_rays_async")
            return rays

    def lens_features(self, device: int, cam: Camera, lens: Lens, feat_ptr: int, stream: int = 0) -> None:
        """Enqueue the first-hit features of a lens frame (crt_lens_features_async) into the device
        buffer at feat_ptr: one 88-byte crt_feature (FEATURE_DTYPE) per pixel, row-major."""
        check(lib().crt_lens_features_async(self._h, device, C.byref(cam), C.byref(lens), C.c_void_p(feat_ptr or None),
                                            C.c_void_p(stream)), "crt_lens_features_async")

    def render_lens_passes(self, cam: Camera, lens: Lens, threshold: Optional[float] = None, min_samples: int = 0,
                           samples_per_pass: int = 0, params: Optional[DenoiseParams] = None, denoise: bool = False,
                           callback=None, preview: bool = False, noisy: bool = False, counts: bool = False,
                           device: int = 0, lighting: Optional[Lighting] = None):
        """Blocking lens render in passes on `device` (crt_render_lens_passes): plain passes, or with
        `threshold` adaptive ones (render_adaptive's rule); with denoise=True (or `params`) the frame is
        filtered (a cube map one face at a time). Returns render_denoised's shape: (frame, unfiltered
        frame or None, samples rendered over all pixels), with counts=True also the blocks' sample
        counts. The frame is the denoised one with denoise, else the unfiltered one (noisy=True then
        needs denoise). callback(samples_done, samples_total, active_blocks, total_blocks, noisy,
        frame) runs after every pass; a true return stops the render. preview=True (needs
        `threshold`; min_samples >= the job's samples renders plain passes) hands every call the
        frames of the state so far (views of the returned arrays), else both are None. lighting (a
        Lighting): every pass is lit by it (crt_render_lens_passes_lit: the call copies the map's texels
        to the host and makes its own samplers for its duration; the features keep the background)."""
        denoise = denoise or params is not None
        if lighting is not None and not isinstance(lighting, Lighting):
            raise CrtError("render_lens_passes: lighting must be a Lighting")
        if lighting is not None and lighting.lights is not None and (lighting.lights.scene is not self or
                                                                     lighting.lights.device != device):
            raise CrtError("render_lens_passes: the LightSampler belongs to another scene or device (it is on device "
                           f"{lighting.lights.device})")
        if preview and threshold is None:
            raise CrtError("render_lens_passes: preview needs an adaptive render (threshold; min_samples >= the job's "
                           "samples renders plain passes)")
        if noisy and not denoise:
            raise CrtError("render_lens_passes: noisy=True needs denoise (without it the frame is the unfiltered one)")
        out = np.empty((cam.image_h, cam.image_w, 3), np.float64)
        raw = np.empty_like(out) if noisy else None
        prm = (params if params is not None else denoise_params()) if denoise else None
        ad = None
        if threshold is not None:
            ad = _capi.AdaptiveParams(threshold, min_samples, samples_per_pass,
                                      _capi.CRT_PROGRESS_PREVIEW if preview else 0, 0)
        elif samples_per_pass or min_samples:
            raise CrtError("render_lens_passes: samples_per_pass and min_samples need `threshold`")
        blocks = np.zeros(((cam.image_h + 3) // 4, (cam.image_w + 15) // 16), np.uint32)
        rendered = C.c_uint64(0)
        raised = []

        def trampoline(_user, done, total, active, nblocks, h_noisy, h_rgb):
            try:
                return 1 if callback(done, total, active, nblocks, raw if h_noisy else None, out if h_rgb else None) else 0
            except BaseException as e:  # not through the C frames: stop, raise after the call
                raised.append(e)
                return 1

        fn = _capi.DENOISED_FN(trampoline) if callback is not None else _capi.DENOISED_FN()
        tail = (C.byref(ad) if ad is not None else None, C.byref(prm) if prm is not None else None, fn, None,
                raw.ctypes.data if noisy else None, out.ctypes.data, blocks.ctypes.data, C.byref(rendered))
        if lighting is not None:
            what = "crt_render_lens_passes_lit"
            host_env, texels = None, None
            if lighting.env is not None:
                view = _env_on("render_lens_passes", lighting.env, device)
                texels = np.ascontiguousarray(lighting.env.texels.cpu().numpy())  # the entry takes HOST texels
                host_env = EnvView(texels.ctypes.data, view.face_size, view.filter, view.right, view.up, view.forward)
            rc = lib().crt_render_lens_passes_lit(self._h, device, C.byref(cam), C.byref(lens),
                                                  C.byref(host_env) if host_env is not None else None,
                                                  1 if lighting.env is not None and lighting.env.sampler else 0,
                                                  1 if lighting.lights is not None else 0, *tail)
        else:
            what = "crt_render_lens_passes"
            rc = lib().crt_render_lens_passes(self._h, device, C.byref(cam), C.byref(lens), *tail)
        if raised:
            raise raised[0]
        check(rc, what)
        return (out, raw, int(rendered.value), blocks) if counts else (out, raw, int(rendered.value))


def __getattr__(name):
    # LensRender lives in lens_passes.py, which imports this module: resolved on first use
    if name == "LensRender":
        from .lens_passes import LensRender
        return LensRender
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
