"""A lens render driven pass by pass on one device: ProgressiveRender / AdaptiveRender for the frames
of GpuScene.render_lens (panoramic, fisheye, cube-map, orthographic, pinhole).

LensRender keeps the whole frame's running sums, noise state and frame in device tensors and issues
crt_render_lens_pass_async passes in order at chunk boundaries, so the frame after the last pass is
bit-identical to GpuScene.render_lens'. With a threshold it also keeps one word per 16 x 4 block and
applies crt_adaptive_update after every pass: stopped blocks cost no rays. features() and denoised()
go through crt_lens_features_async and the camera-agnostic crt_pixel_variance_async and
crt_denoise_async; a cube map is filtered one face at a time.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import (CRT_BLOCK_STOPPED, CRT_LENS_CUBE, FEATURE_DTYPE, Camera, CrtError, GpuScene, Lens, Lighting, adaptive_update,
               block_count, denoise, denoise_params, noise_estimate, pixel_variance, sample_chunk_len)
from .progressive import _resume_job

BLOCK_W, BLOCK_H = 16, 4


class LensRender:
    """Samples [0, cam.samples_per_pixel) of `scene` through `lens` on `device`, a step at a time, on
    the device's current stream. threshold=None: every pixel gets every sample. Otherwise a block
    stops once the sum of its pixels' standard errors is at most `threshold` times the sum of their
    means, not before min_samples samples (AdaptiveRender's rule). lighting (a Lighting of this scene
    on `device`): every pass is lit by it (crt_render_lens_pass_lit_async); state() does not store it,
    so resume() takes the same one again."""

    def __init__(self, scene: GpuScene, cam: Camera, lens: Lens, threshold: Optional[float] = None, min_samples: int = 0,
                 device: int = 0, lighting=None):
        import torch
        if not isinstance(cam, Camera) or not isinstance(lens, Lens):
            raise CrtError("LensRender: cam must be a resolved Camera (resolve_camera) and lens a Lens (make_lens)")
        if cam.samples_per_pixel == 0:
            raise CrtError("LensRender: samples_per_pixel is 0")
        if threshold is not None and not (threshold >= 0 and np.isfinite(threshold)):
            raise CrtError("LensRender: threshold must be finite and >= 0")
        if lighting is not None and not isinstance(lighting, Lighting):
            raise CrtError("LensRender: lighting must be a Lighting")
        self.scene, self.cam, self.lens, self.device = scene, cam, lens, device
        self.lighting = lighting
        self.threshold = None if threshold is None else float(threshold)
        self.min_samples = int(min_samples)
        self.chunk_len = sample_chunk_len(cam.samples_per_pixel)
        self.samples_done = 0
        scene.upload(device)
        dev = torch.device("cuda", device)
        h, w = cam.image_h, cam.image_w
        self._sum = torch.zeros(h, w, 3, dtype=torch.float64, device=dev)
        self._noise = torch.zeros(h, w, 2, dtype=torch.float64, device=dev)
        self._out = torch.zeros(h, w, 3, dtype=torch.float64, device=dev)
        self.total_blocks = block_count(w, h)
        # int32 storage of the uint32 words (the stopped bit is the sign bit)
        self._blocks = torch.zeros(self.total_blocks, dtype=torch.int32, device=dev) if threshold is not None else None
        self.active_blocks = self.total_blocks
        self._feat = self._var = self._den = None

    def _stream(self) -> int:
        import torch
        with torch.cuda.device(self.device):
            return torch.cuda.current_stream().cuda_stream

    @property
    def samples_total(self) -> int:
        return int(self.cam.samples_per_pixel)

    @property
    def finished(self) -> bool:
        return self.samples_done >= self.samples_total or (self._blocks is not None and self.active_blocks == 0)

    def step(self, count: int = 0):
        """Render the next `count` samples per pixel (of the active blocks), rounded up to whole
        chunks and cut at the job's end (0: one chunk), then with a threshold the stopping rule.
        Returns the frame so far: the same device tensor every call, (h, w, 3) float64."""
        if self.finished:
            raise CrtError("LensRender.step: the render is finished")
        if count < 0:
            raise CrtError("LensRender.step: negative count")
        L = self.chunk_len
        count = max(L, (count + L - 1) // L * L)
        count = min(count, self.samples_total - self.samples_done)
        st = self._stream()
        blocks = self._blocks.data_ptr() if self._blocks is not None else 0
        self.scene.render_lens_pass(self.device, self.cam, self.lens, self.samples_done, count, self._sum.data_ptr(),
                                    self._noise.data_ptr(), self._out.data_ptr(), blocks, self.active_blocks, st,
                                    lighting=self.lighting)
        self.samples_done += count
        if self._blocks is not None:
            self.active_blocks = adaptive_update(self.device, self.cam, self._noise.data_ptr(), blocks, self.samples_done,
                                                 self.threshold, self.min_samples, st)
        return self._out

    def frame(self):
        """The frame so far (the tensor step() returns)."""
        return self._out

    def noise(self) -> float:
        """The frame's relative noise so far (crt_noise_estimate); NaN before two chunks are done.
        Not defined with a threshold: the blocks hold different sample counts."""
        if self._blocks is not None:
            raise CrtError("LensRender.noise: blocks hold different sample counts; see active_blocks / block_samples")
        se, mean = noise_estimate(self.device, self._noise.data_ptr(), self.cam.image_h * self.cam.image_w,
                                  self.samples_total, self.samples_done, self._stream())
        return se / mean if mean == mean and mean != 0 else float("nan")

    def features(self):
        """The first-hit features of the frame through the lens (crt_lens_features_async), computed
        once per render object: a device tensor of h * w 88-byte records (FEATURE_DTYPE) as uint8."""
        import torch
        if self._feat is None:
            feat = torch.zeros(self.cam.image_h * self.cam.image_w, FEATURE_DTYPE.itemsize, dtype=torch.uint8,
                               device=torch.device("cuda", self.device))
            self.scene.lens_features(self.device, self.cam, self.lens, feat.data_ptr(), self._stream())
            self._feat = feat
        return self._feat

    def denoised(self, params=None):
        """The denoised frame of the state so far: the frame of the last step() filtered by
        crt_denoise_async (a cube map one face at a time) with crt_pixel_variance_async's variance.
        Returns a device tensor (h, w, 3) float64, the same one every call."""
        import torch
        if self.samples_done == 0:
            raise CrtError("LensRender.denoised: no pass rendered yet")
        feat = self.features()
        h, w = self.cam.image_h, self.cam.image_w
        if self._var is None:
            dev = torch.device("cuda", self.device)
            self._var = torch.zeros(h, w, dtype=torch.float64, device=dev)
            self._den = torch.zeros(h, w, 3, dtype=torch.float64, device=dev)
        st = self._stream()
        prm = params if params is not None else denoise_params()
        pixel_variance(self.device, self.cam, self._noise.data_ptr(), self._var.data_ptr(), self.samples_done,
                       self._blocks.data_ptr() if self._blocks is not None else 0, st)
        faces = 6 if self.lens.kind == CRT_LENS_CUBE else 1
        fh = h // faces
        for f in range(faces):
            px = f * fh * w
            denoise(self.device, w, fh, self._out.data_ptr() + px * 24, self._var.data_ptr() + px * 8,
                    feat.data_ptr() + px * FEATURE_DTYPE.itemsize, prm, self._den.data_ptr() + px * 24, 0, st)
        return self._den

    def block_words(self) -> np.ndarray:
        """The block state: (block rows, block columns) uint32, counts with CRT_BLOCK_STOPPED (every
        word samples_done without a threshold)."""
        bx = (self.cam.image_w + BLOCK_W - 1) // BLOCK_W
        if self._blocks is None:
            return np.full((self.total_blocks // bx, bx), self.samples_done, np.uint32)
        return self._blocks.cpu().numpy().view(np.uint32).reshape(-1, bx)

    def block_samples(self) -> np.ndarray:
        """The blocks' sample counts (the stopped bit cleared)."""
        return self.block_words() & np.uint32(CRT_BLOCK_STOPPED - 1)

    @property
    def samples_rendered(self) -> int:
        """The samples traced so far, over all pixels."""
        per = np.repeat(np.repeat(self.block_samples(), BLOCK_H, axis=0), BLOCK_W, axis=1)
        return int(per[:self.cam.image_h, :self.cam.image_w].astype(np.uint64).sum())

    def state(self) -> dict:
        """A checkpoint: the running sums, the noise state and the block words as numpy arrays, and
        what identifies the job (ProgressiveRender.state's keys, and the lens' bytes)."""
        d = {
            "sum": self._sum.cpu().numpy(),
            "noise": self._noise.cpu().numpy(),
            "samples_done": self.samples_done,
            "spp": self.samples_total,
            "base_seed": int(self.cam.base_seed),
            "width": int(self.cam.image_w),
            "height": int(self.cam.image_h),
            "tiling": np.array([1, 1, 0, 0], np.uint32),
            "lens": np.frombuffer(bytes(self.lens), np.uint8).copy(),
        }
        if self._blocks is not None:
            d["blocks"] = self.block_words().reshape(-1).copy()
            d["threshold"] = self.threshold
            d["min_samples"] = self.min_samples
        return d

    @classmethod
    def resume(cls, scene: GpuScene, cam: Camera, lens: Lens, state: dict, device: int = 0, lighting=None) -> "LensRender":
        """Continue the render of a state() checkpoint of this job: the same samples per pixel, base
        seed, frame size and lens as `cam` and `lens`, and the lighting the job had (it is not stored)."""
        import torch
        done, tiling, rows, total = _resume_job("LensRender", cam, state)
        if tiling is not None:
            raise CrtError("LensRender.resume: the state has a tiling (lens renders take none)")
        if "lens" not in state or bytes(np.asarray(state["lens"], np.uint8)) != bytes(lens):
            raise CrtError("LensRender.resume: the state's lens is not `lens`")
        noise = np.asarray(state["noise"]) if "noise" in state else None
        if noise is None or noise.shape != (rows, cam.image_w, 2):
            raise CrtError("LensRender.resume: the state has no noise state of the job's shape")
        adaptive = "blocks" in state
        r = cls(scene, cam, lens, float(state["threshold"]) if adaptive else None,
                int(state["min_samples"]) if adaptive else 0, device, lighting)
        r._sum.copy_(torch.from_numpy(np.ascontiguousarray(total)))
        r._noise.copy_(torch.from_numpy(np.ascontiguousarray(noise.astype(np.float64))))
        r.samples_done = done
        if adaptive:
            words = np.asarray(state["blocks"]).reshape(-1)
            if words.shape != (r.total_blocks,) or words.dtype != np.uint32:
                raise CrtError(f"LensRender.resume: the state has {words.size} block words, the job {r.total_blocks}")
            counts = words & np.uint32(CRT_BLOCK_STOPPED - 1)
            stopped = (words & np.uint32(CRT_BLOCK_STOPPED)) != 0
            if (counts > done).any() or (counts[~stopped] != done).any():
                raise CrtError("LensRender.resume: the block words do not fit samples_done")
            r._blocks.copy_(torch.from_numpy(words.view(np.int32).copy()))
            r.active_blocks = int((~stopped).sum()) if done else r.total_blocks
        return r
