"""A render driven pass by pass on one device: previews, a noise readout, checkpoint and resume.

ProgressiveRender keeps the pixels' running sums (and the noise state) in device tensors and
issues crt_render_pass_async passes in order at chunk boundaries, so the frame after the last pass
is bit-identical to GpuScene.render_async's. state() / resume() carry a render across processes:
the sums are copied exactly, so a resumed render ends on the same bits too.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import (FEATURE_DTYPE, Camera, CrtError, GpuScene, Tiling, denoise, denoise_params, noise_estimate,
               pixel_variance, sample_chunk_len)


def _owned_rows(height: int, tiling: Optional[Tiling]) -> int:
    """The rows of the pixel buffers (running sums, noise state, frame): the whole frame with no
    tiling and with an unpacked one (the owned rows stay at their frame rows), the owned rows only
    with a packed one."""
    if tiling is None or not (tiling.flags & 1):  # CRT_TILING_PACKED
        return height
    return sum(1 for r in range(height) if (r // tiling.row_block) % tiling.tile_count == tiling.tile_index)


def _resume_job(name: str, cam: Camera, state: dict, check_tiling=None):
    """What every resume() checks of a state() checkpoint against `cam`: the job, samples_done at a
    pass boundary, the tiling (check_tiling, if any, sees it before it is used) and the sums' shape.
    name: the class, for the error texts. Returns (samples_done, tiling, buffer rows, sums)."""
    for key, want in (("spp", cam.samples_per_pixel), ("base_seed", cam.base_seed),
                      ("width", cam.image_w), ("height", cam.image_h)):
        got = int(state[key])
        if got != int(want):
            raise CrtError(f"{name}.resume: the state's {key} is {got}, the camera's {int(want)}")
    done = int(state["samples_done"])
    L = sample_chunk_len(cam.samples_per_pixel)
    if done < 0 or done > cam.samples_per_pixel or (done % L and done != cam.samples_per_pixel):
        raise CrtError(f"{name}.resume: samples_done = {done} is not a pass boundary")
    tl = [int(v) for v in np.asarray(state["tiling"]).reshape(-1)]
    tiling = None if tl == [1, 1, 0, 0] else Tiling(*tl)
    if check_tiling is not None:
        check_tiling(tiling)
    rows = _owned_rows(cam.image_h, tiling)
    total = np.asarray(state["sum"])
    if total.shape != (rows, cam.image_w, 3) or total.dtype != np.float64:
        raise CrtError(f"{name}.resume: the state's sums have shape {total.shape}, "
                       f"the job's {(rows, int(cam.image_w), 3)}")
    return done, tiling, rows, total


class ProgressiveRender:
    """Samples [0, cam.samples_per_pixel) of `scene` on `device`, a step at a time.

    tiling: the rows this render owns (crt_tiling semantics; with CRT_TILING_PACKED the buffers
    hold the owned rows only). noise=False drops the noise state (2 doubles a pixel)."""

    def __init__(self, scene: GpuScene, cam: Camera, device: int = 0, tiling: Optional[Tiling] = None,
                 noise: bool = True):
        import torch
        if cam.samples_per_pixel == 0:
            raise CrtError("ProgressiveRender: samples_per_pixel is 0")
        self.scene, self.cam, self.device, self.tiling = scene, cam, device, tiling
        self.chunk_len = sample_chunk_len(cam.samples_per_pixel)
        self.samples_done = 0
        scene.upload(device)
        rows = _owned_rows(cam.image_h, tiling)
        dev = torch.device("cuda", device)
        self._sum = torch.zeros(rows, cam.image_w, 3, dtype=torch.float64, device=dev)
        self._noise = torch.zeros(rows, cam.image_w, 2, dtype=torch.float64, device=dev) if noise else None
        self._out = torch.zeros(rows, cam.image_w, 3, dtype=torch.float64, device=dev)

    @property
    def samples_total(self) -> int:
        return int(self.cam.samples_per_pixel)

    @property
    def finished(self) -> bool:
        return self.samples_done >= self.samples_total

    def step(self, count: int = 0):
        """Render the next `count` samples per pixel, rounded up to whole chunks and cut at the
        job's end (0: one chunk). Returns the frame so far: the same device tensor every call,
        (rows, w, 3) float64, valid once the current stream reaches this point."""
        import torch
        if self.finished:
            raise CrtError("ProgressiveRender.step: every sample is already rendered")
        if count < 0:
            raise CrtError("ProgressiveRender.step: negative count")
        L = self.chunk_len
        count = max(L, (count + L - 1) // L * L)
        count = min(count, self.samples_total - self.samples_done)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
        self.scene.render_pass(self.device, self.cam, self.samples_done, count, self._sum.data_ptr(),
                               self._noise.data_ptr() if self._noise is not None else 0,
                               self._out.data_ptr(), st, self.tiling)
        self.samples_done += count
        return self._out

    def noise(self) -> float:
        """The frame's relative noise so far: the pixels' standard errors summed over their means
        summed (crt_noise_estimate). NaN before two chunks are done."""
        import torch
        if self._noise is None:
            raise CrtError("ProgressiveRender.noise: built with noise=False")
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
        se, mean = noise_estimate(self.device, self._noise.data_ptr(), self._noise.shape[0] * self._noise.shape[1],
                                  self.samples_total, self.samples_done, st)
        return se / mean if mean == mean and mean != 0 else float("nan")

    def _blocks_ptr(self) -> int:
        """The block state whose counts denoised() takes the pixels' sample counts from (0: every
        pixel has samples_done samples)."""
        return 0

    def features(self):
        """The first-hit features of the frame (crt_render_features_async), computed once per
        render object: a device tensor of h * w 88-byte records (FEATURE_DTYPE) as uint8."""
        import torch
        if self.tiling is not None and self.tiling.tile_count != 1:
            raise CrtError("ProgressiveRender.features: needs a render of the whole frame (one tile)")
        if getattr(self, "_feat", None) is None:
            dev = torch.device("cuda", self.device)
            feat = torch.zeros(self.cam.image_h * self.cam.image_w, FEATURE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            with torch.cuda.device(self.device):
                st = torch.cuda.current_stream().cuda_stream
            self.scene.render_features(self.device, self.cam, feat.data_ptr(), st)
            self._feat = feat
        return self._feat

    def denoised(self, params=None):
        """The denoised frame of the state so far (the preview between passes): the frame of the
        last step() filtered by crt_denoise_async with the variance crt_pixel_variance_async takes
        from the noise state. Returns a device tensor (h, w, 3) float64, the same one every call,
        valid once the current stream reaches this point. params: denoise_params(...)."""
        import torch
        if self._noise is None:
            raise CrtError("ProgressiveRender.denoised: built with noise=False (the variance comes from the noise state)")
        if self.samples_done == 0:
            raise CrtError("ProgressiveRender.denoised: no pass rendered yet")
        feat = self.features()
        if getattr(self, "_var", None) is None:
            dev = torch.device("cuda", self.device)
            self._var = torch.zeros(self.cam.image_h, self.cam.image_w, dtype=torch.float64, device=dev)
            self._den = torch.zeros(self.cam.image_h, self.cam.image_w, 3, dtype=torch.float64, device=dev)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
        pixel_variance(self.device, self.cam, self._noise.data_ptr(), self._var.data_ptr(), self.samples_done,
                       self._blocks_ptr(), st, self.tiling)
        denoise(self.device, self.cam.image_w, self.cam.image_h, self._out.data_ptr(), self._var.data_ptr(),
                feat.data_ptr(), params if params is not None else denoise_params(), self._den.data_ptr(), 0, st)
        return self._den

    def state(self) -> dict:
        """A checkpoint: the running sums (and noise state) as numpy arrays, and what identifies
        the job. np.savez(path, **state) stores it."""
        t = self.tiling
        d = {
            "sum": self._sum.cpu().numpy(),
            "samples_done": self.samples_done,
            "spp": self.samples_total,
            "base_seed": int(self.cam.base_seed),
            "width": int(self.cam.image_w),
            "height": int(self.cam.image_h),
            "tiling": np.array([t.row_block, t.tile_count, t.tile_index, t.flags] if t is not None else [1, 1, 0, 0],
                               np.uint32),
        }
        if self._noise is not None:
            d["noise"] = self._noise.cpu().numpy()
        return d

    @classmethod
    def resume(cls, scene: GpuScene, cam: Camera, state: dict, device: int = 0) -> "ProgressiveRender":
        """Continue the render of a state() checkpoint. The state must be of this job: the same
        samples per pixel (they fix the chunking), base seed and frame size as `cam`."""
        done, tiling, _, total = _resume_job("ProgressiveRender", cam, state)
        import torch
        r = cls(scene, cam, device, tiling, noise="noise" in state)
        r._sum.copy_(torch.from_numpy(np.ascontiguousarray(total)))
        if r._noise is not None:
            r._noise.copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(state["noise"], np.float64))))
        r.samples_done = done
        return r
