"""An adaptive render driven pass by pass on one device: blocks of 16 x 4 pixels stop between
passes once their noise is low enough, and later passes trace the others only.

AdaptiveRender works on ProgressiveRender's buffers (running sums, noise state, frame) plus the
block state: one uint32 per block, the samples accumulated in its pixels and CRT_BLOCK_STOPPED.
step() is one masked pass (crt_render_pass_masked_async) and one update (crt_adaptive_update). A
block that stops after n samples holds, bit for bit, what ProgressiveRender holds after n samples,
and its pixels in the frame are its sums times 1 / n.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import CRT_BLOCK_STOPPED, Camera, CrtError, GpuScene, Tiling, adaptive_update, block_count, sample_chunk_len
from .progressive import ProgressiveRender, _resume_job

BLOCK_W, BLOCK_H = 16, 4


def _check_tiling(tiling: Optional[Tiling]) -> None:
    if tiling is None:
        return
    if tiling.row_block == 0 or tiling.tile_count == 0 or tiling.tile_index >= tiling.tile_count:
        raise CrtError("AdaptiveRender: bad tiling")
    if tiling.tile_count != 1 and tiling.row_block % BLOCK_H:
        raise CrtError("AdaptiveRender: the tiling needs tile_count == 1 or row_block a multiple of 4")


def _rank_rows(height: int, tiling: Optional[Tiling]) -> int:
    """The rows the block state covers (one word per 16 x 4 block of them) and sample_map() lists:
    the rows the tiling owns, packed or not, the whole frame with no tiling."""
    # not progressive._owned_rows: an unpacked tiling's pixel buffers hold the whole frame, while
    # its blocks are numbered over the owned rows only; the two agree for None and packed tilings
    if tiling is None:
        return height
    return sum(1 for r in range(height) if (r // tiling.row_block) % tiling.tile_count == tiling.tile_index)


class AdaptiveRender(ProgressiveRender):
    """Samples [0, cam.samples_per_pixel) of `scene` on `device`, a step at a time, for the blocks
    still active: a block stops once the sum of its pixels' standard errors is at most `threshold`
    times the sum of their means, not before min_samples samples (and two chunks).
    min_samples >= cam.samples_per_pixel never stops a block."""

    def __init__(self, scene: GpuScene, cam: Camera, threshold: float, min_samples: int = 0, device: int = 0,
                 tiling: Optional[Tiling] = None):
        import torch
        if not (threshold >= 0 and np.isfinite(threshold)):
            raise CrtError("AdaptiveRender: threshold must be finite and >= 0")
        _check_tiling(tiling)
        super().__init__(scene, cam, device, tiling, noise=True)
        self.threshold, self.min_samples = float(threshold), int(min_samples)
        self._rows = _rank_rows(cam.image_h, tiling)
        self.total_blocks = block_count(cam.image_w, self._rows)
        # int32 storage of the uint32 words (the stopped bit is the sign bit)
        self._blocks = torch.zeros(max(1, self.total_blocks), dtype=torch.int32, device=torch.device("cuda", device))
        self.active_blocks = self.total_blocks

    @property
    def finished(self) -> bool:
        return self.samples_done >= self.samples_total or self.active_blocks == 0

    def step(self, count: int = 0):
        """One masked pass of the next `count` samples (rounded as ProgressiveRender.step's) for
        the active blocks, then the stopping rule. Returns the frame so far (the same device tensor
        every call); active_blocks is up to date on return."""
        import torch
        if self.finished:
            raise CrtError("AdaptiveRender.step: the render is finished")
        if count < 0:
            raise CrtError("AdaptiveRender.step: negative count")
        L = self.chunk_len
        count = max(L, (count + L - 1) // L * L)
        count = min(count, self.samples_total - self.samples_done)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
        self.scene.render_pass_masked(self.device, self.cam, self.samples_done, count, self._sum.data_ptr(),
                                      self._noise.data_ptr(), self._out.data_ptr(), self._blocks.data_ptr(),
                                      self.active_blocks, st, self.tiling)
        self.samples_done += count
        self.active_blocks = adaptive_update(self.device, self.cam, self._noise.data_ptr(), self._blocks.data_ptr(),
                                             self.samples_done, self.threshold, self.min_samples, st, self.tiling)
        return self._out

    def noise(self) -> float:
        """Not defined here: the blocks hold different sample counts, so one figure over all
        pixels at samples_done means nothing. The stopping rule works per block (active_blocks,
        sample_map)."""
        raise CrtError("AdaptiveRender.noise: blocks hold different sample counts; see active_blocks / sample_map")

    def _blocks_ptr(self) -> int:
        """denoised() (ProgressiveRender's) takes every pixel's sample count from its block word."""
        return self._blocks.data_ptr()

    def block_words(self) -> np.ndarray:
        """The block state: (block rows, block columns) uint32, counts with CRT_BLOCK_STOPPED."""
        bx = (self.cam.image_w + BLOCK_W - 1) // BLOCK_W
        words = self._blocks[:self.total_blocks].cpu().numpy().view(np.uint32)
        return words.reshape(-1, bx)

    def block_samples(self) -> np.ndarray:
        """The blocks' sample counts (the stopped bit cleared)."""
        return self.block_words() & np.uint32(CRT_BLOCK_STOPPED - 1)

    def sample_map(self) -> np.ndarray:
        """Samples per pixel, (rows, w) uint32 over the rows this render owns, in order."""
        per = np.repeat(np.repeat(self.block_samples(), BLOCK_H, axis=0), BLOCK_W, axis=1)
        return np.ascontiguousarray(per[:self._rows, :self.cam.image_w])

    @property
    def samples_rendered(self) -> int:
        """The samples traced so far, over all pixels."""
        return int(self.sample_map().astype(np.uint64).sum())

    def state(self) -> dict:
        d = super().state()
        d["blocks"] = self.block_words().reshape(-1).copy()
        d["threshold"] = self.threshold
        d["min_samples"] = self.min_samples
        return d

    @classmethod
    def resume(cls, scene: GpuScene, cam: Camera, state: dict, device: int = 0) -> "AdaptiveRender":
        """Continue the render of a state() checkpoint of this job (ProgressiveRender.resume's
        rules, and block words that fit the frame and the checkpoint's samples_done)."""
        done, tiling, rows, total = _resume_job("AdaptiveRender", cam, state, _check_tiling)
        L = sample_chunk_len(cam.samples_per_pixel)
        noise = np.asarray(state["noise"]) if "noise" in state else None
        if noise is None or noise.shape != (rows, cam.image_w, 2):
            raise CrtError("AdaptiveRender.resume: the state has no noise state of the job's shape")
        if "blocks" not in state or "threshold" not in state or "min_samples" not in state:
            raise CrtError("AdaptiveRender.resume: not the state of an adaptive render")
        words = np.asarray(state["blocks"]).reshape(-1)
        n_blocks = block_count(cam.image_w, _rank_rows(cam.image_h, tiling))
        if words.shape != (n_blocks,) or words.dtype != np.uint32:
            raise CrtError(f"AdaptiveRender.resume: the state has {words.size} block words, the job {n_blocks}")
        counts = words & np.uint32(CRT_BLOCK_STOPPED - 1)
        stopped = (words & np.uint32(CRT_BLOCK_STOPPED)) != 0
        if (counts > done).any() or (counts[~stopped] != done).any() or (counts % L != 0)[counts != cam.samples_per_pixel].any():
            raise CrtError("AdaptiveRender.resume: the block words do not fit samples_done")
        import torch
        r = cls(scene, cam, float(state["threshold"]), int(state["min_samples"]), device, tiling)
        r._sum.copy_(torch.from_numpy(np.ascontiguousarray(total)))
        r._noise.copy_(torch.from_numpy(np.ascontiguousarray(noise.astype(np.float64))))
        r._blocks[:n_blocks].copy_(torch.from_numpy(words.view(np.int32).copy()))
        r.samples_done = done
        r.active_blocks = int((~stopped).sum()) if done else n_blocks
        return r
