"""The coloured scene point cloud of demo.py:121-127 / :193, and a bounded map of it on the device.

`frame_cloud` is the reference's per-frame `xyzrgb`: the image resized to the depth size as PIL does
(bf_resize_bicubic_u8), `torch.cat((xyz, image / 255.0), -1)[valid]` as one stable compaction
(bf_cloud_pack).  The reference gets its scene from rerun accumulating those points over time; a
headless run has no viewer, so `SceneCloud` does the accumulation: a voxel hash map of fixed
capacity whose per-voxel state is integers only (point count, sums of the points' 1/256-voxel
offsets, sums of their colours), so what it holds after a set of frames is the same bits whatever
order the frames, or the waves inside a launch, arrive in ("Scene cloud").
"""
from __future__ import annotations

import numpy as np
import torch

from boxfusion_amd import _abi, _lib

KEY_BITS = _abi.constants()["BF_KEY_BITS"]          # voxel indices are stored biased, KEY_BITS per axis
KEY_BIAS, KEY_MASK = _abi.constants()["BF_KEY_BIAS"], (1 << KEY_BITS) - 1


def _batched(xyz, valid, rgb_u8):
    if xyz.dim() == 3:
        xyz, valid, rgb_u8 = xyz[None], valid[None], rgb_u8[None]
    if rgb_u8.dim() != 4 or rgb_u8.shape[-1] != 3 or rgb_u8.shape[0] != xyz.shape[0]:
        raise ValueError(f"rgb_u8: one RGB image [H,W,3] per frame, got {tuple(rgb_u8.shape)} for xyz {tuple(xyz.shape)}")
    H, W = xyz.shape[1:3]
    if tuple(rgb_u8.shape[1:3]) != (H, W):         # demo.py:124: the image at the depth size
        rgb_u8 = _lib.resize_bicubic_u8(rgb_u8, H, W)
    return xyz, valid, rgb_u8


def frame_cloud(xyz, valid, rgb_u8):
    """demo.py:124-127 for a batch: xyz f32 [B,H,W,3] and valid bool [B,H,W] (unproject's outputs),
    rgb_u8 u8 [B,Hi,Wi,3] at any size (resized to (H, W) as PIL's Image.resize does) -> (xyzrgb f32
    [n,6], offsets int32 [B+1] on the device): frame b's points are rows offsets[b]..offsets[b+1], in
    row-major pixel order.  [H,W,...] inputs are a batch of one.  Reads the total back once to
    trim the rows."""
    xyz, valid, rgb_u8 = _batched(xyz, valid, rgb_u8)
    out, offsets = _lib.cloud_pack(xyz, valid, rgb_u8)
    return out[:int(offsets[-1].item())], offsets


class SceneCloud:
    """A voxel map of the scene's coloured points: one table tensor (int64 [capacity,5]: the voxel
    key, then count / offset sums / colour sums as uint32) and one stats tensor on the device.  The
    map only grows until reset(); a point whose voxel finds no free slot is dropped and counted."""

    def __init__(self, voxel=0.02, capacity=1 << 22, device="cuda", merge=True):
        if not voxel > 0:
            raise ValueError("voxel must be positive")
        self.voxel = float(voxel)
        self.fine_step = np.float32(self.voxel / 256.0)          # what the kernel divides by
        self.device = torch.device(device)
        self.merge = merge
        self.table, self._stats = _lib.cloud_table(capacity, self.device)

    @property
    def capacity(self):
        return self.table.shape[0]

    def reset(self):
        self.table.zero_()
        self.table[:, 0] = -1
        self._stats.zero_()

    def integrate(self, xyz, valid, rgb_u8):
        """add the valid points of xyz f32 [B,H,W,3] / valid bool [B,H,W] / rgb_u8 u8 [B,Hi,Wi,3]
        (frame_cloud's arguments); nothing is read back"""
        xyz, valid, rgb_u8 = _batched(xyz, valid, rgb_u8)
        _lib.cloud_integrate(xyz, valid, rgb_u8, self.fine_step, self.table, self._stats, merge=self.merge)

    def stats(self):
        """the counters so far (one read-back): points stored / skipped as nonfinite / skipped as
        out_of_range (voxel index outside +-2^20) / dropped_full (no slot left for their voxel) /
        saturated (their voxel holds 2^24 points), and runs, the sets of atomic adds issued"""
        v = self._stats.cpu().tolist()
        return dict(zip(_lib.CLOUD_STATS, v))

    def raw(self):
        """the occupied voxels sorted by key, as integers on the device: (key int64 [n], count
        int64 [n], sums int64 [n,6] = offset x y z, colour r g b)"""
        key, count, sums, n = _lib.cloud_extract(self.table)
        n = int(n.item())
        key, order = torch.sort(key[:n])
        u32 = 0xFFFFFFFF
        return key, count[:n][order].long() & u32, sums[:n][order].long() & u32

    def points(self):
        """(xyz f32 [n,3], rgb u8 [n,3], count int32 [n]) sorted by voxel key: the mean position
        ((index * 256 + mean offset + 0.5) * fine_step, in f64 until the cast) and the rounded mean
        colour of every occupied voxel"""
        key, count, sums = self.raw()
        idx = torch.stack([(key >> 2 * KEY_BITS) & KEY_MASK, (key >> KEY_BITS) & KEY_MASK, key & KEY_MASK], 1) - KEY_BIAS
        c = count[:, None]
        xyz = ((idx * 256).double() + sums[:, :3].double() / c.double() + 0.5) * float(self.fine_step)
        rgb = (sums[:, 3:] + c // 2) // c
        return xyz.float(), rgb.to(torch.uint8), count.to(torch.int32)

    def save_ply(self, path):
        from boxfusion_amd.visualize import points_to_ply
        xyz, rgb, _ = self.points()
        points_to_ply(xyz.cpu().numpy(), rgb.cpu().numpy(), path)
        return int(xyz.shape[0])
