"""The scene mesh (`mesh.ply`, the reference's "Reconstructed 3D mesh") from posed depth frames.

The reference's preparation guide leaves this file to open3d (data_process/README.md:48) and
filter_gt_boxes.py reads the scene's points from it.  `TsdfVolume` makes it on the device: a sparse
truncated-signed-distance volume of 8x8x8-voxel blocks in a hash map of fixed capacity whose
per-voxel state is integers only (bf_tsdf_touch / bf_tsdf_update), so what it holds after a set of
frames is the same bits whatever the order or the batching of the frames, and a naive-surface-nets
extractor over it (bf_tsdf_surface_*), whose vertex and face orders are fixed, so the mesh is the
same bits too ("Scene mesh").

`python -m boxfusion_amd.scene_mesh SEQ_DIR` writes SEQ_DIR/mesh.ply for a CA-1M sequence directory
(depth/<i>.png, rgb/<i>.png, K_depth.txt, all_poses.npy: what capture_stream.py:323-338 reads).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from boxfusion_amd import _lib

MAX_FRAMES = _lib.TSDF_MAX_FRAMES       # frames of one launch: the bits of a block's touched word


class TsdfVolume:
    """A TSDF of the scene: keys / touched int64 [capacity], vox int32 [capacity,6,512] and a stats
    tensor on the device (the layout is in _lib.tsdf_volume).  The volume only grows until reset();
    a block that finds no free slot is dropped and counted.  max_weight is the observation count at
    which a voxel refuses further observations (counted in `saturated`)."""

    def __init__(self, voxel=0.02, trunc_voxels=4, capacity=1 << 16, max_depth=10.0, device="cuda",
                 max_weight=_lib.TSDF_MAX_WEIGHT):
        if not voxel > 0:
            raise ValueError("voxel must be positive")
        if not 1 <= int(trunc_voxels) <= 64:
            raise ValueError("trunc_voxels must lie in 1..64")
        if not max_depth > 0:
            raise ValueError("max_depth must be positive")
        if not 1 <= int(max_weight) <= _lib.TSDF_MAX_WEIGHT:
            raise ValueError(f"max_weight must lie in 1..{_lib.TSDF_MAX_WEIGHT}")
        self.voxel = np.float32(voxel)
        self.trunc_voxels, self.max_depth, self.max_weight = int(trunc_voxels), float(max_depth), int(max_weight)
        self.device = torch.device(device)
        self.keys, self.touched, self.vox, self._stats = _lib.tsdf_volume(capacity, self.device)

    @property
    def capacity(self):
        return self.keys.shape[0]

    def reset(self):
        self.keys.fill_(-1)
        self.touched.zero_()
        self.vox.zero_()
        self._stats.zero_()

    def integrate(self, depth_m, K, poses, rgb_u8=None):
        """fuse depth_m f32 [B,H,W] (metres; [H,W] is a batch of one) seen through the pinhole K
        [3,3] from the camera-to-world poses [B,4,4] (array or tensor); rgb_u8 u8 [B,Hi,Wi,3] at any
        size colours the surface (resized to the depth size as PIL's Image.resize does).  Frames
        whose pose has a non-finite entry are skipped and counted; nothing is read back."""
        if depth_m.dim() == 2:
            depth_m = depth_m[None]
        poses = torch.as_tensor(np.asarray(poses, np.float32) if not torch.is_tensor(poses) else poses)
        poses = poses.to(self.device, torch.float32).reshape(-1, 4, 4)
        if rgb_u8 is not None:
            if rgb_u8.dim() == 3:
                rgb_u8 = rgb_u8[None]
            if rgb_u8.dim() != 4 or rgb_u8.shape[-1] != 3 or rgb_u8.shape[0] != depth_m.shape[0]:
                raise ValueError(f"rgb_u8: one RGB image [H,W,3] per frame, got {tuple(rgb_u8.shape)} for depth "
                                 f"{tuple(depth_m.shape)}")
            if tuple(rgb_u8.shape[1:3]) != tuple(depth_m.shape[1:3]):
                rgb_u8 = _lib.resize_bicubic_u8(rgb_u8, *depth_m.shape[1:3])
        if poses.shape[0] != depth_m.shape[0]:
            raise ValueError(f"poses: one [4,4] per frame, got {tuple(poses.shape)} for depth {tuple(depth_m.shape)}")
        K = np.asarray(K.cpu() if torch.is_tensor(K) else K, np.float32).reshape(3, 3)
        intr = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        for a in range(0, depth_m.shape[0], MAX_FRAMES):
            d, p = depth_m[a:a + MAX_FRAMES], poses[a:a + MAX_FRAMES]
            c = None if rgb_u8 is None else rgb_u8[a:a + MAX_FRAMES]
            _lib.tsdf_touch(d, p, intr, self.voxel, self.trunc_voxels, self.max_depth, self.keys, self.touched,
                            self._stats)
            _lib.tsdf_update(d, p, intr, self.voxel, self.trunc_voxels, self.max_depth, self.keys, self.touched,
                             self.vox, self._stats, rgb=c, max_weight=self.max_weight)

    def stats(self):
        """the counters so far (one read-back): blocks claimed, voxel observations stored, frames
        skipped for a non-finite pose (skipped_pose), ray samples whose block index lies outside
        +-2^20 (out_of_range), probes that found no slot for their block (dropped_full) and
        observations refused by a voxel at max_weight (saturated)"""
        return dict(zip(_lib.TSDF_STATS, self._stats.cpu().tolist()))

    def _blocks(self):
        key, slot, n = _lib.tsdf_extract(self.keys)
        n = int(n.item())
        key, order = torch.sort(key[:n])
        return key, slot[:n][order].contiguous()

    def raw(self):
        """the occupied blocks sorted by key, as integers on the device: (key int64 [n], state int32
        [n,6,512] = w, sum q, cw, sum r, sum g, sum b of voxel x + 8 y + 64 z)"""
        key, slot = self._blocks()
        return key, self.vox[slot.long()]

    def mesh(self):
        """(vertices f32 [n,3], rgb u8 [n,3], faces int32 [m,3]) on the device: naive surface nets,
        vertices in (block key, cell) order and faces in (block key, cell, axis) order"""
        key, slot = self._blocks()
        return _lib.tsdf_surface(self.keys, self.vox, key, slot, self.voxel)

    def raycast(self, poses, K, H, W, near=0.05, far=None, min_weight=1, colour=False):
        """the volume seen from the camera-to-world poses [V,4,4] (or [4,4]) through the pinhole K at H x W
        (bf_tsdf_raycast): depth f32 [V,H,W] (0: no hit), world vertex and normal f32 [V,H,W,3], rgb u8
        [V,H,W,3] with colour=True else None, and counters int64 [8] (_lib.TSDF_RAYCAST_STATS), all on
        the device.  far defaults to max_depth; a view with a non-finite pose is all zero and counted."""
        poses = torch.as_tensor(np.asarray(poses, np.float32) if not torch.is_tensor(poses) else poses)
        poses = poses.to(self.device, torch.float32).reshape(-1, 4, 4)
        K = np.asarray(K.cpu() if torch.is_tensor(K) else K, np.float32).reshape(3, 3)
        far = self.max_depth if far is None else float(far)
        if not 0 <= near < far or int(min_weight) < 1:
            raise ValueError("raycast: 0 <= near < far and min_weight >= 1")
        # every step is at least a quarter voxel long: the range in quarter voxels bounds the march
        steps = int(min(max(np.ceil((far - float(near)) / (0.25 * float(self.voxel))) + 16, 16), 1 << 20))
        counters = torch.zeros(_lib.STATS_WORDS, dtype=torch.int64, device=self.device)
        d, v, n, c = _lib.tsdf_raycast(self.keys, self.vox, poses, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), H, W, self.voxel,
                                       self.trunc_voxels, near, far, min_weight, steps, counters, colour=colour)
        return d, v, n, c, counters

    def save_ply(self, path):
        from boxfusion_amd.visualize import mesh_to_ply
        v, c, f = self.mesh()
        mesh_to_ply(v.cpu().numpy(), c.cpu().numpy(), f.cpu().numpy(), path)
        return int(v.shape[0]), int(f.shape[0])

    def stats_line(self):
        return " ".join(f"{k}={v}" for k, v in self.stats().items())


# ---- command line -------------------------------------------------------------------------------------
def add_volume_arguments(p):
    p.add_argument("--voxel", type=float, default=0.02, help="voxel edge in metres")
    p.add_argument("--trunc-voxels", type=int, default=4, help="truncation distance in voxels")
    p.add_argument("--start", type=int, default=0)
    p.add_argument("--stop", type=int, default=None)
    p.add_argument("--step", type=int, default=1)
    p.add_argument("--max-depth", type=float, default=10.0)
    p.add_argument("--capacity", type=int, default=1 << 16, help="blocks of 8x8x8 voxels, a power of two")


def check_volume_arguments(p, a):
    if not a.voxel > 0:
        p.error("--voxel must be positive")
    if not 1 <= a.trunc_voxels <= 64:
        p.error("--trunc-voxels must lie in 1..64")
    if a.step < 1:
        p.error("--step must be at least 1")
    if not a.max_depth > 0:
        p.error("--max-depth must be positive")
    if a.capacity <= 0 or a.capacity & (a.capacity - 1) or a.capacity >= 1 << 31:
        p.error("--capacity must be a power of two below 2^31")


def sequence_frames(seq_dir):
    """the rgb/<i>.png and depth/<i>.png paths of a CA-1M sequence directory, each sorted by the
    integer in the name (capture_stream.py:323-327)"""
    def numbered(sub):
        d = os.path.join(seq_dir, sub)
        names = [n for n in (os.listdir(d) if os.path.isdir(d) else []) if n.endswith(".png") and n[:-4].isdigit()]
        return [os.path.join(d, n) for n in sorted(names, key=lambda n: int(n[:-4]))]
    return numbered("rgb"), numbered("depth")


def fuse_sequence(seq_dir, vol, depth_scale=1000.0, start=0, stop=None, step=1, batch=16, colour=True):
    """the frames start, start + step, ... below stop of a CA-1M sequence directory into vol: the
    depth PNGs / png_depth_scale (capture_stream.py:404-411), times 1 / K_scales.npy[i] where the
    directory has that file (:413-415), K_depth.txt, all_poses.npy and the colour PNGs, both decoded
    on the device; returns the number of frames.  K_all.npy (per-frame intrinsics) is not read: one
    pinhole serves the whole volume, and a line says so."""
    from boxfusion_amd.capture_stream import decode_color_pngs, decode_depth_pngs
    from boxfusion_amd.evaluation import png_size
    rgbs, depths = sequence_frames(seq_dir)
    K = np.loadtxt(os.path.join(seq_dir, "K_depth.txt")).reshape(3, 3)
    poses = np.load(os.path.join(seq_dir, "all_poses.npy")).reshape(-1, 4, 4)
    if len(poses) < len(depths):
        raise ValueError(f"{seq_dir}: {len(depths)} depth frames, {len(poses)} poses")
    if colour and len(rgbs) != len(depths):
        raise ValueError(f"{seq_dir}: rgb/ holds {len(rgbs)} <i>.png and depth/ {len(depths)}; colour=False "
                         "(--no-colour) fuses the depth alone")
    scales = None
    if os.path.isfile(os.path.join(seq_dir, "K_scales.npy")):
        scales = np.load(os.path.join(seq_dir, "K_scales.npy")).reshape(-1).astype(np.float64)
        if len(scales) < len(depths):
            raise ValueError(f"{seq_dir}: {len(depths)} depth frames, {len(scales)} entries in K_scales.npy")
        print(f"K_scales.npy: depth times 1 / scale per frame ({scales.min():g} .. {scales.max():g})")
    if os.path.isfile(os.path.join(seq_dir, "K_all.npy")):
        print("K_all.npy is not used: every frame is fused with K_depth.txt")
    ids = list(range(len(depths))[start:stop:step])

    def blobs(paths):
        out = []
        for p in paths:
            with open(p, "rb") as fh:
                out.append(fh.read())
        return out
    scale = torch.full((), float(depth_scale), dtype=torch.float32, device=vol.device)
    if ids:
        H, W = png_size(depths[ids[0]])
        Hc, Wc = png_size(rgbs[ids[0]]) if colour else (0, 0)
    for a in range(0, len(ids), batch):
        sel = ids[a:a + batch]
        d = decode_depth_pngs(blobs([depths[i] for i in sel]), H, W, vol.device)
        # a tensor divisor: torch divides by a host scalar by multiplying with its reciprocal, and the
        # reference divides (capture_stream.py:411)
        d = d.view(torch.int16).to(torch.int32).bitwise_and_(0xFFFF).to(torch.float32) / scale
        if scales is not None:               # the f32 depth times the f64 factor, rounded to f32
            d = (d.double() * torch.from_numpy(1.0 / scales[sel]).to(vol.device)[:, None, None]).float()
        c = decode_color_pngs(blobs([rgbs[i] for i in sel]), Hc, Wc, vol.device) if colour else None
        vol.integrate(d, K, poses[sel], c)
    return len(ids)


def parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m boxfusion_amd.scene_mesh",
                                description="mesh.ply of a CA-1M sequence directory (a TSDF of its depth frames)")
    p.add_argument("seq_dir")
    p.add_argument("--out", help="the PLY file (default: SEQ_DIR/mesh.ply)")
    p.add_argument("--depth-scale", type=float, default=1000.0, help="depth PNG units per metre")
    p.add_argument("--no-colour", action="store_true", help="do not read rgb/")
    add_volume_arguments(p)
    return p


def main(argv=None):
    p = parser()
    a = p.parse_args(argv)
    check_volume_arguments(p, a)
    if not a.depth_scale > 0:
        p.error("--depth-scale must be positive")
    if not os.path.isdir(a.seq_dir):
        p.error(f"{a.seq_dir} is not a directory")
    for need in ("K_depth.txt", "all_poses.npy"):
        if not os.path.isfile(os.path.join(a.seq_dir, need)):
            p.error(f"{os.path.join(a.seq_dir, need)} is missing")
    rgbs, depths = sequence_frames(a.seq_dir)
    if not depths:
        p.error(f"{os.path.join(a.seq_dir, 'depth')} holds no <i>.png")
    if not a.no_colour and len(rgbs) != len(depths):
        p.error(f"rgb/ holds {len(rgbs)} <i>.png and depth/ {len(depths)}: --no-colour fuses the depth alone")
    out = a.out or os.path.join(a.seq_dir, "mesh.ply")
    vol = TsdfVolume(voxel=a.voxel, trunc_voxels=a.trunc_voxels, capacity=a.capacity, max_depth=a.max_depth)
    n = fuse_sequence(a.seq_dir, vol, a.depth_scale, a.start, a.stop, a.step, colour=not a.no_colour)
    nv, nf = vol.save_ply(out)
    print(f"{n} frames -> {nv} vertices, {nf} faces -> {out}")
    print(vol.stats_line())
    return 0


if __name__ == "__main__":
    sys.exit(main())
