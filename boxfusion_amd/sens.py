"""ScanNet `.sens` containers read directly: one file per scene holding the colour frames (baseline
JPEG), the depth frames (bare zlib streams of little-endian uint16) and the camera -> world poses
that the reference's ScannetDataset (capture_stream.py:119-311) reads from an exported
color/*.jpg, depth/*.png, pose/*.txt tree.

`SensFile` maps the file and indexes its frame records; `SensFrameStream` yields the sample dicts
of `DecodedFrameStream` for the exported tree of the same scene, the colour frames through
bf_jpeg_decode_rgb and the depth streams through bf_zlib_decode_u16 (or PIL / zlib on the host);
`python -m boxfusion_amd.sens export scene.sens OUT` writes the tree, `... info scene.sens` prints
the header, `... cloud scene.sens out.ply` writes the scene's coloured point cloud, `... mesh
scene.sens out.ply` its surface (a TSDF of the depth frames, scene_mesh.TsdfVolume), `... track scene.sens
POSES.npy [--recover-lost | --from-scratch] [--photometric] [--relocalise] [--level]` poses from tracking the depth
frames against that TSDF (tracking.track_sequence; for `SensFrameStream(poses=...)`; --level turns them into a z-up
world with the floor at z = 0, scene_level.level_mesh) and `... render
scene.sens OUT_DIR [--boxes SEQ_boxes.pkl] [--mesh]` orbit and top-down PNG views of the cloud, or with
--mesh of the TSDF surface (no model needed).

Layout (little-endian, packed): uint32 version (4), uint64 n + n bytes sensor name, four row-major
4x4 float32 matrices (colour intrinsics / extrinsics, depth intrinsics / extrinsics), int32 colour
and depth compression, uint32 colour width, height, depth width, height, float32 depth_shift,
uint64 frame count; per frame a 4x4 float32 camera -> world pose (all -inf when tracking was
lost), uint64 colour and depth timestamps, uint64 colour and depth byte counts, the colour bytes,
the depth bytes.
"""
from __future__ import annotations

import mmap
import os
import struct
import sys

import numpy as np

COLOR_COMPRESSION = {-1: "unknown", 0: "raw", 1: "png", 2: "jpeg"}
DEPTH_COMPRESSION = {-1: "unknown", 0: "raw_ushort", 1: "zlib_ushort", 2: "occi_ushort"}
_REC = struct.Struct("<16f4Q")           # pose, colour / depth timestamps, colour / depth sizes
_TAIL = struct.Struct("<2i4IfQ")         # compressions, the four sizes, depth_shift, frame count


class SensFile:
    """a `.sens` file mapped read-only: header fields as attributes (`sensor_name`,
    `intrinsic_color`, `extrinsic_color`, `intrinsic_depth`, `extrinsic_depth` [4,4] f32,
    `color_compression`, `depth_compression`, `color_width`, `color_height`, `depth_width`,
    `depth_height`, `depth_shift`, `num_frames`) and an index built by one walk over the frame
    records: `color_index` / `depth_index` int64 [N,2] (byte offset, size), `timestamps` uint64
    [N,2] (colour, depth), `poses` f32 [N,4,4] as written."""

    def __init__(self, path):
        self.path = os.fspath(path)
        self._fh = open(self.path, "rb")
        self._map = self._view = None
        try:
            size = os.fstat(self._fh.fileno()).st_size
            if size == 0:
                raise ValueError(f"{self.path}: empty file")
            self._map = mmap.mmap(self._fh.fileno(), 0, access=mmap.ACCESS_READ)
            self._view = memoryview(self._map)
            self._parse(size)
        except BaseException:
            self.close()
            raise

    def _parse(self, size):
        buf, path = self._map, self.path

        def need(pos, n, what):
            if pos + n > size:
                raise ValueError(f"{path}: {what} runs past the end of the file ({pos} + {n} > {size} bytes)")

        need(0, 12, "the file header")
        version, nlen = struct.unpack_from("<IQ", buf, 0)
        if version != 4:
            raise ValueError(f"{path}: .sens version {version}, expected 4")
        pos = 12
        need(pos, nlen, "the sensor name")
        self.sensor_name = bytes(buf[pos:pos + nlen]).decode("utf-8", "replace")
        pos += nlen
        need(pos, 4 * 64 + _TAIL.size, "the file header")
        mats = np.frombuffer(buf, "<f4", 64, pos).reshape(4, 4, 4).astype(np.float32)
        self.intrinsic_color, self.extrinsic_color, self.intrinsic_depth, self.extrinsic_depth = mats
        pos += 4 * 64
        (self.color_compression, self.depth_compression, self.color_width, self.color_height, self.depth_width,
         self.depth_height, self.depth_shift, n) = _TAIL.unpack_from(buf, pos)
        pos += _TAIL.size
        if n * _REC.size > size - pos:
            raise ValueError(f"{path}: {n} frames do not fit in the {size - pos} bytes after the header")
        self.num_frames = n
        self.color_index = np.zeros((n, 2), np.int64)
        self.depth_index = np.zeros((n, 2), np.int64)
        self.timestamps = np.zeros((n, 2), np.uint64)
        self.poses = np.zeros((n, 4, 4), np.float32)
        for i in range(n):
            need(pos, _REC.size, f"the record of frame {i} (of {n})")
            rec = _REC.unpack_from(buf, pos)
            pos += _REC.size
            self.poses[i] = np.asarray(rec[:16], np.float32).reshape(4, 4)
            self.timestamps[i] = rec[16:18]
            csz, dsz = rec[18], rec[19]
            need(pos, csz, f"the colour data of frame {i}")
            self.color_index[i] = (pos, csz)
            pos += csz
            need(pos, dsz, f"the depth data of frame {i}")
            self.depth_index[i] = (pos, dsz)
            pos += dsz

    def __len__(self):
        return self.num_frames

    def color_bytes(self, i):
        """frame i's colour data, a memoryview into the map (no copy; release it before close())"""
        o, n = self.color_index[i]
        return self._view[int(o):int(o + n)]

    def depth_bytes(self, i):
        """frame i's depth data, a memoryview into the map (no copy; release it before close())"""
        o, n = self.depth_index[i]
        return self._view[int(o):int(o + n)]

    def poses_filled(self):
        """the poses as the reference's load_poses keeps them (capture_stream.py:171-174): a pose
        with any inf becomes the last valid pose before it; frames before the first valid pose
        (the reference would hand out None there) get the first valid pose of the file"""
        out = self.poses.copy()
        bad = np.isinf(out).any(axis=(1, 2))
        good = np.flatnonzero(~bad)
        if len(good) == 0:
            if len(out):
                raise ValueError(f"{self.path}: no frame has a valid pose")
            return out
        last = out[good[0]]
        for i in range(len(out)):
            if bad[i]:
                out[i] = last
            else:
                last = out[i]
        return out

    def depth_u16(self, i):
        """frame i's depth decoded on the host -> u16 [depth_height, depth_width]"""
        H, W = self.depth_height, self.depth_width
        b = self.depth_bytes(i)
        if self.depth_compression == 1:
            import zlib
            raw = zlib.decompress(b)
        elif self.depth_compression == 0:
            raw = b
        else:
            raise ValueError(f"{self.path}: depth compression "
                             f"{DEPTH_COMPRESSION.get(self.depth_compression, self.depth_compression)} is not supported")
        if len(raw) != 2 * H * W:
            raise ValueError(f"{self.path}: depth frame {i} holds {len(raw)} bytes, expected {2 * H * W}")
        return np.frombuffer(raw, "<u2").reshape(H, W)

    def close(self):
        if self._view is not None:
            self._view.release()
            self._view = None
        if self._map is not None:
            self._map.close()
            self._map = None
        if self._fh is not None:
            self._fh.close()
            self._fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class SensFrameStream:
    """a `.sens` file as demo.py's dataset: the samples DecodedFrameStream yields for the exported
    tree of the same scene, without the tree.  Per batch of `batch` frames the colour JPEGs are
    decoded by bf_jpeg_decode_rgb (color_decode="host": PIL) and the zlib depth streams by
    bf_zlib_decode_u16 (depth_decode="host": zlib.decompress); raw-ushort depth is uploaded as it
    is.  K defaults to the depth intrinsics (the colour image is resized to the depth size, as the
    reference's cv2.resize(color, (W, H)) does), depth_scale to the file's depth_shift; poses are
    `poses_filled()` unless `poses` ([num_frames,4,4], e.g. from `sens track`) replaces them; frames
    start, start + step, ... below stop, `timestamp` = the frame's index in the file."""

    def __init__(self, sens, K=None, depth_scale=None, device="cuda", video_id=0, batch=16, start=0, stop=None,
                 step=1, color_decode="gpu", depth_decode="gpu", poses=None):
        self.sens = sens if isinstance(sens, SensFile) else SensFile(sens)
        s = self.sens
        if s.color_compression != 2:
            raise ValueError(f"{s.path}: colour compression {COLOR_COMPRESSION.get(s.color_compression, s.color_compression)}"
                             " is not supported (jpeg only)")
        if s.depth_compression not in (0, 1):
            raise ValueError(f"{s.path}: depth compression {DEPTH_COMPRESSION.get(s.depth_compression, s.depth_compression)}"
                             " is not supported (zlib_ushort or raw_ushort)")
        if depth_decode not in ("gpu", "host"):
            raise ValueError("depth_decode: 'gpu' or 'host'")
        if color_decode not in ("gpu", "host"):
            raise ValueError("color_decode: 'gpu' or 'host'")
        self.K = np.asarray(s.intrinsic_depth[:3, :3] if K is None else K, np.float32)
        self.scale = float(s.depth_shift if depth_scale is None else depth_scale)
        self.dev, self.video_id, self.batch = device, video_id, max(1, int(batch))
        self.frames = range(s.num_frames)[start:stop:step]
        self.color_decode, self.depth_decode = color_decode, depth_decode
        if poses is None:
            self.poses = s.poses_filled()
        else:                                       # e.g. what `sens track --recover-lost` wrote
            self.poses = np.asarray(poses, np.float32)
            if self.poses.shape != (s.num_frames, 4, 4):
                raise ValueError(f"poses: [{s.num_frames},4,4] (one per frame of the file), got {self.poses.shape}")

    def __len__(self):
        return len(self.frames)

    def _depths(self, idx):
        import torch
        from boxfusion_amd.capture_stream import decode_depth_zlib
        s = self.sens
        H, W = s.depth_height, s.depth_width
        if s.depth_compression == 1 and self.depth_decode == "gpu":
            return decode_depth_zlib([s.depth_bytes(i) for i in idx], H, W, self.dev)
        arr = np.stack([s.depth_u16(i) for i in idx])
        return torch.from_numpy(arr.view(np.int16)).to(self.dev).view(torch.uint16)

    def _colors(self, idx):
        import torch
        from boxfusion_amd.capture_stream import decode_color_jpegs
        s = self.sens
        if self.color_decode == "gpu":
            return decode_color_jpegs([s.color_bytes(i) for i in idx], s.color_height, s.color_width, self.dev)
        import io
        from PIL import Image
        out = []
        for i in idx:
            rgb = np.array(Image.open(io.BytesIO(s.color_bytes(i))).convert("RGB"))
            out.append(torch.from_numpy(rgb).to(self.dev, non_blocking=True))
        return out

    def __iter__(self):
        import torch
        from boxfusion_amd.capture_stream import make_sample_decoded
        for b0 in range(0, len(self.frames), self.batch):
            idx = list(self.frames[b0:b0 + self.batch])
            deps, cols = self._depths(idx), self._colors(idx)
            for j, i in enumerate(idx):
                yield make_sample_decoded(cols[j], deps[j].view(torch.int16), self.scale, self.K, self.poses[i],
                                          video_id=self.video_id, index=i, src_bgr=False)


def _matrix_text(m):
    return "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in np.asarray(m, np.float32))


def export(sens, out_dir, start=0, stop=None, step=1):
    """write the reference's tree for the frames start, start + step, ... below stop:
    color/<i>.jpg (the container's bytes), depth/<i>.png (16-bit grey), pose/<i>.txt (the pose as
    written, -inf included) and intrinsic/intrinsic_{color,depth}.txt; returns the frame indices"""
    from PIL import Image
    if sens.color_compression != 2:
        raise ValueError(f"{sens.path}: colour compression "
                         f"{COLOR_COMPRESSION.get(sens.color_compression, sens.color_compression)} is not supported (jpeg only)")
    for d in ("color", "depth", "pose", "intrinsic"):
        os.makedirs(os.path.join(out_dir, d), exist_ok=True)
    for name in ("intrinsic_color", "intrinsic_depth"):
        with open(os.path.join(out_dir, "intrinsic", name + ".txt"), "w") as fh:
            fh.write(_matrix_text(getattr(sens, name)))
    frames = list(range(sens.num_frames)[start:stop:step])
    for i in frames:
        with open(os.path.join(out_dir, "color", f"{i}.jpg"), "wb") as fh:
            fh.write(sens.color_bytes(i))
        Image.fromarray(np.ascontiguousarray(sens.depth_u16(i)).astype(np.uint16)).save(
            os.path.join(out_dir, "depth", f"{i}.png"))
        with open(os.path.join(out_dir, "pose", f"{i}.txt"), "w") as fh:
            fh.write(_matrix_text(sens.poses[i]))
    return frames


def info(sens, out=None):
    out = sys.stdout if out is None else out
    print(f"{sens.path}: version 4, sensor {sens.sensor_name!r}", file=out)
    print(f"frames       {sens.num_frames}", file=out)
    print(f"colour       {sens.color_width} x {sens.color_height}, "
          f"{COLOR_COMPRESSION.get(sens.color_compression, sens.color_compression)}", file=out)
    print(f"depth        {sens.depth_width} x {sens.depth_height}, "
          f"{DEPTH_COMPRESSION.get(sens.depth_compression, sens.depth_compression)}, depth_shift {sens.depth_shift:g}",
          file=out)
    for name in ("intrinsic_color", "extrinsic_color", "intrinsic_depth", "extrinsic_depth"):
        print(name, file=out)
        out.write(_matrix_text(getattr(sens, name)))
    if sens.num_frames:
        lost = int(np.isinf(sens.poses).any(axis=(1, 2)).sum())
        print(f"poses        {lost} of {sens.num_frames} without tracking (-inf)", file=out)
        print(f"data         colour {int(sens.color_index[:, 1].sum())} bytes, depth {int(sens.depth_index[:, 1].sum())} bytes",
              file=out)


def cloud(sens, voxel=0.02, start=0, stop=None, step=1, max_depth=10.0, capacity=1 << 22, device="cuda", batch=16):
    """the scene as a voxel map: every selected frame through SensFrameStream, demo.py:123-126's
    unproject of its depth with gt.depth.K and gt.RT, coloured by its image, into a SceneCloud
    (returned)"""
    from boxfusion_amd.scene_cloud import SceneCloud
    from boxfusion_amd.tools_utils import unproject
    sc = SceneCloud(voxel=voxel, capacity=capacity, device=device)
    for sample in SensFrameStream(sens, device=device, batch=batch, start=start, stop=stop, step=step):
        gt = sample["sensor_info"].gt
        xyz, valid = unproject(sample["wide"]["depth"][-1], gt.depth.K[-1], gt.RT[-1], max_depth=max_depth)
        sc.integrate(xyz, valid, sample["wide"]["image"][-1].permute(1, 2, 0).contiguous())
    return sc


def mesh(sens, voxel=0.02, trunc_voxels=4, start=0, stop=None, step=1, max_depth=10.0, capacity=1 << 16, device="cuda",
         batch=16):
    """the scene as a TSDF: every selected frame through SensFrameStream, its depth with gt.depth.K, its
    image and its pose as the file has it, `batch` frames per call, into a scene_mesh.TsdfVolume
    (returned); frames without tracking (a -inf pose) are skipped and counted by the volume"""
    import torch
    from boxfusion_amd.scene_mesh import TsdfVolume
    vol = TsdfVolume(voxel=voxel, trunc_voxels=trunc_voxels, capacity=capacity, max_depth=max_depth, device=device)
    stream = SensFrameStream(sens, device=device, batch=batch, start=start, stop=stop, step=step)
    poses = stream.sens.poses                      # as written, -inf included (the stream's are filled)
    held = []

    def flush():
        if held:
            vol.integrate(torch.stack([h[0] for h in held]), held[0][1], np.stack([h[2] for h in held]),
                          torch.stack([h[3] for h in held]))
            held.clear()
    for sample in stream:
        gt = sample["sensor_info"].gt
        held.append((sample["wide"]["depth"][-1], gt.depth.K[-1], poses[sample["meta"]["timestamp"]],
                     sample["wide"]["image"][-1].permute(1, 2, 0).contiguous()))
        if len(held) == batch:
            flush()
    flush()
    return vol


def track(sens, mode="recover-lost", voxel=0.02, trunc_voxels=4, start=0, stop=None, step=1, max_depth=10.0,
          capacity=1 << 16, device="cuda", batch=16, photometric=False, relocalise=False, ferns=512, fern_cell=16,
          harvest=0.15, level=False, **tracker_args):
    """poses for the frames start, start + step, ... below stop by tracking.track_sequence: mode
    "recover-lost" keeps the file's finite poses and tracks the frames written as -inf; "from-scratch"
    starts at the first selected frame's pose (identity if it has none) and tracks every later frame.
    photometric=True adds the colour frames' intensity residual to the depth ICP, which places views
    that a single plane fills.  relocalise=True keeps fern keyframes of the placed frames
    (tracking.Relocaliser with ferns, fern_cell and harvest) and restarts the tracker from the nearest
    ones when a frame is lost from the last good pose, e.g. after the camera moved on while it was lost.
    The selected frames are decoded first and held on the device (2.1 MB per 480 x 640 frame): --step /
    --stop bound that for a long capture.
    Returns (poses f32 [num_frames,4,4]: the file's with the selected frames replaced, -inf where a
    frame stayed lost; the frame indices; info per selected frame; the TsdfVolume).
    level=True levels the tracked volume's surface afterwards (scene_level.level_mesh with the tracked
    poses) and returns a fifth item, the Levelling.  When it is ok the selected frames' poses are the
    levelled ones (z up, the floor at z = 0, the walls along x and y) and the volume is a fresh one, the
    held frames fused again with those poses: a sparse TSDF cannot be rotated in place.  When it is not
    ok, poses and volume are as without level."""
    import torch
    from boxfusion_amd.scene_mesh import TsdfVolume
    from boxfusion_amd.tracking import Relocaliser, track_sequence
    if mode not in ("recover-lost", "from-scratch"):
        raise ValueError("mode: 'recover-lost' or 'from-scratch'")
    s = sens if isinstance(sens, SensFile) else SensFile(sens)
    # a plain RGB-D recording has no pose at all: the stream, used here only to decode the frames, cannot fill them in
    plain = s.num_frames > 0 and not np.isfinite(s.poses).all((1, 2)).any()
    stream = SensFrameStream(s, device=device, batch=batch, start=start, stop=stop, step=step,
                             poses=np.tile(np.eye(4, dtype=np.float32), (s.num_frames, 1, 1)) if plain else None)
    ids = list(stream.frames)
    vol = TsdfVolume(voxel=voxel, trunc_voxels=trunc_voxels, capacity=capacity, max_depth=max_depth, device=device)
    poses = s.poses.copy()
    if not ids:
        return (poses, ids, [], vol, None) if level else (poses, ids, [], vol)
    depths, colours, K = [], [], None
    for sample in stream:
        gt = sample["sensor_info"].gt
        K = gt.depth.K[-1]
        depths.append(sample["wide"]["depth"][-1])
        colours.append(sample["wide"]["image"][-1].permute(1, 2, 0).contiguous())
    first = s.poses[ids[0]] if np.isfinite(s.poses[ids[0]]).all() else np.eye(4, dtype=np.float32)
    known = s.poses[ids] if mode == "recover-lost" else None
    depths = torch.stack(depths)
    rl = Relocaliser(depths.shape[1], depths.shape[2], device, ferns=ferns, cell=fern_cell, harvest=harvest,
                     max_depth=min(max_depth, 65.535)) if relocalise else None
    colours = torch.stack(colours)
    got, infos = track_sequence(depths, K, first_pose=first, known_poses=known, volume=vol, colours=colours,
                                photometric=photometric, relocaliser=rl, **tracker_args)
    poses[ids] = got
    if not level:
        return poses, ids, infos, vol
    from boxfusion_amd.scene_level import level_mesh
    levelling = level_mesh(vol, poses=np.asarray(got, np.float32))
    if levelling.ok:
        got = levelling.apply(np.asarray(got, np.float32))
        poses[ids] = got
        vol = TsdfVolume(voxel=voxel, trunc_voxels=trunc_voxels, capacity=capacity, max_depth=max_depth, device=device)
        vol.integrate(depths, K, got, colours)
    return poses, ids, infos, vol, levelling


def track_line(file_poses, poses, ids, infos, relocalise=False):
    """`sens track`'s summary: frames tracked / lost (with relocalise=True also how many of the tracked
    came back by relocalisation) and, over the tracked frames for which the file has a finite pose, the
    RMS translation difference after moving the first selected frame onto the file's pose of it"""
    tracked = [i for i, f in zip(ids, infos) if f.get("tracked") and not f["lost"]]
    lost = [i for i, f in zip(ids, infos) if f["lost"]]
    line = f"{len(ids)} frames: {len(tracked)} tracked, {len(lost)} lost"
    if relocalise:
        line += f", {sum(1 for f in infos if f.get('relocalised'))} relocalised"
    both = [i for i in tracked if np.isfinite(file_poses[i]).all()]
    if ids and both and np.isfinite(file_poses[ids[0]]).all() and np.isfinite(poses[ids[0]]).all():
        align = file_poses[ids[0]].astype(np.float64) @ np.linalg.inv(poses[ids[0]].astype(np.float64))
        d = [(align @ poses[i].astype(np.float64))[:3, 3] - file_poses[i][:3, 3].astype(np.float64) for i in both]
        rms = float(np.sqrt(np.mean(np.sum(np.square(d), 1))))
        line += f", rms translation difference to the file's poses {rms:.4f} m over {len(both)}"
    return line


def _cloud_arguments(p):
    p.add_argument("--voxel", type=float, default=0.02, help="voxel edge in metres")
    p.add_argument("--start", type=int, default=0)
    p.add_argument("--stop", type=int, default=None)
    p.add_argument("--step", type=int, default=1)
    p.add_argument("--max-depth", type=float, default=10.0)


def parser():
    import argparse
    from boxfusion_amd.render import add_render_arguments
    p = argparse.ArgumentParser(prog="python -m boxfusion_amd.sens", description="ScanNet .sens containers")
    sub = p.add_subparsers(dest="cmd", required=True)
    pi = sub.add_parser("info", help="print the header fields")
    pi.add_argument("sens")
    pe = sub.add_parser("export", help="write the color/ depth/ pose/ intrinsic/ tree")
    pe.add_argument("sens")
    pe.add_argument("out")
    pe.add_argument("--start", type=int, default=0)
    pe.add_argument("--stop", type=int, default=None)
    pe.add_argument("--step", type=int, default=1)
    pc = sub.add_parser("cloud", help="write the scene's coloured point cloud (a voxel map) as a PLY")
    pc.add_argument("sens")
    pc.add_argument("out")
    _cloud_arguments(pc)
    pm = sub.add_parser("mesh", help="write the scene's surface (a TSDF of the depth frames) as a PLY")
    pm.add_argument("sens")
    pm.add_argument("out")
    from boxfusion_amd.scene_mesh import add_volume_arguments
    add_volume_arguments(pm)
    pt = sub.add_parser("track", help="track the camera against a TSDF of the depth frames and write the poses as .npy")
    pt.add_argument("sens")
    pt.add_argument("poses", help="the output: float32 [num_frames,4,4], -inf where a frame stayed lost")
    mode = pt.add_mutually_exclusive_group()
    mode.add_argument("--recover-lost", action="store_true",
                      help="keep the file's finite poses and track the frames it wrote as -inf (the default)")
    mode.add_argument("--from-scratch", action="store_true", help="ignore the file's poses after the first frame's")
    pt.add_argument("--mesh", help="also write the fused surface as a PLY")
    pt.add_argument("--level", action="store_true",
                    help="level the tracked scene (z up, the floor at z = 0, the walls along x and y) and write the poses, "
                         "and with --mesh the surface fused again from them, in that world")
    pt.add_argument("--photometric", action="store_true",
                    help="track with the colour frames too (an intensity residual against the last placed frame): "
                         "places a textured wall, floor or table top that fills the view")
    pt.add_argument("--relocalise", action="store_true",
                    help="keep fern keyframes of the placed frames and restart the tracker from the nearest ones when a "
                         "frame is lost from the last good pose")
    pt.add_argument("--ferns", type=int, default=512, help="--relocalise: ferns per code, a multiple of 8")
    pt.add_argument("--fern-cell", type=int, default=16, help="--relocalise: the cell of the block means in pixels, 1 .. 64")
    pt.add_argument("--harvest", type=float, default=0.15,
                    help="--relocalise: a frame becomes a keyframe when more than this share of its ferns differs from "
                         "the nearest keyframe's")
    add_volume_arguments(pt)
    pr = sub.add_parser("render", help="write orbit and top-down PNG views of the scene's point cloud (and boxes)")
    pr.add_argument("sens")
    pr.add_argument("out", help="the directory of overview_<k>.png and overview_top.png")
    _cloud_arguments(pr)
    add_render_arguments(pr)
    pr.add_argument("--mesh", action="store_true",
                    help="fuse the depth frames into a TSDF and draw its surface instead of the point cloud")
    pr.add_argument("--trunc-voxels", type=int, default=4, help="--mesh: truncation distance in voxels")
    pr.add_argument("--capacity", type=int, default=1 << 16, help="--mesh: blocks of 8x8x8 voxels, a power of two")
    return p


def main(argv=None):
    p = parser()
    a = p.parse_args(argv)
    if a.cmd in ("cloud", "render"):
        if not a.voxel > 0:
            p.error("--voxel must be positive")
        if a.step < 1:
            p.error("--step must be at least 1")
        if not a.max_depth > 0:
            p.error("--max-depth must be positive")
    if a.cmd == "render":
        from boxfusion_amd import render
        render.check_render_arguments(p, a)
        if a.mesh:
            from boxfusion_amd.scene_mesh import check_volume_arguments
            check_volume_arguments(p, a)
    if a.cmd in ("mesh", "track"):
        from boxfusion_amd.scene_mesh import check_volume_arguments
        check_volume_arguments(p, a)
        if not os.path.isfile(a.sens):
            p.error(f"{a.sens} is missing")
    if a.cmd == "track" and a.relocalise:
        if a.ferns < 8 or a.ferns % 8:
            p.error("--ferns must be a positive multiple of 8")
        if not 1 <= a.fern_cell <= 64:
            p.error("--fern-cell must be 1 .. 64")
        if not 0 <= a.harvest <= 1:
            p.error("--harvest must be within 0 .. 1")
    with SensFile(a.sens) as s:
        if a.cmd == "info":
            info(s)
        elif a.cmd == "cloud":
            sc = cloud(s, a.voxel, a.start, a.stop, a.step, a.max_depth)
            n = sc.save_ply(a.out)
            print(f"{n} points -> {a.out}")
            print(" ".join(f"{k}={v}" for k, v in sc.stats().items()))
        elif a.cmd == "mesh":
            vol = mesh(s, a.voxel, a.trunc_voxels, a.start, a.stop, a.step, a.max_depth, a.capacity)
            nv, nf = vol.save_ply(a.out)
            print(f"{nv} vertices, {nf} faces -> {a.out}")
            print(vol.stats_line())
        elif a.cmd == "track":
            mode = "from-scratch" if a.from_scratch else "recover-lost"
            poses, ids, infos, vol, *levelling = track(s, mode, a.voxel, a.trunc_voxels, a.start, a.stop, a.step,
                                                       a.max_depth, a.capacity, photometric=a.photometric,
                                                       relocalise=a.relocalise, ferns=a.ferns, fern_cell=a.fern_cell,
                                                       harvest=a.harvest, level=a.level)
            np.save(a.poses, poses)
            print(track_line(s.poses, poses, ids, infos, a.relocalise) + f" -> {a.poses}")
            if a.level and levelling[0] is not None:
                print(levelling[0].summary())
                if not levelling[0].ok:
                    print("warning: this does not look like a room from here; the poses are written unlevelled",
                          file=sys.stderr)
            if a.mesh:
                nv, nf = vol.save_ply(a.mesh)
                print(f"{nv} vertices, {nf} faces -> {a.mesh}")
        elif a.cmd == "render" and a.mesh:
            vol = mesh(s, a.voxel, a.trunc_voxels, a.start, a.stop, a.step, a.max_depth, a.capacity)
            paths = render.write_overviews(None, render.load_boxes_argument(a.boxes), a.out, views=a.views, size=a.size,
                                           mesh=vol, shade=not a.no_shade, cull=not a.no_cull)
            print(f"{vol.stats_line()} -> {len(paths)} views in {a.out}")
        elif a.cmd == "render":
            sc = cloud(s, a.voxel, a.start, a.stop, a.step, a.max_depth)
            paths = render.write_overviews(sc, render.load_boxes_argument(a.boxes), a.out, views=a.views, size=a.size,
                                           radius=a.radius)
            print(f"{sc.stats()['stored']} points -> {len(paths)} views in {a.out}")
        else:
            frames = export(s, a.out, a.start, a.stop, a.step)
            print(f"{len(frames)} frames -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
