"""Builds ScanNet `.sens` containers for the tests, from the layout in boxfusion_amd/sens.py
(struct + zlib only, independent of the reader under test)."""
import io
import struct
import zlib

import numpy as np

LOST = np.full((4, 4), -np.inf, np.float32)          # the pose ScanNet writes when tracking was lost


def header(n_frames, color_hw, depth_hw, version=4, sensor_name="StructureSensor", intrinsic_color=None,
           extrinsic_color=None, intrinsic_depth=None, extrinsic_depth=None, color_compression=2,
           depth_compression=1, depth_shift=1000.0):
    eye = np.eye(4, dtype=np.float32)
    name = sensor_name.encode()
    out = struct.pack("<IQ", version, len(name)) + name
    for m in (intrinsic_color, extrinsic_color, intrinsic_depth, extrinsic_depth):
        out += np.asarray(eye if m is None else m, "<f4").reshape(16).tobytes()
    out += struct.pack("<ii", color_compression, depth_compression)
    out += struct.pack("<IIII", color_hw[1], color_hw[0], depth_hw[1], depth_hw[0])
    out += struct.pack("<fQ", depth_shift, n_frames)
    return out


def record(pose, color, depth, t_color=0, t_depth=0):
    return (np.asarray(pose, "<f4").reshape(16).tobytes() + struct.pack("<QQQQ", t_color, t_depth, len(color), len(depth))
            + color + depth)


def write_sens(path, colors, depths, poses, color_hw, depth_hw=None, num_frames=None, level=6, timestamps=None, **hdr):
    """colors: the colour payloads (bytes, written verbatim); depths: u16 [H,W] arrays, compressed
    per hdr['depth_compression'] (1 zlib at `level`, 0 raw), or bytes written verbatim; returns
    (the file's bytes, the depth payloads as written)"""
    dc = hdr.get("depth_compression", 1)
    blobs = []
    for d in depths:
        if isinstance(d, (bytes, bytearray)):
            blobs.append(bytes(d))
        else:
            raw = np.ascontiguousarray(d, "<u2").tobytes()
            blobs.append(zlib.compress(raw, level) if dc == 1 else raw)
    if depth_hw is None:
        depth_hw = depths[0].shape
    n = len(colors) if num_frames is None else num_frames
    data = header(n, color_hw, depth_hw, **hdr)
    for i, (c, z, p) in enumerate(zip(colors, blobs, poses)):
        tc, td = timestamps[i] if timestamps is not None else (1000 * i, 1000 * i + 7)
        data += record(p, c, z, tc, td)
    with open(path, "wb") as fh:
        fh.write(data)
    return data, blobs


def jpeg_bytes(rgb, quality=90):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, format="JPEG", quality=quality)
    return b.getvalue()


def upright_pose(t=(0.0, 0.0, 0.0)):
    """camera y down the world z (the upright roll), at t"""
    p = np.eye(4, dtype=np.float32)
    p[1:3, :3] = [[0, 0, 1], [0, -1, 0]]
    p[:3, 3] = t
    return p
