"""Scene-mesh kernels per call of 8 synthetic 480x640 frames at 2 cm voxels, truncation 4 voxels: the
"wall" scene of cloud_probe.py (a smooth surface 1.5-3 m away with holes) with synthetic.frame_rgbd's
colours and synthetic.Scene's poses, timed with the KernelTimer hook: bf_tsdf_touch and bf_tsdf_update
(the first batch into an empty volume, a second batch beside it, the first batch again into its own
blocks), bf_tsdf_extract and the surface pass (bf_tsdf_surface_count + the read-back of the totals +
bf_tsdf_surface_write), with bf_depth_preprocess and bf_cloud_integrate on the same frames in the same
run as yardsticks.  Medians of 5 after a warm-up; also the blocks allocated and the volume's memory.
One JSON line at the end."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boxfusion_amd import _lib  # noqa: E402
from boxfusion_amd.scene_cloud import SceneCloud  # noqa: E402
from boxfusion_amd.scene_mesh import TsdfVolume  # noqa: E402
from boxfusion_amd.synthetic import SCANNET_K, Scene, frame_rgbd  # noqa: E402

B, VOXEL, TRUNC, CAP, REPS = 8, 0.02, 4, 1 << 16, 5
dev = torch.device("cuda")
scene = Scene(seed=0)


def wall_depth(i):
    v, u = np.mgrid[:480, :640].astype(np.float32)
    d = 2.2 + 0.7 * np.sin(u / 210.0 + 0.3 * i) * np.cos(v / 170.0) + 0.001 * (u - 320)
    d[(u.astype(int) // 40 + v.astype(int) // 40 + i) % 23 == 0] = 0.0          # holes
    return d.astype(np.float32)


def batch(first):
    ids = range(first, first + B)
    rgb = torch.from_numpy(np.stack([frame_rgbd(i)[0] for i in ids])).to(dev)
    depth = torch.from_numpy(np.stack([wall_depth(i) for i in ids])).to(dev)
    return rgb, depth, np.stack([scene.pose(i) for i in ids]).astype(np.float32)


K = torch.from_numpy(np.stack([SCANNET_K] * B).astype(np.float32)).to(dev)
batches = [batch(0), batch(B)]


def kind_us(timer, kind):
    """the recorded times of a kind, in microseconds and call order"""
    torch.cuda.synchronize()
    return [s.elapsed_time(e) * 1e3 for tags, _, _, s, e in timer.records if tags.get("kind") == kind]


rows = {k: [] for k in ("touch_first", "update_first", "touch_beside", "update_beside", "touch_again", "update_again",
                        "extract", "surface", "depth_preprocess", "cloud_integrate")}
for rep in range(REPS + 1):                   # rep 0 warms up
    vol = TsdfVolume(voxel=VOXEL, trunc_voxels=TRUNC, capacity=CAP, device=dev)
    cloud = SceneCloud(voxel=VOXEL, capacity=1 << 22, device=dev)
    torch.cuda.synchronize()
    with _lib.KernelTimer() as t:
        for rgb, depth, poses in (batches[0], batches[1], batches[0]):
            vol.integrate(depth, SCANNET_K, poses, rgb)
        vol.mesh()
        RT = torch.from_numpy(batches[0][2]).to(dev)
        _, _, xyz, valid = _lib.depth_preprocess(batches[0][1], K, RT, 10.0)
        cloud.integrate(xyz, valid, batches[0][0])
    if rep:
        touch, update = kind_us(t, "tsdf_touch"), kind_us(t, "tsdf_update")
        for j, name in enumerate(("first", "beside", "again")):
            rows["touch_" + name].append(touch[j])
            rows["update_" + name].append(update[j])
        rows["extract"].append(kind_us(t, "tsdf_extract")[0])
        rows["surface"].append(kind_us(t, "tsdf_surface")[0])
        rows["depth_preprocess"].append(kind_us(t, "depth")[0])
        rows["cloud_integrate"].append(kind_us(t, "cloud_integrate")[0])

st = vol.stats()
nv, nf = [int(x.shape[0]) for x in vol.mesh()[::2]]
bytes_per_block = 8 + 8 + _lib.TSDF_FIELDS * _lib.TSDF_VOX * 4
out = dict(frames=B, hw=[480, 640], voxel=VOXEL, trunc_voxels=TRUNC, capacity=CAP,
           volume_mib=round(CAP * bytes_per_block / 2 ** 20, 1),
           used_mib=round(st["blocks"] * bytes_per_block / 2 ** 20, 1), vertices=nv, faces=nf, **st,
           **{k + "_us": round(float(np.median(v)), 1) for k, v in rows.items()})
print(json.dumps(out))
