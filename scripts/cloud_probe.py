"""Scene-cloud kernels on a batch of 8 synthetic 480x640 frames at 2 cm voxels (argument "random",
the default: synthetic.frame_rgbd's per-pixel random depth, every point a voxel of its own, the worst
case for the map; "wall": a smooth surface 1.5-3 m away, a few pixels of a row per voxel), timed with
the KernelTimer hook: bf_cloud_pack, bf_cloud_integrate (the first batch into an empty map, a later
batch into the populated map), bf_cloud_extract, and bf_depth_preprocess on the same frames in the
same run as the yardstick.  Also the sets of atomic adds issued per stored point with and without the
in-wave run merge (stats()["runs"]) and the table's memory.  One JSON line at the end."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boxfusion_amd import _lib  # noqa: E402
from boxfusion_amd.scene_cloud import SceneCloud  # noqa: E402
from boxfusion_amd.synthetic import SCANNET_K, Scene, frame_rgbd  # noqa: E402

B, VOXEL, CAP, REPS = 8, 0.02, 1 << 22, 5
dev = torch.device("cuda")
scene = Scene(seed=0)


SCENE = sys.argv[1] if len(sys.argv) > 1 else "random"


def wall_depth(i):
    v, u = np.mgrid[:480, :640].astype(np.float32)
    d = 2.2 + 0.7 * np.sin(u / 210.0 + 0.3 * i) * np.cos(v / 170.0) + 0.001 * (u - 320)
    d[(u.astype(int) // 40 + v.astype(int) // 40 + i) % 23 == 0] = 0.0          # holes
    return d.astype(np.float32)


def batch(first):
    ids = range(first, first + B)
    rgb = torch.from_numpy(np.stack([frame_rgbd(i)[0] for i in ids])).to(dev)
    depth = torch.from_numpy(np.stack([wall_depth(i) if SCENE == "wall" else frame_rgbd(i)[1] for i in ids])).to(dev)
    RT = torch.from_numpy(np.stack([scene.pose(i) for i in ids]).astype(np.float32)).to(dev)
    return rgb, depth, RT


K = torch.from_numpy(np.stack([SCANNET_K] * B).astype(np.float32)).to(dev)
batches = [batch(0), batch(B)]


def us(timer, kind, **tags):
    s = timer.summary(lambda t: t.get("kind") == kind and all(t.get(k) == v for k, v in tags.items()))
    return round(s["avg_us"], 1) if s["launches"] else None


rows = {}
for merge in (True, False):
    first, later, pack, extract, depth_us = [], [], [], [], []
    for rep in range(REPS + 1):               # rep 0 warms up
        sc = SceneCloud(voxel=VOXEL, capacity=CAP, device=dev, merge=merge)
        torch.cuda.synchronize()
        with _lib.KernelTimer() as t:
            _, _, xyz0, valid0 = _lib.depth_preprocess(batches[0][1], K, batches[0][2], 10.0)
            _lib.cloud_pack(xyz0, valid0, batches[0][0])
            sc.integrate(xyz0, valid0, batches[0][0])
            a = t.summary(lambda g: g.get("kind") == "cloud_integrate")["ms"] * 1e3
            _, _, xyz1, valid1 = _lib.depth_preprocess(batches[1][1], K, batches[1][2], 10.0)
            sc.integrate(xyz1, valid1, batches[1][0])
            sc.integrate(xyz0, valid0, batches[0][0])          # every voxel already present
            _lib.cloud_extract(sc.table)
            tot = t.summary(lambda g: g.get("kind") == "cloud_integrate")
            if rep:
                first.append(a)
                later.append((tot["ms"] * 1e3 - a) / 2)
                pack.append(us(t, "cloud_pack"))
                extract.append(us(t, "cloud_extract"))
                depth_us.append(us(t, "depth"))
    st = sc.stats()
    n_vox = int(sc.points()[0].shape[0])
    rows[merge] = dict(integrate_first_us=round(float(np.median(first)), 1),
                       integrate_later_us=round(float(np.median(later)), 1), pack_us=float(np.median(pack)),
                       extract_us=float(np.median(extract)), depth_preprocess_us=float(np.median(depth_us)),
                       stored=st["stored"], runs=st["runs"], atomic_sets_per_point=round(st["runs"] / st["stored"], 4),
                       voxels=n_vox, dropped_full=st["dropped_full"])
    print(("merge   " if merge else "no merge"), rows[merge], flush=True)

out = dict(scene=SCENE, frames=B, hw=[480, 640], voxel=VOXEL, capacity=CAP,
           table_mib=round(CAP * _lib.CLOUD_SLOT_WORDS * 8 / 2 ** 20, 1), merge=rows[True], no_merge=rows[False])
print(json.dumps(out))
