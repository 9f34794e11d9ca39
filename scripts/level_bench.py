"""The levelling kernels per call, timed with the KernelTimer hook: bf_level_face_samples, bf_level_vote (G = 32),
bf_level_score (the candidates of a 40 degree cone about +z) and bf_level_refine (with a 256-bin height histogram) on
the "wall" mesh of mesh_probe.py (8 synthetic 480x640 frames at 2 cm voxels, 167 674 triangles) and on 2 M random
samples, with bf_tsdf_surface on the same volume in the same run as yardstick, and level_mesh end to end on the wall
mesh (host solve and read-backs included, wall clock).  Medians of 5 after a warm-up.  One JSON line at the end."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boxfusion_amd import _lib  # noqa: E402
from boxfusion_amd import scene_level as SL  # noqa: E402
from boxfusion_amd.scene_mesh import TsdfVolume  # noqa: E402
from boxfusion_amd.synthetic import SCANNET_K, Scene  # noqa: E402

B, VOXEL, TRUNC, CAP, REPS, G, RANDOM = 8, 0.02, 4, 1 << 16, 5, 32, 2_000_000
dev = torch.device("cuda")
scene = Scene(seed=0)


def wall_depth(i):
    v, u = np.mgrid[:480, :640].astype(np.float32)
    d = 2.2 + 0.7 * np.sin(u / 210.0 + 0.3 * i) * np.cos(v / 170.0) + 0.001 * (u - 320)
    d[(u.astype(int) // 40 + v.astype(int) // 40 + i) % 23 == 0] = 0.0          # holes
    return d.astype(np.float32)


def kind_us(timer, kind):
    torch.cuda.synchronize()
    return [s.elapsed_time(e) * 1e3 for tags, _, _, s, e in timer.records if tags.get("kind") == kind]


depth = torch.from_numpy(np.stack([wall_depth(i) for i in range(B)])).to(dev)
poses = np.stack([scene.pose(i) for i in range(B)]).astype(np.float32)
vol = TsdfVolume(voxel=VOXEL, trunc_voxels=TRUNC, capacity=CAP, device=dev)
vol.integrate(depth, SCANNET_K, poses)

rng = np.random.default_rng(0)
rn = rng.normal(size=(RANDOM, 3)).astype(np.float32)
rn /= np.linalg.norm(rn, axis=1, keepdims=True).astype(np.float32)
random = (torch.from_numpy(rng.uniform(-5, 5, (RANDOM, 3)).astype(np.float32)).to(dev), torch.from_numpy(rn).to(dev),
          torch.from_numpy(rng.integers(1, 256, RANDOM).astype(np.int32)).to(dev))

cand = torch.from_numpy(np.nonzero(SL.bin_directions(G)[:, 2] >= np.cos(np.radians(40.0)))[0].astype(np.int32)).to(dev)
tau = np.radians(10.0)
cos_par, sin_perp = np.float32(np.cos(tau)), np.float32(np.sin(tau))
frame = torch.tensor([0, 0, 1, 1, 0, 0, 0, 1, 0], dtype=torch.float32, device=dev)

rows = {k: [] for k in ("surface", "face_samples", "vote_mesh", "score_mesh", "refine_mesh", "vote_random", "score_random",
                        "refine_random", "level_mesh_wall_clock")}
for rep in range(REPS + 1):                   # rep 0 warms up
    torch.cuda.synchronize()
    with _lib.KernelTimer() as t:
        v, _, f = vol.mesh()
        c, n, w, _ = _lib.level_face_samples(v, f, np.float32(VOXEL * VOXEL / 256))
        for p_, n_, w_ in ((c, n, w), random):
            hist, _ = _lib.level_vote(n_, w_, G)
            _lib.level_score(hist, G, cand, cos_par, sin_perp)
            _lib.level_refine(p_, n_, w_, frame, cos_par, sin_perp, -5.12, 0.04, 256)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lv = SL.level_mesh(vol, poses=poses)
    wall = (time.perf_counter() - t0) * 1e6
    if rep:
        rows["surface"].append(kind_us(t, "tsdf_surface")[0])
        rows["face_samples"].append(kind_us(t, "level_face_samples")[0])
        for j, name in enumerate(("mesh", "random")):
            for kind in ("vote", "score", "refine"):
                rows[f"{kind}_{name}"].append(kind_us(t, "level_" + kind)[j])
        rows["level_mesh_wall_clock"].append(wall)

out = dict(frames=B, hw=[480, 640], voxel=VOXEL, vertices=int(v.shape[0]), faces=int(f.shape[0]), random_samples=RANDOM, G=G,
           candidates=int(cand.shape[0]), wall_share=round(lv.share, 3), wall_ok=bool(lv.ok),
           **{k + "_us": round(float(np.median(x)), 1) for k, x in rows.items()})
print(json.dumps(out))
