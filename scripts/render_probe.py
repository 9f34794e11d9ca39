"""Renderer kernels at V = 8 orbit views of 480 x 640, timed with the KernelTimer hook: bf_render_points
at radius 0 and 1, bf_render_edges with 100 boxes (half-width 1) and bf_render_resolve, on two scenes of
the same number of points -- "surface": a SceneCloud (2 cm voxels) of 8 synthetic 480 x 640 frames of a
smooth wall 1.5-3 m away; "scattered": as many points uniform in the surface's bounding box.  Per
kernel the median of REPS launches after a warm-up and their min..max, each launch into a cleared
target; from one more (untimed) launch with the counters on, the fraction of offered pixels that issued
an atomic after the early-out.  One JSON line at the end."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boxfusion_amd import _lib, render  # noqa: E402
from boxfusion_amd.scene_cloud import SceneCloud  # noqa: E402
from boxfusion_amd.synthetic import SCANNET_K, Scene, frame_rgbd  # noqa: E402
from boxfusion_amd.tools_utils import unproject  # noqa: E402

B, V, H, W, REPS, N_BOXES = 8, 8, 480, 640, 9, 100
dev = torch.device("cuda")
scene = Scene(seed=0)


def wall_depth(i):
    v, u = np.mgrid[:480, :640].astype(np.float32)
    d = 2.2 + 0.7 * np.sin(u / 210.0 + 0.3 * i) * np.cos(v / 170.0) + 0.001 * (u - 320)
    d[(u.astype(int) // 40 + v.astype(int) // 40 + i) % 23 == 0] = 0.0          # holes
    return d.astype(np.float32)


sc = SceneCloud(voxel=0.02, capacity=1 << 22, device=dev)
for i in range(B):
    xyz, valid = unproject(torch.from_numpy(wall_depth(i)).to(dev), SCANNET_K, scene.pose(40 * i), max_depth=10.0)
    sc.integrate(xyz, valid, torch.from_numpy(frame_rgbd(i)[0]).to(dev))
surf_xyz, surf_rgb, _ = sc.points()
n = int(surf_xyz.shape[0])
lo, hi = surf_xyz.min(0).values.cpu().numpy(), surf_xyz.max(0).values.cpu().numpy()
rng = np.random.default_rng(0)
scat_xyz = torch.from_numpy(rng.uniform(lo, hi, (n, 3)).astype(np.float32)).to(dev)
scenes = dict(surface=(surf_xyz.contiguous(), surf_rgb.contiguous()), scattered=(scat_xyz, surf_rgb.contiguous()))

poses = render.orbit_poses(lo, hi, V, K3=SCANNET_K, H=H, W=W)
far = 4.0 * float(np.linalg.norm(hi - lo)) + 10.0
centres = rng.uniform(lo, hi, (N_BOXES, 3))
dims = rng.uniform(0.3, 1.2, (N_BOXES, 3))
signs = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1.0]])
corners = torch.from_numpy((centres[:, None] + signs[None] * dims[:, None] / 2).astype(np.float32)).to(dev)
colors = torch.from_numpy(render.box_colors(N_BOXES)).to(dev)
ren = render.Renderer(H, W, SCANNET_K, views=V, device=dev)


def stat(v):
    return dict(median_us=round(float(np.median(v)), 1), min_us=round(float(np.min(v)), 1), max_us=round(float(np.max(v)), 1))


out = dict(points=n, views=V, hw=[H, W], boxes=N_BOXES, reps=REPS, scenes={})
for name, (xyz, rgb) in scenes.items():
    row = {}
    for r in (0, 1):
        t_points, t_edges, t_resolve = [], [], []
        for rep in range(REPS + 1):           # rep 0 warms up
            ren.clear()
            torch.cuda.synchronize()
            with _lib.KernelTimer() as t:
                ren.draw_points(xyz, rgb, poses, radius=r, far=far)
                ren.draw_boxes(corners, colors, poses, half_width=1)
                ren.resolve()
                us = {k: t.summary(lambda g, k=k: g.get("kind") == k)["avg_us"] for k in ("render_points", "render_edges", "render_resolve")}
            if rep:
                t_points.append(us["render_points"])
                t_edges.append(us["render_edges"])
                t_resolve.append(us["render_resolve"])
        ren.clear()
        counters = torch.zeros(2, dtype=torch.int64, device=dev)
        ren.draw_points(xyz, rgb, poses, radius=r, far=far, stats=counters)
        offered, issued = counters.cpu().tolist()
        covered = float((ren.keys != -1).float().mean().item())
        row[f"radius_{r}"] = dict(points=stat(t_points), edges=stat(t_edges), resolve=stat(t_resolve), pixels_offered=offered,
                                  atomics_issued=issued, issued_fraction=round(issued / max(offered, 1), 4),
                                  covered=round(covered, 4))
        print(name, f"radius {r}", row[f"radius_{r}"], flush=True)
    out["scenes"][name] = row
print(json.dumps(out))
