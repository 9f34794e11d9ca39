"""bf_render_triangles at V = 8 orbit views of 480 x 640, timed with the KernelTimer hook, over a sweep of
coop_pixels (the rectangle size from which a triangle is filled by its whole wave instead of its own
lane), on two meshes:
  "wall":   mesh_probe.py's scene mesh (its three batches of a smooth wall at 2 cm voxels), culled and
            unculled, beside the same vertices drawn by bf_render_points at radius 0 and 1 in the same run;
  "coarse": a 4 x 6 grid of vertices (30 triangles) bent a little, as wide as the wall, so that every
            triangle covers a good part of every view.
Per setting the median of REPS launches after a warm-up and their min..max, each into a cleared target;
from one more (untimed) launch the counters: pairs drawn and dropped, pixels covered, atomics issued.
One JSON line at the end."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from boxfusion_amd import _lib, render  # noqa: E402
from boxfusion_amd.scene_mesh import TsdfVolume  # noqa: E402
from boxfusion_amd.synthetic import SCANNET_K, Scene, frame_rgbd  # noqa: E402

B, V, H, W, REPS = 8, 8, 480, 640, 9
SWEEP = [0, 4, 8, 16, 64, 256, 512, 1024, 2048, 4096, 1 << 30]
dev = torch.device("cuda")
scene = Scene(seed=0)


def wall_depth(i):
    v, u = np.mgrid[:480, :640].astype(np.float32)
    d = 2.2 + 0.7 * np.sin(u / 210.0 + 0.3 * i) * np.cos(v / 170.0) + 0.001 * (u - 320)
    d[(u.astype(int) // 40 + v.astype(int) // 40 + i) % 23 == 0] = 0.0          # holes
    return d.astype(np.float32)


vol = TsdfVolume(voxel=0.02, trunc_voxels=4, capacity=1 << 16, device=dev)
for first in (0, B, 0):                       # mesh_probe.py's three batches: 83 229 vertices, 167 674 triangles
    ids = range(first, first + B)
    vol.integrate(torch.from_numpy(np.stack([wall_depth(i) for i in ids])).to(dev), SCANNET_K,
                  np.stack([scene.pose(i) for i in ids]).astype(np.float32),
                  torch.from_numpy(np.stack([frame_rgbd(i)[0] for i in ids])).to(dev))
verts, vrgb, faces = vol.mesh()
lo, hi = verts.min(0).values.cpu().numpy(), verts.max(0).values.cpu().numpy()
poses = render.orbit_poses(lo, hi, V, K3=SCANNET_K, H=H, W=W)
far = 4.0 * float(np.linalg.norm(hi - lo)) + 10.0

# the coarse mesh: a 4 x 6 grid over the wall's two widest axes at its middle, bent along the third
ax = np.argsort(hi - lo)
gi, gj = np.mgrid[:4, :6]
cv = np.zeros((4, 6, 3))
cv[..., ax[2]] = lo[ax[2]] + (hi - lo)[ax[2]] * gj / 5.0
cv[..., ax[1]] = lo[ax[1]] + (hi - lo)[ax[1]] * gi / 3.0
cv[..., ax[0]] = (lo + hi)[ax[0]] / 2 + 0.2 * (hi - lo)[ax[0]] * np.sin(gi + 2.0 * gj)
cf = []
for j in range(3):
    for i in range(5):
        a, b, c, d = j * 6 + i, j * 6 + i + 1, (j + 1) * 6 + i + 1, (j + 1) * 6 + i
        cf += [(a, b, c), (a, c, d)]
coarse = (torch.from_numpy(cv.reshape(-1, 3).astype(np.float32)).to(dev),
          torch.from_numpy(np.random.default_rng(0).integers(0, 256, (24, 3), dtype=np.uint8)).to(dev),
          torch.from_numpy(np.array(cf, np.int32)).to(dev))

ren = render.Renderer(H, W, SCANNET_K, views=V, device=dev)


def stat(v):
    return dict(median_us=round(float(np.median(v)), 1), min_us=round(float(np.min(v)), 1), max_us=round(float(np.max(v)), 1))


def timed(kind, draw):
    us = []
    for rep in range(REPS + 1):               # rep 0 warms up
        ren.clear()
        torch.cuda.synchronize()
        with _lib.KernelTimer() as t:
            draw(None)
            us.append(t.summary(lambda g: g.get("kind") == kind)["avg_us"])
    ren.clear()
    n = 6 if kind == "render_triangles" else 2
    counters = torch.zeros(n, dtype=torch.int64, device=dev)
    draw(counters)
    covered = float((ren.keys != -1).float().mean().item())
    return dict(stat(us[1:]), counters=counters.cpu().tolist(), covered=round(covered, 4))


out = dict(views=V, hw=[H, W], reps=REPS, wall=dict(vertices=int(verts.shape[0]), faces=int(faces.shape[0])),
           coarse=dict(vertices=24, faces=30), default_coop_pixels=_lib.RENDER_COOP_PIXELS, rows={})
for r in (0, 1):
    row = timed("render_points", lambda st, r=r: ren.draw_points(verts, vrgb, poses, radius=r, far=far, stats=st))
    out["rows"][f"wall_points_r{r}"] = row
    print(f"wall as points, radius {r}", row, flush=True)
for name, (v, c, f), culls in (("wall", (verts, vrgb, faces), (False, True)), ("coarse", coarse, (False,))):
    for cull in culls:
        for coop in SWEEP:
            row = timed("render_triangles", lambda st, coop=coop: ren.draw_mesh(v, f, c, poses, cull=cull, far=far, stats=st,
                                                                                coop_pixels=coop))
            out["rows"][f"{name}_cull{int(cull)}_coop{coop}"] = row
            print(name, f"cull {int(cull)} coop_pixels {coop}", row, flush=True)
print(json.dumps(out))
