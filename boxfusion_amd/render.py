"""A headless view of the run: the scene cloud and the fused boxes drawn on the device, as PNG files.

The reference shows its scene in the rerun viewer (demo.py:35-65: a 3-D view, and the camera image
with the boxes on it); a headless node has no viewer.  `Renderer` is a small z-buffer on the device
(bf_render.hip): points, oriented-box wireframes and filled, shaded triangles become 64-bit keys
(layer, depth bits, colour) that an atomicMin per pixel sorts, for several cameras at once, so the
picture is the same bits whatever order the primitives arrive in (DESIGN.md §4 "Renderer").
`render_scene` draws a mesh, a cloud and boxes from given cameras, `orbit_poses` / `topdown_pose`
place cameras around a bounding box, `SnapshotWriter` is what `Pipeline.run(snapshots=...)` calls, and

    python -m boxfusion_amd.render SCENE.ply OUT_DIR [--boxes SEQ_boxes.pkl] [--views 8] [--size H W]
                                   [--as-points] [--no-cull] [--no-shade]

writes the orbit and top-down views of any PLY this package writes: a PLY with faces (scene_mesh) as
a surface, one without as points.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from boxfusion_amd import _lib
from boxfusion_amd.synthetic import SCANNET_K

MAX_RADIUS, MAX_HALF_WIDTH = 4, 2
MESH_GREY = 128


def camera_rows(poses):
    """camera -> world poses [V,4,4] (host array or tensor) -> world -> camera rows f32 [V,12] (R
    row-major, then t): the inverse in f64 on the host, cast to f32 once"""
    if torch.is_tensor(poses):
        poses = poses.detach().cpu().numpy()
    poses = np.asarray(poses, np.float64)
    if poses.ndim == 2:
        poses = poses[None]
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        raise ValueError(f"poses: camera->world [V,4,4], got {poses.shape}")
    inv = np.linalg.inv(poses)
    return np.concatenate([inv[:, :3, :3].reshape(-1, 9), inv[:, :3, 3]], 1).astype(np.float32)


class Renderer:
    """A key buffer int64 [views,H,W] (the uint64 keys of bf_render.hip) and the draws into it.  One
    pinhole K3 for all views; every draw call of a picture must be given the same poses."""

    def __init__(self, H, W, K3, views=1, device="cuda"):
        K = np.asarray(K3, np.float64)
        if K.shape != (3, 3):
            raise ValueError(f"K3: a 3x3 pinhole matrix, got {K.shape}")
        self.H, self.W, self.views = int(H), int(W), int(views)
        if self.H < 1 or self.W < 1 or self.views < 1:
            raise ValueError("Renderer: H, W and views must be at least 1")
        self.intr = tuple(np.float32(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
        self.device = torch.device(device)
        self.keys = torch.empty((self.views, self.H, self.W), dtype=torch.int64, device=self.device)
        self.clear()

    def clear(self):
        _lib.render_clear(self.keys)

    def _cams(self, poses):
        rows = camera_rows(poses)
        if rows.shape[0] != self.views:
            raise ValueError(f"poses: {rows.shape[0]} cameras for a renderer of {self.views} views")
        return torch.from_numpy(rows).to(self.device)

    def _dev(self, a, dtype, tail, name):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype != dtype:
            if dtype == torch.uint8:
                raise ValueError(f"{name}: expected uint8, got {t.dtype}")
            t = t.to(dtype)
        if t.dim() < len(tail) or tuple(t.shape[t.dim() - len(tail):]) != tuple(tail):
            raise ValueError(f"{name}: expected [...,{','.join(map(str, tail))}], got {tuple(t.shape)}")
        return t.to(self.device).reshape(-1, *tail).contiguous()

    def draw_points(self, xyz, rgb_u8, poses, radius=1, near=0.05, far=20.0, overlay=False, stats=None):
        """xyz [n,3] float and rgb_u8 [n,3] uint8 (host or device) as square splats of
        (2 radius + 1)^2 pixels, depth-tested; overlay draws them over the scene layer"""
        if not 0 <= int(radius) <= MAX_RADIUS:
            raise ValueError(f"radius: 0..{MAX_RADIUS}")
        xyz = self._dev(xyz, torch.float32, (3,), "xyz")
        rgb = self._dev(rgb_u8, torch.uint8, (3,), "rgb_u8")
        if xyz.shape[0] != rgb.shape[0]:
            raise ValueError(f"draw_points: {xyz.shape[0]} positions, {rgb.shape[0]} colours")
        _lib.render_points(self.keys, xyz, rgb, self._cams(poses), self.intr, near, far, radius, 0 if overlay else 1,
                           stats=stats)

    def draw_boxes(self, corners, colors_u8, poses, half_width=0, xray=False, mask=None, near=0.05):
        """the wireframes of corners [B,8,3] (v0..v7) in colors_u8 [B,3], lines 2 half_width + 1
        pixels wide; xray draws them over the scene (still depth-sorted among themselves); mask:
        None or [B], a false entry skips its box"""
        if not 0 <= int(half_width) <= MAX_HALF_WIDTH:
            raise ValueError(f"half_width: 0..{MAX_HALF_WIDTH}")
        corners = self._dev(corners, torch.float32, (8, 3), "corners")
        colors = self._dev(colors_u8, torch.uint8, (3,), "colors_u8")
        if mask is not None:
            mask = (mask if torch.is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(mask))).to(self.device)
            mask = (mask != 0).reshape(-1)
        _lib.render_edges(self.keys, corners, colors, mask, self._cams(poses), self.intr, near, half_width,
                          0 if xray else 1)

    def draw_mesh(self, vertices, faces, rgb_u8=None, poses=None, shade=True, cull=False, near=0.05, far=20.0,
                  overlay=False, stats=None, coop_pixels=None):
        """the triangles faces int [m,3] of vertices [n,3] float (host or device), filled and
        depth-tested, the colours rgb_u8 [n,3] uint8 (None: mid-grey) interpolated between the
        vertices; shade: a two-sided headlight; cull: drop the triangles seen from behind (the side a
        scene_mesh surface was not observed from).  A triangle with a vertex outside near < Z < far is
        dropped whole: there is no near-plane clipping.  stats: None or int64 [6] on the device
        (_lib.render_triangles)"""
        if poses is None:
            raise ValueError("draw_mesh: poses")
        vertices = self._dev(vertices, torch.float32, (3,), "vertices")
        if rgb_u8 is None:
            rgb = torch.full((vertices.shape[0], 3), MESH_GREY, dtype=torch.uint8, device=self.device)
        else:
            rgb = self._dev(rgb_u8, torch.uint8, (3,), "rgb_u8")
        t = faces if torch.is_tensor(faces) else torch.from_numpy(np.ascontiguousarray(faces))
        if t.dtype not in (torch.int32, torch.int64) or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"faces: an integer [m,3], got {t.dtype} {tuple(t.shape)}")
        if t.dtype == torch.int64:                               # an index beyond int32 is a bad index: -1 is one
            t = torch.where((t >= 0) & (t < 2 ** 31), t, torch.full_like(t, -1)).to(torch.int32)
        faces = t.to(self.device).contiguous()
        if vertices.shape[0] != rgb.shape[0]:
            raise ValueError(f"draw_mesh: {vertices.shape[0]} vertices, {rgb.shape[0]} colours")
        _lib.render_triangles(self.keys, vertices, rgb, faces, self._cams(poses), self.intr, near, far, 1 if cull else 0,
                              1 if shade else 0, 0 if overlay else 1, coop_pixels=coop_pixels, stats=stats)

    def resolve(self, background=(0, 0, 0)):
        """-> (rgb u8 [views,H,W,3], depth f32 [views,H,W]) on the device; empty pixels take the
        background, an (r, g, b) constant or a u8 image [views,H,W,3], and depth 0"""
        if torch.is_tensor(background) or isinstance(background, np.ndarray) and background.ndim > 1:
            background = self._dev(background, torch.uint8, (self.H, self.W, 3), "background")
        return _lib.render_resolve(self.keys, background)


# ---- cameras -------------------------------------------------------------------------------------------
def _centre_ray(K3, H, W):
    K = np.asarray(K3, np.float64)
    d = np.array([((W - 1) / 2.0 - K[0, 2]) / K[0, 0], ((H - 1) / 2.0 - K[1, 2]) / K[1, 1], 1.0])
    return d / np.linalg.norm(d)


def _cone_half_angle(K3, H, W):
    """the half-angle of the widest cone around the image centre's ray that stays inside the view
    frustum: the smallest angle between that ray and the four side planes"""
    K = np.asarray(K3, np.float64)
    ray = lambda u, v: np.array([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], 1.0])
    c = [ray(-0.5, -0.5), ray(W - 0.5, -0.5), ray(W - 0.5, H - 0.5), ray(-0.5, H - 0.5)]
    d = _centre_ray(K3, H, W)
    angles = []
    for a, b in zip(c, c[1:] + c[:1]):
        n = np.cross(a, b)
        angles.append(np.arcsin(abs(n @ d) / np.linalg.norm(n)))
    return min(angles)


def _place(R, lo, hi, K3, H, W, margin=1.05):
    """the camera -> world pose with rotation R whose image centre looks at the centre of the box
    lo..hi from far enough that the box's bounding sphere is inside the frustum"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    centre, radius = (lo + hi) / 2.0, max(np.linalg.norm(hi - lo) / 2.0, 1e-3)
    dist = margin * radius / np.sin(_cone_half_angle(K3, H, W))
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = centre - dist * (R @ _centre_ray(K3, H, W))
    return P.astype(np.float32)


def orbit_poses(lo, hi, n, elevation_deg=35.0, K3=SCANNET_K, H=480, W=640):
    """n camera -> world poses [n,4,4] on a circle around the centre of the box lo..hi, elevation_deg
    above it and looking at it (z-up world, camera y down), far enough that the box's bounding
    sphere fits the smaller field of view of the pinhole K3 at H x W"""
    e = np.deg2rad(float(elevation_deg))
    up = np.array([0.0, 0.0, 1.0])
    out = []
    for k in range(int(n)):
        a = 2.0 * np.pi * k / int(n)
        z = -np.array([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)])
        x = np.cross(z, up)
        x /= np.linalg.norm(x)
        out.append(_place(np.stack([x, np.cross(z, x), z], 1), lo, hi, K3, H, W))
    return np.stack(out) if out else np.zeros((0, 4, 4), np.float32)


def topdown_pose(lo, hi, K3, H, W):
    """a camera -> world pose [4,4] above the box lo..hi looking straight down (image x = world x,
    image y = world -y), the box's centre at the image centre and its bounding sphere in view"""
    R = np.array([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, -1.0]])
    return _place(R, lo, hi, K3, H, W)


def overview_K(H, W, hfov_deg=60.0):
    """a pinhole with the principal point at the image centre and a horizontal field of view"""
    f = (W / 2.0) / np.tan(np.deg2rad(hfov_deg) / 2.0)
    return np.array([[f, 0.0, (W - 1) / 2.0], [0.0, f, (H - 1) / 2.0], [0.0, 0.0, 1.0]], np.float32)


# ---- pictures ------------------------------------------------------------------------------------------
def box_colors(n):
    """the colour of box i of n as the box PLY writer picks it (visualize.random_color_v2(i / n),
    the jet table), u8 [n,3]"""
    from boxfusion_amd.visualize import random_color_v2
    cols = np.array([random_color_v2(i / n) for i in range(n)], np.float64).reshape(-1, 3)
    return np.clip(np.rint(cols * 255.0), 0, 255).astype(np.uint8)


def _points_of(points):
    if points is None:
        return None
    if hasattr(points, "points") and callable(points.points):        # a SceneCloud
        xyz, rgb, _ = points.points()
        return xyz, rgb
    xyz, rgb = points
    return xyz, rgb


def _boxes_of(boxes):
    if boxes is None:
        return None
    corners, colors = boxes if isinstance(boxes, (tuple, list)) and len(boxes) == 2 else (boxes, None)
    n = int(corners.shape[0])
    if n == 0:
        return None
    return corners, (box_colors(n) if colors is None else colors)


def _mesh_of(mesh):
    if mesh is None:
        return None
    if hasattr(mesh, "mesh") and callable(mesh.mesh):                # a TsdfVolume
        return mesh.mesh()
    vertices, rgb, faces = mesh
    return vertices, rgb, faces


def render_scene(points, boxes, poses, K3, H, W, radius=1, half_width=1, xray=False, background=(0, 0, 0),
                 near=0.05, far=100.0, device="cuda", mesh=None, shade=True, cull=False):
    """points: a SceneCloud, an (xyz [n,3], rgb u8 [n,3]) pair or None; boxes: corners [B,8,3], a
    (corners, colours u8 [B,3]) pair or None (default colours: box_colors); mesh: a TsdfVolume, a
    (vertices [n,3], rgb u8 [n,3] or None, faces [m,3]) triple or None, drawn filled (shade, cull:
    Renderer.draw_mesh); poses: camera -> world [V,4,4] -> (rgb u8 [V,H,W,3], depth f32 [V,H,W]) on
    the device"""
    rows = camera_rows(poses)
    r = Renderer(H, W, K3, views=rows.shape[0], device=device)
    pts, bx, tri = _points_of(points), _boxes_of(boxes), _mesh_of(mesh)
    if tri is not None:
        r.draw_mesh(tri[0], tri[2], tri[1], poses, shade=shade, cull=cull, near=near, far=far)
    if pts is not None:
        r.draw_points(pts[0], pts[1], poses, radius=radius, near=near, far=far)
    if bx is not None:
        r.draw_boxes(bx[0], bx[1], poses, half_width=half_width, xray=xray, near=near)
    return r.resolve(background)


def save_png(rgb_u8, path):
    """one image u8 [H,W,3] (host array or tensor) as a PNG"""
    from PIL import Image
    if torch.is_tensor(rgb_u8):
        rgb_u8 = rgb_u8.detach().cpu().numpy()
    rgb_u8 = np.ascontiguousarray(rgb_u8)
    if rgb_u8.dtype != np.uint8 or rgb_u8.ndim != 3 or rgb_u8.shape[2] != 3:
        raise ValueError(f"save_png: a uint8 [H,W,3] image, got {rgb_u8.dtype} {rgb_u8.shape}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(rgb_u8).save(path, format="PNG")


def _bounds(xyz, boxes, vertices=None):
    parts = []
    if vertices is not None and len(vertices):
        x = vertices.detach().cpu().numpy() if torch.is_tensor(vertices) else np.asarray(vertices)
        parts.append(x.reshape(-1, 3))
    if xyz is not None and len(xyz):
        x = xyz.detach().cpu().numpy() if torch.is_tensor(xyz) else np.asarray(xyz)
        parts.append(x.reshape(-1, 3))
    if boxes is not None:
        c = boxes[0].detach().cpu().numpy() if torch.is_tensor(boxes[0]) else np.asarray(boxes[0])
        parts.append(c.reshape(-1, 3))
    pts = np.concatenate(parts).astype(np.float64) if parts else np.zeros((0, 3))
    pts = pts[np.isfinite(pts).all(1)]
    if len(pts) == 0:
        return np.full(3, -1.0), np.full(3, 1.0)
    return pts.min(0), pts.max(0)


def write_overviews(points, boxes, out_dir, views=8, size=(480, 640), radius=1, half_width=1, K3=None, device="cuda",
                    mesh=None, shade=True, cull=True, prefix="overview"):
    """`views` orbit views (<prefix>_<k>.png) and one from above (<prefix>_top.png) of a cloud, a
    mesh and depth-tested boxes, the cameras placed around what is drawn; returns the paths written.
    A mesh is drawn culled by default: the orbit cameras stand outside a room whose walls face
    inwards, so culling shows the doll's house rather than the outside of four walls"""
    H, W = int(size[0]), int(size[1])
    K3 = overview_K(H, W) if K3 is None else K3
    pts, bx, tri = _points_of(points), _boxes_of(boxes), _mesh_of(mesh)
    lo, hi = _bounds(None if pts is None else pts[0], bx, None if tri is None else tri[0])
    poses = np.concatenate([orbit_poses(lo, hi, views, K3=K3, H=H, W=W), topdown_pose(lo, hi, K3, H, W)[None]])
    far = 4.0 * float(np.linalg.norm(hi - lo)) + 10.0
    rgb, _ = render_scene(pts, bx, poses, K3, H, W, radius=radius, half_width=half_width, far=far, device=device,
                          mesh=tri, shade=shade, cull=cull)
    rgb = rgb.cpu().numpy()
    names = [f"{prefix}_{k}.png" for k in range(int(views))] + [f"{prefix}_top.png"]
    paths = [os.path.join(out_dir, n) for n in names]
    for img, p in zip(rgb, paths):
        save_png(img, p)
    return paths


class SnapshotWriter:
    """What Pipeline.run(snapshots=...) calls: after every keyframe's fusion step (and after the last
    frame) `snap_<count:06d>.png`, the frame's RGB with the current global boxes as x-ray wireframes
    from the frame's camera; at the end, when the run also filled a SceneCloud and cloud_views > 0,
    `overview_<k>.png` and `overview_top.png` of the cloud with depth-tested boxes, and, when finish
    is given the run's TsdfVolume, `mesh_<k>.png` and `mesh_top.png` of its surface with them."""

    def __init__(self, out_dir, K3, H, W, every="keyframes", cloud_views=0, half_width=1, device="cuda"):
        if every != "keyframes":
            raise ValueError("every: 'keyframes'")
        self.out_dir, self.K3, self.H, self.W = str(out_dir), np.asarray(K3, np.float32), int(H), int(W)
        self.cloud_views, self.half_width, self.device = int(cloud_views), int(half_width), device
        self.renderer = None
        self.written = []

    @staticmethod
    def _corners(all_pred_box):
        if all_pred_box is None or len(all_pred_box) == 0:
            return None
        return all_pred_box.pred_boxes_3d.corners.detach().to(torch.float32)

    def snapshot(self, count, pose, rgb_u8, all_pred_box):
        """frame `count`: rgb_u8 u8 [H,W,3] on the device, pose camera -> world [4,4]"""
        if tuple(rgb_u8.shape) != (self.H, self.W, 3):
            raise ValueError(f"snapshot: a frame of {self.H} x {self.W}, got {tuple(rgb_u8.shape)}")
        if self.renderer is None:
            self.renderer = Renderer(self.H, self.W, self.K3, views=1, device=self.device)
        r = self.renderer
        r.clear()
        corners = self._corners(all_pred_box)
        if corners is not None:
            r.draw_boxes(corners, box_colors(corners.shape[0]), np.asarray(pose)[None], half_width=self.half_width,
                         xray=True)
        rgb, _ = r.resolve(rgb_u8[None])
        path = os.path.join(self.out_dir, f"snap_{int(count):06d}.png")
        save_png(rgb[0], path)
        self.written.append(path)
        return path

    def finish(self, cloud, all_pred_box, mesh=None):
        if self.cloud_views <= 0:
            return []
        paths = []
        if cloud is not None:
            paths += write_overviews(cloud, self._corners(all_pred_box), self.out_dir, views=self.cloud_views,
                                     size=(self.H, self.W), half_width=self.half_width, device=self.device)
        if mesh is not None:
            paths += write_overviews(None, self._corners(all_pred_box), self.out_dir, views=self.cloud_views,
                                     size=(self.H, self.W), half_width=self.half_width, device=self.device, mesh=mesh,
                                     prefix="mesh")
        self.written += paths
        return paths


# ---- command line --------------------------------------------------------------------------------------
def add_render_arguments(p):
    p.add_argument("--boxes", default=None, help="a <seq>_boxes.pkl of results.export to draw as wireframes")
    p.add_argument("--views", type=int, default=8, help="orbit views")
    p.add_argument("--size", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    p.add_argument("--radius", type=int, default=1, help=f"point splat radius in pixels, 0..{MAX_RADIUS}")
    p.add_argument("--no-cull", action="store_true", help="a mesh: also draw the triangles seen from behind")
    p.add_argument("--no-shade", action="store_true", help="a mesh: the vertex colours as they are, no headlight")


def check_render_arguments(p, a):
    if a.views < 0:
        p.error("--views must not be negative")
    if min(a.size) < 1 or max(a.size) > 16384:
        p.error("--size: H and W in 1..16384")
    if not 0 <= a.radius <= MAX_RADIUS:
        p.error(f"--radius must be in 0..{MAX_RADIUS}")


def load_boxes_argument(path):
    from boxfusion_amd.results import load_global_boxes
    return None if path is None else load_global_boxes(path).astype(np.float32)


def parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m boxfusion_amd.render",
                                description="orbit and top-down PNG views of a point or mesh PLY (and boxes)")
    p.add_argument("cloud", help="a PLY written by SceneCloud.save_ply / visualize.points_to_ply (points) or "
                                 "TsdfVolume.save_ply / visualize.mesh_to_ply (drawn as a surface)")
    p.add_argument("out_dir")
    add_render_arguments(p)
    p.add_argument("--as-points", action="store_true", help="draw a mesh PLY's vertices as points")
    return p


def main(argv=None):
    from boxfusion_amd.visualize import read_ply_surface
    p = parser()
    a = p.parse_args(argv)
    check_render_arguments(p, a)
    xyz, rgb, faces = read_ply_surface(a.cloud)
    if len(faces) and not a.as_points:
        paths = write_overviews(None, load_boxes_argument(a.boxes), a.out_dir, views=a.views, size=a.size,
                                mesh=(xyz, rgb, faces), shade=not a.no_shade, cull=not a.no_cull)
        print(f"{len(xyz)} vertices, {len(faces)} faces -> {len(paths)} views in {a.out_dir}")
        return 0
    paths = write_overviews((xyz, rgb), load_boxes_argument(a.boxes), a.out_dir, views=a.views, size=a.size, radius=a.radius)
    print(f"{len(xyz)} points -> {len(paths)} views in {a.out_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
