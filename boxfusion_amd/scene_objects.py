"""Objects in the scene: the cloud's points and the mesh's faces labelled by the fused boxes.

The reference ends at `<seq>_boxes.pkl`; its ground-truth filter (data_process/filter_gt_boxes.py:75-93)
keeps a GT box when scene points are near its corners.  This module turns the same idea towards the
predictions: bf_label_points (bf_objects.hip) tests every point of a scene against every oriented box in
one launch, gives each point to the smallest box that contains it, and counts per box what lies inside
it (its support: a box with none is a phantom), what it owns, and how far the owned points reach along
its own axes.  The outputs are integers and integer keys, the same bits in any order of arrival
(DESIGN.md §4 "Objects").

  box_rows(corners)                         corners [B,8,3] in any vertex order -> the kernel's f32 [B,16] rows
  label_points / label_cloud / label_mesh   -> ObjectLabels (label_mesh adds a label per face)
  supported(labels, min_points)             the phantom filter: boxes with enough points inside
  instance_colours(labels, rgb)             the scene colours with every object tinted in its box's colour
  object_meshes / save_objects              one PLY per object, labels.txt, objects.json
  instance_maps(scene, labels, poses, ...)  a per-pixel instance map of given views, through the renderer

    python -m boxfusion_amd.scene_objects SCENE.ply BOXES.pkl OUT_DIR [--margin 0.0] [--min-points 1]
                                          [--views 8 --size 480 640]

reads a PLY this package writes (with faces: a mesh, without: a cloud) and the boxes of results.export,
writes what save_objects writes and, with --views > 0, instance-coloured overviews with the supported
boxes drawn.
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
import sys

import numpy as np
import torch

from boxfusion_amd.evaluation import boxes_from_corners

ID_LIMIT = (1 << 24) - 1            # ids that fit the 24 colour bits beside the background's 0


# ---- small codes ---------------------------------------------------------------------------------------
def extent_keys(values):
    """f32 values -> the uint32 keys bf_label_points orders them by: the sign bit flipped where it is
    clear, every bit flipped where it is set, so that the keys order as the floats do"""
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def extent_values(keys):
    """the inverse of extent_keys: uint32 keys -> f32 values"""
    keys = np.ascontiguousarray(keys, np.uint32)
    bits = np.where(keys & np.uint32(0x80000000), keys ^ np.uint32(0x80000000), ~keys).astype(np.uint32)
    return bits.view(np.float32)


def id_colours(ids):
    """integer ids [n] in -1..ID_LIMIT - 1 -> u8 [n,3]: id + 1 in the 24 colour bits, red the high byte,
    so that -1 (no object) is black, the renderer's background"""
    tensor = torch.is_tensor(ids)
    v = (ids.to(torch.int64) if tensor else np.asarray(ids, np.int64)) + 1
    if v.numel() if tensor else v.size:
        if int(v.min()) < 0 or int(v.max()) > ID_LIMIT:
            raise ValueError(f"id_colours: ids in -1..{ID_LIMIT - 1}")
    if tensor:
        return torch.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).to(torch.uint8)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8)


def colour_ids(rgb):
    """the inverse of id_colours: u8 [...,3] -> int32 [...] ids, -1 for black"""
    if torch.is_tensor(rgb):
        c = rgb.to(torch.int32)
        return ((c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]) - 1
    c = np.asarray(rgb).astype(np.int32)
    return ((c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2]) - 1


# ---- boxes -----------------------------------------------------------------------------------------------
def box_rows(corners):
    """corners [B,8,3] of cuboids, the vertices in any order -> (rows f32 [B,16], degenerate bool [B]).
    A row is the centre, three unit axes, the half-lengths and the volume 8 h0 h1 h2, worked out in
    f64 from evaluation.boxes_from_corners and cast to f32 once.  A box with a half-length that is
    not finite or not > 0 (a flat box, a box of NaN) is degenerate: its row is NaN and contains
    nothing."""
    c = corners.detach().cpu().numpy() if torch.is_tensor(corners) else np.asarray(corners)
    c = np.asarray(c, np.float64)
    if c.ndim != 3 or c.shape[1:] != (8, 3):
        raise ValueError(f"box_rows: corners [B,8,3], got {c.shape}")
    n = c.shape[0]
    bad = ~np.isfinite(c).all((1, 2))
    if bad.any():                                    # any cuboid stands in: the row is replaced below
        c = c.copy()
        c[bad] = np.array(list(np.ndindex(2, 2, 2)), np.float64)
    b = boxes_from_corners(c)
    half = b[:, 3:].reshape(n, 3, 3)
    h = np.linalg.norm(half, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        axes = half / h[..., None]
    rows = np.concatenate([b[:, :3], axes.reshape(n, 9), h, (8.0 * h[:, 0] * h[:, 1] * h[:, 2])[:, None]], 1)
    with np.errstate(over="ignore"):
        rows = rows.astype(np.float32)
    h32 = rows[:, 12:15]
    degenerate = bad | ~(np.isfinite(h32) & (h32 > 0)).all(1) | ~np.isfinite(rows).all(1)
    rows[degenerate] = np.nan
    return rows, degenerate


@dataclasses.dataclass
class ObjectLabels:
    """What label_points returns.  labels: int32 [n] on the device, the owning box of every point or
    -1; support / owned: int64 [B], the points inside each box and the points it owns; extents: f32
    [B,3,2], min and max of the owned points along the box's own axes (NaN where owned == 0); fill:
    f64 [B], the volume of that tight extent over the box's volume (0 where nothing is owned);
    degenerate: bool [B] (box_rows); stats: the kernel's counters by name; face_labels: int32 [m] on
    the device, only from label_mesh."""
    labels: object
    support: np.ndarray
    owned: np.ndarray
    extents: np.ndarray
    fill: np.ndarray
    degenerate: np.ndarray
    stats: dict
    face_labels: object = None

    @property
    def boxes(self):
        return int(self.support.shape[0])


def _device_points(xyz, device=None):
    t = xyz if torch.is_tensor(xyz) else torch.from_numpy(np.ascontiguousarray(xyz))
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"xyz: [n,3], got {tuple(t.shape)}")
    if device is None:
        device = t.device if t.is_cuda else torch.device("cuda")
    return t.to(device=device, dtype=torch.float32).contiguous()


def label_points(xyz, corners, margin=0.0, device=None):
    """xyz [n,3] (tensor or array) against the boxes corners [B,8,3] -> ObjectLabels.  A point is
    inside a box when it is within half-length + margin of the centre along each of the box's axes
    (include/boxfusion_objects.h has the arithmetic), and is owned by the smallest box it is inside."""
    from boxfusion_amd import _lib
    margin = float(margin)
    if not math.isfinite(margin):
        raise ValueError("margin must be finite")
    rows, degenerate = box_rows(corners)
    xyz = _device_points(xyz, device)
    labels, counts, keys, stats = _lib.label_points(xyz, torch.from_numpy(rows).to(xyz.device), margin)
    counts = counts.cpu().numpy()
    support, owned = counts[:, 0].copy(), counts[:, 1].copy()
    extents = extent_values(keys.cpu().numpy().view(np.uint32)).reshape(-1, 3, 2).copy()
    extents[owned == 0] = np.nan
    with np.errstate(invalid="ignore"):
        tight = np.prod((extents[:, :, 1].astype(np.float64) - extents[:, :, 0].astype(np.float64)), axis=1)
        fill = np.where(owned > 0, tight / rows[:, 15].astype(np.float64), 0.0)
    return ObjectLabels(labels=labels, support=support, owned=owned, extents=extents, fill=fill, degenerate=degenerate,
                        stats=dict(zip(_lib.OBJ_STATS, stats.cpu().tolist())))


def _cloud_of(cloud):
    """(xyz, rgb) of a SceneCloud or of an (xyz, rgb) pair"""
    if hasattr(cloud, "points") and callable(cloud.points):
        xyz, rgb, _ = cloud.points()
        return xyz, rgb
    xyz, rgb = cloud
    return xyz, rgb


def _mesh_of(mesh):
    """(vertices, rgb, faces) of a TsdfVolume or of such a triple"""
    if hasattr(mesh, "mesh") and callable(mesh.mesh):
        return mesh.mesh()
    vertices, rgb, faces = mesh
    return vertices, rgb, faces


def label_cloud(cloud, corners, margin=0.0):
    """label_points over the points of a SceneCloud (sorted by voxel key) or an (xyz, rgb) pair"""
    return label_points(_cloud_of(cloud)[0], corners, margin)


def face_labels(vertex_labels, faces):
    """the common label of each face's three vertices, else -1; tensors or arrays, int32 [m] of the
    same kind.  A face with a vertex index outside the labels is -1."""
    if torch.is_tensor(vertex_labels):
        f = torch.as_tensor(faces, device=vertex_labels.device).long().reshape(-1, 3)
        ok = ((f >= 0) & (f < vertex_labels.shape[0])).all(1)
        l = vertex_labels.to(torch.int32)[f.clamp(0, max(vertex_labels.shape[0] - 1, 0))] if len(vertex_labels) else \
            torch.full_like(f, -1, dtype=torch.int32)
        same = ok & (l[:, 0] == l[:, 1]) & (l[:, 1] == l[:, 2])
        return torch.where(same, l[:, 0], torch.full_like(l[:, 0], -1))
    v = np.asarray(vertex_labels, np.int32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < len(v))).all(1)
    l = v[np.clip(f, 0, max(len(v) - 1, 0))] if len(v) else np.full(f.shape, -1, np.int32)
    return np.where(ok & (l[:, 0] == l[:, 1]) & (l[:, 1] == l[:, 2]), l[:, 0], -1).astype(np.int32)


def label_mesh(mesh, corners, margin=0.0):
    """label_points over the vertices of a TsdfVolume's surface (in block order) or of a (vertices,
    rgb, faces) triple; face_labels holds each face's label: its three vertices' common one, else -1"""
    vertices, _, faces = _mesh_of(mesh)
    out = label_points(vertices, corners, margin)
    out.face_labels = face_labels(out.labels, faces)
    return out


def supported(labels, min_points=1):
    """bool [B]: the boxes with at least min_points points inside them.  A predicted box below it has
    no geometry behind it: a phantom."""
    return np.asarray(labels.support) >= int(min_points)


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def instance_colours(labels, rgb, blend=0.6):
    """rgb u8 [n,3] with every labelled point tinted: blend of its box's colour (render.box_colors)
    over (1 - blend) of its own, rounded; unlabelled points are kept as they are.  u8 [n,3] on the host."""
    from boxfusion_amd.render import box_colors
    if not 0.0 <= float(blend) <= 1.0:
        raise ValueError("blend: 0..1")
    lab = _host(labels.labels if isinstance(labels, ObjectLabels) else labels).astype(np.int64)
    rgb = _host(rgb)
    if rgb.dtype != np.uint8 or rgb.shape != (len(lab), 3):
        raise ValueError(f"rgb: uint8 [{len(lab)},3], got {rgb.dtype} {rgb.shape}")
    out = rgb.copy()
    hit = lab >= 0
    if hit.any():
        n_boxes = labels.boxes if isinstance(labels, ObjectLabels) else int(lab.max()) + 1
        tint = box_colors(n_boxes)[lab[hit]].astype(np.float64)
        out[hit] = np.clip(np.rint(float(blend) * tint + (1.0 - float(blend)) * rgb[hit]), 0, 255).astype(np.uint8)
    return out


# ---- objects as files --------------------------------------------------------------------------------------
def object_meshes(mesh, labels):
    """{box: (vertices f32 [k,3], rgb u8 [k,3], faces int32 [j,3])} on the host for every box that owns
    a face of the (vertices, rgb, faces) mesh: the faces with that label, in their order, and the
    vertices they use, in their order, re-indexed.  labels: an ObjectLabels of label_mesh, or the
    labels of the vertices."""
    vertices, rgb, faces = (_host(a) for a in _mesh_of(mesh))
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    if isinstance(labels, ObjectLabels):
        fl = _host(labels.face_labels) if labels.face_labels is not None else face_labels(_host(labels.labels), faces)
    else:
        fl = face_labels(_host(labels), faces)
    out = {}
    for b in np.unique(fl[fl >= 0]):
        f = faces[fl == b]
        used = np.unique(f)                                     # ascending: the vertices keep their order
        remap = np.full(len(vertices), -1, np.int64)
        remap[used] = np.arange(len(used))
        out[int(b)] = (np.asarray(vertices, np.float32)[used], np.asarray(rgb, np.uint8)[used], remap[f].astype(np.int32))
    return out


def _json_floats(a):
    return [None if not np.isfinite(v) else float(v) for v in np.asarray(a, np.float64).reshape(-1)]


def save_objects(out_dir, scene, labels):
    """scene: a mesh (a TsdfVolume or a (vertices, rgb, faces) triple, with labels from label_mesh) or a
    cloud (a SceneCloud or an (xyz, rgb) pair).  Writes object_<box:04d>.ply for every box that owns
    something (its faces and their vertices for a mesh, its points for a cloud), labels.txt (one label
    per vertex or point) and objects.json (support, owned, extents, fill and degenerate per box, and the
    kernel's stats); returns the paths."""
    from boxfusion_amd.visualize import mesh_to_ply, points_to_ply
    os.makedirs(out_dir, exist_ok=True)
    lab = _host(labels.labels).astype(np.int32)
    paths = []
    if labels.face_labels is not None:
        for b, (v, c, f) in sorted(object_meshes(scene, labels).items()):
            paths.append(os.path.join(out_dir, f"object_{b:04d}.ply"))
            mesh_to_ply(v, c, f, paths[-1])
    else:
        xyz, rgb = (_host(a) for a in _cloud_of(scene))
        for b in np.unique(lab[lab >= 0]):
            paths.append(os.path.join(out_dir, f"object_{int(b):04d}.ply"))
            points_to_ply(xyz[lab == b], rgb[lab == b], paths[-1])
    paths.append(os.path.join(out_dir, "labels.txt"))
    np.savetxt(paths[-1], lab, fmt="%d")
    boxes = [dict(box=b, support=int(labels.support[b]), owned=int(labels.owned[b]),
                  extents=[_json_floats(e) for e in labels.extents[b]], fill=float(labels.fill[b]),
                  degenerate=bool(labels.degenerate[b])) for b in range(labels.boxes)]
    paths.append(os.path.join(out_dir, "objects.json"))
    with open(paths[-1], "w") as fh:
        json.dump(dict(kind="mesh" if labels.face_labels is not None else "cloud", boxes=boxes,
                       stats={k: int(v) for k, v in labels.stats.items()}), fh, indent=1)
    return paths


# ---- instance maps ---------------------------------------------------------------------------------------
def instance_maps(scene, labels, poses, K, H, W, radius=1, near=0.05, far=100.0):
    """The instance each pixel of the views poses [V,4,4] (camera -> world) sees through the pinhole K
    at H x W: int32 [V,H,W] on the device, -1 where nothing, or nothing labelled, is seen.  The scene
    goes through the renderer with id + 1 in the 24 colour bits (id_colours).  A cloud (labels from
    label_points / label_cloud) is drawn as splats of the given radius; a mesh (labels from label_mesh)
    as a flat-coloured triangle soup, every face's three vertices duplicated with the face's label and
    no shading, so a pixel carries one face's id and never a blend.  Unlabelled geometry is drawn as id
    0: it hides the labelled geometry behind it."""
    from boxfusion_amd.render import Renderer, camera_rows
    views = camera_rows(poses).shape[0]
    if labels.boxes > ID_LIMIT:
        raise ValueError(f"instance_maps: at most {ID_LIMIT} boxes")
    if labels.face_labels is not None:
        vertices, _, faces = _mesh_of(scene)
        dev = labels.face_labels.device
        r = Renderer(H, W, K, views=views, device=dev)
        v = _device_points(vertices, dev)
        f = torch.as_tensor(faces, device=dev).long().reshape(-1, 3)
        ok = ((f >= 0) & (f < v.shape[0])).all(1)
        f, fl = f[ok], labels.face_labels[ok]
        soup = v[f.reshape(-1)]
        r.draw_mesh(soup, torch.arange(soup.shape[0], dtype=torch.int32, device=dev).reshape(-1, 3),
                    id_colours(fl.repeat_interleave(3)), poses, shade=False, cull=False, near=near, far=far)
    else:
        xyz = _cloud_of(scene)[0] if not torch.is_tensor(scene) and not isinstance(scene, np.ndarray) else scene
        dev = labels.labels.device
        r = Renderer(H, W, K, views=views, device=dev)
        r.draw_points(_device_points(xyz, dev), id_colours(labels.labels), poses, radius=radius, near=near, far=far)
    rgb, _ = r.resolve((0, 0, 0))
    return colour_ids(rgb)


# ---- command line ----------------------------------------------------------------------------------------
def parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m boxfusion_amd.scene_objects",
                                description="label a scene PLY by the fused boxes: one PLY per object, labels.txt, "
                                            "objects.json and instance-coloured overviews")
    p.add_argument("scene", help="a PLY written by SceneCloud.save_ply / visualize.points_to_ply (a cloud) or "
                                 "TsdfVolume.save_ply / visualize.mesh_to_ply (a mesh)")
    p.add_argument("boxes", help="a <seq>_boxes.pkl of results.export")
    p.add_argument("out_dir")
    p.add_argument("--margin", type=float, default=0.0, help="metres added to every half-length")
    p.add_argument("--min-points", type=int, default=1, help="points inside a box below which it is a phantom")
    p.add_argument("--views", type=int, default=8, help="orbit views of the overviews; 0 writes none")
    p.add_argument("--size", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    return p


def check_arguments(p, a):
    if not (math.isfinite(a.margin) and a.margin >= 0):
        p.error("--margin must be finite and not negative")
    if a.min_points < 0:
        p.error("--min-points must not be negative")
    if a.views < 0:
        p.error("--views must not be negative")
    if min(a.size) < 1 or max(a.size) > 16384:
        p.error("--size: H and W in 1..16384")


def main(argv=None):
    from boxfusion_amd.render import box_colors, write_overviews
    from boxfusion_amd.results import load_global_boxes
    from boxfusion_amd.visualize import read_ply_surface
    p = parser()
    a = p.parse_args(argv)
    check_arguments(p, a)
    xyz, rgb, faces = read_ply_surface(a.scene)
    corners = load_global_boxes(a.boxes).astype(np.float32)
    is_mesh = len(faces) > 0
    labels = label_mesh((xyz, rgb, faces), corners, a.margin) if is_mesh else label_points(xyz, corners, a.margin)
    scene = (xyz, rgb, faces) if is_mesh else (xyz, rgb)
    paths = save_objects(a.out_dir, scene, labels)
    keep = supported(labels, a.min_points)
    if a.views > 0:
        tint = instance_colours(labels, rgb)
        boxes = (corners[keep], box_colors(len(corners))[keep]) if keep.any() else None
        if is_mesh:
            paths += write_overviews(None, boxes, a.out_dir, views=a.views, size=a.size, mesh=(xyz, tint, faces),
                                     prefix="objects")
        else:
            paths += write_overviews((xyz, tint), boxes, a.out_dir, views=a.views, size=a.size, prefix="objects")
    s = labels.stats
    print(f"{len(xyz)} {'vertices' if is_mesh else 'points'}, {len(corners)} boxes: {int(keep.sum())} supported, "
          f"{int(labels.degenerate.sum())} degenerate, {s['labelled']} labelled, {s['shared']} shared -> "
          f"{len(paths)} files in {a.out_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
