"""Score a run against ground truth.

The ground-truth half restates the reference's data_process/filter_gt_boxes.py, which turns CA-1M's
`instances.json` into `after_filter_boxes.npy`:

  frustum_visible(corners, K, poses, image_hw)   frustum_culling_bbox_level (:24-68): a box is kept
                                                 when >= 6 of its corners project into some frame
  proximity_mask(corners, points, threshold)     check_bbox_proximity (:75-93): a box survives when
                                                 >= 4 of its corners have a scene point nearer than
                                                 the threshold
  filter_gt_boxes(...)                           filter_3d_corners (:7-22): both, same return

The scoring half has no counterpart in the reference (its evaluation code is unreleased):

  boxes_from_corners(corners)                    eight corners in any order -> centre + half-axes
  iou_matrix(pred, gt)                           exact oriented-box IoU (bf_obb_iou_exact)
  match(iou) / score(pred, gt, thresholds)       one-to-one greedy matching; precision, recall, F1

The three kernels (bf_gt_frustum, bf_nn_min_dist2, bf_obb_iou_exact) run on the device in f64; the
rest is host bookkeeping on a few thousand boxes.  Command line:

  python -m boxfusion_amd.evaluation filter SEQ_DIR [--points mesh.ply] [--dist 0.1]
  python -m boxfusion_amd.evaluation score BOXES.pkl GT.npy [--iou 0.25 0.5] [--json OUT]
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import struct
import sys

import numpy as np

_TRIPLES = np.array(list(itertools.combinations(range(6), 3)))          # [20,3]
_SIGNS = np.array(list(itertools.product((-1.0, 1.0), repeat=3)))       # [8,3]


# ---- boxes ---------------------------------------------------------------------------------------
def boxes_from_corners(corners):
    """corners [n,8,3] of cuboids, the eight vertices in any order -> f64 [n,12]: the centre and
    three half-axis vectors, longest first, each signed so that its largest component is positive.
    The centre is the corners' mean.  From corner 0 the farthest corner gives the space diagonal d;
    of the other six corners the three whose offsets e_i + e_j + e_k come nearest to d are the
    edges at corner 0.  Raises ValueError when the box rebuilt from the result misses a given
    corner by more than 1e-3 of the diagonal, or when its edges are out of square by as much."""
    c = np.asarray(corners, np.float64)
    if c.ndim != 3 or c.shape[1:] != (8, 3):
        raise ValueError(f"boxes_from_corners: expected [n,8,3], got {c.shape}")
    n = c.shape[0]
    out = np.zeros((n, 12))
    if n == 0:
        return out
    rows = np.arange(n)
    e = c - c[:, :1]                                                     # offsets from corner 0
    far = np.argmax((e * e).sum(-1), 1)
    d = e[rows, far]
    rest = np.stack([np.delete(np.arange(1, 8), np.where(np.arange(1, 8) == f)[0]) for f in far])
    er = e[rows[:, None], rest]                                          # [n,6,3]
    miss = np.linalg.norm(er[:, _TRIPLES].sum(2) - d[:, None], axis=-1)  # [n,20]
    tri = _TRIPLES[np.argmin(miss, 1)]                                   # [n,3]
    half = 0.5 * er[rows[:, None], tri]                                  # [n,3,3]
    # a canonical form: longest axis first, the largest component of each axis positive
    order = np.argsort(-np.linalg.norm(half, axis=-1), axis=1, kind="stable")
    half = half[rows[:, None], order]
    big = np.argmax(np.abs(half), -1)
    sign = np.sign(np.take_along_axis(half, big[..., None], -1))
    half = half * np.where(sign == 0, 1.0, sign)
    centre = c.mean(1)
    rebuilt = centre[:, None] + np.einsum("sk,nkj->nsj", _SIGNS, half)   # [n,8,3]
    gap = np.linalg.norm(c[:, :, None] - rebuilt[:, None], axis=-1)      # [n,8,8]
    worst = np.maximum(gap.min(2).max(1), gap.min(1).max(1))
    diag = np.linalg.norm(d, axis=-1)
    # a sheared box rebuilds exactly from its three edges, so the edges must also be at right angles:
    # the foot of one edge along another, taken over the diagonal, is held to the same 1e-3
    ln = np.linalg.norm(half, axis=-1)
    gram = np.abs(np.einsum("nik,njk->nij", half, half)) / np.maximum(ln[:, :, None], 1e-300)
    skew = 2.0 * np.max(gram * (1.0 - np.eye(3)), axis=(1, 2))
    worst = np.maximum(worst, skew)
    bad = np.where(~(worst <= 1e-3 * diag))[0]
    if len(bad):
        raise ValueError(f"boxes_from_corners: box {int(bad[0])} is not a cuboid (corner off by "
                         f"{worst[bad[0]]:.3g} with a diagonal of {diag[bad[0]]:.3g})")
    out[:, :3] = centre
    out[:, 3:] = half.reshape(n, 9)
    return out


def _device(*arrays):
    """the device of the first device tensor among `arrays`, else the current HIP device"""
    import torch
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return torch.device("cuda")


def _to_device_f64(a, device):
    import torch
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(device)


# ---- the ground-truth filter -----------------------------------------------------------------------
def frustum_visible(corners, K, poses, image_hw, near=0.1, far=100.0):
    """frustum_culling_bbox_level (filter_gt_boxes.py:24-68): corners [N,8,3] in the world frame, K
    [3,3], poses [M,4,4] (inverted here with np.linalg.inv, as :40 does), image_hw = (H, W) of the
    depth maps -> (box_mask bool [N]: >= 6 corners seen, seen bool [N,8])"""
    from boxfusion_amd import _lib
    corners = np.asarray(corners, np.float64).reshape(-1, 8, 3)
    K = np.asarray(K, np.float64)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    H, W = int(image_hw[0]), int(image_hw[1])
    if len(corners) == 0 or len(poses) == 0:
        seen = np.zeros((len(corners), 8), bool)
        return seen.sum(1) >= 6, seen
    with np.errstate(all="ignore"):
        pose_inv = np.linalg.inv(poses)
    dev = _device()
    seen = _lib.gt_frustum_seen(_to_device_f64(corners, dev), _to_device_f64(pose_inv, dev), float(K[0, 0]),
                                float(K[1, 1]), float(K[0, 2]), float(K[1, 2]), W, H, float(near), float(far))
    seen = seen.cpu().numpy().astype(bool)
    return seen.sum(1) >= 6, seen


def proximity_mask(corners, points, threshold=0.3):
    """check_bbox_proximity (filter_gt_boxes.py:75-93): corners [N,8,3], points [P,3] (an array or a
    tensor on either side) -> (mask bool [N]: >= 4 corners with a point nearer than `threshold`,
    dist f64 [N,8]: each corner's distance to its nearest point, inf without points)"""
    from boxfusion_amd import _lib
    corners = np.asarray(corners, np.float64).reshape(-1, 8, 3)
    n = len(corners)
    if n == 0 or len(points) == 0:
        dist = np.full((n, 8), np.inf)
        return np.zeros(n, bool), dist
    dev = _device(points)
    pts = _to_device_f64(points, dev).reshape(-1, 3)
    d2 = _lib.nn_min_dist2(_to_device_f64(corners.reshape(-1, 3), dev), pts)
    dist = np.sqrt(d2.cpu().numpy()).reshape(n, 8)
    return (dist < threshold).sum(1) >= 4, dist


def filter_gt_boxes(corners, K, poses, image_hw, points, near=0.1, far=100.0, dist_threshold=0.3):
    """filter_3d_corners (filter_gt_boxes.py:7-22) with the depth maps replaced by their size and the
    mesh by its points: -> (filtered_corners [B,8,3], frustum_mask bool [N])"""
    corners = np.asarray(corners, np.float64).reshape(-1, 8, 3)
    frustum_mask, _ = frustum_visible(corners, K, poses, image_hw, near, far)
    visible = corners[frustum_mask]
    near_mask, _ = proximity_mask(visible, points, dist_threshold)
    return visible[near_mask], frustum_mask


# ---- scoring -----------------------------------------------------------------------------------------
def iou_matrix(pred_corners, gt_corners):
    """exact IoU of every predicted box with every ground-truth box (bf_obb_iou_exact): corners
    [P,8,3] and [G,8,3] in any vertex order -> f64 [P,G] on the device"""
    from boxfusion_amd import _lib
    dev = _device(pred_corners, gt_corners)
    a = _to_device_f64(boxes_from_corners(_host(pred_corners)), dev)
    b = _to_device_f64(boxes_from_corners(_host(gt_corners)), dev)
    return _lib.obb_iou_exact(a, b)


def _host(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64).reshape(-1, 8, 3)


def match(iou):
    """one-to-one greedy matching of an IoU matrix [P,G] by descending IoU; equal IoUs go to the
    lower pred index, then the lower gt index, and pairs that do not overlap are never matched ->
    (pred_idx int64 [m], gt_idx int64 [m], iou f64 [m]) in the order they were matched"""
    if hasattr(iou, "detach"):
        iou = iou.detach().cpu().numpy()
    iou = np.asarray(iou, np.float64)
    if iou.ndim != 2:
        raise ValueError(f"match: expected an IoU matrix [P,G], got {iou.shape}")
    P, G = iou.shape
    flat = iou.reshape(-1)
    cand = np.flatnonzero(flat > 0)                                      # row-major: pred, then gt
    cand = cand[np.argsort(-flat[cand], kind="stable")]
    used_p, used_g = np.zeros(P, bool), np.zeros(G, bool)
    pi, gi, vi = [], [], []
    for k in cand:
        p, g = divmod(int(k), G)
        if used_p[p] or used_g[g]:
            continue
        used_p[p] = used_g[g] = True
        pi.append(p)
        gi.append(g)
        vi.append(flat[k])
    return np.array(pi, np.int64), np.array(gi, np.int64), np.array(vi, np.float64)


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


def score_from_iou(iou, thresholds=(0.25, 0.5)):
    """the summary of score() from an IoU matrix [P,G]"""
    if hasattr(iou, "detach"):
        iou = iou.detach().cpu().numpy()
    iou = np.asarray(iou, np.float64)
    P, G = iou.shape
    pi, gi, vi = match(iou)
    out = {"n_pred": int(P), "n_gt": int(G), "mean_iou": float(vi.mean()) if len(vi) else 0.0,
           "matches": [(int(p), int(g), float(v)) for p, g, v in zip(pi, gi, vi)], "at": {}}
    for t in thresholds:
        tp = int((vi >= t).sum())
        prec, rec = _ratio(tp, P), _ratio(tp, G)
        out["at"][float(t)] = {"tp": tp, "precision": prec, "recall": rec,
                               "f1": _ratio(2.0 * prec * rec, prec + rec)}
    return out


def score(pred_corners, gt_corners, thresholds=(0.25, 0.5)):
    """class-agnostic detection scores of predicted boxes [P,8,3] against ground truth [G,8,3] (the
    run's result file carries class 0 and score 1.0 for every box): a dict with n_pred, n_gt,
    mean_iou (over the matched pairs), matches [(pred, gt, iou)] and, under "at", per IoU threshold
    tp, precision, recall and f1; 0/0 is reported as 0.0"""
    pred, gt = _host(pred_corners), _host(gt_corners)
    if len(pred) == 0 or len(gt) == 0:
        iou = np.zeros((len(pred), len(gt)))
    else:
        iou = iou_matrix(pred, gt)
    return score_from_iou(iou, thresholds)


# ---- files -------------------------------------------------------------------------------------------
def load_boxes_pkl(path):
    """the corners f64 [n,8,3] of `<seq>_boxes.pkl` (results.global_save_list: [[(class, corners
    [8,3], score), ...]])"""
    from boxfusion_amd.results import load_global_boxes
    return load_global_boxes(path)


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def read_ply_points(path):
    """the vertex positions f64 [n,3] of a PLY file, ascii or binary_little_endian, whose vertex
    element has scalar properties with x, y and z as float or double among them (what
    visualize.points_to_ply and the usual mesh exporters write); other properties are skipped"""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.find(b"end_header")
    if not data.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    nl = data.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in data[:end].decode("ascii").splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append((w[1], int(w[2]), []))
        elif w[0] == "property" and elements:
            elements[-1][2].append(w[1:])
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported")
    if not elements or elements[0][0] != "vertex":
        raise ValueError(f"{path}: the vertex element must come first")
    _, nv, props = elements[0]
    if any(p[0] == "list" or p[0] not in _PLY_TYPES for p in props):
        raise ValueError(f"{path}: the vertex element has a list or unknown property")
    names = [p[1] for p in props]
    for ax in "xyz":
        if ax not in names or _PLY_TYPES[props[names.index(ax)][0]] not in ("f4", "f8"):
            raise ValueError(f"{path}: vertex property {ax} must be float or double")
    if fmt == "ascii":
        rows = data[nl:].split(b"\n", nv)[:nv]
        if len(rows) < nv:
            raise ValueError(f"{path}: {len(rows)} vertex lines, header says {nv}")
        tab = np.array([r.split() for r in rows], np.float64).reshape(nv, len(names))
        return np.stack([tab[:, names.index(ax)] for ax in "xyz"], 1).reshape(-1, 3)
    dt = np.dtype([(nm, "<" + _PLY_TYPES[p[0]]) for nm, p in zip(names, props)])
    if len(data) - nl < nv * dt.itemsize:
        raise ValueError(f"{path}: truncated vertex data")
    v = np.frombuffer(data, dt, nv, nl)
    return np.stack([v[ax].astype(np.float64) for ax in "xyz"], 1).reshape(-1, 3)


def png_size(path):
    """(H, W) from a PNG file's IHDR chunk"""
    with open(path, "rb") as fh:
        head = fh.read(24)
    if len(head) < 24 or head[:8] != b"\x89PNG\r\n\x1a\n" or head[12:16] != b"IHDR":
        raise ValueError(f"{path}: not a PNG file")
    w, h = struct.unpack(">II", head[16:24])
    return int(h), int(w)


def load_sequence(seq_dir):
    """a CA-1M sequence directory as filter_gt_boxes.py:120-138 reads it: (corners [N,8,3] of
    instances.json, K [3,3] of K_depth.txt, poses [M,4,4] of all_poses.npy, (H, W) of depth/0.png)"""
    with open(os.path.join(seq_dir, "instances.json")) as fh:
        items = json.load(fh)
    corners = (np.stack([np.array(it["corners"], np.float64) for it in items]) if items
               else np.zeros((0, 8, 3)))
    K = np.loadtxt(os.path.join(seq_dir, "K_depth.txt")).reshape(3, 3)
    poses = np.load(os.path.join(seq_dir, "all_poses.npy"))
    return corners, K, poses, png_size(os.path.join(seq_dir, "depth", "0.png"))


# ---- command line -------------------------------------------------------------------------------------
def _parser():
    ap = argparse.ArgumentParser(prog="python -m boxfusion_amd.evaluation", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("filter", help="instances.json -> after_filter_boxes.npy (filter_gt_boxes.py)")
    f.add_argument("seq_dir")
    f.add_argument("--points", help="scene points as a PLY file (default: SEQ_DIR/mesh.ply)")
    f.add_argument("--dist", type=float, default=0.1, help="proximity threshold in metres (the reference's call: 0.1)")
    f.add_argument("--near", type=float, default=0.1)
    f.add_argument("--far", type=float, default=100.0)
    s = sub.add_parser("score", help="score <seq>_boxes.pkl against after_filter_boxes.npy")
    s.add_argument("boxes")
    s.add_argument("gt")
    s.add_argument("--iou", type=float, nargs="+", default=[0.25, 0.5])
    s.add_argument("--json", help="also write the result as JSON")
    return ap


def main(argv=None):
    ap = _parser()
    args = ap.parse_args(argv)
    if args.cmd == "filter":
        if not os.path.isdir(args.seq_dir):
            ap.error(f"{args.seq_dir} is not a directory")
        points = args.points or os.path.join(args.seq_dir, "mesh.ply")
        for need in (points, *(os.path.join(args.seq_dir, n) for n in
                               ("instances.json", "K_depth.txt", "all_poses.npy", os.path.join("depth", "0.png")))):
            if not os.path.isfile(need):
                ap.error(f"{need} is missing")
        if not args.dist > 0 or not args.far > args.near:
            ap.error("--dist must be positive and --far above --near")
        corners, K, poses, hw = load_sequence(args.seq_dir)
        print("before frustum culling", corners.shape)
        kept, frustum_mask = filter_gt_boxes(corners, K, poses, hw, read_ply_points(points), near=args.near,
                                             far=args.far, dist_threshold=args.dist)
        print("after frustum culling", (int(frustum_mask.sum()), 8, 3))
        print("after_filter", kept.shape)
        out = os.path.join(args.seq_dir, "after_filter_boxes.npy")
        np.save(out, kept)
        print(f"wrote {out}")
        return 0
    for need in (args.boxes, args.gt):
        if not os.path.isfile(need):
            ap.error(f"{need} is missing")
    if any(not 0.0 < t <= 1.0 for t in args.iou):
        ap.error("--iou thresholds must lie in (0, 1]")
    res = score(load_boxes_pkl(args.boxes), np.load(args.gt), thresholds=tuple(args.iou))
    print(f"pred {res['n_pred']}  gt {res['n_gt']}  matched {len(res['matches'])}  mean IoU {res['mean_iou']:.4f}")
    for t, r in res["at"].items():
        print(f"IoU >= {t:g}: tp {r['tp']}  precision {r['precision']:.4f}  recall {r['recall']:.4f}  f1 {r['f1']:.4f}")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
