"""Seeded inputs for the association kernels (bf_assoc.hip) and the analysis that says which paths
a case reaches.  Importable without a GPU: tests/test_assoc_cases_host.py runs every case through
the oracle alone and asserts the paths, tests/test_gpu_assoc.py and tests/test_gpu_fusion.py run
the same cases on the device."""
from __future__ import annotations

import copy

import numpy as np

from boxfusion_amd.synthetic import SCANNET_K, Scene, look_at_pose
from oracle import oracle as OR
from tests import trace_util as TU

W, H = 640, 480
CUR_POSE = look_at_pose([0.0, -3.0, 1.2], [0.0, 0.0, 0.8])
POISON = 0          # tail value of the chained mask buffer: a valid global index if it were read


def corr_cfg(cap=64, max_list=5, cfg=TU.SCANNET_CFG):
    c = OR.CorrCfg()
    c.small_size = cfg["box_fusion"]["small_size"]
    c.threshold = cfg["association"]["small_threshold"]
    c.translation_gap = cfg["association"]["translation_gap"]
    c.rotation_gap = cfg["association"]["rotation_gap"]
    c.W, c.H = float(W), float(H)
    c.max_list = max_list
    c.list_capacity = cap
    return c


def nms_cfg(cap=64, cfg=TU.SCANNET_CFG):
    c = OR.NmsCfg()
    c.iou_threshold = cfg["box_fusion"]["nms_threshold"]
    c.translation_gap = cfg["association"]["translation_gap"]
    c.rotation_gap = cfg["association"]["rotation_gap"]
    c.center_gap = 0.5
    c.max_list = 5
    c.list_capacity = cap
    return c


def as_cfg(cls, src):
    """a config structure as another class with the same fields (the oracle's <-> the library's)"""
    c = cls()
    for name, _ in cls._fields_:
        setattr(c, name, getattr(src, name))
    return c


def to_dev(a, dtype=None):
    """host array -> contiguous tensor on the HIP device (f32 unless a dtype is given)"""
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", torch.float32 if dtype is None else dtype)


def _yaw_R(yaw):
    return np.stack([[[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
                     for a in yaw]).astype(np.float32).reshape(-1, 3, 3)


def _world(u, v, z):
    """world point of pixel (u, v) at depth z of the CUR_POSE camera"""
    K = SCANNET_K.astype(np.float64)
    cam = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z, np.ones_like(z)], -1)
    return (cam @ CUR_POSE.astype(np.float64).T)[:, :3]


def _in_view(rng, n, margin=-40.0):
    """n centres uniform over the image (margin < 0: a border outside it) at 1 .. 5.5 m"""
    return _world(rng.uniform(margin, W - margin, n), rng.uniform(margin, H - margin, n),
                  rng.uniform(1.0, 5.5, n))


# Pairs that make one edge of project_2d_box decide the answer.  right / bottom / left / top: the
# global box hangs over that image edge with only a sliver (1.2 .. 1.6 px) inside, and the new
# box's 2-D box overlaps just the last 0.8 px before the edge, so a clamp off by one pixel leaves
# no overlap and no event.  far_out: every corner between 8 and 9 m, the projection is all zero
# and the new box (its 2-D box the projection without the 8 m test) must find no match.  far_in:
# every corner between 7 and 8 m, an ordinary match.  behind: a long box through the camera
# plane; the corners behind it are left out of the extent, and the new box's 2-D box covers 0.81
# of that extent, which is under the threshold against the extent of all eight corners.  wide /
# tall: a close box whose corners all fall outside the image, left and right (above and below)
# of it, so no corner is valid and the projection is all zero; the new box's 2-D box is the
# clamped extent a projection without that test would give.
EDGE_KINDS = ("right", "bottom", "left", "top", "far_out", "far_in", "behind", "wide", "tall")
EDGE_NO_MATCH = ("far_out", "wide", "tall")
_EDGE_EXT, _EDGE_YAW = np.array([0.2, 0.2, 0.2]), 0.3
_EDGES = {}


def _project(xyz, ext, yaw):
    """(oracle projection, camera-frame z of the corners, pinhole extent of all corners unclamped)
    of one box, through the same f32 roundings corr_case applies"""
    b = np.concatenate([xyz, ext])[None].astype(np.float32)
    c = OR.box_corners(b, _yaw_R([yaw])).reshape(8, 3).astype(np.float64)
    cam = (np.c_[c, np.ones(8)] @ np.linalg.inv(CUR_POSE.astype(np.float64)).T)[:, :3]
    K = SCANNET_K.astype(np.float64)
    u = K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2]
    v = K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]
    return (OR.project_2d_box(c[None], CUR_POSE, SCANNET_K, W, H)[0], cam[:, 2],
            np.array([u.min(), v.min(), u.max(), v.max()]))


def clamp_box(full):
    """an unclamped pinhole extent clamped to the image"""
    return np.array([min(max(full[0], 0), W), min(max(full[1], 0), H),
                     min(max(full[2], 0), W), min(max(full[3], 0), H)], np.float64)


def edge_box(kind):
    """(centre, extents, yaw, the new box's 2-D box) of the pair for one EDGE_KINDS entry"""
    if kind in _EDGES:
        return _EDGES[kind]
    one = lambda u, v, z: _world(np.array([u]), np.array([v]), np.array([z]))[0]
    found = None
    if kind in ("right", "bottom", "left", "top"):
        ax, hi = (0, kind == "right") if kind in ("right", "left") else (1, kind == "bottom")
        lim = (W, H)[ax]
        for c in np.arange(0.0, 80.0, 0.05):
            p = [W / 2.0, H / 2.0]
            p[ax] = lim + c if hi else -c
            xyz = one(p[0], p[1], 3.0)
            b, _, _ = _project(xyz, _EDGE_EXT, _EDGE_YAW)
            inside = (lim - b[ax]) if hi else b[ax + 2]
            if b[ax + 2 if hi else ax] == (lim if hi else 0) and 1.2 <= inside <= 1.6:
                box2d = b.copy()
                box2d[ax], box2d[ax + 2] = (lim - 0.8, lim + 0.4) if hi else (-0.4, 0.8)
                found = (xyz, _EDGE_EXT, _EDGE_YAW, box2d.astype(np.float32))
                break
    elif kind in ("far_out", "far_in"):
        xyz = one(W / 4.0, H / 4.0, 8.5) if kind == "far_out" else one(0.75 * W, 0.75 * H, 7.5)
        b, z, full = _project(xyz, _EDGE_EXT, _EDGE_YAW)
        lo, hi = (8.0, 9.0) if kind == "far_out" else (7.0, 8.0)
        if (z > lo).all() and (z < hi).all() and (b == 0).all() == (kind == "far_out"):
            found = (xyz, _EDGE_EXT, _EDGE_YAW, (full if kind == "far_out" else b).astype(np.float32))
    elif kind == "behind":
        xyz, ext = one(W / 2.0, H / 2.0, 0.19), np.array([0.05, 0.44, 0.05])
        b, z, full = _project(xyz, ext, 0.0)
        w, h = b[2] - b[0], b[3] - b[1]
        box2d = np.array([b[0] + w / 20, b[1] + h / 20, b[2] - w / 20, b[3] - h / 20], np.float32)
        thr = corr_cfg().threshold
        if ((z < 0).any() and (z > 0).any() and w > 0 and h > 0 and
                iou_2d(box2d, b[None])[0] > thr > iou_2d(box2d, clamp_box(full)[None])[0]):
            found = (xyz, ext, 0.0, box2d)
    else:
        xyz = one(W / 2.0, H / 2.0, 0.15)
        ext = np.array([0.44, 0.05, 0.05]) if kind == "wide" else np.array([0.05, 0.05, 0.44])
        b, z, full = _project(xyz, ext, 0.0)
        alt = clamp_box(full)
        if (z > 0).all() and (b == 0).all() and (alt[2] - alt[0]) * (alt[3] - alt[1]) > 0:
            found = (xyz, ext, 0.0, alt.astype(np.float32))
    if found is None:
        raise AssertionError(f"no box for edge {kind}")
    _EDGES[kind] = found
    return found


def wants_edges(ng, n_new, all_large=False, all_success=False, empty_mask=False, **_):
    """whether corr_case gives a case the EDGE_KINDS pairs: ng kept global boxes (positions 10 ..
    below the pinned last one), n_new new boxes (0 and 1 are the pinned ones; the pairs' new boxes
    are always kept), and every new box is not skipped anyway"""
    return ng >= 20 and n_new >= 2 + len(EDGE_KINDS) and not (all_large or all_success or empty_mask)


def corr_case(n_glo, n_new, seed, *, cap=64, max_list=5, list_len=5, keep_all_globals=False,
              keep_globals=True, empty_mask=False, all_large=False, all_success=False, tie=None):
    """Inputs of one correspondence-association call: n_glo global boxes seen from CUR_POSE and
    n_new detections, most of them near copies of a global box.

    list_len          longest fusion list a global box starts with (at most cap)
    keep_all_globals  the mask keeps every global box (ng == n_glo)
    keep_globals      False: the mask keeps no global box (ng == 0)
    empty_mask        the mask is empty
    all_large         every new box is larger than small_size (all skipped)
    all_success       every kept new box is in `success` (all skipped)
    tie               (distance d, lower_first): the global box matched by new box 0 sits at kept
                      position p and an exact duplicate (corners, dims) at p + d, so the argmax
                      meets two equal maxima; the new box's score lies between the two copies',
                      the lower-scored copy first or second

    New box 0 is pinned: it copies a clean, small, in-view global box (the last kept one, or the
    one at tie position p), both are kept and the new box is not in `success`.  With more than
    257 kept global boxes new box 1 is pinned in the same way to kept position 256 (in a tie
    case to the last one), so a maximum lies in the second trip of a lane's loop.  With at least
    20 kept global boxes and 11 new ones, new boxes 2 .. 10 are the EDGE_KINDS pairs (case["edges"]
    = (kind, new box, global box))."""
    rng = np.random.default_rng(seed)
    n = n_glo + n_new
    # --- global boxes
    xyz = _in_view(rng, n_glo)
    ext = rng.uniform(0.05, 0.28, (n_glo, 3))
    ext[rng.random(n_glo) < 0.2] *= 3.0                         # not small
    kind = rng.random(n_glo)
    far = kind < 0.1                                             # straddling the 8 m test
    behind = (kind >= 0.1) & (kind < 0.2)                        # at or behind the camera plane
    xyz[far] = _world(rng.uniform(0, W, far.sum()), rng.uniform(0, H, far.sum()),
                      rng.uniform(6.0, 9.0, far.sum()))
    xyz[behind] = _world(rng.uniform(0, W, behind.sum()), rng.uniform(0, H, behind.sum()),
                         rng.uniform(-1.0, 0.1, behind.sum()))
    yaw = rng.uniform(-np.pi, np.pi, n_glo)
    # --- mask over the global boxes, then the pinned pairs (new box k <-> kept position pos)
    gkeep = np.ones(n_glo, bool) if keep_all_globals else rng.random(n_glo) < 0.9
    if not keep_globals:
        gkeep[:] = False
    gk = np.flatnonzero(gkeep)
    pins = []
    if len(gk) and n_new:
        pins.append((0, 7 if tie else len(gk) - 1))
        if len(gk) > 257 and n_new > 1:
            pins.append((1, len(gk) - 1 if tie else 256))
    for _, pos in pins:
        g = gk[pos]
        xyz[g] = _in_view(rng, 1, margin=80.0)
        ext[g] = rng.uniform(0.15, 0.28, 3)
    # the projection's edges, each decided by one pair: new boxes 2.. <-> kept positions 10..
    edges = []
    if wants_edges(len(gk), n_new, all_large, all_success, empty_mask):
        edges = [(2 + e, 10 + e, kind) for e, kind in enumerate(EDGE_KINDS)]
    for _, pos, kind in edges:
        g = gk[pos]
        xyz[g], ext[g], yaw[g] = edge_box(kind)[:3]
    # --- new boxes: near copies of global ones (several share one), or fresh boxes without any
    if n_glo:
        pool = rng.choice(n_glo, max(1, min(n_glo, n_new // 2)), replace=False)
        src = pool[rng.integers(0, len(pool), n_new)]
        for k, pos in pins:
            src[k] = gk[pos]
        nxyz = xyz[src] + rng.normal(0, 0.01, (n_new, 3))
        next_ = ext[src] * rng.uniform(0.9, 1.1, (n_new, 3))
        nyaw = yaw[src]
        for k, pos, _ in edges:                                  # copies, small enough to be visited
            g = gk[pos]
            nxyz[k], next_[k], nyaw[k] = xyz[g], np.minimum(ext[g], 0.3), yaw[g]
    else:
        nxyz, next_ = _in_view(rng, n_new), rng.uniform(0.05, 0.28, (n_new, 3))
        nyaw = rng.uniform(-np.pi, np.pi, n_new)
    if all_large:
        next_ = rng.uniform(0.4, 0.8, (n_new, 3))
    b = np.concatenate([np.concatenate([xyz, nxyz]), np.concatenate([ext, next_])], 1).astype(np.float32)
    R = _yaw_R(np.concatenate([yaw, nyaw]))
    scores = rng.permutation(np.linspace(0.3, 0.99, n)).astype(np.float32)
    if tie:
        d, lower_first = tie
        a, c = gk[7], gk[7 + d]
        b[c], R[c] = b[a], R[a]
        lo, mid, hi = np.sort(scores[[a, c, n_glo]])
        scores[n_glo] = mid
        scores[a], scores[c] = (lo, hi) if lower_first else (hi, lo)
    corners = OR.box_corners(b, R).reshape(n, 8, 3)
    dims = np.ascontiguousarray(b[:, 3:6])
    boxes2d = np.zeros((n, 4), np.float32)
    if n_new:
        boxes2d[n_glo:] = (OR.project_2d_box(corners[n_glo:], CUR_POSE, SCANNET_K, W, H) +
                           rng.normal(0, 1.5, (n_new, 4))).astype(np.float32)
    for k, _, kind in edges:
        boxes2d[n_glo + k] = edge_box(kind)[3]
    scene = Scene(seed=3)
    frames = 80 * rng.integers(0, 12, n) + rng.integers(0, 2, n)
    cam_poses = np.stack([scene.pose(int(f)) for f in frames]).astype(np.float32).reshape(n, 4, 4)
    # --- fusion lists: earlier merges on the global boxes, the new ones their own id
    max_len = min(list_len, cap)
    fusion_list = [sorted(set([i] + rng.integers(0, n_glo, rng.integers(0, max_len)).tolist()))
                   for i in range(n_glo)] + [[i] for i in range(n_glo, n)]
    nkeep = rng.random(n_new) < 0.9
    for k in [k for k, _ in pins] + [k for k, _, _ in edges]:
        nkeep[k] = True
    mask = np.concatenate([gk, n_glo + np.flatnonzero(nkeep)]).astype(np.int32)
    if empty_mask:
        mask = mask[:0]
    kept_new = mask[mask >= n_glo]
    if all_success:
        success = kept_new.copy()
    else:
        pinned = [n_glo + k for k, _ in pins] + [n_glo + k for k, _, _ in edges]
        cand = np.array([m for m in kept_new if m not in pinned], np.int32)
        success = np.concatenate([cand[rng.random(len(cand)) < 0.125],
                                  rng.choice(gk, min(3, len(gk)), replace=False)
                                  if len(gk) and len(mask) else np.zeros(0, np.int32)])
    success = np.sort(success).astype(np.int32)
    valid_num = rng.integers(0, 3, n).astype(np.float32)
    return dict(corners=corners, dims=dims, scores=scores, boxes2d=boxes2d,
                init_id=np.arange(n, dtype=np.int32), cam_poses=cam_poses, cur_pose=CUR_POSE,
                K=SCANNET_K, n_glo=n_glo, mask=mask, success=success, fusion_list=fusion_list,
                valid_num=valid_num, cap=cap, max_list=max_list, tie=tie,
                pins=[(n_glo + k, pos) for k, pos in pins],
                edges=[(kind, n_glo + k, int(gk[pos])) for k, pos, kind in edges])


def corr_oracle(case):
    c = case
    return OR.corr_assoc(c["corners"], c["dims"], c["scores"], c["boxes2d"], c["init_id"],
                         c["cam_poses"], c["cur_pose"], c["K"], c["n_glo"], c["mask"], c["success"],
                         c["fusion_list"], c["valid_num"], corr_cfg(c["cap"], c["max_list"]))


def iou_2d(a32, b):
    """IoU_2D_box in f64 (the oracle's expression order) of one f32 box against f64 boxes [g, 4]"""
    a = np.asarray(a32, np.float32).astype(np.float64)
    area_a = (a[2] - a[0]) * (a[3] - a[1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = np.maximum(np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]), 0.0)
    ih = np.maximum(np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]), 0.0)
    inter = iw * ih
    return inter / ((area_a + area_b - inter) + 1e-6)


def corr_paths(case, ref):
    """What a case reaches, from its inputs and the oracle's result `ref`: the argmax of every
    visited new box restated in numpy (it depends on no state of the scan), and the branches,
    list growth and keep edits read off the oracle's events and lists."""
    c, cfg = case, corr_cfg(case["cap"], case["max_list"])
    n_glo, mask = c["n_glo"], c["mask"]
    gk = mask[mask < n_glo]
    ng = len(gk)
    b2d = (OR.project_2d_box(c["corners"][gk], c["cur_pose"], c["K"], W, H) if ng
           else np.zeros((0, 4)))
    small_lim = np.float32(cfg.small_size + 0.1)
    gsmall = (c["dims"][gk].max(1) < small_lim).astype(np.float64) if ng else np.zeros(0)
    zero = (b2d == 0).all(1)
    clamped = ~zero & ((b2d[:, [0, 2]] == 0) | (b2d[:, [0, 2]] == W) | (b2d[:, [1, 3]] == 0) |
                       (b2d[:, [1, 3]] == H)).any(1)
    visited, winners, pairs, ious = [], [], [], {}
    for m in mask[mask >= n_glo]:
        if c["dims"][m].max() > cfg.small_size or m in c["success"] or ng == 0:
            continue
        visited.append(int(m))
        v = iou_2d(c["boxes2d"][m], b2d) * gsmall
        ious[int(m)] = v
        best = int(np.argmax(v))                                # first maximum
        if v[best] > cfg.threshold:
            corr = int(gk[best])
            winners.append(best)
            pairs.append((int(m), corr) if c["scores"][corr] < c["scores"][m] else (corr, int(m)))
    ev = ref["events"]
    b2 = ev[ev[:, 2] == 2] if len(ev) else ev
    grown = sum(len(ref["fusion_list"][cur]) > len(c["fusion_list"][cur]) for cur in set(ev[:, 0].tolist()))
    # branch 2 has a new box as cur, visited once: its list grew, or keep was edited instead
    b2_grew = sum(len(ref["fusion_list"][cur]) > 1 for cur in b2[:, 0])
    return dict(ng=ng, visited=visited, winners=winners, pairs=pairs, ious=ious, gk=gk,
                events=len(ev), branch1=int((ev[:, 2] == 1).sum()) if len(ev) else 0,
                branch2=len(b2), lists_grown=grown, b2_grew=b2_grew, b2_replaced=len(b2) - b2_grew,
                cur_new=int((ev[:, 0] >= n_glo).sum()) if len(ev) else 0,
                cur_glo=int((ev[:, 0] < n_glo).sum()) if len(ev) else 0,
                zero_proj=int(zero.sum()), clamped=int(clamped.sum()),
                best_pos=max(winners) if winners else -1)


# name -> (corr_case arguments, what the case must reach: see tests/test_assoc_cases_host.py)
_BIG = dict(events=8, each_branch=3, grow=1, replace=1, cur_both=True, proj_edges=True)
CORR_CASES = {
    "0x3": ((0, 3, 1), dict(), dict(events=0, ng=0)),
    "1x1": ((1, 1, 2), dict(keep_all_globals=True), dict(events=1, ng=1)),
    "5x0": ((5, 0, 3), dict(), dict(events=0)),
    "40x12": ((40, 12, 4), dict(), dict(events=2)),
    "255x20": ((255, 20, 5), dict(keep_all_globals=True), dict(events=3, ng=255, best_pos=254)),
    "256x20": ((256, 20, 6), dict(keep_all_globals=True), dict(events=3, ng=256, best_pos=255)),
    "257x20": ((257, 20, 7), dict(keep_all_globals=True), dict(events=3, ng=257, best_pos=256)),
    "300x40": ((300, 40, 8), dict(), _BIG),
    "600x60": ((600, 60, 10), dict(), _BIG),
    "70x150": ((70, 150, 10), dict(), _BIG),
    "no_global_kept": ((40, 12, 11), dict(keep_globals=False), dict(events=0, ng=0)),
    "empty_mask": ((40, 12, 12), dict(empty_mask=True), dict(events=0, ng=0, n_mask=0)),
    "all_large": ((40, 12, 13), dict(all_large=True), dict(events=0, visited=0)),
    "all_success": ((40, 12, 14), dict(all_success=True), dict(events=0, visited=0)),
    "cap4": ((70, 150, 15), dict(cap=4), dict(events=8, overflow=True)),
    "cap8": ((70, 150, 16), dict(cap=8, max_list=12, list_len=8), dict(events=8, overflow=True)),
}
for _d in (1, 64, 256):
    for _lf in (True, False):
        CORR_CASES[f"tie{_d}_{'lower_first' if _lf else 'lower_second'}"] = (
            (300, 12, 20 + _d + _lf), dict(keep_all_globals=True, tie=(_d, _lf)), dict(events=1, tie=True))

_CACHE = {}


def corr_named(name):
    """(case, oracle result) of a named case, computed once; neither is to be modified"""
    if name not in _CACHE:
        args, kw, _ = CORR_CASES[name]
        case = corr_case(*args, **kw)
        _CACHE[name] = (case, corr_oracle(case))
    return _CACHE[name]


def over_capacity_case(order, cap=8):
    """The 40x12 case at capacity `cap` with the global box g that pinned new box m matches
    carrying a full row, for a device run that claims a length above the capacity for that row.
    order "cur": g has the higher score and is record_corr's cur (branch 1); "idx": g is its idx
    (branch 2, as a full row is no single view).  Returns (case, oracle result, g, m)."""
    case = copy.deepcopy(corr_named("40x12")[0])
    case["cap"] = cap
    n_glo = case["n_glo"]
    m, pos = case["pins"][0]
    g = int(case["mask"][case["mask"] < n_glo][pos])
    s = case["scores"]
    lo, hi = sorted([float(s[m]), float(s[g])])
    s[g], s[m] = (hi, lo) if order == "cur" else (lo, hi)
    rng = np.random.default_rng(5)
    case["fusion_list"][g] = sorted(rng.choice(n_glo, cap, replace=False).tolist())
    return case, corr_oracle(case), g, m


def nms_case(n_glo, n_new, seed, *, spread=2.5, n_centres=None, scene_seed=1, max_extra=4):
    """Clustered boxes for the greedy scan: n_glo global boxes that carry earlier merges (lists of
    up to max_extra views) plus n_new new ones, around n_centres cluster centres so that
    suppressions, list merges and pose gates all occur."""
    rng = np.random.default_rng(seed)
    n = n_glo + n_new
    centres = rng.uniform(-spread, spread, (n // 3 + 1 if n_centres is None else n_centres, 3))
    xyz = centres[rng.integers(0, len(centres), n)] + rng.normal(0, 0.04, (n, 3))
    lhw = rng.uniform(0.2, 0.9, (n, 3))
    b = np.concatenate([xyz, lhw], 1).astype(np.float32)
    yaw = rng.uniform(-0.2, 0.2, n)
    R = np.stack([[[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
                  for a in yaw]).astype(np.float32)
    corners = OR.box_corners(b, R)
    scores = rng.permutation(np.linspace(0.3, 0.99, n)).astype(np.float32)
    init_id = np.arange(n, dtype=np.int32)
    scene = Scene(seed=scene_seed)
    cam_poses = np.stack([scene.pose(int(f)) for f in rng.integers(0, 1000, n)]).astype(np.float32)
    fusion_list = [sorted(set([i] + rng.integers(0, max(1, n_glo), rng.integers(0, max_extra)).tolist()))
                   if i < n_glo else [i] for i in range(n)]
    valid_num = rng.integers(0, 3, n).astype(np.float32)
    return dict(corners=corners, scores=scores, init_id=init_id, cam_poses=cam_poses,
                fusion_list=fusion_list, valid_num=valid_num)


# the cases of the 256-thread k_nms_scan:
# (n_glo, n_new, list capacity, workspace, the form bf_nms_scan_form must name)
BLOCK_SCANS = [
    (321, 20, 64, True, 3),          # 341: the first size past the bit-mask scan's LDS budget
    (370, 30, 64, True, 3),
    (90, 7, 64, False, 2),           # bf_nms_scan has no workspace: the block scan from 97 on,
    (110, 10, 64, False, 2),         # IoU in LDS up to 120
    (111, 10, 64, False, 3),         # and read from global memory from 121 on
    (90, 6, 512, True, 2),           # lists too large for the one-wave scans' LDS
    (36, 4, 2048, True, 2),
]


def block_scan_case(n_glo, n_new):
    """lists of up to 6 views: record()'s L < max_list gate meets lists below, at and above 5"""
    return nms_case(n_glo, n_new, 7000 + n_glo + n_new, max_extra=6)


def nms_oracle(case, iou, cap):
    c = case
    return OR.nms_scan(iou, c["corners"], c["scores"], c["init_id"], c["cam_poses"], c["fusion_list"],
                       c["valid_num"], nms_cfg(cap))


def nms_paths(case, ref):
    """what a scan reached, from the oracle's result"""
    ev = ref["events"]
    b2 = ev[ev[:, 2] == 2]
    # a suppressed box's list is still its initial one: its length at record()'s max_list gate
    idx_len = np.array([len(case["fusion_list"][i]) for i in b2[:, 1]])
    return dict(success=len(ref["success"]), events=len(ev), branch1=int((ev[:, 2] == 1).sum()),
                branch2=len(b2),
                lists_grown=sum(len(a) > len(b) for a, b in zip(ref["fusion_list"], case["fusion_list"])),
                # a suppressed box in the final keep: record()'s branch-2 keep edit put it there
                keep_replaced=int(np.isin(b2[:, 1], ref["keep"]).sum()),
                gate_below=int((idx_len < 5).sum()), gate_at=int((idx_len == 5).sum()),
                gate_above=int((idx_len > 5).sum()))


def assert_block_scan_paths(p):
    """the paths every BLOCK_SCANS case must reach (floors far under the smallest case's counts)"""
    assert p["success"] >= 4 and p["events"] >= 6 and p["branch1"] >= 1 and p["branch2"] >= 1
    assert p["lists_grown"] >= 1 and p["keep_replaced"] >= 1
    assert p["gate_below"] >= 1 and p["gate_at"] >= 1 and p["gate_above"] >= 1
