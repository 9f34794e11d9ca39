"""Level a tracked scene: find up, the floor and the wall directions.

Tracking from scratch places every frame in the first camera's frame, but the detect path takes a z-up
world for granted (sensor.camera_to_gravity, the yaw-only fusion, the top-down view).  The fused surface
of an indoor scene is mostly a floor and walls, a Manhattan world: the floor's normal is parallel to up,
wall normals are perpendicular to up and cluster four-fold about it, and the floor is the lowest large
level surface.  This module reads those three things off a mesh, or off any oriented samples (point,
unit normal, integer weight), and returns the rigid transform after which z is up, the floor lies at
z = 0 and the walls run along x and y.

The device reduces, the host solves (the division of labour of tracking.IcpTracker): bf_level.hip turns
the samples into integer sums that are the same bits in any order (include/boxfusion_level.h has the
rules), and `procedure` below works out the 3 x 3 problems in f64 from those integers.  The numpy
restatement of the kernels (tests/level_ref.py) runs the same `procedure`, so equal sums give equal
transforms.  DESIGN.md §4 "Levelling" has the rules, the overflow bounds and the measured accuracies.

  estimate(points, normals, weights, prior, ...)   oriented samples -> Levelling
  level_mesh(mesh_or_volume, poses, prior, ...)    a TsdfVolume or (vertices, faces) -> Levelling
  Levelling.apply(poses) / .apply_points(xyz)      into the levelled world

    python -m boxfusion_amd.scene_level MESH.ply OUT.ply [--poses IN.npy --poses-out OUT.npy]
                                        [--json level.json] [--voxel 0.02] [--prior X Y Z]

reads a PLY with faces that this package writes and writes it levelled.
"""
from __future__ import annotations

import dataclasses
import json
import math
import os
import sys

import numpy as np

from boxfusion_amd import _abi

F, D = np.float32, np.float64
_LC = _abi.constants(header=_abi.EXTENSION_HEADERS[1])
MAX_G, MAX_HEIGHT_BINS, NORMAL_SHIFT, METRE_SHIFT = (
    _LC["BF_LEVEL_" + n] for n in ("MAX_G", "MAX_HEIGHT_BINS", "NORMAL_SHIFT", "METRE_SHIFT"))
STATS = _abi.enum_names("BF_LEVEL_STAT_", header=_abi.EXTENSION_HEADERS[1])
FLOOR_FRACTION = 5                  # the floor is the lowest height bin with at least 1/5 of the largest bin's weight


# ---- small geometry -------------------------------------------------------------------------------------
def bin_directions(G):
    """the centre direction of every cube-map bin, f32 [6 G G,3], by the header's rule and in its operation
    order: what bf_level_score computes for a bin"""
    G = int(G)
    face, iv, iu = np.unravel_index(np.arange(6 * G * G), (6, G, G))
    s = np.where(face & 1, F(-1.0), F(1.0)).astype(F)
    u = (2 * iu + 1 - G).astype(F) / F(G)
    v = (2 * iv + 1 - G).astype(F) / F(G)
    ln = np.sqrt((u * u + v * v) + F(1.0))
    dk, dp, dq = s / ln, (u * s) / ln, (v * s) / ln
    k = face >> 1
    out = np.stack([np.where(k == 0, dk, dp), np.where(k == 0, dp, np.where(k == 1, dk, dq)), np.where(k == 2, dk, dq)], -1)
    assert out.dtype == F
    return out


def _unit(v, what):
    v = np.asarray(v, D).reshape(3)
    n = float(np.linalg.norm(v))
    if not (np.isfinite(v).all() and n > 0):
        raise ValueError(f"{what}: a finite direction that is not zero")
    return v / n


def finite_poses(poses):
    """[k,4,4] f64 of the poses without a non-finite entry (a lost frame is -inf)"""
    if poses is None:
        return np.zeros((0, 4, 4))
    P = np.asarray(poses, D).reshape(-1, 4, 4)
    return P[np.isfinite(P).all((1, 2))]


def prior_from_poses(poses):
    """the normalised sum of the cameras' image-up axes (-pose[:3,1]) over the finite poses, or None when
    there is none or they cancel"""
    P = finite_poses(poses)
    s = -P[:, :3, 1].sum(0) if len(P) else np.zeros(3)
    n = float(np.linalg.norm(s))
    return s / n if n > 1e-9 else None


def horizontal_basis(c):
    """e1, e2 with (e1, e2, c) right-handed and orthonormal: e1 is the world axis least aligned with c (the
    lowest on ties) with its part along c removed"""
    c = np.asarray(c, D)
    a = np.zeros(3)
    a[int(np.argmin(np.abs(c)))] = 1.0
    e1 = a - (a @ c) * c
    e1 /= np.linalg.norm(e1)
    return e1, np.cross(c, e1)


def _sym(w):
    xx, xy, xz, yy, yz, zz = (float(int(v)) for v in w)
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def solve_axis(sums, previous):
    """the top eigenvector of S_par - S_perp from bf_level_refine's integer sums, in f64, its sign towards
    the previous axis; None when the sums are all zero"""
    A = _sym(sums[0:6]) - _sym(sums[6:12])
    if not A.any():
        return None
    _, vec = np.linalg.eigh(A)
    v = vec[:, -1]
    v = v / np.linalg.norm(v)
    return -v if v @ np.asarray(previous, D) < 0 else v


# ---- the result -----------------------------------------------------------------------------------------
@dataclasses.dataclass
class Levelling:
    """What estimate and level_mesh return.  T: f64 [4,4], the old world -> the levelled world (z up, the
    floor at z = 0, walls along x and y); up: the unit up direction in the old world; axis: the wall
    direction that becomes +x; floor: the floor's height along up in the old world; share: the part of the
    surface weight that is parallel or perpendicular to up within tau / 2; yaw_resultant: the length of the
    mean four-fold wall direction, 0 .. 1; floor_share: the part of the upward-facing weight in the floor's
    three bins; angle_deg: the angle between the old z axis and up; in_cone: up lies within cone_deg of the
    prior; ok: share >= min_share, a floor was found and in_cone.  stats: the kernels' counters of the last
    pass by name; trace: the integer sums of every step (for tests)."""
    T: np.ndarray
    up: np.ndarray
    axis: np.ndarray
    floor: float
    share: float
    yaw_resultant: float
    floor_share: float
    angle_deg: float
    in_cone: bool
    ok: bool
    stats: dict = dataclasses.field(default_factory=dict)
    trace: dict = dataclasses.field(default_factory=dict, repr=False)

    def apply(self, poses):
        """T @ pose for every finite camera-to-world pose of [N,4,4] (or [4,4]), f32; a pose with a
        non-finite entry (a lost frame, -inf) is left as it is"""
        P = np.asarray(poses, F)
        out = P.reshape(-1, 4, 4).copy()
        fin = np.isfinite(out).all((1, 2))
        out[fin] = (self.T[None] @ out[fin].astype(D)).astype(F)
        return out.reshape(P.shape)

    def apply_points(self, xyz):
        """points [...,3] (clouds, vertices, box corners; an array or a tensor) into the levelled world, in
        the input's kind and f32"""
        R, t = self.T[:3, :3], self.T[:3, 3]
        if hasattr(xyz, "is_cuda"):
            import torch
            Rt = torch.as_tensor(R.T.astype(F), device=xyz.device)
            return xyz.to(torch.float32) @ Rt + torch.as_tensor(t.astype(F), device=xyz.device)
        return (np.asarray(xyz, D) @ R.T + t).astype(F)

    def summary(self):
        return (f"levelled: moved {self.angle_deg:.2f} deg, share {self.share:.3f}, floor {self.floor:.3f} m, "
                f"ok {self.ok}")

    def to_json(self):
        return dict(T=[[float(v) for v in r] for r in self.T], up=[float(v) for v in self.up],
                    axis=[float(v) for v in self.axis], floor=float(self.floor), share=float(self.share),
                    yaw_resultant=float(self.yaw_resultant), floor_share=float(self.floor_share),
                    angle_deg=float(self.angle_deg), in_cone=bool(self.in_cone), ok=bool(self.ok),
                    stats={k: int(v) for k, v in self.stats.items()})


def _failed(trace, stats=None):
    return Levelling(T=np.eye(4), up=np.array([0.0, 0.0, 1.0]), axis=np.array([1.0, 0.0, 0.0]), floor=float("nan"),
                     share=0.0, yaw_resultant=0.0, floor_share=0.0, angle_deg=0.0, in_cone=False, ok=False,
                     stats=stats or {}, trace=trace)


# ---- the procedure, shared by the device and its restatement -----------------------------------------------
def procedure(be, prior, first_pose=None, *, G=32, tau_deg=10.0, cone_deg=40.0, iters=3, height_bin, min_share=0.5):
    """The host side of levelling over a backend `be` that holds the samples and offers vote(G) -> (hist,
    stats), score(hist, G, candidates, cos_par, sin_perp) -> [k,2], refine(frame, cos_par, sin_perp, h0,
    height_bin, n_bins) -> (sums, heights, stats) and bounds() -> (lo, hi) or None, all as numpy integers
    and f32: the device (DeviceSamples) or tests/level_ref.py."""
    G, iters = int(G), int(iters)
    if not 0 < float(cone_deg) < 45:
        raise ValueError("cone_deg must lie in (0, 45): two Manhattan axes are 90 degrees apart, so a cone below 45 "
                         "holds at most one of them")
    if not 0 < float(tau_deg) < 45 or iters < 1 or not 1 <= G <= MAX_G:
        raise ValueError(f"tau_deg in (0, 45), iters >= 1 and G in 1..{MAX_G}")
    if not (math.isfinite(float(height_bin)) and float(height_bin) > 0):
        raise ValueError("height_bin must be positive")
    prior = _unit(prior, "prior")
    cos_cone = math.cos(math.radians(float(cone_deg)))
    tau = math.radians(float(tau_deg))
    trace = dict(passes=[])
    # candidates: the bins whose centre lies within the cone of the prior
    dirs = bin_directions(G).astype(D)
    cand = np.nonzero(dirs @ prior >= cos_cone)[0].astype(np.int32)
    hist, vstats = be.vote(G)
    scores = be.score(hist, G, cand, F(math.cos(tau)), F(math.sin(tau)))
    trace.update(hist=hist, candidates=cand, scores=scores, vote_stats=vstats)
    total = scores.sum(1) if len(cand) else np.zeros(0, np.int64)
    if not len(cand) or int(total.max()) == 0:
        return _failed(trace)
    c = dirs[cand[int(np.argmax(total))]]                      # the largest par + perp, the lower bin on ties
    c = c / np.linalg.norm(c)
    for it in range(iters):
        t = tau if it < iters - 1 else tau / 2
        e1, e2 = horizontal_basis(c)
        frame = np.concatenate([c, e1, e2]).astype(F)
        sums, _, st = be.refine(frame, F(math.cos(t)), F(math.sin(t)), F(0.0), F(1.0), 0)
        trace["passes"].append(dict(frame=frame, sums=sums, stats=st))
        new = solve_axis(sums, c)
        if new is None:
            break
        c = new
    # the read-out pass for the final axis: share, yaw and the heights of the upward samples
    e1, e2 = horizontal_basis(c)
    frame = np.concatenate([c, e1, e2]).astype(F)
    bounds = be.bounds()
    if bounds is None:
        return _failed(trace)
    lo, hi = (np.asarray(b, D) for b in bounds)
    hb = float(F(height_bin))
    mid, reach = float((lo + hi) / 2 @ c), float(np.linalg.norm(hi - lo)) / 2
    n_bins = int(math.ceil(2 * reach / hb)) + 3
    if n_bins > MAX_HEIGHT_BINS:
        raise ValueError(f"the samples span {2 * reach:.3g} m: more than {MAX_HEIGHT_BINS} height bins of {hb:.3g} m; "
                         "pass a larger height_bin")
    h0 = F((math.floor((mid - reach) / hb) - 1) * hb)
    sums, heights, st = be.refine(frame, F(math.cos(tau / 2)), F(math.sin(tau / 2)), h0, F(hb), n_bins)
    stats = dict(zip(STATS, (int(v) for v in st)))
    trace["passes"].append(dict(frame=frame, sums=sums, heights=heights, stats=st, h0=h0, n_bins=n_bins))
    w_all, w_par, w_perp, w_up = (stats["refine_weight" + k] for k in ("", "_par", "_perp", "_up"))
    share = (w_par + w_perp) / w_all if w_all else 0.0
    # yaw: the mean of the wall normals' directions four-fold about up
    C, S = int(sums[12]), int(sums[13])
    theta = math.atan2(S, C) / 4 if (C or S) else 0.0
    resultant = math.hypot(C, S) / (float(1 << NORMAL_SHIFT) * w_perp) if w_perp else 0.0
    wall = math.cos(theta) * e1 + math.sin(theta) * e2
    first = finite_poses(first_pose)
    if len(first):                                                # of the four, the nearest to the viewing axis
        view = first[0][:3, 2] - (first[0][:3, 2] @ c) * c
        if np.linalg.norm(view) > 1e-9:
            four = [wall, np.cross(c, wall), -wall, -np.cross(c, wall)]
            wall = four[int(np.argmax([f @ view for f in four]))]
    # floor: the lowest height bin with a fifth of the largest one's weight, refined over it and its neighbours
    W = np.asarray(heights[:, 0], np.int64) if n_bins else np.zeros(0, np.int64)
    found = bool(len(W)) and int(W.max()) > 0
    floor, floor_share, ox, oy = float("nan"), 0.0, 0.0, 0.0
    if found:
        b = int(np.nonzero(FLOOR_FRACTION * W >= W.max())[0][0])
        rows = heights[max(b - 1, 0):min(b + 1, n_bins - 1) + 1]
        ws = int(rows[:, 0].sum())
        unit = float(1 << METRE_SHIFT) * ws
        floor = float(h0) + int(rows[:, 1].sum()) / unit
        floor_share = ws / w_up if w_up else 0.0
        ox, oy = int(rows[:, 2].sum()) / unit, int(rows[:, 3].sum()) / unit
        if len(first):                                            # the first camera's centre dropped onto the floor
            ox, oy = float(first[0][:3, 3] @ e1), float(first[0][:3, 3] @ e2)
    R = np.stack([wall, np.cross(c, wall), c])
    T = np.eye(4)
    T[:3, :3] = R
    if found:
        T[:3, 3] = -R @ (ox * e1 + oy * e2 + floor * c)
    in_cone = bool(c @ prior >= cos_cone)
    return Levelling(T=T, up=c, axis=wall, floor=floor, share=float(share), yaw_resultant=float(resultant),
                     floor_share=float(floor_share), angle_deg=float(np.degrees(np.arccos(np.clip(c[2], -1.0, 1.0)))),
                     in_cone=in_cone, ok=bool(share >= float(min_share) and found and in_cone), stats=stats, trace=trace)


# ---- the device ---------------------------------------------------------------------------------------------
class DeviceSamples:
    """the samples on the device and the four kernels over them, returning numpy integers"""

    def __init__(self, device=None):
        self.device, self.p, self.n, self.w, self.face_stats = device, None, None, None, None

    def _tensor(self, a, dtype):
        import torch
        if torch.is_tensor(a):
            if self.device is None:
                self.device = a.device if a.is_cuda else torch.device("cuda")
            return a.to(device=self.device, dtype=dtype).contiguous()
        if self.device is None:
            self.device = torch.device("cuda")
        if dtype == torch.int32 and np.asarray(a).dtype == np.uint32:
            a = np.ascontiguousarray(a).view(np.int32)
        return torch.from_numpy(np.ascontiguousarray(a)).to(device=self.device, dtype=dtype).contiguous()

    def load(self, points, normals, weights):
        import torch
        self.p, self.n = self._tensor(points, torch.float32).reshape(-1, 3), self._tensor(normals, torch.float32).reshape(-1, 3)
        self.w = self._tensor(weights, torch.int32).reshape(-1)
        if not self.p.shape[0] == self.n.shape[0] == self.w.shape[0]:
            raise ValueError("one normal and one weight per point")
        return self

    def face_samples(self, vertices, faces, area_unit):
        import torch
        from boxfusion_amd import _lib
        v, f = self._tensor(vertices, torch.float32).reshape(-1, 3), self._tensor(faces, torch.int32).reshape(-1, 3)
        self.p, self.n, self.w, st = _lib.level_face_samples(v, f, area_unit)
        self.face_stats = st.cpu().numpy()
        return self

    def bounds(self):
        fin = self.p.isfinite().all(1)
        if not bool(fin.any()):
            return None
        q = self.p[fin]
        return q.amin(0).cpu().numpy(), q.amax(0).cpu().numpy()

    def vote(self, G):
        from boxfusion_amd import _lib
        hist, st = _lib.level_vote(self.n, self.w, G)
        return hist.cpu().numpy(), st.cpu().numpy()

    def score(self, hist, G, candidates, cos_par, sin_perp):
        import torch
        from boxfusion_amd import _lib
        out = _lib.level_score(torch.from_numpy(hist).to(self.device), G,
                               torch.from_numpy(np.ascontiguousarray(candidates, np.int32)).to(self.device), cos_par, sin_perp)
        return out.cpu().numpy()

    def refine(self, frame, cos_par, sin_perp, h0, height_bin, n_bins):
        import torch
        from boxfusion_amd import _lib
        sums, heights, st = _lib.level_refine(self.p, self.n, self.w, torch.from_numpy(np.asarray(frame, F)).to(self.device),
                                              cos_par, sin_perp, h0, height_bin, n_bins)
        return sums.cpu().numpy(), heights.cpu().numpy(), st.cpu().numpy()


def estimate(points, normals, weights, prior=None, *, poses=None, first_pose=None, G=32, tau_deg=10.0, cone_deg=40.0, iters=3,
             height_bin, min_share=0.5, backend=None):
    """Oriented samples -> Levelling.  points, normals f32 [n,3] (unit normals that point to free space),
    weights uint32 [n], arrays or tensors.

    1. prior: the given direction, else the normalised sum of the cameras' image-up axes (-pose[:3,1]) over
       the finite poses, else (0, 0, 1), which refines an almost-level scene.  Pass one for images that are
       not upright.
    2. candidates: the cube-map bins (G x G per face) whose centre lies within cone_deg of the prior.
       cone_deg must be below 45: two Manhattan axes are 90 degrees apart, so at most one lies in the cone,
       and that decides between the floor's normal and a wall's.
    3. the winner has the largest weight parallel plus perpendicular to it within tau_deg.
    4. `iters` refinement passes, the last with tau_deg / 2: the new axis is the top eigenvector of
       S_par - S_perp, solved here in f64 from the device's integer sums.  One more pass reads out the
       share, the yaw sums and the heights for the final axis.
    5. yaw is atan2(S, C) / 4; of the four equal wall directions the one nearest the first finite pose's
       viewing axis on the floor (first_pose, else the first of poses), else nearest e1.
    6. the floor is the lowest height bin (of height_bin metres) with at least a fifth of the largest bin's
       weight among the upward-facing samples, refined by the weighted mean over it and its two neighbours;
       the x / y origin is the first finite pose's camera centre, else the floor samples' centroid.
    ok says whether to trust it: share >= min_share, a floor was found, and the refined up stayed within the
    cone of the prior.  min_share = 0.5 and the fifth are defaults from two synthetic scenes (a box room
    scores 0.9, a sphere in a shell 0.3), not from a real capture.  cone_deg >= 45 raises ValueError."""
    be = (backend or DeviceSamples()).load(points, normals, weights)
    return _run(be, prior, poses, first_pose, dict(G=G, tau_deg=tau_deg, cone_deg=cone_deg, iters=iters,
                                                   height_bin=height_bin, min_share=min_share))


def _run(be, prior, poses, first_pose, args):
    if prior is None:
        prior = prior_from_poses(poses)
    if prior is None:
        prior = (0.0, 0.0, 1.0)
    if first_pose is None:
        first_pose = finite_poses(poses)[:1]
    return procedure(be, prior, first_pose, **args)


def level_mesh(mesh_or_volume, poses=None, prior=None, first_pose=None, *, voxel=None, backend=None, **args):
    """Levelling of a scene mesh: a scene_mesh.TsdfVolume (its surface, its voxel) or (vertices, faces) /
    (vertices, rgb, faces) with `voxel` the mesh's resolution in metres (0.02 when not given).  A face votes
    with its area in units of voxel^2 / 256; the height bins are one voxel.  poses: the cameras' poses [N,4,4]
    (-inf for lost frames), which give the prior, the yaw's quadrant and the x / y origin; further
    arguments as estimate's."""
    if hasattr(mesh_or_volume, "mesh") and callable(mesh_or_volume.mesh):
        vertices, _, faces = mesh_or_volume.mesh()
        voxel = float(mesh_or_volume.voxel)
    else:
        vertices, faces = mesh_or_volume[0], mesh_or_volume[-1]
        voxel = 0.02 if voxel is None else float(voxel)
    if not voxel > 0:
        raise ValueError("voxel must be positive")
    be = (backend or DeviceSamples()).face_samples(vertices, faces, F(voxel * voxel / 256.0))
    args.setdefault("height_bin", voxel)
    lv = _run(be, prior, poses, first_pose, args)
    if be.face_stats is not None:
        lv.stats.update({k: int(v) for k, v in zip(STATS, be.face_stats) if k.startswith("face")})
    return lv


# ---- command line ----------------------------------------------------------------------------------------
def parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m boxfusion_amd.scene_level",
                                description="level a scene mesh: z up, the floor at z = 0, the walls along x and y")
    p.add_argument("mesh", help="a PLY with faces written by TsdfVolume.save_ply / visualize.mesh_to_ply")
    p.add_argument("out", help="the levelled PLY")
    p.add_argument("--poses", help="the cameras' poses, float32 [N,4,4] .npy (-inf for lost frames): the prior, the yaw's "
                                   "quadrant and the origin")
    p.add_argument("--poses-out", help="the levelled poses as .npy (needs --poses)")
    p.add_argument("--json", help="write the Levelling's fields here")
    p.add_argument("--voxel", type=float, default=0.02, help="the mesh's resolution in metres")
    p.add_argument("--prior", type=float, nargs=3, metavar=("X", "Y", "Z"), help="roughly up, instead of the cameras' image-up")
    p.add_argument("--cone", type=float, default=40.0, help="degrees about the prior searched for up, below 45")
    p.add_argument("--tau", type=float, default=10.0, help="degrees within which a normal counts as parallel / perpendicular")
    p.add_argument("--min-share", type=float, default=0.5, help="the explained share of the surface below which the "
                                                                 "scene is not taken for a room")
    return p


def main(argv=None):
    from boxfusion_amd.visualize import mesh_to_ply, read_ply_surface
    p = parser()
    a = p.parse_args(argv)
    if not a.voxel > 0:
        p.error("--voxel must be positive")
    if not 0 < a.cone < 45:
        p.error("--cone must lie in (0, 45)")
    if not 0 < a.tau < 45:
        p.error("--tau must lie in (0, 45)")
    if a.poses_out and not a.poses:
        p.error("--poses-out needs --poses")
    if a.prior is not None and not (np.isfinite(a.prior).all() and np.any(a.prior)):
        p.error("--prior must be a finite direction that is not zero")
    if not os.path.isfile(a.mesh):
        p.error(f"{a.mesh} is missing")
    xyz, rgb, faces = read_ply_surface(a.mesh)
    if not len(faces):
        p.error(f"{a.mesh} has no faces")
    poses = np.load(a.poses) if a.poses else None
    lv = level_mesh((xyz, faces), poses=poses, prior=a.prior, voxel=a.voxel, cone_deg=a.cone, tau_deg=a.tau,
                    min_share=a.min_share)
    print(lv.summary())
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(lv.to_json(), fh, indent=1)
    if not lv.ok:
        print("warning: this does not look like a room from here; nothing levelled", file=sys.stderr)
        return 1
    mesh_to_ply(lv.apply_points(xyz), rgb, faces, a.out)
    if a.poses_out:
        np.save(a.poses_out, lv.apply(poses))
    print(f"{len(xyz)} vertices, {len(faces)} faces -> {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
