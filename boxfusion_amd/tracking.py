"""Camera tracking against the scene's TSDF: the KinectFusion loop over a `scene_mesh.TsdfVolume`.

`TsdfVolume.raycast` reads the fused model back as a predicted vertex / normal map from a pose
(bf_tsdf_raycast); `IcpTracker.track` aligns a new depth frame to that prediction by projective
point-to-plane ICP: per iteration one bf_icp_reduce (the 6-DoF normal equations, summed on the
device in a fixed order), one read-back of 32 doubles, a 6 x 6 solve on the host and T <- exp(xi) T.
With a colour image beside the depth frame, `track(depth, guess, rgb)` adds a photometric term: the
new frame's intensities against the last placed frame's image (bf_photo_reduce, the same 32 doubles),
A = A_geo + w^2 A_photo.  A texture fixes the directions a plane leaves free, so a wall, a floor or a
table top that fills the view can be placed.
`track_sequence` alternates tracking and integration over a run of depth frames, either for every
frame (a recording without poses) or only for the frames whose pose is not finite (a capture that
lost tracking: ScanNet writes -inf there and `SensFile.poses_filled()` repeats the last valid pose).

A frame the tracker cannot place is *lost*: its pose is all -inf, the capture format's own
convention, which `TsdfVolume.integrate`, the renderer and the GT filter already skip.  When the camera
moved on while it was lost, the last good pose is no guess any more: `Relocaliser` keeps keyframes of
the placed frames as randomised-fern codes (bf_fern.hip) and restarts the tracker from the poses of
the keyframes nearest to the lost frame's code.
"""
from __future__ import annotations

import numpy as np
import torch

from boxfusion_amd import _lib

LOST = np.full((4, 4), -np.inf, np.float32)


def se3_exp(xi):
    """the closed-form SE(3) exponential of xi = (omega, t) -> f64 [4,4]"""
    w, t = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = float(np.sqrt(w @ w))
    Wx = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-9:
        A, B, C = 1.0 - th * th / 6, 0.5 - th * th / 24, 1.0 / 6 - th * th / 120
    else:
        A, B, C = np.sin(th) / th, (1 - np.cos(th)) / (th * th), (th - np.sin(th)) / (th ** 3)
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + A * Wx + B * (Wx @ Wx)
    out[:3, 3] = (np.eye(3) + B * Wx + C * (Wx @ Wx)) @ t
    return out


def world_to_camera(pose):
    """rows f64 [3,4] of the inverse of a rigid camera-to-world pose"""
    P = np.asarray(pose, np.float64).reshape(4, 4)
    Rt = P[:3, :3].T
    return np.concatenate([Rt, -(Rt @ P[:3, 3])[:, None]], 1)


def normal_matrix(out):
    """J^T J f64 [6,6] from bf_icp_reduce's 21 upper-triangle entries"""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = out[:21]
    return A + np.triu(A, 1).T


class IcpTracker:
    """projective point-to-plane ICP of depth frames (H x W, pinhole K) against `volume`.

    strides / iters: the coarse-to-fine schedule (pixels (stride i, stride j) of the live frame; the
    stride stands in for a depth pyramid).  dist_max (default 4 truncation distances) and cos_min gate
    a correspondence by its distance and by the angle between the normals; jump (default one truncation
    distance) is the depth step across which no live normal is formed.  A frame is lost when fewer
    than min_inlier_frac of the sampled pixels are inliers or J^T J's condition number exceeds
    cond_max (a single plane leaves three directions unobserved: rank 3).

    photo_weight / intensity_max: the photometric term of `track(depth, guess, rgb)`.  Its normal
    equations enter with photo_weight squared (intensities are 0 .. 1, the geometric residual is in
    metres); a sample whose intensity differs from the reference by more than intensity_max is left
    out, and so is one whose depth differs from the reference frame's by more than dist_max.  The
    inlier share is still judged on the geometric count, the condition number on the combined matrix:
    an untextured plane adds exactly nothing and stays lost."""

    def __init__(self, volume, K, H, W, strides=(4, 2, 1), iters=(4, 4, 4), dist_max=None, cos_min=0.8,
                 min_inlier_frac=0.4, cond_max=1000.0, jump=None, near=0.05, photo_weight=1.0, intensity_max=0.3):
        if len(strides) != len(iters) or not strides or min(strides) < 1 or min(iters) < 1:
            raise ValueError("strides and iters: one positive iteration count per positive stride")
        self.volume, self.H, self.W = volume, int(H), int(W)
        self.K = np.asarray(K.cpu() if torch.is_tensor(K) else K, np.float32).reshape(3, 3)
        self.intr = (self.K[0, 0], self.K[1, 1], self.K[0, 2], self.K[1, 2])
        trunc = float(volume.voxel) * volume.trunc_voxels
        self.strides, self.iters = tuple(int(s) for s in strides), tuple(int(i) for i in iters)
        self.dist_max = 4 * trunc if dist_max is None else float(dist_max)
        self.jump = trunc if jump is None else float(jump)
        self.cos_min, self.min_inlier_frac = float(cos_min), float(min_inlier_frac)
        self.cond_max, self.near = float(cond_max), float(near)
        self.photo_weight, self.intensity_max = float(photo_weight), float(intensity_max)
        if not self.photo_weight >= 0 or not self.intensity_max >= 0:
            raise ValueError("photo_weight and intensity_max: not negative")
        self._out = torch.empty(32, dtype=torch.float64, device=volume.device)
        self._both = torch.empty((2, 32), dtype=torch.float64, device=volume.device)
        self._ref = None                                     # (intensity f32 [H,W], depth f32 [H,W], world -> camera)

    def _depth(self, depth_m, who):
        depth_m = torch.as_tensor(depth_m).to(self.volume.device, torch.float32)
        if tuple(depth_m.shape) != (self.H, self.W):
            raise ValueError(f"{who}: depth [{self.H},{self.W}], got {tuple(depth_m.shape)}")
        return depth_m

    def _grey(self, rgb, who):
        """rgb u8 [Hc,Wc,3] (tensor or array) -> intensity f32 [H,W], resized first as TsdfVolume.integrate does"""
        rgb = torch.as_tensor(rgb).to(self.volume.device)
        if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
            raise ValueError(f"{who}: rgb u8 [Hc,Wc,3], got {rgb.dtype} {tuple(rgb.shape)}")
        if tuple(rgb.shape[:2]) != (self.H, self.W):
            rgb = _lib.resize_bicubic_u8(rgb, self.H, self.W)
        return _lib.grey_u8(rgb)

    def set_reference(self, rgb, depth_m, pose):
        """the frame the photometric term compares with: rgb u8 [Hc,Wc,3] and depth_m f32 [H,W] of a frame
        whose camera-to-world pose [4,4] is known.  A pose with a non-finite entry clears the reference."""
        pose = np.asarray(pose.cpu() if torch.is_tensor(pose) else pose, np.float32).reshape(4, 4)
        if not np.isfinite(pose).all():
            self._ref = None
            return
        self._ref = (self._grey(rgb, "set_reference"), self._depth(depth_m, "set_reference").contiguous(),
                     world_to_camera(pose))

    def track(self, depth_m, pose_guess, rgb=None):
        """depth_m f32 [H,W] metres (tensor or array) seen from about pose_guess [4,4] -> (pose f32 [4,4]
        camera-to-world, or all -inf when the frame is lost; info: lost, iterations, inliers, sampled,
        rms (metres, point to plane), cond).  With rgb u8 [Hc,Wc,3] and a reference (set_reference, or
        the last frame this call placed with an image) the photometric term joins in: both reductions
        per iteration, one read-back of the two rows, and info gains photo_inliers and photo_rms
        (intensity, 0 .. 1).  A frame placed with rgb becomes the reference; a lost one never does."""
        vol = self.volume
        depth_m = self._depth(depth_m, "track")
        guess = np.asarray(pose_guess.cpu() if torch.is_tensor(pose_guess) else pose_guess, np.float32).reshape(4, 4)
        info = dict(lost=True, iterations=0, inliers=0, sampled=0, rms=float("inf"), cond=float("inf"))
        photo = rgb is not None and self._ref is not None
        if photo:
            info.update(photo_inliers=0, photo_rms=float("inf"))
        if not np.isfinite(guess).all():
            return LOST.copy(), info
        if photo:
            live = self._grey(rgb, "track")
            ri, rd, Mr = self._ref
            lam2 = np.float64(self.photo_weight) * np.float64(self.photo_weight)
        _, mv, mn, _, _ = vol.raycast(guess, self.K, self.H, self.W, near=self.near)
        mv, mn = mv[0], mn[0]
        lv, ln = _lib.depth_vertex_normal(depth_m, self.intr, vol.max_depth, self.jump)
        T = guess.astype(np.float64)[:3].copy()
        M = world_to_camera(guess)
        for stride, n_it in zip(self.strides, self.iters):
            sampled = -(-self.H // stride) * -(-self.W // stride)
            for _ in range(n_it):
                if photo:
                    _lib.icp_reduce(lv, ln, stride, T, mv, mn, M, self.intr, self.dist_max, self.cos_min, out=self._both[0])
                    _lib.photo_reduce(lv, live, stride, T, ri, rd, Mr, self.intr, self.dist_max, self.intensity_max,
                                      out=self._both[1])
                    out, po = self._both.cpu().numpy()
                    info.update(photo_inliers=int(po[28]),
                                photo_rms=float(np.sqrt(po[27] / po[28])) if po[28] > 0 else float("inf"))
                else:
                    _lib.icp_reduce(lv, ln, stride, T, mv, mn, M, self.intr, self.dist_max, self.cos_min, out=self._out)
                    out = self._out.cpu().numpy()
                info.update(iterations=info["iterations"] + 1, inliers=int(out[28]), sampled=sampled)
                if out[28] < 6 or out[28] < self.min_inlier_frac * sampled:
                    return LOST.copy(), info
                A, b = normal_matrix(out), out[21:27]
                if photo:
                    A, b = A + lam2 * normal_matrix(po), b + lam2 * po[21:27]
                ev = np.linalg.eigvalsh(A)
                info["cond"] = float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")
                info["rms"] = float(np.sqrt(out[27] / out[28]))
                if not info["cond"] <= self.cond_max:
                    return LOST.copy(), info
                xi = np.linalg.solve(A, b)
                T = (se3_exp(xi) @ np.concatenate([T, [[0.0, 0.0, 0.0, 1.0]]]))[:3]
        pose = np.eye(4, dtype=np.float32)
        pose[:3] = T.astype(np.float32)
        info["lost"] = False
        if rgb is not None:
            self._ref = (live if photo else self._grey(rgb, "track"), depth_m.contiguous(), world_to_camera(pose))
        return pose, info


def fern_table(ferns, cells, seed=0, depth_range_m=(0.4, 4.0)):
    """the randomised ferns of a Relocaliser: i32 [ferns, 5] of (cell index below `cells`, the thresholds of R, G
    and B in grey levels 0 .. 254, the depth threshold in millimetres within depth_range_m), drawn from
    numpy.random.default_rng(seed): the same table for the same arguments"""
    ferns, cells = int(ferns), int(cells)
    lo, hi = (int(round(float(v) * 1000.0)) for v in depth_range_m)
    if ferns < 8 or ferns % 8:
        raise ValueError("fern_table: ferns a positive multiple of 8")
    if cells < 1 or not 0 <= lo < hi <= 65535:
        raise ValueError("fern_table: at least one cell and 0 <= depth_range_m[0] < depth_range_m[1] <= 65.535")
    rng = np.random.default_rng(seed)
    table = np.empty((ferns, 5), np.int32)
    table[:, 0] = rng.integers(0, cells, ferns)
    table[:, 1:4] = rng.integers(0, 255, (ferns, 3))
    table[:, 4] = rng.integers(lo, hi, ferns)
    return table


class Relocaliser:
    """keyframe relocalisation with randomised ferns (Glocker et al.; bf_fern.hip) for frames of H x W.

    Every placed frame is offered to `observe`: its depth (and colour) means over cells of `cell` pixels
    are compared with `ferns` random thresholds (`fern_table`: seed, depth_range in metres) into a code
    of four bits per fern; the code joins the keyframe table, with the frame's pose, when more than
    floor(harvest * ferns) of its ferns differ from the nearest keyframe's (or the table is empty); a
    table of `capacity` keyframes that is full counts the frame and drops it.  `query` returns the
    nearest keyframes of a frame, `relocalise` restarts an IcpTracker from their poses.  Without images
    the colour bits are 0 in the table and the query alike and the distance counts the depth bits only;
    use the same choice for every call.  max_depth (<= 65.535) is the depth beyond which a pixel is
    invalid, as in TsdfVolume.

    The defaults of harvest and of relocalise's max_distance come from the range the literature uses
    and from a 48 x 64 synthetic room; nobody has measured them on a real capture."""

    def __init__(self, H, W, device, ferns=512, cell=16, capacity=4096, harvest=0.15, seed=0, depth_range=(0.4, 4.0),
                 max_depth=10.0):
        self.H, self.W, self.device = int(H), int(W), torch.device(device)
        self.ferns, self.cell, self.capacity = int(ferns), int(cell), int(capacity)
        if self.ferns < 8 or self.ferns % 8:
            raise ValueError("Relocaliser: ferns a positive multiple of 8")
        if not 1 <= self.cell <= 64 or self.H // self.cell < 1 or self.W // self.cell < 1:
            raise ValueError("Relocaliser: 1 <= cell <= 64, and no larger than the image")
        if self.capacity < 1 or not 0 <= float(harvest) <= 1 or not 0 < float(max_depth) <= 65.535:
            raise ValueError("Relocaliser: capacity >= 1, 0 <= harvest <= 1, 0 < max_depth <= 65.535")
        self.max_depth, self.harvest = float(max_depth), float(harvest)
        self.threshold = int(np.floor(self.harvest * self.ferns))
        self.cells = (self.H // self.cell) * (self.W // self.cell)
        self.table = fern_table(self.ferns, self.cells, seed, depth_range)
        self._ferns = _lib.fern_upload(self.table, self.cells, self.device)
        words = self.ferns // 8
        self._codes = torch.zeros((self.capacity, words), dtype=torch.int32, device=self.device)
        self._poses = torch.zeros((self.capacity, 16), dtype=torch.float32, device=self.device)
        self._ids = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
        self._state = torch.zeros(4, dtype=torch.int32, device=self.device)        # n, then _lib.FERN_COUNTERS
        self._code = torch.empty((1, words), dtype=torch.int32, device=self.device)
        self._best = torch.empty((1, 1, 2), dtype=torch.int32, device=self.device)
        self._offered = 0                                    # the host's bound of n: the frames observe has passed on

    def _frame(self, depth, rgb, who):
        """(depth f32 [H,W], rgb u8 [H,W,3] or None) on the device; an image of another size is resized as
        TsdfVolume.integrate does"""
        depth = depth if torch.is_tensor(depth) else _lib.h2d(np.asarray(depth, np.float32), self.device)
        depth = depth.to(self.device, torch.float32)
        if tuple(depth.shape) != (self.H, self.W):
            raise ValueError(f"{who}: depth [{self.H},{self.W}], got {tuple(depth.shape)}")
        if rgb is not None:
            rgb = rgb if torch.is_tensor(rgb) else _lib.h2d(np.asarray(rgb), self.device)
            rgb = rgb.to(self.device)
            if rgb.dtype != torch.uint8 or rgb.dim() != 3 or rgb.shape[2] != 3:
                raise ValueError(f"{who}: rgb u8 [Hc,Wc,3], got {rgb.dtype} {tuple(rgb.shape)}")
            if tuple(rgb.shape[:2]) != (self.H, self.W):
                rgb = _lib.resize_bicubic_u8(rgb, self.H, self.W)
        return depth, rgb

    def __len__(self):
        return int(self._state[0].item())

    def observe(self, depth, pose, rgb=None, frame=-1):
        """offer a placed frame (depth f32 [H,W] metres, camera-to-world pose [4,4], rgb u8 [Hc,Wc,3] or None,
        its frame id): four launches and no synchronisation; a pose with a non-finite entry is ignored"""
        pose = np.asarray(pose.cpu() if torch.is_tensor(pose) else pose, np.float32).reshape(4, 4)
        if not np.isfinite(pose).all():
            return
        depth, rgb = self._frame(depth, rgb, "observe")
        _lib.fern_encode(depth, rgb, self.cell, self.max_depth, self._ferns, codes=self._code)
        _lib.fern_search(self._codes, self._state[:1], min(max(self._offered, 1), self.capacity), self._code, 1, top=self._best)
        _lib.fern_append(self._codes, self._state[:1], self._code[0], self._best[0, 0], self.threshold, pose, frame,
                         self._poses, self._ids, self._state[1:])
        self._offered += 1

    def query(self, depth, rgb=None, k=4):
        """the k (<= 8) nearest keyframes of a frame, nearest first: [(distance in ferns, keyframe index, its
        pose f32 [4,4], its frame id)], fewer when the table holds fewer; one read-back"""
        k = int(k)
        if not 1 <= k <= _lib.FERN_K_MAX:
            raise ValueError(f"query: 1 <= k <= {_lib.FERN_K_MAX}")
        depth, rgb = self._frame(depth, rgb, "query")
        _lib.fern_encode(depth, rgb, self.cell, self.max_depth, self._ferns, codes=self._code)
        top = _lib.fern_search(self._codes, self._state[:1], min(max(self._offered, 1), self.capacity), self._code, k)[0]
        at = top[:, 1].clamp(min=0).long()
        # integers below 2^31 and f32 poses: exact in f64, so one row comes back
        row = torch.cat([top.double(), self._poses[at].double(), self._ids[at].double()[:, None]], 1).cpu().numpy()
        return [(int(r[0]), int(r[1]), r[2:18].astype(np.float32).reshape(4, 4), int(r[18])) for r in row if r[1] >= 0]

    def relocalise(self, tracker, depth, rgb=None, k=4, max_distance=0.5):
        """place a frame the tracker has lost: the nearest k keyframes whose distance is at most max_distance *
        ferns, nearest first, each as the guess of tracker.track(depth, pose) (without the image: the
        tracker's photometric reference is the last placed frame, somewhere else, so the geometric gates
        verify); the first that places the frame wins.  With rgb the placed frame becomes the tracker's
        photometric reference.  Going by code distance and stopping at max_distance, instead of trying
        every keyframe, matters: the gates alone cannot tell one corner of a box room from another.
        -> (pose f32 [4,4] or all -inf, the tracker's info with relocalised, candidates_tried and, when
        placed, keyframe and fern_distance)"""
        info = dict(lost=True, iterations=0, inliers=0, sampled=0, rms=float("inf"), cond=float("inf"))
        tried = 0
        for distance, keyframe, guess, _ in self.query(depth, rgb, k):
            if distance > max_distance * self.ferns:
                break
            tried += 1
            pose, info = tracker.track(depth, guess)
            if not info["lost"]:
                if rgb is not None:
                    tracker.set_reference(rgb, depth, pose)
                info.update(relocalised=True, keyframe=keyframe, fern_distance=distance, candidates_tried=tried)
                return pose, info
        info.update(lost=True, relocalised=False, candidates_tried=tried)
        return LOST.copy(), info

    def keyframes(self):
        """(poses f32 [n,4,4], frame ids i32 [n], codes u32 [n, ferns/8]) of the table, read back"""
        n = len(self)
        return (self._poses[:n].cpu().numpy().reshape(n, 4, 4), self._ids[:n].cpu().numpy(),
                self._codes[:n].cpu().numpy().view(np.uint32))

    def counters(self):
        """dict(keyframes, observed, added, dropped_full), read back"""
        s = self._state.cpu().tolist()
        return dict(keyframes=s[0], **dict(zip(_lib.FERN_COUNTERS, s[1:])))


def track_sequence(depths, K, first_pose=None, known_poses=None, volume=None, colours=None, photometric=False,
                   relocaliser=None, **tracker_args):
    """track and fuse a run of depth frames (depths f32 [N,H,W] metres, tensor or array) into `volume`
    (a scene_mesh.TsdfVolume): frame 0 is integrated at its pose (known_poses[0], or without known_poses
    first_pose, default identity); every later frame takes its known finite pose, or is tracked from
    the last good pose, and is integrated unless it is lost.  known_poses [N,4,4] with -inf rows
    recovers the lost frames of a capture; None tracks every frame.  colours u8 [N,Hc,Wc,3] colours
    the volume; photometric=True (which needs colours) also hands each tracked frame's image to the
    tracker, with the last frame that has a pose as the photometric reference.  Returns (poses f32
    [N,4,4] with -inf for lost frames, info per frame; info['tracked'] says whether the pose came from
    the tracker).  relocaliser (a Relocaliser for H x W): every frame that ends up with a pose is offered
    to it after it is integrated, a frame the tracker loses from the last good pose is handed to its
    `relocalise` before it is given up, and every info gains `relocalised`."""
    if volume is None:
        raise ValueError("track_sequence: volume=TsdfVolume(...) is required")
    depths = torch.as_tensor(depths)
    if depths.dim() != 3:
        raise ValueError(f"track_sequence: depths [N,H,W], got {tuple(depths.shape)}")
    depths = depths.to(volume.device, torch.float32)
    N, H, W = depths.shape
    if known_poses is not None:
        known_poses = np.asarray(known_poses, np.float32).reshape(-1, 4, 4)
        if len(known_poses) != N:
            raise ValueError(f"track_sequence: {N} frames, {len(known_poses)} known poses")
    if photometric and colours is None:
        raise ValueError("track_sequence: photometric=True needs colours")
    tracker = IcpTracker(volume, K, H, W, **tracker_args)
    poses = np.tile(LOST, (N, 1, 1))
    infos, last = [], None
    for i in range(N):
        known = known_poses is not None and bool(np.isfinite(known_poses[i]).all())
        if known:
            pose, info = known_poses[i].copy(), dict(lost=False, tracked=False)
        elif last is None and i == 0 and known_poses is None:
            pose = np.eye(4, dtype=np.float32) if first_pose is None else np.asarray(first_pose, np.float32).reshape(4, 4)
            info = dict(lost=False, tracked=False)
        elif last is None:                                   # nothing fused yet: nothing to track against
            pose, info = LOST.copy(), dict(lost=True, tracked=False)
        else:
            pose, info = tracker.track(depths[i], last, colours[i]) if photometric else tracker.track(depths[i], last)
            info["tracked"] = True
            if relocaliser is not None and info["lost"]:
                pose, info = relocaliser.relocalise(tracker, depths[i], None if colours is None else colours[i])
                info["tracked"] = True
        if relocaliser is not None:
            info.setdefault("relocalised", False)
        infos.append(info)
        poses[i] = pose
        if info["lost"]:
            continue
        volume.integrate(depths[i], K, pose[None], None if colours is None else colours[i])
        if photometric and not info.get("tracked"):
            tracker.set_reference(colours[i], depths[i], pose)
        if relocaliser is not None:
            relocaliser.observe(depths[i], pose, None if colours is None else colours[i], i)
        last = pose
    return poses, infos
