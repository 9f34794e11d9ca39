"""A numpy restatement of the tracker's photometric term (bf_grey_u8 and bf_photo_reduce in bf_track.hip, the
combination in boxfusion_amd/tracking.py) for test_photo_host.py and test_gpu_photo.py: the intensity of an RGB
image, the per-sample terms of the intensity residual against the last placed frame in f64 with the kernel's
operation order, and the tracker loop with both rows.  Plus the textured scenes the tests follow: a single wall
that fills the view (which the geometry alone cannot place) and track_ref.Room() with the same texture."""
import functools

import numpy as np

from tests import mesh_ref as R
from tests import track_ref as TR

F = np.float32
D = np.float64
LOST = TR.LOST


# ---- intensity ---------------------------------------------------------------------------------------------
def grey(rgb):
    """bf_grey_u8: u8 [...,3] -> f32 [...]: Y = (77 R + 150 G + 29 B + 128) >> 8, I = (float)Y / 255.0f"""
    c = np.asarray(rgb, np.uint8).astype(np.int64)
    y = (77 * c[..., 0] + 150 * c[..., 1] + 29 * c[..., 2] + 128) >> 8
    out = y.astype(F) / F(255.0)
    assert out.dtype == F
    return out


# ---- the photometric normal equations --------------------------------------------------------------------------
def photo_terms(lv, I_live, stride, T, I_ref, D_ref, M, K, dist_max, intensity_max, parts=False):
    """bf_photo_reduce's per-sample terms in f64: (terms [n_inliers, 28], sampled pixels); a row is the 21 upper-
    triangle entries of J J^T, the 6 of J r and r^2.  parts=True returns (terms, sampled, the inlier mask over the
    sampled pixels, the residuals of the inliers, J [n_inliers, 6])"""
    lv = np.asarray(lv, F)[::stride, ::stride].reshape(-1, 3).astype(D)
    il = np.asarray(I_live, F)[::stride, ::stride].reshape(-1).astype(D)
    I_ref, D_ref = np.asarray(I_ref, F), np.asarray(D_ref, F)
    T, M = np.asarray(T, D).reshape(-1)[:12].reshape(3, 4), np.asarray(M, D).reshape(-1)[:12].reshape(3, 4)
    Hr, Wr = I_ref.shape
    fx, fy, cx, cy = [D(a) for a in R.intrinsics(K)]
    n_sampled = len(lv)
    x, y, z = lv.T
    with np.errstate(all="ignore"):
        ok = z > 0
        p = [T[i, 0] * x + T[i, 1] * y + T[i, 2] * z + T[i, 3] for i in range(3)]
        q = [M[i, 0] * p[0] + M[i, 1] * p[1] + M[i, 2] * p[2] + M[i, 3] for i in range(3)]
        ok &= q[2] > 0
        qz = np.where(ok, q[2], 1.0)
        u, w = fx * q[0] / qz + cx, fy * q[1] / qz + cy
        u0, w0 = np.floor(u), np.floor(w)
        ok &= (u0 >= 0) & (u0 <= Wr - 2) & (w0 >= 0) & (w0 <= Hr - 2)
        iu, iw = np.where(ok, u0, 0).astype(np.int64), np.where(ok, w0, 0).astype(np.int64)
        ru, rw = np.where(ok, np.floor(u + 0.5), 0).astype(np.int64), np.where(ok, np.floor(w + 0.5), 0).astype(np.int64)
        if Hr < 2 or Wr < 2:
            terms = np.zeros((0, 28))
            return (terms, n_sampled, ok & False, np.zeros(0), np.zeros((0, 6))) if parts else (terms, n_sampled)
        dr = D_ref[rw, ru].astype(D)
        ok &= (dr > 0) & (np.abs(dr - qz) <= D(dist_max))
        fu, fv = u - u0, w - w0
        i00, i10 = I_ref[iw, iu].astype(D), I_ref[iw, iu + 1].astype(D)
        i01, i11 = I_ref[iw + 1, iu].astype(D), I_ref[iw + 1, iu + 1].astype(D)
        top, bot = i00 + fu * (i10 - i00), i01 + fu * (i11 - i01)
        c = top + fv * (bot - top)
        gx = (i10 - i00) + fv * ((i11 - i01) - (i10 - i00))
        gy = (i01 - i00) + fu * ((i11 - i10) - (i01 - i00))
        r = il - c
        ok &= np.abs(r) <= D(intensity_max)
        a, b = gx * fx, gy * fy
        h = [a / qz, b / qz, -(a * q[0] + b * q[1]) / (qz * qz)]
        g = [M[0, i] * h[0] + M[1, i] * h[1] + M[2, i] * h[2] for i in range(3)]
        J = [p[1] * g[2] - p[2] * g[1], p[2] * g[0] - p[0] * g[2], p[0] * g[1] - p[1] * g[0], g[0], g[1], g[2]]
        cols = [J[a_] * J[b_] for a_ in range(6) for b_ in range(a_, 6)] + [J[a_] * r for a_ in range(6)] + [r * r]
    terms = np.stack(cols, -1)[ok]
    if parts:
        return terms, n_sampled, ok, r[ok], np.stack(J, -1)[ok]
    return terms, n_sampled


def track(vol, depth, guess, K, voxel, T, max_depth, rgb=None, ref=None, photo_weight=1.0, intensity_max=0.3,
          strides=(4, 2, 1), iters=(4, 4, 4), dist_max=None, cos_min=0.8, min_inlier_frac=0.4, cond_max=1000.0, jump=None,
          near=0.05):
    """IcpTracker.track(depth, guess, rgb) in numpy, as track_ref.track with the photometric row: rgb u8 [H,W,3] at
    the depth size, ref dict(grey f32 [H,W], depth f32 [H,W], pose [4,4]) the last placed frame (or None: the
    geometry alone); A = A_geo + w^2 A_photo, b = b_geo + w^2 b_photo.  -> (pose f32 [4,4] or LOST, info)"""
    H, W = depth.shape
    dist_max = 4 * T * voxel if dist_max is None else dist_max
    jump = T * voxel if jump is None else jump
    model = TR.raycast(vol, guess, K, H, W, voxel, T, near, max_depth)
    lv, ln = TR.vertex_normal(depth, K, max_depth, jump)
    Tm = np.asarray(guess, F).astype(D)[:3].copy()
    M = TR.w2c(np.asarray(guess, F))
    photo = rgb is not None and ref is not None
    info = dict(lost=False, iterations=0, inliers=0, sampled=0, rms=float("inf"), cond=float("inf"))
    if photo:
        il, Mr = grey(rgb), TR.w2c(np.asarray(ref["pose"], F))
        info.update(photo_inliers=0, photo_rms=float("inf"))
    lam2 = D(photo_weight) * D(photo_weight)
    for stride, n_it in zip(strides, iters):
        for _ in range(n_it):
            terms, n_s = TR.icp_terms(lv, ln, stride, Tm, model["vertex"], model["normal"], M, K, dist_max, cos_min)
            out = TR.icp_sums(terms)
            info.update(iterations=info["iterations"] + 1, inliers=int(out[28]), sampled=n_s)
            if photo:
                pt, _ = photo_terms(lv, il, stride, Tm, ref["grey"], ref["depth"], Mr, K, dist_max, intensity_max)
                po = TR.icp_sums(pt)
                info.update(photo_inliers=int(po[28]),
                            photo_rms=float(np.sqrt(po[27] / po[28])) if po[28] > 0 else float("inf"))
            if out[28] < 6 or out[28] < min_inlier_frac * n_s:
                info["lost"] = True
                return LOST.copy(), info
            A, b = TR.normal_matrix(out), out[21:27]
            if photo:
                A, b = A + lam2 * TR.normal_matrix(po), b + lam2 * po[21:27]
            ev = np.linalg.eigvalsh(A)
            info["cond"] = float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")
            info["rms"] = float(np.sqrt(out[27] / out[28]))
            if not info["cond"] <= cond_max:
                info["lost"] = True
                return LOST.copy(), info
            xi = np.linalg.solve(A, b)
            Tm = (TR.se3_exp(xi) @ np.concatenate([Tm, [[0, 0, 0, 1]]]))[:3]
    pose = np.eye(4, dtype=F)
    pose[:3] = Tm.astype(F)
    return pose, info


# ---- the textured scenes ---------------------------------------------------------------------------------------
def texture(x, y, z=None):
    """the walls' brightness at a world point (0.02 .. 0.98)"""
    return (0.5 + 0.16 * np.sin(5 * x + 1) + 0.14 * np.sin(6 * y - 0.5) + 0.10 * np.sin(3.5 * (x + y) + 2)
            + 0.08 * np.sin(4 * (x - 2 * y)))


def render_texture(pose, K, depth, uniform=None):
    """u8 [H,W,3] of the texture at each pixel's depth hit (the same value in the three channels; 0 where the depth
    is 0), in float64 with the pose as the kernels get it (f32); uniform: that brightness everywhere instead"""
    P = np.asarray(pose, F).astype(D)
    H, W = depth.shape
    fx, fy, cx, cy = [float(a) for a in R.intrinsics(K)]
    v, u = np.mgrid[:H, :W].astype(D)
    d = np.asarray(depth, F).astype(D)
    a, b = (u - cx) / fx * d, (v - cy) / fy * d
    wx, wy = [P[i, 0] * a + P[i, 1] * b + P[i, 2] * d + P[i, 3] for i in range(2)]
    t = texture(wx, wy) if uniform is None else np.full((H, W), float(uniform))
    y8 = np.where(d > 0, np.rint(255.0 * t), 0).astype(np.uint8)
    return np.repeat(y8[..., None], 3, -1)


class Wall:
    """one textured wall (z = 1) that fills the view, from six cameras 35 mm and 1.1 degrees apart"""

    def __init__(self, H=48, W=64, focal=40.0, frames=6):
        self.H, self.W = H, W
        self.K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1]], F)
        self.lo, self.hi = np.array([-4.0, -4.0, -4.0]), np.array([4.0, 4.0, 1.0])
        self.poses = []
        for s in range(frames):
            P = np.eye(4)
            P[:3, :3] = R.rotation(2, 1.0 * s) @ R.rotation(1, 0.5 * s)
            P[:3, 3] = (0.03 * s, -0.015 * s, 0.01 * s)
            self.poses.append(P.astype(F))

    def depth(self, pose, H=None, W=None, K=None):
        return TR.render_room(pose, self.K if K is None else K, self.H if H is None else H, self.W if W is None else W,
                              self.lo, self.hi)

    def depths(self):
        return [self.depth(p) for p in self.poses]


def images(scene, depths, uniform=None):
    return [render_texture(p, scene.K, d, uniform) for p, d in zip(scene.poses, depths)]


def run_sequence(scene, depths, rgbs, known=None, photometric=True, track_rgb=None, **args):
    """tracking.track_sequence(..., photometric=...) in numpy: (poses [N,4,4], infos).  The reference is the last
    frame with a pose.  track_rgb: the images the tracker sees, where they differ from rgbs"""
    V = TR.ROOM_VOLUME
    poses, infos, used_d, used_p, last, ref = [], [], [], [], None, None
    for i, d in enumerate(depths):
        if known is not None and np.isfinite(known[i]).all():
            pose, info = np.asarray(known[i], F), dict(lost=False, tracked=False)
        elif i == 0 and known is None:
            pose, info = scene.poses[0], dict(lost=False, tracked=False)
        elif last is None:
            pose, info = LOST.copy(), dict(lost=True, tracked=False)
        else:
            vol, _ = TR.fuse_room(scene, used_d, used_p)
            pose, info = track(vol, d, last, scene.K, V["voxel"], V["T"], V["max_depth"],
                               rgb=rgbs[i] if photometric else None, ref=ref, **{**TR.TRACKER, **args})
            info["tracked"] = True
        poses.append(pose)
        infos.append(info)
        if not info["lost"]:
            used_d.append(d)
            used_p.append(pose)
            last = pose
            if photometric:
                ref = dict(grey=grey(rgbs[i]), depth=np.asarray(d, F), pose=pose)
    return np.stack(poses), infos


WALL_UNKNOWN = (2, 3, 4)                                   # the frames track_sequence must place on the wall


@functools.lru_cache(None)
def wall_scene():
    wall = Wall()
    depths = wall.depths()
    return dict(scene=wall, depths=depths, rgbs=images(wall, depths))


@functools.lru_cache(None)
def room_scene():
    room = TR.Room()
    depths = room.depths()
    return dict(scene=room, depths=depths, rgbs=images(room, depths))


@functools.lru_cache(None)
def reference(which, mode, photo_weight=1.0):
    """the restatement's run over the wall or the room: mode 'scratch' (every frame after the first tracked),
    'known' (the wall's WALL_UNKNOWN or the room's LOST_FRAMES unknown) or 'geometry' (scratch without images):
    dict(scene, depths, rgbs, known, poses, infos)"""
    s = wall_scene() if which == "wall" else room_scene()
    known = None
    if mode == "known":
        known = np.stack(s["scene"].poses)
        known[list(WALL_UNKNOWN if which == "wall" else TR.LOST_FRAMES)] = LOST
    poses, infos = run_sequence(s["scene"], s["depths"], s["rgbs"], known, photometric=mode != "geometry",
                                photo_weight=photo_weight)
    return dict(s, known=known, poses=poses, infos=infos)
