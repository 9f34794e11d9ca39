"""A numpy restatement of camera tracking (bf_tsdf_raycast in bf_tsdf.hip, bf_track.hip, boxfusion_amd/tracking.py)
for test_track_host.py and test_gpu_track.py: the raycast in f32 with the kernel's operation order over
mesh_ref.fuse's dict, the live vertex / normal maps in f32, the per-pixel ICP terms and their sums in f64, and the
tracker loop.  Plus the analytic scene the tracker tests follow: an axis-aligned box room seen from inside,
rendered in float64 by ray-slab intersection, with a short trajectory that keeps a corner (three walls) in view."""
import numpy as np

from tests import mesh_ref as R

F = np.float32
D = np.float64
LOST = np.full((4, 4), -np.inf, F)


# ---- the volume as a lookup ------------------------------------------------------------------------------
class Volume:
    """mesh_ref.fuse's dict (or TsdfVolume.raw()'s arrays) as w / q / cw / rgb sums per voxel"""

    def __init__(self, key, state):
        self.key = np.asarray(key, np.int64)
        self.state = np.asarray(state, np.int64)

    def block(self, bx, by, bz):
        """position of the blocks (integer arrays) in key, -1 where absent or out of the index range"""
        ok = (bx >= -R.BIAS) & (bx < R.BIAS) & (by >= -R.BIAS) & (by < R.BIAS) & (bz >= -R.BIAS) & (bz < R.BIAS)
        k = ((np.where(ok, bx, 0) + R.BIAS) << 42) | ((np.where(ok, by, 0) + R.BIAS) << 21) | (np.where(ok, bz, 0) + R.BIAS)
        if not len(self.key):
            return np.full(k.shape, -1, np.int64)
        at = np.minimum(np.searchsorted(self.key, k), len(self.key) - 1)
        return np.where(ok & (self.key[at] == k), at, -1)

    def voxel(self, ix, iy, iz):
        """(block position or -1, local index) of voxels (integer arrays)"""
        return self.block(ix >> 3, iy >> 3, iz >> 3), (ix & 7) | ((iy & 7) << 3) | ((iz & 7) << 6)

    def sample(self, px, py, pz, voxel, min_weight):
        """rc_sample: (valid, s) of the trilinear field at f32 points"""
        voxel = F(voxel)
        with np.errstate(all="ignore"):
            g = [p / voxel - F(0.5) for p in (px, py, pz)]
            g0 = [np.floor(a) for a in g]
            lim = F(8388600.0)
            ok = np.ones(px.shape, bool)
            for a in g0:
                ok &= (a >= -lim) & (a < lim)
            t = [a - b for a, b in zip(g, g0)]
            i = [np.where(ok, a, 0).astype(np.int64) for a in g0]
            v = []
            for c in range(8):
                b, l = self.voxel(i[0] + (c & 1), i[1] + ((c >> 1) & 1), i[2] + (c >> 2))
                ok &= b >= 0
                bb = np.maximum(b, 0)
                if len(self.key):
                    w, q = self.state[bb, 0, l], self.state[bb, 1, l]
                else:
                    w = q = np.zeros(px.shape, np.int64)
                ok &= w >= min_weight
                v.append(q.astype(F) / np.where(w > 0, w, 1).astype(F) / F(1024.0))
            c00, c10 = v[0] + t[0] * (v[1] - v[0]), v[2] + t[0] * (v[3] - v[2])
            c01, c11 = v[4] + t[0] * (v[5] - v[4]), v[6] + t[0] * (v[7] - v[6])
            c0, c1 = c00 + t[1] * (c10 - c00), c01 + t[1] * (c11 - c01)
            s = c0 + t[2] * (c1 - c0)
        assert s.dtype == F
        return ok, s


def max_steps(near, far, voxel):
    """the step budget TsdfVolume.raycast hands the kernel: the range in quarter voxels (every step is
    at least that long), capped"""
    return int(min(max(np.ceil((float(far) - float(near)) / (0.25 * float(F(voxel)))) + 16, 16), 1 << 20))


def raycast(vol, pose, K, H, W, voxel, T, near, far, min_weight=1, colour=False, steps=None):
    """bf_tsdf_raycast for one view: dict(depth [H,W], vertex [H,W,3], normal [H,W,3], rgb u8 [H,W,3] or
    None, hits, behind, left_range, skipped_pose, no_normal)"""
    P = np.asarray(pose, F).reshape(4, 4)
    out = dict(depth=np.zeros((H, W), F), vertex=np.zeros((H, W, 3), F), normal=np.zeros((H, W, 3), F),
               rgb=np.zeros((H, W, 3), np.uint8) if colour else None, hits=0, behind=0, left_range=0, skipped_pose=0,
               no_normal=0)
    if not np.isfinite(P).all():
        out["skipped_pose"] = 1
        return out
    fx, fy, cx, cy = R.intrinsics(K)
    steps = max_steps(near, far, voxel) if steps is None else steps
    voxel, near, far = F(voxel), F(near), F(far)
    v, u = np.mgrid[:H, :W]
    u, v = u.reshape(-1).astype(F), v.reshape(-1).astype(F)
    n = H * W
    a, b = (u - cx) / fx, (v - cy) / fy
    d = [P[i, 0] * a + P[i, 1] * b + P[i, 2] for i in range(3)]
    o = [P[i, 3] for i in range(3)]
    ln = np.sqrt(a * a + b * b + F(1.0))
    trunc, bs, min_m = F(T) * voxel, F(8.0) * voxel, F(0.25) * voxel
    assert ln.dtype == F and d[0].dtype == F and trunc.dtype == F
    t = np.full(n, near, F)
    t0, s0 = np.zeros(n, F), np.zeros(n, F)
    have, hit, behind = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    th = np.zeros(n, F)
    active = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            active &= t < far
            if not active.any():
                break
            p = [o[i] + d[i] * t for i in range(3)]
            bf = [np.floor(c / bs) for c in p]
            lim = F(R.BIAS)
            inr = np.ones(n, bool)
            for c in bf:
                inr &= (c >= -lim) & (c < lim)
            bi = [np.where(inr, c, 0).astype(np.int64) for c in bf]
            present = inr & (vol.block(*bi) >= 0)
            # the block is absent: out through its face
            e = np.full(n, np.inf, F)
            for i in range(3):
                bound = np.where(d[i] > 0, (bf[i] + F(1.0)) * bs, bf[i] * bs)
                e = np.where(d[i] != 0, np.fmin(e, (bound - p[i]) / np.where(d[i] != 0, d[i], F(1))), e)
            t_absent = t + (np.fmax(e, F(0)) + min_m / ln)
            ok, s = vol.sample(p[0], p[1], p[2], voxel, min_weight)
            t_invalid = t + voxel / ln
            is_hit = present & ok & have & (s0 >= 0) & (s < 0)
            is_behind = present & ok & have & (s0 < 0) & (s >= 0)
            th_new = t0 + (t - t0) * (s0 / (s0 - s))
            t_valid = t + np.fmax(F(0.5) * np.abs(s) * trunc, min_m) / ln
            assert t_absent.dtype == F and t_valid.dtype == F and th_new.dtype == F
            new_hit, new_behind = active & is_hit, active & is_behind
            th = np.where(new_hit, th_new, th)
            hit |= new_hit
            behind |= new_behind
            go = active & ~is_hit & ~is_behind
            keep = go & present & ok                              # this sample becomes the one before
            t0, s0 = np.where(keep, t, t0), np.where(keep, s, s0)
            have = np.where(go, present & ok, have)
            t = np.where(go, np.where(~present, t_absent, np.where(ok, t_valid, t_invalid)), t)
            active = go
        left = ~hit & ~behind
        vtx = [np.where(hit, o[i] + d[i] * th, F(0)) for i in range(3)]
        h = F(0.5) * voxel
        taps, okn = [], hit.copy()
        for i in range(3):
            for sgn in (1, -1):
                q = [vtx[j] + h if (j == i and sgn > 0) else (vtx[j] - h if j == i else vtx[j]) for j in range(3)]
                ok, s = vol.sample(q[0], q[1], q[2], voxel, min_weight)
                okn &= ok
                taps.append(s)
        g = [taps[0] - taps[1], taps[2] - taps[3], taps[4] - taps[5]]
        norm = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
        okn &= norm > 0
        nrm = [np.where(okn, c / np.where(okn, norm, F(1)), F(0)) for c in g]
        assert norm.dtype == F and nrm[0].dtype == F
    no_normal = hit & ~okn
    hit = hit & okn
    out["depth"] = np.where(hit, th, F(0)).reshape(H, W)
    out["vertex"] = np.stack([np.where(hit, c, F(0)) for c in vtx], -1).reshape(H, W, 3)
    out["normal"] = np.stack(nrm, -1).reshape(H, W, 3)
    out.update(hits=int(hit.sum()), behind=int(behind.sum()), left_range=int(left.sum()), no_normal=int(no_normal.sum()))
    if colour:
        rgb = np.zeros((n, 3), np.int64)
        with np.errstate(all="ignore"):
            qi = [np.where(hit, np.floor(c / voxel), 0).astype(np.int64) for c in vtx]
        b, l = vol.voxel(*qi)
        bb = np.maximum(b, 0)
        if len(vol.key):
            cw = np.where(b >= 0, vol.state[bb, 2, l], 0)
            cwd = np.where(cw > 0, cw, 1)
            for j in range(3):
                rgb[:, j] = np.where(cw > 0, (vol.state[bb, 3 + j, l] + cwd // 2) // cwd, 128)
        else:
            rgb[:] = 128
        out["rgb"] = np.where(hit[:, None], rgb, 0).astype(np.uint8).reshape(H, W, 3)
    return out


# ---- the live maps ----------------------------------------------------------------------------------------
def vertex_normal(depth, K, max_depth, jump):
    """bf_depth_vertex_normal: (vertex f32 [H,W,3], normal f32 [H,W,3])"""
    depth = np.asarray(depth, F)
    H, W = depth.shape
    fx, fy, cx, cy = R.intrinsics(K)
    max_depth, jump = F(max_depth), F(jump)
    v, u = np.mgrid[:H, :W]
    xu, yv = u.astype(F) - cx, v.astype(F) - cy
    with np.errstate(all="ignore"):
        ok = (depth > 0) & (depth < max_depth)
        d = np.where(ok, depth, F(0))
        x, y = np.where(ok, xu * d / fx, F(0)), np.where(ok, yv * d / fy, F(0))        # +0 where invalid, not -0
        vert = np.stack([x, y, d], -1)
        dr, dd = np.zeros_like(depth), np.zeros_like(depth)
        dr[:, :-1], dd[:-1] = depth[:, 1:], depth[1:]
        inner = np.zeros((H, W), bool)
        inner[:-1, :-1] = True
        okr = (dr > 0) & (dr < max_depth) & (np.abs(dr - d) <= jump)
        okd = (dd > 0) & (dd < max_depth) & (np.abs(dd - d) <= jump)
        good = ok & inner & okr & okd
        dr, dd = np.where(good, dr, F(0)), np.where(good, dd, F(0))
        ax, ay, az = (xu + F(1.0)) * dr / fx - x, yv * dr / fy - y, dr - d
        bx, by, bz = xu * dd / fx - x, (yv + F(1.0)) * dd / fy - y, dd - d
        c = [by * az - bz * ay, bz * ax - bx * az, bx * ay - by * ax]
        ln = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
        good &= ln > 0
        c = [a / np.where(good, ln, F(1)) for a in c]
        flip = c[0] * x + c[1] * y + c[2] * d > 0
        nrm = np.stack([np.where(good, np.where(flip, -a, a), F(0)) for a in c], -1)
    assert vert.dtype == F and nrm.dtype == F
    return vert, nrm


# ---- the normal equations ---------------------------------------------------------------------------------
def icp_terms(lv, ln, stride, T, mv, mn, M, K, dist_max, cos_min):
    """bf_icp_reduce's per-sample terms in f64: (terms [n_inliers, 28], sampled pixels); a row is the 21 upper-
    triangle entries of J J^T, the 6 of J r and r^2"""
    lv, ln = np.asarray(lv, F)[::stride, ::stride].reshape(-1, 3).astype(D), \
        np.asarray(ln, F)[::stride, ::stride].reshape(-1, 3).astype(D)
    T, M = np.asarray(T, D).reshape(-1)[:12].reshape(3, 4), np.asarray(M, D).reshape(-1)[:12].reshape(3, 4)
    Hm, Wm = mv.shape[:2]
    fx, fy, cx, cy = [D(a) for a in R.intrinsics(K)]
    n_sampled = len(lv)
    x, y, z = lv.T
    nl = ln.T
    with np.errstate(all="ignore"):
        ok = ~((nl[0] == 0) & (nl[1] == 0) & (nl[2] == 0))
        p = [T[i, 0] * x + T[i, 1] * y + T[i, 2] * z + T[i, 3] for i in range(3)]
        q = [M[i, 0] * p[0] + M[i, 1] * p[1] + M[i, 2] * p[2] + M[i, 3] for i in range(3)]
        ok &= q[2] > 0
        qz = np.where(ok, q[2], 1.0)
        fu, fv = np.floor(fx * q[0] / qz + cx + 0.5), np.floor(fy * q[1] / qz + cy + 0.5)
        ok &= (fu >= 0) & (fu < Wm) & (fv >= 0) & (fv < Hm)
        iu, iv = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
        vm, nm = np.asarray(mv, F)[iv, iu].astype(D).T, np.asarray(mn, F)[iv, iu].astype(D).T
        ok &= ~((nm[0] == 0) & (nm[1] == 0) & (nm[2] == 0))
        e = [vm[i] - p[i] for i in range(3)]
        ok &= e[0] * e[0] + e[1] * e[1] + e[2] * e[2] <= D(dist_max) * D(dist_max)
        rn = [T[i, 0] * nl[0] + T[i, 1] * nl[1] + T[i, 2] * nl[2] for i in range(3)]
        ok &= rn[0] * nm[0] + rn[1] * nm[1] + rn[2] * nm[2] >= D(cos_min)
        r = nm[0] * e[0] + nm[1] * e[1] + nm[2] * e[2]
        J = [p[1] * nm[2] - p[2] * nm[1], p[2] * nm[0] - p[0] * nm[2], p[0] * nm[1] - p[1] * nm[0], nm[0], nm[1], nm[2]]
        cols = [J[a] * J[b] for a in range(6) for b in range(a, 6)] + [J[a] * r for a in range(6)] + [r * r]
    return np.stack(cols, -1)[ok], n_sampled


def icp_sums(terms):
    """out f64 [32] of bf_icp_reduce from icp_terms' rows (numpy's own summation order)"""
    out = np.zeros(32)
    out[:28] = terms.sum(0)
    out[28] = len(terms)
    return out


def se3_exp(xi):
    """the closed-form SE(3) exponential of xi = (omega, t) as a 4x4 f64 matrix"""
    w, t = np.asarray(xi[:3], D), np.asarray(xi[3:], D)
    th = np.sqrt(w @ w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-9:
        A, B, C = 1.0 - th * th / 6, 0.5 - th * th / 24, 1.0 / 6 - th * th / 120
    else:
        A, B, C = np.sin(th) / th, (1 - np.cos(th)) / (th * th), (th - np.sin(th)) / (th ** 3)
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + A * Wx + B * (Wx @ Wx)
    out[:3, 3] = (np.eye(3) + B * Wx + C * (Wx @ Wx)) @ t
    return out


def normal_matrix(out):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = out[:21]
    return A + np.triu(A, 1).T


def w2c(pose):
    """world-to-camera rows f64 [3,4] of a rigid camera-to-world pose"""
    P = np.asarray(pose, D).reshape(4, 4)
    Rt = P[:3, :3].T
    return np.concatenate([Rt, -(Rt @ P[:3, 3])[:, None]], 1)


def track(vol, depth, guess, K, voxel, T, max_depth, strides=(4, 2, 1), iters=(4, 4, 4), dist_max=None, cos_min=0.8,
          min_inlier_frac=0.4, cond_max=1000.0, jump=None, near=0.05, reduce=None):
    """IcpTracker.track in numpy: (pose f32 [4,4] or LOST, info)"""
    H, W = depth.shape
    dist_max = 4 * T * voxel if dist_max is None else dist_max
    jump = T * voxel if jump is None else jump
    model = raycast(vol, guess, K, H, W, voxel, T, near, max_depth)
    lv, ln = vertex_normal(depth, K, max_depth, jump)
    Tm = np.asarray(guess, F).astype(D)[:3].copy()
    M = w2c(np.asarray(guess, F))
    info = dict(lost=False, iterations=0, inliers=0, sampled=0, rms=float("inf"), cond=float("inf"))
    for stride, n_it in zip(strides, iters):
        for _ in range(n_it):
            terms, n_s = icp_terms(lv, ln, stride, Tm, model["vertex"], model["normal"], M, K, dist_max, cos_min)
            out = icp_sums(terms) if reduce is None else reduce(terms)
            info.update(iterations=info["iterations"] + 1, inliers=int(out[28]), sampled=n_s)
            if out[28] < 6 or out[28] < min_inlier_frac * n_s:
                info["lost"] = True
                return LOST.copy(), info
            A = normal_matrix(out)
            ev = np.linalg.eigvalsh(A)
            info["cond"] = float(ev[-1] / ev[0]) if ev[0] > 0 else float("inf")
            info["rms"] = float(np.sqrt(out[27] / out[28]))
            if not info["cond"] <= cond_max:
                info["lost"] = True
                return LOST.copy(), info
            xi = np.linalg.solve(A, out[21:27])
            Tm = (se3_exp(xi) @ np.concatenate([Tm, [[0, 0, 0, 1]]]))[:3]
    pose = np.eye(4, dtype=F)
    pose[:3] = Tm.astype(F)
    return pose, info


# ---- the box room -------------------------------------------------------------------------------------------
class Room:
    """an axis-aligned room lo .. hi seen from inside; a trajectory of cameras near the middle that look into one
    lower corner (two walls and the floor in view) and drift sideways while turning"""

    def __init__(self, H=48, W=64, focal=40.0, lo=(-1.0, -0.8, -0.6), hi=(0.9, 1.0, 0.7), frames=8):
        self.H, self.W = H, W
        self.K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1]], F)
        self.lo, self.hi = np.asarray(lo, D), np.asarray(hi, D)
        self.poses = []
        for i in range(frames):
            s = i / max(frames - 1, 1)
            eye = np.array([0.25 - 0.25 * s, 0.30 - 0.10 * s, 0.10 + 0.08 * s])
            target = np.array([-1.0 + 0.30 * s, -0.8 + 0.10 * s, -0.6 + 0.15 * s])
            self.poses.append(R.look_at(eye, target))

    def depth(self, pose, H=None, W=None, K=None):
        return render_room(pose, self.K if K is None else K, self.H if H is None else H, self.W if W is None else W,
                           self.lo, self.hi)

    def depths(self):
        return [self.depth(p) for p in self.poses]


def render_room(pose, K, H, W, lo, hi):
    """z-depth f32 [H,W] of the inside of the box lo .. hi from a camera inside it: per pixel the nearest exit
    through one of the six slabs, in float64 with the pose as the kernels get it (f32)"""
    P = np.asarray(pose, F).astype(D)
    fx, fy, cx, cy = [float(a) for a in R.intrinsics(K)]
    v, u = np.mgrid[:H, :W].astype(D)
    a, b = (u - cx) / fx, (v - cy) / fy
    best = np.full((H, W), np.inf)
    with np.errstate(all="ignore"):
        for i in range(3):
            d = P[i, 0] * a + P[i, 1] * b + P[i, 2]                                # per unit of z
            t = np.where(d > 0, (hi[i] - P[i, 3]) / d, np.where(d < 0, (lo[i] - P[i, 3]) / d, np.inf))
            best = np.minimum(best, np.where(t > 0, t, np.inf))
    return np.where(np.isfinite(best), best, 0.0).astype(F)


def plane_depth(H, W, K, dist=1.0):
    """a single wall facing the camera and filling the view"""
    return np.full((H, W), dist, F)


def pose_error(a, b):
    """(translation distance, rotation angle in degrees) between two poses"""
    a, b = np.asarray(a, D), np.asarray(b, D)
    dt = float(np.linalg.norm(a[:3, 3] - b[:3, 3]))
    rel = a[:3, :3].T @ b[:3, :3]
    # atan2 of the skew part and the trace: exact zero for equal matrices, where arccos of the trace alone turns the
    # f32 rounding of the rotation (1e-7) into 0.02 degrees
    sk = np.array([rel[2, 1] - rel[1, 2], rel[0, 2] - rel[2, 0], rel[1, 0] - rel[0, 1]]) / 2
    return dt, float(np.degrees(np.arctan2(np.linalg.norm(sk), (np.trace(rel) - 1) / 2)))


def perturb(pose, degrees, metres, seed=0):
    """pose moved by a rotation of `degrees` about a random axis and `metres` along a random direction"""
    rng = np.random.default_rng(seed)
    ax, dr = rng.normal(size=3), rng.normal(size=3)
    xi = np.concatenate([ax / np.linalg.norm(ax) * np.deg2rad(degrees), np.zeros(3)])
    out = np.asarray(pose, D).copy()
    out[:3, :3] = se3_exp(xi)[:3, :3] @ out[:3, :3]
    out[:3, 3] += dr / np.linalg.norm(dr) * metres
    return out.astype(F)


# ---- references shared by test_track_host.py and test_gpu_track.py (computed once) ---------------------------
import functools  # noqa: E402

ROOM_VOLUME = dict(voxel=0.05, T=3, max_depth=4.0)
TRACKER = dict(strides=(4, 2, 1), iters=(4, 4, 4), dist_max=0.6, cos_min=0.8, min_inlier_frac=0.4, cond_max=1000.0,
               jump=0.15)
LOST_FRAMES = (3, 4, 5)                                     # the frames `sens track --recover-lost` must bring back


def quantise_mm(depth):
    """a depth map through a .sens file: u16 millimetres, read back as SensFrameStream does (f32 / f32)"""
    mm = np.rint(np.asarray(depth, D) * 1000.0).astype(np.uint16)
    return mm, mm.astype(F) / F(1000.0)


def fuse_room(room, depths, poses):
    ref = R.fuse(depths, poses, room.K, ROOM_VOLUME["voxel"], ROOM_VOLUME["T"], ROOM_VOLUME["max_depth"])
    return Volume(ref["key"], ref["state"]), ref


def run_sequence(room, depths, known=None):
    """tracking.track_sequence in numpy: (poses [N,4,4], infos)"""
    poses, infos, used_d, used_p, last = [], [], [], [], None
    for i, d in enumerate(depths):
        if known is not None and np.isfinite(known[i]).all():
            pose, info = np.asarray(known[i], F), dict(lost=False, tracked=False)
        elif i == 0 and known is None:
            pose, info = room.poses[0], dict(lost=False, tracked=False)
        elif last is None:
            pose, info = LOST.copy(), dict(lost=True, tracked=False)
        else:
            vol, _ = fuse_room(room, used_d, used_p)
            pose, info = track(vol, d, last, room.K, ROOM_VOLUME["voxel"], ROOM_VOLUME["T"], ROOM_VOLUME["max_depth"],
                               **TRACKER)
            info["tracked"] = True
        poses.append(pose)
        infos.append(info)
        if not info["lost"]:
            used_d.append(d)
            used_p.append(pose)
            last = pose
    return np.stack(poses), infos


@functools.lru_cache(None)
def room_reference(mode):
    """the restatement's run over the room trajectory: mode 'scratch' (every frame tracked), 'known' (the poses of
    LOST_FRAMES unknown) or 'quantised' (as 'known', the depth through u16 millimetres): dict(room, depths, known,
    poses, infos)"""
    room = Room()
    depths = room.depths()
    known = None
    if mode == "quantised":
        depths = [quantise_mm(d)[1] for d in depths]
    if mode != "scratch":
        known = np.stack(room.poses)
        known[list(LOST_FRAMES)] = LOST
    poses, infos = run_sequence(room, depths, known)
    return dict(room=room, depths=depths, known=known, poses=poses, infos=infos)


def trajectory_errors(poses, truth):
    """(max translation error, max rotation error in degrees, final translation, final rotation) over the frames"""
    e = [pose_error(p, t) for p, t in zip(poses, truth)]
    return max(a for a, _ in e), max(b for _, b in e), e[-1][0], e[-1][1]


# the restatement's own largest |depth - analytic| in voxels over the six scene cameras (test_track_host.py),
# rounded up: with every one-surface pixel, and without the rays that pass another surface within its band
ANALYTIC_MAX_ALL, ANALYTIC_MAX = 35.1, 2.1
SCENE_VOLUME = dict(voxel=0.05, T=4, max_depth=3.5)          # as test_gpu_mesh.test_surface_sphere_48x64 fuses it


@functools.lru_cache(None)
def scene_reference(colour=False):
    """mesh_ref.Scene() fused, with the views the raycast tests look through: dict(scene, ref, vol, views [(name,
    pose, H, W, K, min_weight)], rgbs)"""
    sc = R.Scene()
    rng = np.random.default_rng(3)
    rgbs = [rng.integers(0, 256, (sc.H, sc.W, 3), dtype=np.uint8) for _ in sc.poses] if colour else None
    ref = R.fuse(sc.depths(), sc.poses, sc.K, SCENE_VOLUME["voxel"], SCENE_VOLUME["T"], SCENE_VOLUME["max_depth"], rgbs)
    views = [(f"camera{i}", p, sc.H, sc.W, sc.K, 1) for i, p in enumerate(sc.poses)]
    K_odd = np.array([[47.0, 0, 25.7], [0, 49.0, 18.2], [0, 0, 1]], F)
    views.append(("odd", sc.poses[1], 37, 53, K_odd, 1))
    views.append(("on_wall", sc.pose_on_wall(), sc.H, sc.W, sc.K, 1))
    # below the wall, looking further down: the wall and everything fused is behind the camera
    below = sc.centre + (sc.wall_at - 0.4) * sc.normal
    views.append(("behind_wall", R.look_at(below, below - sc.normal + np.array([0.05, 0.0, 0.0])), sc.H, sc.W, sc.K, 1))
    lost = sc.poses[2].copy()
    lost[1, 3] = -np.inf
    views.append(("lost_pose", lost, sc.H, sc.W, sc.K, 1))
    views.append(("heavy", sc.poses[0], sc.H, sc.W, sc.K, 1000))
    return dict(scene=sc, ref=ref, vol=Volume(ref["key"], ref["state"]), views=views, rgbs=rgbs)


@functools.lru_cache(None)
def scene_raycast(name, colour=False):
    s = scene_reference(colour)
    _, pose, H, W, K, mw = next(v for v in s["views"] if v[0] == name)
    return raycast(s["vol"], pose, K, H, W, SCENE_VOLUME["voxel"], SCENE_VOLUME["T"], 0.05, SCENE_VOLUME["max_depth"],
                   min_weight=mw, colour=colour)


def scene_surface_ids(sc, pose):
    """per pixel which of the scene's surfaces the ray meets first: 0 the wall, 1 the sphere, 2 the shell"""
    each = [R.render_depth(pose, sc.K, sc.H, sc.W, (sc.normal, sc.wall_at), None, None),
            R.render_depth(pose, sc.K, sc.H, sc.W, None, (sc.centre, sc.radius), None),
            R.render_depth(pose, sc.K, sc.H, sc.W, None, None, (sc.centre, sc.shell))]
    return np.stack([np.where(d > 0, d.astype(D), np.inf) for d in each]).argmin(0)


def one_surface(sid):
    """pixels whose 3 x 3 neighbourhood lies inside the image and on one surface"""
    same = np.zeros(sid.shape, bool)
    same[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            same &= np.roll(np.roll(sid, dy, 0), dx, 1) == sid
    return same


def analytic_error(sc, pose, depth):
    """(|depth - analytic| in voxels over the hit pixels of one_surface, the share of one_surface pixels within
    max_depth that are hits, the surface ids of those error pixels)"""
    an = sc.depth(pose)
    sid = scene_surface_ids(sc, pose)
    inner = one_surface(sid) & (an > 0) & (an < F(SCENE_VOLUME["max_depth"]))
    hit = np.asarray(depth) > 0
    sel = inner & hit
    err = np.abs(np.asarray(depth, D) - an.astype(D))[sel] / SCENE_VOLUME["voxel"]
    return err, float(sel.sum()) / max(int(inner.sum()), 1), sid[sel]


def outside_pose():
    """a camera outside the room, behind the wall x = lo, looking in: every ray enters the band from its inside"""
    return R.look_at([-1.3, -0.2, -0.2], [0.0, -0.3, -0.3])
