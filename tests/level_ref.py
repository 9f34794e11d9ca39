"""A numpy restatement of levelling (bf_level.hip, include/boxfusion_level.h) for test_level_host.py and
test_gpu_level.py: f32 where the kernels are f32 and in their operation order, np.rint, integer sums.  The host side
is not restated: `Samples` below offers what scene_level.DeviceSamples offers, and scene_level.procedure runs over
either, so equal sums give equal transforms.  Plus the scenes the tests level: track_ref.Room fused and meshed by
mesh_ref, tilted rigidly."""
import functools

import numpy as np

from boxfusion_amd import _abi
from boxfusion_amd import scene_level as SL
from tests import mesh_ref as R
from tests import track_ref as TR

F, D = np.float32, np.float64
HEADER = _abi.EXTENSION_HEADERS[1]
C = _abi.constants(header=HEADER)
STATS = _abi.enum_names("BF_LEVEL_STAT_", header=HEADER)
CAP, STATS_WORDS, SUM_WORDS, HEIGHT_WORDS = (C["BF_LEVEL_" + n] for n in ("WEIGHT_CAP", "STATS_WORDS", "SUM_WORDS", "HEIGHT_WORDS"))
NSCALE, MSCALE, LIMIT = F(1 << C["BF_LEVEL_NORMAL_SHIFT"]), F(1 << C["BF_LEVEL_METRE_SHIFT"]), F(C["BF_LEVEL_COORD_LIMIT"])


def _stats(**named):
    out = np.zeros(STATS_WORDS, np.int64)
    for k, v in named.items():
        out[STATS.index(k)] = int(v)
    return out


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def face_samples(vertices, faces, area_unit):
    """bf_level_face_samples: (centroids f32 [m,3], normals f32 [m,3], weights uint32 [m], stats int64)"""
    v, f = np.asarray(vertices, F).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)
    m = len(f)
    bad = ((f < 0) | (f >= len(v))).any(1)
    g = np.where(bad[:, None], 0, f)
    if len(v):
        a, b, c = v[g[:, 0]], v[g[:, 1]], v[g[:, 2]]
    else:
        a = b = c = np.zeros((m, 3), F)
    with np.errstate(all="ignore"):
        e, q = b - a, c - a
        x = np.stack([e[:, 1] * q[:, 2] - e[:, 2] * q[:, 1], e[:, 2] * q[:, 0] - e[:, 0] * q[:, 2],
                      e[:, 0] * q[:, 1] - e[:, 1] * q[:, 0]], -1)
        ln = np.sqrt((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
        nonfinite = ~bad & ~(np.isfinite(a).all(1) & np.isfinite(b).all(1) & np.isfinite(c).all(1) & np.isfinite(ln))
        zero = ~bad & ~nonfinite & (ln == 0)
        good = ~bad & ~nonfinite & ~zero
        normal = x / ln[:, None]
        centroid = ((a + b) + c) / F(3.0)
        r = np.rint((F(0.5) * ln) / F(area_unit))
        assert normal.dtype == F and centroid.dtype == F and r.dtype == F
        capped = good & (r > F(CAP))
        w = np.where(good, np.where(capped, CAP, np.where(good & ~capped, r, 0)), 0).astype(np.uint32)
    normal[~good], centroid[~good] = np.nan, np.nan
    return centroid, normal, w, _stats(faces=m, face_bad_index=bad.sum(), face_nonfinite=nonfinite.sum(),
                                       face_zero_area=zero.sum(), face_saturated=capped.sum())


def bins_of(normals, G):
    """the bin of every normal that is finite and not zero (others: -1)"""
    n = np.asarray(normals, F).reshape(-1, 3)
    use = np.isfinite(n).all(1) & (n != 0).any(1)
    ab = np.abs(n)
    k = np.where((ab[:, 0] >= ab[:, 1]) & (ab[:, 0] >= ab[:, 2]), 0, np.where(ab[:, 1] >= ab[:, 2], 1, 2))
    major = np.take_along_axis(n, k[:, None], 1)[:, 0]
    p, q = np.where(k == 0, n[:, 1], n[:, 0]), np.where(k == 2, n[:, 1], n[:, 2])
    with np.errstate(all="ignore"):
        u, v = p / major, q / major
        half = F(0.5) * F(G)
        fu, fv = np.floor((u + F(1.0)) * half), np.floor((v + F(1.0)) * half)
        assert fu.dtype == F
    iu = np.minimum(np.where(use, fu, 0).astype(np.int64), G - 1)
    iv = np.minimum(np.where(use, fv, 0).astype(np.int64), G - 1)
    face = 2 * k + (major < 0)
    return np.where(use, (face * G + iv) * G + iu, -1)


def vote(normals, weights, G):
    """bf_level_vote: (hist int64 [6 G G], stats)"""
    w = np.asarray(weights).astype(np.uint32).reshape(-1).astype(np.int64)
    b = bins_of(normals, G)
    use = (b >= 0) & (w != 0)
    hist = np.zeros(6 * G * G, np.int64)
    np.add.at(hist, b[use], w[use])
    return hist, _stats(vote_samples=len(w), vote_skipped=(~use).sum(), vote_weight=w[use].sum())


def score(hist, G, candidates, cos_par, sin_perp):
    """bf_level_score: int64 [k,2]"""
    d = SL.bin_directions(G)
    cand = np.asarray(candidates, np.int64).reshape(-1)
    out = np.zeros((len(cand), 2), np.int64)
    for j, cb in enumerate(cand):
        if not 0 <= cb < len(d):
            continue
        a = np.abs(dot(d[cb][None], d))
        assert a.dtype == F
        out[j] = hist[a >= F(cos_par)].sum(), hist[a <= F(sin_perp)].sum()
    return out


def fix(v, scale):
    assert v.dtype == F
    return np.rint(v * scale).astype(np.int64)


def refine(points, normals, weights, frame, cos_par, sin_perp, h0=0.0, height_bin=1.0, n_bins=0):
    """bf_level_refine: (sums int64 [SUM_WORDS], heights int64 [n_bins,HEIGHT_WORDS], stats)"""
    p, n = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
    w = np.asarray(weights).astype(np.uint32).reshape(-1).astype(np.int64)
    fr = np.asarray(frame, F).reshape(3, 3)
    c, e1, e2 = fr[0][None], fr[1][None], fr[2][None]
    cos_par, sin_perp, h0, height_bin = F(cos_par), F(sin_perp), F(h0), F(height_bin)
    use = (w != 0) & np.isfinite(p).all(1) & np.isfinite(n).all(1)
    p, n = np.where(use[:, None], p, F(0)), np.where(use[:, None], n, F(0))
    sums = np.zeros(SUM_WORDS, np.int64)
    heights = np.zeros((n_bins, HEIGHT_WORDS), np.int64)
    with np.errstate(all="ignore"):
        t = dot(n, c)
        par, perp, up = use & (np.abs(t) >= cos_par), use & (np.abs(t) <= sin_perp), use & (t >= cos_par)
        pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        q = np.stack([fix(n[:, i] * n[:, j], NSCALE) * w for i, j in pairs], -1)
        sums[0:6], sums[6:12] = q[par].sum(0), q[perp].sum(0)
        pa, pb = dot(n, e1), dot(n, e2)
        r = np.sqrt(pa * pa + pb * pb)
        yaw = perp & (r > 0)
        rs = np.where(yaw, r, F(1))
        a, b = pa / rs, pb / rs
        a2, b2 = a * a, b * b
        sums[12] = (fix(F(1.0) - (F(8.0) * a2) * b2, NSCALE) * w)[yaw].sum()
        sums[13] = (fix(((F(4.0) * a) * b) * (a2 - b2), NSCALE) * w)[yaw].sum()
        inside = np.zeros(len(w), bool)
        if n_bins > 0:
            d = dot(p, c) - h0
            fb = np.floor(d / height_bin)
            x1, x2 = dot(p, e1), dot(p, e2)
            assert fb.dtype == F and x1.dtype == F
            inside = up & (d >= 0) & (fb < F(n_bins)) & (np.abs(x1) < LIMIT) & (np.abs(x2) < LIMIT)
            rows = fb[inside].astype(np.int64)
            for word, val in enumerate((w, fix(d, MSCALE) * w, fix(x1, MSCALE) * w, fix(x2, MSCALE) * w)):
                np.add.at(heights[:, word], rows, val[inside])
    return sums, heights, _stats(refine_samples=len(w), refine_skipped=(~use).sum(), refine_par=par.sum(),
                                 refine_perp=perp.sum(), refine_up=up.sum(), refine_outside=(up & ~inside).sum(),
                                 refine_weight=w[use].sum(), refine_weight_par=w[par].sum(),
                                 refine_weight_perp=w[perp].sum(), refine_weight_up=w[up].sum())


class Samples:
    """scene_level.DeviceSamples in numpy"""

    def __init__(self):
        self.p = self.n = self.w = self.face_stats = None

    def load(self, points, normals, weights):
        self.p, self.n = np.asarray(points, F).reshape(-1, 3), np.asarray(normals, F).reshape(-1, 3)
        self.w = np.asarray(weights).astype(np.uint32).reshape(-1)
        return self

    def face_samples(self, vertices, faces, area_unit):
        self.p, self.n, self.w, self.face_stats = face_samples(vertices, faces, area_unit)
        return self

    def bounds(self):
        fin = np.isfinite(self.p).all(1)
        return (self.p[fin].min(0), self.p[fin].max(0)) if fin.any() else None

    def vote(self, G):
        return vote(self.n, self.w, G)

    def score(self, hist, G, candidates, cos_par, sin_perp):
        return score(hist, G, candidates, cos_par, sin_perp)

    def refine(self, frame, cos_par, sin_perp, h0, height_bin, n_bins):
        return refine(self.p, self.n, self.w, frame, cos_par, sin_perp, h0, height_bin, n_bins)


def estimate(points, normals, weights, prior=None, **args):
    return SL.estimate(points, normals, weights, prior, backend=Samples(), **args)


def level_mesh(mesh, poses=None, prior=None, first_pose=None, **args):
    return SL.level_mesh(mesh, poses, prior, first_pose, backend=Samples(), **args)


# ---- the scenes ------------------------------------------------------------------------------------------------
VOXEL = TR.ROOM_VOLUME["voxel"]
TILTS = (0.0, 15.0, 30.0, 40.0)


def tilt_transform(degrees, seed):
    """a rigid transform f64 [4,4]: a rotation of `degrees` about a seeded random axis and a seeded translation"""
    rng = np.random.default_rng(seed)
    ax, t = rng.normal(size=3), rng.uniform(-0.5, 0.5, size=3)
    ax /= np.linalg.norm(ax)
    A = TR.se3_exp(np.concatenate([ax * np.deg2rad(degrees), np.zeros(3)]))
    A[:3, 3] = t
    return A


@functools.lru_cache(None)
def room_mesh(degrees=0.0, seed=0):
    """track_ref.Room with the whole scene (cameras included) moved by tilt_transform, fused and meshed by mesh_ref at
    ROOM_VOLUME: dict(room, A, poses f32 [8,4,4], fused, vertices, faces)"""
    room = TR.Room()
    A = tilt_transform(degrees, seed)
    poses = np.stack([(A @ np.asarray(p, D)).astype(F) for p in room.poses])
    fused = R.fuse(room.depths(), poses, room.K, VOXEL, TR.ROOM_VOLUME["T"], TR.ROOM_VOLUME["max_depth"])
    v, _, f = R.surface(fused["key"], fused["state"], VOXEL)
    return dict(room=room, A=A, poses=poses, fused=fused, vertices=v, faces=f)


def room_errors(lv, A, room):
    """(up error in degrees, wall-direction error mod 90 in degrees, floor error in voxels) of a Levelling of the room
    moved by A"""
    up_true = A[:3, :3] @ np.array([0.0, 0.0, 1.0])
    up_err = np.degrees(np.arccos(np.clip(lv.up @ up_true, -1, 1)))
    ax = A[:3, :3].T @ lv.axis                                   # in the room's own frame: should be +-x or +-y
    ang = np.degrees(np.arctan2(ax[1], ax[0])) % 90.0
    wall_err = min(ang, 90.0 - ang)
    floor_true = up_true @ (A[:3, :3] @ np.array([0.0, 0.0, room.lo[2]]) + A[:3, 3])
    return float(up_err), float(wall_err), float(abs(lv.floor - floor_true) / VOXEL)
