"""A numpy restatement of keyframe relocalisation with randomised ferns (bf_fern.hip, tracking.Relocaliser) for
test_fern_host.py and test_gpu_fern.py: the cell means of a frame, the fern codes, the code distance, the top-k
search, the conditional append, the harvest over a run of frames and `relocalise` on track_ref.track.  All of it
is integer arithmetic, so the kernels must give the same bits.  Plus the kidnap scene: track_ref.Room() with
photo_ref's texture, the eight trajectory frames, four views of the +x wall, and two new views near the trajectory
whose poses are unknown and which cannot be tracked from the last wall view."""
import functools

import numpy as np

from tests import mesh_ref as R
from tests import photo_ref as P
from tests import track_ref as TR

F = np.float32
LOST = TR.LOST


# ---- cell means --------------------------------------------------------------------------------------------------
def cell_means(depth, rgb, cell, max_depth):
    """i32 [Hc * Wc, 4] (R, G, B, D) of one frame: depth f32 [H,W] metres, rgb u8 [H,W,3] or None.  Colour: (2 S +
    n) // (2 n) over the n = cell^2 pixels; depth: millimetres rint(d * 1000.0f) of the m pixels with 0 < d <
    max_depth, (2 Sd + m) // (2 m) when 2 m >= n, else -1"""
    depth = np.asarray(depth, F)
    H, W = depth.shape
    c = int(cell)
    Hc, Wc = H // c, W // c
    if not 1 <= c <= 64 or Hc < 1 or Wc < 1:
        raise ValueError("cell_means: 1 <= cell <= 64 and at least one cell")
    n = c * c
    out = np.zeros((Hc, Wc, 4), np.int64)
    if rgb is not None:
        px = np.asarray(rgb, np.uint8)[:Hc * c, :Wc * c].astype(np.int64).reshape(Hc, c, Wc, c, 3)
        out[..., :3] = (2 * px.sum((1, 3)) + n) // (2 * n)
    d = depth[:Hc * c, :Wc * c]
    with np.errstate(all="ignore"):
        ok = (d > 0) & (d < F(max_depth))
        mm = np.rint(np.where(ok, d, F(0)) * F(1000.0))
    assert mm.dtype == F
    mm = mm.astype(np.int64).reshape(Hc, c, Wc, c)
    m = ok.reshape(Hc, c, Wc, c).sum((1, 3)).astype(np.int64)
    Sd = mm.sum((1, 3))
    out[..., 3] = np.where(2 * m >= n, (2 * Sd + m) // np.maximum(2 * m, 1), -1)
    return out.reshape(Hc * Wc, 4).astype(np.int32)


# ---- codes -------------------------------------------------------------------------------------------------------
def nibbles(means, table):
    """the ferns' nibbles u8 [F] of one frame's means under table i32 [F,5] (cell, tR, tG, tB, tD)"""
    table = np.asarray(table, np.int64)
    v = np.asarray(means, np.int64)[table[:, 0]]
    return ((v[:, 0] > table[:, 1]).astype(np.uint8) | ((v[:, 1] > table[:, 2]).astype(np.uint8) << 1)
            | ((v[:, 2] > table[:, 3]).astype(np.uint8) << 2) | (((v[:, 3] >= 0) & (v[:, 3] > table[:, 4])).astype(np.uint8) << 3))


def pack(nib):
    """nibbles u8 [F] -> code u32 [F / 8]: fern f at bits 4 (f mod 8) of word f / 8"""
    nib = np.asarray(nib, np.uint32).reshape(-1, 8)
    return (nib << (4 * np.arange(8, dtype=np.uint32))).sum(1, dtype=np.uint32)


def unpack(code):
    code = np.asarray(code, np.uint32)
    return ((code[:, None] >> (4 * np.arange(8, dtype=np.uint32))) & 15).astype(np.uint8).reshape(-1)


def encode(depth, rgb, cell, max_depth, table):
    """(code u32 [F / 8], means i32 [cells, 4]) of one frame"""
    means = cell_means(depth, rgb, cell, max_depth)
    return pack(nibbles(means, table)), means


# ---- distance and search -----------------------------------------------------------------------------------------
def distance(a, b):
    """the number of ferns whose nibbles differ, over the last axis of u32 codes"""
    x = np.asarray(a, np.uint32) ^ np.asarray(b, np.uint32)
    y = (x | (x >> 1) | (x >> 2) | (x >> 3)) & np.uint32(0x11111111)
    return np.unpackbits(np.ascontiguousarray(y)[..., None].view(np.uint8), axis=-1).sum((-1, -2)).astype(np.int32)


def search(codes, n, n_upper, queries, k):
    """(top i32 [Q, k, 2] of (distance, index) by distance then index, (-1, -1) beyond n; rows i32 [Q, n_upper]
    with -1 at and beyond n)"""
    queries = np.asarray(queries, np.uint32).reshape(len(queries), -1)
    rows = np.full((len(queries), n_upper), -1, np.int32)
    top = np.full((len(queries), k, 2), -1, np.int32)
    for q, code in enumerate(queries):
        if n:
            rows[q, :n] = distance(np.asarray(codes, np.uint32)[:n], code[None])
        order = sorted(range(n), key=lambda i: (rows[q, i], i))[:k]
        for r, i in enumerate(order):
            top[q, r] = rows[q, i], i
    return top, rows


class Table:
    """the keyframe table and its counters, as the device holds them"""

    def __init__(self, capacity, words):
        self.codes = np.zeros((capacity, words), np.uint32)
        self.poses = np.zeros((capacity, 16), F)
        self.ids = np.zeros(capacity, np.int32)
        self.n = self.observed = self.added = self.dropped_full = 0

    def append(self, code, best, threshold, pose, frame):
        """bf_fern_append: the code joins when the table is empty or its best distance exceeds threshold"""
        self.observed += 1
        if self.n and not best > threshold:
            return False
        if self.n == len(self.codes):
            self.dropped_full += 1
            return False
        self.codes[self.n], self.poses[self.n], self.ids[self.n] = code, np.asarray(pose, F).reshape(16), frame
        self.n += 1
        self.added += 1
        return True

    def counters(self):
        return dict(keyframes=self.n, observed=self.observed, added=self.added, dropped_full=self.dropped_full)


class Relocaliser:
    """tracking.Relocaliser in numpy, on track_ref.track"""

    def __init__(self, H, W, table, cell, capacity=4096, harvest=0.15, max_depth=10.0):
        self.table, self.cell, self.max_depth = np.asarray(table, np.int32), cell, max_depth
        self.ferns = len(self.table)
        self.threshold = int(np.floor(harvest * self.ferns))
        self.kf = Table(capacity, self.ferns // 8)

    def observe(self, depth, pose, rgb=None, frame=-1):
        if not np.isfinite(np.asarray(pose, F)).all():
            return
        code, _ = encode(depth, rgb, self.cell, self.max_depth, self.table)
        top, _ = search(self.kf.codes, self.kf.n, max(self.kf.n, 1), code[None], 1)
        self.kf.append(code, int(top[0, 0, 0]), self.threshold, pose, frame)

    def query(self, depth, rgb=None, k=4):
        code, _ = encode(depth, rgb, self.cell, self.max_depth, self.table)
        top, _ = search(self.kf.codes, self.kf.n, max(self.kf.n, 1), code[None], k)
        return [(int(d), int(i), self.kf.poses[i].reshape(4, 4).copy(), int(self.kf.ids[i])) for d, i in top[0] if i >= 0]

    def relocalise(self, track, depth, rgb=None, k=4, max_distance=0.5):
        """track(depth, guess) -> (pose, info), e.g. track_ref.track bound to a volume"""
        tried = 0
        info = dict(lost=True, iterations=0, inliers=0, sampled=0, rms=float("inf"), cond=float("inf"))
        for d, i, guess, _ in self.query(depth, rgb, k):
            if d > max_distance * self.ferns:
                break
            tried += 1
            pose, info = track(depth, guess)
            if not info["lost"]:
                return pose, dict(info, relocalised=True, keyframe=i, fern_distance=d, candidates_tried=tried)
        return LOST.copy(), dict(info, lost=True, relocalised=False, candidates_tried=tried)


# ---- the kidnap scene ----------------------------------------------------------------------------------------------
KIDNAP = dict(ferns=256, cell=4, harvest=0.1, depth_range=(0.4, 3.0), seed=0)


@functools.lru_cache(None)
def kidnap_scene(twice=False):
    """dict(room, poses (the truth), depths, rgbs, known [N,4,4] with -inf for the unknown frames, unknown): frames
    0-7 the trajectory, 8-11 the +x wall, then the two new views 12 and 13.  twice=True shows the last wall view (frame
    11, pose known) once more between them, so the camera is away again when the second new view arrives: the
    unknown frames are then 12 and 14, each to be found from poses[11]"""
    room = TR.Room()
    poses = list(room.poses)
    for i in range(4):
        poses.append(R.look_at((-0.03 * i, 0.1 + 0.03 * i, 0.1), (0.9, 0.1 + 0.05 * i, 0.1 + 0.02 * i)))
    new = [TR.perturb(room.poses[2], 4.0, 0.06, seed=1), TR.perturb(room.poses[5], 6.0, 0.10, seed=2)]
    unknown = (12, 14) if twice else (12, 13)
    poses += [new[0], poses[11], new[1]] if twice else new
    depths = [room.depth(p) for p in poses]
    rgbs = [P.render_texture(p, room.K, d) for p, d in zip(poses, depths)]
    known = np.stack(poses)
    known[list(unknown)] = LOST
    return dict(room=room, poses=poses, depths=depths, rgbs=rgbs, known=known, unknown=unknown)


def kidnap_table():
    from boxfusion_amd.tracking import fern_table
    room = TR.Room()
    cells = (room.H // KIDNAP["cell"]) * (room.W // KIDNAP["cell"])
    return fern_table(KIDNAP["ferns"], cells, KIDNAP["seed"], KIDNAP["depth_range"])


def run_sequence(scene, depths, rgbs, known, table=None, relocalise=True, k=4, max_distance=0.5):
    """tracking.track_sequence(..., relocaliser=...) in numpy over the scene's frames: (poses [N,4,4], infos, the
    Relocaliser)"""
    V = TR.ROOM_VOLUME
    room = scene
    rl = Relocaliser(room.H, room.W, kidnap_table() if table is None else table, KIDNAP["cell"], harvest=KIDNAP["harvest"],
                     max_depth=V["max_depth"]) if relocalise else None
    poses, infos, used_d, used_p, last = [], [], [], [], None
    for i, d in enumerate(depths):
        if np.isfinite(known[i]).all():
            pose, info = np.asarray(known[i], F), dict(lost=False, tracked=False)
        elif last is None:
            pose, info = LOST.copy(), dict(lost=True, tracked=False)
        else:
            vol, _ = TR.fuse_room(room, used_d, used_p)

            def track(depth, guess):
                return TR.track(vol, depth, guess, room.K, V["voxel"], V["T"], V["max_depth"], **TR.TRACKER)
            pose, info = track(d, last)
            info["tracked"] = True
            if rl is not None:
                info["relocalised"] = False
                if info["lost"]:
                    pose, more = rl.relocalise(track, d, rgbs[i], k, max_distance)
                    info = dict(more, tracked=True, first=info)
        if rl is not None:
            info.setdefault("relocalised", False)
        poses.append(pose)
        infos.append(info)
        if not info["lost"]:
            used_d.append(d)
            used_p.append(pose)
            last = pose
            if rl is not None:
                rl.observe(d, pose, rgbs[i], i)
    return np.stack(poses), infos, rl


@functools.lru_cache(None)
def kidnap_reference(twice=False, relocalise=True):
    """the restatement's run over the kidnap scene: kidnap_scene's dict with got (poses), infos and rl"""
    s = kidnap_scene(twice)
    poses, infos, rl = run_sequence(s["room"], s["depths"], s["rgbs"], s["known"], relocalise=relocalise)
    return dict(s, got=poses, infos=infos, rl=rl)
