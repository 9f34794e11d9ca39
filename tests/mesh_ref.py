"""A numpy restatement of the scene mesh (bf_tsdf.hip), for test_mesh_host.py and test_gpu_mesh.py: f32
arrays and the kernels' operation order, np.rint, integer sums, the same vertex and face orders.  Plus
the analytic scene the tests fuse: a tilted wall and a sphere inside a shell (so that every ray ends on a
surface and the free space beside the sphere is seen as free), rendered to depth maps in float64."""
import numpy as np

F = np.float32
BIAS = 1 << 20
MASK = (1 << 21) - 1
MAX_WEIGHT = 1 << 20


def block_key(b):
    b = np.asarray(b, np.int64) + BIAS
    return (b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2]


def key_block(key):
    key = np.asarray(key, np.int64)
    return np.stack([(key >> 42) & MASK, (key >> 21) & MASK, key & MASK], -1) - BIAS


def intrinsics(K):
    K = np.asarray(K, F).reshape(3, 3)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def touched_blocks(depth, pose, K, voxel, T, max_depth):
    """bf_tsdf_touch for one frame: (sorted unique block keys, samples out of range), or (None, 0)
    for a pose with a non-finite entry"""
    P = np.asarray(pose, F).reshape(4, 4)
    if not np.isfinite(P).all():
        return None, 0
    fx, fy, cx, cy = intrinsics(K)
    voxel, depth = F(voxel), np.asarray(depth, F)
    H, W = depth.shape
    v, u = np.mgrid[:H, :W]
    with np.errstate(invalid="ignore"):
        live = (depth > 0) & (depth < F(max_depth))
    d = depth[live]
    xu, yv = u[live].astype(F) - cx, v[live].astype(F) - cy
    bs = F(8.0) * voxel
    keys, oor = [], 0
    for k in range(-T, T + 1):
        z = d + F(k) * voxel
        xc, yc = xu * z / fx, yv * z / fy
        b = np.stack([np.floor((P[r, 0] * xc + P[r, 1] * yc + P[r, 2] * z + P[r, 3]) / bs) for r in range(3)], -1)
        assert b.dtype == F
        ok = ((b >= -F(BIAS)) & (b < F(BIAS))).all(-1)
        oor += int((~ok).sum())
        keys.append(block_key(b[ok].astype(np.int64)))
    return np.unique(np.concatenate(keys)) if keys else np.zeros(0, np.int64), oor


def update_blocks(state, keys, depth, pose, K, voxel, T, max_depth, rgb=None, max_weight=MAX_WEIGHT, seen=None):
    """bf_tsdf_update's work for one frame on the blocks `keys` (int64 [n]) with state int64 [n,6,512],
    in place; returns (observations, saturated).  seen: a dict that counts the voxels behind the camera
    and those that project outside the image"""
    P = np.asarray(pose, F).reshape(4, 4)
    fx, fy, cx, cy = intrinsics(K)
    voxel, depth = F(voxel), np.asarray(depth, F)
    H, W = depth.shape
    trunc = F(T) * voxel
    t = np.arange(512)
    local = np.stack([t & 7, (t >> 3) & 7, t >> 6], -1)
    i = key_block(keys)[:, None, :] * 8 + local[None]                          # [n,512,3]
    p = (i.astype(F) + F(0.5)) * voxel
    dx, dy, dz = p[..., 0] - P[0, 3], p[..., 1] - P[1, 3], p[..., 2] - P[2, 3]
    z = P[0, 2] * dx + P[1, 2] * dy + P[2, 2] * dz
    x = P[0, 0] * dx + P[1, 0] * dy + P[2, 0] * dz
    y = P[0, 1] * dx + P[1, 1] * dy + P[2, 1] * dz
    assert z.dtype == F
    with np.errstate(all="ignore"):
        ok = z > 0
        zs = np.where(ok, z, F(1))
        fu, fv = np.floor(fx * x / zs + cx + F(0.5)), np.floor(fy * y / zs + cy + F(0.5))
        if seen is not None:
            seen["behind"] = seen.get("behind", 0) + int((~ok).sum())
            seen["outside"] = seen.get("outside", 0) + int((ok & ~((fu >= 0) & (fu < F(W)) & (fv >= 0) & (fv < F(H)))).sum())
        ok &= (fu >= 0) & (fu < F(W)) & (fv >= 0) & (fv < F(H))
        pu, pv = np.where(ok, fu, 0).astype(np.int64), np.where(ok, fv, 0).astype(np.int64)
        d = depth[pv, pu]
        ok &= (d > 0) & (d < F(max_depth))
        sdf = np.where(ok, d - z, F(0))
        ok &= ~(sdf < -trunc)
        q = np.rint(np.minimum(sdf / trunc, F(1.0)) * F(1024.0)).astype(np.int64)
    w = state[:, 0]
    refused = ok & (w >= max_weight)
    ok &= ~refused
    state[:, 0] += ok
    state[:, 1] += np.where(ok, q, 0)
    if rgb is not None:
        col = ok & (sdf <= trunc)
        c = np.asarray(rgb, np.uint8)[pv, pu].astype(np.int64)                 # [n,512,3]
        state[:, 2] += col
        for j in range(3):
            state[:, 3 + j] += np.where(col, c[..., j], 0)
    return int(ok.sum()), int(refused.sum())


def fuse(depths, poses, K, voxel, T, max_depth, rgbs=None, max_weight=MAX_WEIGHT, seen=None):
    """TsdfVolume.integrate over the frames, one at a time, with room for every block: dict(key int64
    [n] sorted, state int64 [n,6,512], observations, skipped_pose, out_of_range, saturated)"""
    touched = [touched_blocks(d, p, K, voxel, T, max_depth) for d, p in zip(depths, poses)]
    sets = [t[0] for t in touched if t[0] is not None]
    key = np.unique(np.concatenate(sets)) if sets else np.zeros(0, np.int64)
    state = np.zeros((len(key), 6, 512), np.int64)
    obs = sat = 0
    for j, (ks, _) in enumerate(touched):
        if ks is None or not len(ks):
            continue
        at = np.searchsorted(key, ks)
        part = state[at]
        o, s = update_blocks(part, ks, depths[j], poses[j], K, voxel, T, max_depth,
                             None if rgbs is None else rgbs[j], max_weight, seen)
        state[at] = part
        obs, sat = obs + o, sat + s
    return dict(key=key, state=state, observations=obs, saturated=sat,
                skipped_pose=sum(t[0] is None for t in touched), out_of_range=sum(t[1] for t in touched))


CORNERS = np.array([[c & 1, (c >> 1) & 1, c >> 2] for c in range(8)])
# the twelve edges in the order the crossings are summed: four along x, four along y, four along z
EDGES = [(ax, ca, ca + (1 << ax)) for ax in range(3)
         for ca in ([0, 2, 4, 6], [0, 1, 4, 5], [0, 1, 2, 3])[ax]]


def surface(key, state, voxel):
    """naive surface nets over the blocks (key sorted, state [n,6,512]): (vertices f32 [nv,3], rgb u8
    [nv,3], faces int32 [nf,3]) in bf_tsdf_surface_write's orders"""
    voxel = F(voxel)
    none = (np.zeros((0, 3), F), np.zeros((0, 3), np.uint8), np.zeros((0, 3), np.int32))
    if not len(key):
        return none
    blocks = key_block(key)
    org = blocks.min(0) - 1                                                    # a block of margin below, one above
    dims = (blocks.max(0) - org + 2) * 8
    grid = np.zeros((6, *dims), np.int64)
    order = np.full(tuple(dims // 8), -1, np.int64)                            # a block's position in `key`
    for n, b in enumerate(blocks - org):
        # state's voxel index is x + 8 y + 64 z
        grid[:, b[0] * 8:b[0] * 8 + 8, b[1] * 8:b[1] * 8 + 8, b[2] * 8:b[2] * 8 + 8] = \
            state[n].reshape(6, 8, 8, 8).transpose(0, 3, 2, 1)
        order[tuple(b)] = n
    w, sq, cw = grid[0], grid[1], grid[2]
    has = w > 0
    s = np.where(has, sq.astype(F) / np.where(has, w, 1).astype(F), F(0))
    assert s.dtype == F
    inside = has & (s < 0)
    cwd = np.where(cw > 0, cw, 1)
    mean_rgb = np.stack([(grid[3 + j] + cwd // 2) // cwd for j in range(3)], -1)
    X, Y, Z = dims - 1

    def at(a, c):
        return a[c[0]:c[0] + X, c[1]:c[1] + Y, c[2]:c[2] + Z]
    valid = np.ones((X, Y, Z), bool)
    n_in = np.zeros((X, Y, Z), np.int64)
    for c in CORNERS:
        valid &= at(has, c)
        n_in += at(inside, c)
    active = valid & (n_in > 0) & (n_in < 8)
    cells = np.argwhere(active)                                                # [nv,3] grid coordinates
    if not len(cells):
        return none
    cb, cl = cells // 8, cells % 8
    rank = order[cb[:, 0], cb[:, 1], cb[:, 2]]
    assert (rank >= 0).all()
    srt = np.lexsort((cl[:, 0] + 8 * cl[:, 1] + 64 * cl[:, 2], rank))
    cells = cells[srt]
    vid = np.full((X, Y, Z), -1, np.int64)
    vid[cells[:, 0], cells[:, 1], cells[:, 2]] = np.arange(len(cells))

    def corner(a, c):
        g = cells + CORNERS[c]
        return a[g[:, 0], g[:, 1], g[:, 2]]
    sv = [corner(s, c) for c in range(8)]
    acc = [np.zeros(len(cells), F) for _ in range(3)]
    ne = np.zeros(len(cells), np.int64)
    with np.errstate(all="ignore"):
        for ax, ca, cb_ in EDGES:
            a, b = sv[ca], sv[cb_]
            cross = (a < 0) != (b < 0)
            t = a / (a - b)
            for j in range(3):
                add = t if j == ax else np.full(len(cells), F(CORNERS[ca][j]))
                acc[j] = np.where(cross, acc[j] + add, acc[j])
            ne += cross
        idx = cells + org * 8
        verts = np.stack([((idx[:, j].astype(F) + F(0.5)) + acc[j] / ne.astype(F)) * voxel for j in range(3)], -1)
    assert verts.dtype == F
    csum, cn = np.zeros((len(cells), 3), np.int64), np.zeros(len(cells), np.int64)
    for c in range(8):
        hc = corner(cw, c) > 0
        csum += np.where(hc[:, None], corner(mean_rgb, c), 0)
        cn += hc
    cnd = np.where(cn > 0, cn, 1)[:, None]
    rgb = np.where(cn[:, None] > 0, (csum + cnd // 2) // cnd, 128).astype(np.uint8)
    # a quad per sign-changing edge from a vertex cell's minimum corner whose four cells have vertices
    faces = []
    for ax in range(3):
        e = np.eye(3, dtype=np.int64)
        eb, ec = e[(ax + 1) % 3], e[(ax + 2) % 3]
        in0 = sv[0] < 0
        change = in0 != (sv[1 << ax] < 0)
        quad = []
        for off in (0 * eb, -eb, -eb - ec, -ec):
            g = cells + off                                                    # the margin keeps this inside the grid
            quad.append(vid[g[:, 0], g[:, 1], g[:, 2]])
        quad = np.stack(quad, -1)
        keep = change & (quad >= 0).all(-1)
        v0, v2 = quad[:, 0], quad[:, 2]
        v1, v3 = np.where(in0, quad[:, 1], quad[:, 3]), np.where(in0, quad[:, 3], quad[:, 1])
        tri = np.stack([v0, v1, v2, v0, v2, v3], -1)
        faces.append((np.nonzero(keep)[0], np.full(int(keep.sum()), ax), tri[keep]))
    cell_i = np.concatenate([f[0] for f in faces])
    axis_i = np.concatenate([f[1] for f in faces])
    tris = np.concatenate([f[2] for f in faces])
    tris = tris[np.lexsort((axis_i, cell_i))].reshape(-1, 3).astype(np.int32)
    return verts, rgb, tris


# ---- the analytic scene ------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """camera-to-world pose (x right, y down, z forward) of a camera at eye looking at target"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(up, np.float64))
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = right, down, fwd, eye
    return P.astype(F)


def render_depth(pose, K, H, W, plane=None, sphere=None, shell=None):
    """the z-depth f32 [H,W] of the nearest of a plane (n, d: n . x = d), a sphere (centre, radius) seen
    from outside and a shell (centre, radius) seen from inside along each pixel's ray, 0 where none is
    hit; float64 inside, the pose as the kernels get it (f32)"""
    P = np.asarray(pose, F).astype(np.float64)
    fx, fy, cx, cy = [float(a) for a in intrinsics(K)]
    v, u = np.mgrid[:H, :W].astype(np.float64)
    a_, b_ = (u - cx) / fx, (v - cy) / fy

    def dot(p, q):                                  # elementwise, so the same bits on every machine
        return p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1] + p[..., 2] * q[..., 2]
    dirs = np.stack([P[i, 0] * a_ + P[i, 1] * b_ + P[i, 2] for i in range(3)], -1)         # per unit of z
    o = P[:3, 3]
    best = np.full((H, W), np.inf)
    if plane is not None:
        n, d = np.asarray(plane[0], np.float64), float(plane[1])
        with np.errstate(all="ignore"):
            t = (d - dot(n, o)) / dot(dirs, n)
        best = np.where((t > 0) & np.isfinite(t), np.minimum(best, t), best)
    if sphere is not None:
        c, r = np.asarray(sphere[0], np.float64), float(sphere[1])
        oc = o - c
        a, b, cc = dot(dirs, dirs), 2 * dot(dirs, oc), dot(oc, oc) - r * r
        disc = b * b - 4 * a * cc
        with np.errstate(all="ignore"):
            t = (-b - np.sqrt(disc)) / (2 * a)
        best = np.where((disc > 0) & (t > 0), np.minimum(best, t), best)
    if shell is not None:
        c, r = np.asarray(shell[0], np.float64), float(shell[1])
        oc = o - c
        a, b, cc = dot(dirs, dirs), 2 * dot(dirs, oc), dot(oc, oc) - r * r
        best = np.minimum(best, (-b + np.sqrt(b * b - 4 * a * cc)) / (2 * a))          # the camera is inside
    return np.where(np.isfinite(best), best, 0.0).astype(F)


def rotation(axis, degrees):
    a = np.deg2rad(degrees)
    c, s = np.cos(a), np.sin(a)
    m = np.eye(3)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


class Scene:
    """a sphere of radius 8 voxels (by default) just off the origin, a tilted wall `wall_at` below it and a shell of
    radius 2 m around both; six cameras on a rotated octahedron `dist` from the sphere, looking at it"""

    def __init__(self, voxel=0.05, H=48, W=64, focal=60.0, dist=1.2, wall_at=-1.2, shell=2.0, radius_voxels=8):
        self.voxel, self.H, self.W = voxel, H, W
        self.K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1]], F)
        self.centre, self.radius = np.array([0.013, -0.021, 0.017]), radius_voxels * voxel
        n = np.array([0.2, 0.1, 1.0])
        self.normal, self.wall_at, self.shell = n / np.sqrt((n * n).sum()), wall_at, shell
        Q = rotation(2, 20) @ rotation(0, 15)
        self.poses = [look_at(self.centre + dist * (Q @ d), self.centre, up=Q @ np.roll(d, 1))
                      for d in np.concatenate([np.eye(3), -np.eye(3)])]

    def pose_on_wall(self, height=0.15):
        """a camera `height` above the wall that looks along it: the blocks its nearest pixels touch
        reach behind it and past the image's edges"""
        n = self.normal
        foot = self.centre + np.array([0.2, 0.1, 0.0])
        foot = foot - (foot @ n - self.wall_at) * n
        along = np.cross(n, [0.0, 1.0, 0.0])
        eye = foot + height * n
        return look_at(eye, eye + along / np.sqrt((along * along).sum()) - 0.35 * n)

    def depth(self, pose, wall=True, sphere=True):
        return render_depth(pose, self.K, self.H, self.W, (self.normal, self.wall_at) if wall else None,
                            (self.centre, self.radius) if sphere else None, (self.centre, self.shell))

    def depths(self):
        return [self.depth(p) for p in self.poses]
