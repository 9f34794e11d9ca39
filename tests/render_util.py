"""A numpy restatement of the renderer's three passes (bf_render.hip; DESIGN.md §4 "Renderer"), slow
and obvious: np.float32 scalars and arrays only, the operations in the kernel's order, the target a
uint64 minimum per pixel.  Not a test module; tests/test_render_host.py checks it against cases
worked by hand and tests/test_gpu_render.py compares the kernels with it bit for bit."""
import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
# the twelve edges in the v0..v7 corner order (the reference's Instances3D.augment_vertices)
EDGES = ((0, 1), (0, 4), (1, 5), (4, 5), (2, 3), (2, 6), (6, 7), (3, 7), (0, 3), (4, 7), (1, 2), (5, 6))


def pack_key(layer, z, rgb):
    """layer << 63 | bits(z) << 32 | r << 24 | g << 16 | b << 8 | 0xFF (arrays or scalars)"""
    zb = np.asarray(z, F).view(np.uint32).astype(np.uint64)
    c = np.asarray(rgb, np.uint8).astype(np.uint64)
    col = (c[..., 0] << np.uint64(24)) | (c[..., 1] << np.uint64(16)) | (c[..., 2] << np.uint64(8)) | np.uint64(0xFF)
    return (np.uint64(1 if layer else 0) << np.uint64(63)) | (zb << np.uint64(32)) | col


def unpack_key(key):
    """-> (layer, z f32, rgb u8 [...,3]) of non-empty keys"""
    key = np.asarray(key, np.uint64)
    z = ((key >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).astype(np.uint32).view(F)
    rgb = np.stack([(key >> np.uint64(s)) & np.uint64(0xFF) for s in (24, 16, 8)], -1).astype(np.uint8)
    return (key >> np.uint64(63)).astype(np.int64), z, rgb


def camera_rows(poses):
    """camera -> world [V,4,4] -> world -> camera rows f32 [V,12] (R row-major, then t): the inverse
    in f64, cast once"""
    inv = np.linalg.inv(np.asarray(poses, np.float64).reshape(-1, 4, 4))
    return np.concatenate([inv[:, :3, :3].reshape(-1, 9), inv[:, :3, 3]], 1).astype(F)


def new_keys(V, H, W):
    return np.full((V, H, W), EMPTY, np.uint64)


def to_camera(m, x, y, z):
    X = m[0] * x + m[1] * y + m[2] * z + m[9]
    Y = m[3] * x + m[4] * y + m[5] * z + m[10]
    Z = m[6] * x + m[7] * y + m[8] * z + m[11]
    return X, Y, Z


def splat(keys_v, count_v, u, v, r, key):
    """arrays of samples (u, v f32, key u64) into one view; returns how many passed the window test"""
    H, W = keys_v.shape
    ok = (u >= F(-(r + 1))) & (u <= F(W + r)) & (v >= F(-(r + 1))) & (v <= F(H + r))
    u, v, key = u[ok], v[ok], key[ok]
    ix = np.floor(u + F(0.5)).astype(np.int64)
    iy = np.floor(v + F(0.5)).astype(np.int64)
    flat, cnt = keys_v.reshape(-1), count_v.reshape(-1)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            x, y = ix + dx, iy + dy
            ins = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            np.minimum.at(flat, y[ins] * W + x[ins], key[ins])
            np.add.at(cnt, y[ins] * W + x[ins], 1)
    return int(ok.sum())


def draw_points(keys, xyz, rgb, rows, intr, near, far, r, layer, count=None, drops=None):
    """bf_render_points.  count: int64 [V,H,W] += candidates per pixel; drops: dict += (point, view)
    pairs dropped as nonfinite / near (Z <= near) / far (Z >= far) / outside (the window test), and
    `pairs`, their total"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    rgb = np.asarray(rgb, np.uint8).reshape(-1, 3)
    fx, fy, cx, cy = (F(v) for v in intr)
    near, far = F(near), F(far)
    count = np.zeros(keys.shape, np.int64) if count is None else count
    drops = {} if drops is None else drops
    with np.errstate(all="ignore"):
        for v in range(keys.shape[0]):
            X, Y, Z = to_camera(rows[v], xyz[:, 0], xyz[:, 1], xyz[:, 2])
            assert X.dtype == F
            fin = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
            keep = fin & (Z > near) & (Z < far)
            Xk, Yk, Zk = X[keep], Y[keep], Z[keep]
            u = fx * Xk / Zk + cx
            w = fy * Yk / Zk + cy
            assert u.dtype == F
            shown = splat(keys[v], count[v], u, w, r, pack_key(layer, Zk, rgb[keep]))
            for name, n in (("pairs", len(xyz)), ("nonfinite", (~fin).sum()), ("near", (fin & ~(Z > near)).sum()),
                            ("far", (fin & ~(Z < far)).sum()), ("outside", int(keep.sum()) - shown)):
                drops[name] = drops.get(name, 0) + int(n)
    return drops


def _clip(p, q, t):
    """one Liang-Barsky boundary on t = [t0, t1]; False when nothing is left"""
    if p == 0:
        return bool(q >= 0)
    r = q / p
    if p < 0:
        if r > t[1]:
            return False
        if r > t[0]:
            t[0] = r
    else:
        if r < t[0]:
            return False
        if r < t[1]:
            t[1] = r
    return True


def edge_samples(a, b, intr, H, W, near):
    """camera-space ends a, b (three f32 each) -> (u, v, Z) f32 arrays of the samples, or None when
    the edge draws nothing; `fate` is the reason or 'drawn'"""
    fx, fy, cx, cy = (F(v) for v in intr)
    near = F(near)
    Xa, Ya, Za = a
    Xb, Yb, Zb = b
    if not np.isfinite([Xa, Ya, Za, Xb, Yb, Zb]).all():
        return None, "nonfinite"
    if Za < near and Zb < near:
        return None, "behind"
    fate = "drawn"
    if Za < near:
        t = (near - Za) / (Zb - Za)
        Xa = Xa + t * (Xb - Xa)
        Ya = Ya + t * (Yb - Ya)
        Za = near
        fate = "near_clipped"
    elif Zb < near:
        t = (near - Za) / (Zb - Za)
        Xb = Xa + t * (Xb - Xa)
        Yb = Ya + t * (Yb - Ya)
        Zb = near
        fate = "near_clipped"
    ua, va, wa = fx * Xa / Za + cx, fy * Ya / Za + cy, F(1.0) / Za
    ub, vb, wb = fx * Xb / Zb + cx, fy * Yb / Zb + cy, F(1.0) / Zb
    if not np.isfinite([ua, va, ub, vb]).all():
        return None, "nonfinite"
    du, dv, dw = ub - ua, vb - va, wb - wa
    t = [F(0.0), F(1.0)]
    if not (_clip(-du, ua - F(-0.5), t) and _clip(du, (F(W) - F(0.5)) - ua, t) and
            _clip(-dv, va - F(-0.5), t) and _clip(dv, (F(H) - F(0.5)) - va, t)):
        return None, "offscreen"
    t0, t1 = t
    span = max(abs((ua + t1 * du) - (ua + t0 * du)), abs((va + t1 * dv) - (va + t0 * dv)))
    cap = max(W, H)
    n = int(np.ceil(span)) if span < F(cap) else cap
    i = np.arange(n + 1).astype(F)
    ts = t0 + (t1 - t0) * (i / F(max(n, 1)))
    u, v, w = ua + ts * du, va + ts * dv, wa + ts * dw
    Z = F(1.0) / w
    assert all(x.dtype == F for x in (ts, u, v, w, Z)) and all(type(x) is F for x in (ua, va, wa, du, t0, t1))
    ok = (Z > 0) & (Z < F(np.inf))
    return (u[ok], v[ok], Z[ok]), fate


def draw_edges(keys, corners, colors, rows, intr, near, hw, layer, mask=None, count=None, fates=None):
    """bf_render_edges.  fates: dict += edges per (edge, view) by what became of them"""
    corners = np.asarray(corners, F).reshape(-1, 8, 3)
    colors = np.asarray(colors, np.uint8).reshape(-1, 3)
    V, H, W = keys.shape
    count = np.zeros(keys.shape, np.int64) if count is None else count
    fates = {} if fates is None else fates
    with np.errstate(all="ignore"):
        for v in range(V):
            for b in range(len(corners)):
                if mask is not None and not mask[b]:
                    continue
                if not np.isfinite(corners[b]).all():
                    fates["bad_box"] = fates.get("bad_box", 0) + 12
                    continue
                cam = [to_camera(rows[v], *corners[b, k]) for k in range(8)]
                for i, j in EDGES:
                    s, fate = edge_samples(cam[i], cam[j], intr, H, W, near)
                    fates[fate] = fates.get(fate, 0) + 1
                    if s is not None:
                        splat(keys[v], count[v], s[0], s[1], hw, pack_key(layer, s[2], np.broadcast_to(colors[b], (len(s[2]), 3))))
    return fates


def resolve(keys, background=(0, 0, 0)):
    """bf_render_resolve -> (rgb u8 [V,H,W,3], depth f32 [V,H,W])"""
    empty = keys == EMPTY
    _, z, rgb = unpack_key(keys)
    depth = np.where(empty, F(0), z).astype(F)
    bg = np.asarray(background, np.uint8)
    bg = np.broadcast_to(bg, rgb.shape)
    return np.where(empty[..., None], bg, rgb).astype(np.uint8), depth
