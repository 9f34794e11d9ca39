"""A numpy restatement of the renderer's triangle pass (bf_render_triangles; DESIGN.md §4 "Renderer",
*Triangles*), on the key arrays of tests/render_util.py so that a picture can mix points, box edges and
triangles.  Slow and obvious: the set-up of all triangles of a view in np.float32 arrays in the kernel's
order, coverage in int64 one triangle at a time, depth and colour in float64.  Not a test module;
tests/test_render_mesh_host.py checks it against the properties it must have and
tests/test_gpu_render_mesh.py compares the kernel with it bit for bit.  The scenes both use are below."""
import numpy as np

from tests import mesh_ref as MR
from tests import render_util as RU

F = np.float32
GUARD = F(4194304.0)                                                      # 2^22 px
AMBIENT = F(0.3)
GREY = 128
RULES = ("drawn", "range", "bounds", "culled")                           # the kernel's stats 0..3


def headlight(X, Y, Z):
    """the two-sided headlight factor f32 [m] of triangles with camera-space vertices X, Y, Z f32 [m,3]"""
    ax, ay, az = X[:, 1] - X[:, 0], Y[:, 1] - Y[:, 0], Z[:, 1] - Z[:, 0]
    bx, by, bz = X[:, 2] - X[:, 0], Y[:, 2] - Y[:, 0], Z[:, 2] - Z[:, 0]
    nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
    gx, gy, gz = X[:, 0] + X[:, 1] + X[:, 2], Y[:, 0] + Y[:, 1] + Y[:, 2], Z[:, 0] + Z[:, 1] + Z[:, 2]
    dot = nx * gx + ny * gy + nz * gz
    nn, gg = nx * nx + ny * ny + nz * nz, gx * gx + gy * gy + gz * gz
    q = np.abs(dot) / np.sqrt(nn * gg)
    cs = np.where(np.isfinite(q), np.minimum(q, F(1)), F(0))
    s = AMBIENT + (F(1) - AMBIENT) * cs
    assert all(a.dtype == F for a in (nx, gx, dot, nn, q, cs, s))
    return s


def snap(cam, P, intr):
    """world points f32 [...,3] -> (X, Y, Z, u, v f32, xs, ys int64): the camera-space image, the
    projection and its 1/256 px grid position (xs, ys are only meaningful where |u|, |v| < 2^22)"""
    fx, fy, cx, cy = (F(a) for a in intr)
    X, Y, Z = RU.to_camera(np.asarray(cam, F), P[..., 0], P[..., 1], P[..., 2])
    u, v = fx * X / Z + cx, fy * Y / Z + cy
    assert X.dtype == F and u.dtype == F
    ok = (np.abs(u) < GUARD) & (np.abs(v) < GUARD)
    xs = np.rint(np.where(ok, u, F(0)) * F(256)).astype(np.int64)
    ys = np.rint(np.where(ok, v, F(0)) * F(256)).astype(np.int64)
    return X, Y, Z, u, v, xs, ys


def setup(cam, vertices, faces, near, far, intr, cull):
    """every triangle of one view -> dict(fate [m] of RULES' indices, xs, ys int64 [m,3] and order
    [m,3] after the orientation swap, area2 [m] > 0 where drawn, X, Y, Z f32 [m,3] in the face's
    own order)"""
    n, m = len(vertices), len(faces)
    fate = np.zeros(m, np.int64)
    bad_index = ((faces < 0) | (faces >= n)).any(1)
    P = vertices[np.where(bad_index[:, None], 0, faces)] if n else np.zeros((m, 3, 3), F)
    X, Y, Z, u, v, xs, ys = snap(cam, P, intr)
    finite = np.isfinite(P).all((1, 2)) & np.isfinite(X).all(1) & np.isfinite(Y).all(1) & np.isfinite(Z).all(1)
    in_range = finite & ((Z > near) & (Z < far)).all(1)
    in_band = ((np.abs(u) < GUARD) & (np.abs(v) < GUARD)).all(1)
    area2 = (xs[:, 1] - xs[:, 0]) * (ys[:, 2] - ys[:, 0]) - (ys[:, 1] - ys[:, 0]) * (xs[:, 2] - xs[:, 0])
    # the kernel's order of tests: index, finite and range, guard band, area and cull
    fate[(area2 == 0) | ((area2 > 0) & bool(cull))] = 3
    fate[~in_band] = 2
    fate[~in_range] = 1
    fate[bad_index] = 2
    swap = area2 < 0
    order = np.where(swap[:, None], [0, 2, 1], [0, 1, 2])
    take = lambda a: np.take_along_axis(a, order, 1)
    return dict(fate=fate, xs=take(xs), ys=take(ys), order=order, area2=np.abs(area2), X=X, Y=Y, Z=Z)


def cover(xs, ys, H, W):
    """the pixels of the clipped rectangle of one oriented triangle (three ints each): (ix, iy, E
    int64 [3,...], covered, tie-decided), or None when the rectangle is empty"""
    x0, x1 = max(-(-min(xs) // 256), 0), min(max(xs) // 256, W - 1)
    y0, y1 = max(-(-min(ys) // 256), 0), min(max(ys) // 256, H - 1)
    if x0 > x1 or y0 > y1:
        return None
    iy, ix = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    px, py = 256 * ix, 256 * iy
    E, inside, tied = [], np.ones(ix.shape, bool), np.zeros(ix.shape, bool)
    for i in range(3):
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = xs[b] - xs[a], ys[b] - ys[a]
        e = dx * (py - ys[a]) - dy * (px - xs[a])
        owns = dy < 0 or (dy == 0 and dx > 0)
        inside &= (e > 0) | ((e == 0) & owns)
        tied |= e == 0
        E.append(e)
    return ix, iy, np.stack(E), inside, inside & tied


def draw_triangles(keys, vertices, rgb, faces, rows, intr, near, far, cull, shade, layer, count=None, fates=None):
    """bf_render_triangles.  count: int64 [V,H,W] += triangles that cover each pixel; fates: dict +=
    (triangle, view) pairs by what became of them (RULES, and `pairs`, their total) and `ties`, the
    covered pixels that an E == 0 decided.  rgb None: mid-grey.  Returns (count, fates)."""
    vertices = np.asarray(vertices, F).reshape(-1, 3)
    n = len(vertices)
    rgb = np.full((n, 3), GREY, np.uint8) if rgb is None else np.asarray(rgb, np.uint8).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    near, far = F(near), F(far)
    V, H, W = keys.shape
    count = np.zeros(keys.shape, np.int64) if count is None else count
    fates = {} if fates is None else fates
    for k in RULES + ("pairs", "ties"):
        fates.setdefault(k, 0)
    if n == 0 or len(faces) == 0:                                         # the entry point launches nothing
        return count, fates
    with np.errstate(all="ignore"):
        for v in range(V):
            s = setup(rows[v], vertices, faces, near, far, intr, cull)
            fates["pairs"] += len(faces)
            for i, k in enumerate(RULES):
                fates[k] += int((s["fate"] == i).sum())
            light = headlight(s["X"], s["Y"], s["Z"]).astype(np.float64) if shade else None
            for f in np.nonzero(s["fate"] == 0)[0]:
                c = cover([int(a) for a in s["xs"][f]], [int(a) for a in s["ys"][f]], H, W)
                if c is None or not c[3].any():
                    continue
                ix, iy, E, inside, tied = c
                ix, iy, E = ix[inside], iy[inside], E[:, inside]
                fates["ties"] += int(tied.sum())
                order = s["order"][f]
                iz = [1.0 / np.float64(s["Z"][f, j]) for j in order]
                t = [E[j].astype(np.float64) * iz[j] for j in range(3)]
                iw = (t[0] + t[1]) + t[2]
                r = 1.0 / iw
                Z = (np.float64(s["area2"][f]) * r).astype(F)
                col = rgb[faces[f][order]].astype(np.float64)                # [3 vertices, 3 channels]
                out = np.empty((len(ix), 3), np.uint8)
                for ch in range(3):
                    val = ((t[0] * col[0, ch] + t[1] * col[1, ch]) + t[2] * col[2, ch]) * r
                    if shade:
                        val = val * light[f]
                    out[:, ch] = np.clip(np.rint(val), 0.0, 255.0).astype(np.uint8)
                flat = iy * W + ix
                np.minimum.at(keys[v].reshape(-1), flat, RU.pack_key(layer, Z, out))
                np.add.at(count[v].reshape(-1), flat, 1)
    return count, fates


def stats_of(fates, count):
    """the kernel's stats 0..4 of pictures drawn by draw_triangles alone"""
    return [fates[k] for k in RULES] + [int(count.sum())]


def strictly_inside(poly_x, poly_y, H, W, closed=False):
    """bool [H,W]: the pixel centres strictly inside the closed polygon whose corners are the ints
    poly_x, poly_y in 1/256 px (crossing number in exact integers; centres on the outline are not
    inside, unless closed)"""
    iy, ix = np.mgrid[:H, :W].astype(np.int64)
    px, py = 256 * ix, 256 * iy
    odd, on = np.zeros((H, W), bool), np.zeros((H, W), bool)
    k = len(poly_x)
    for i in range(k):
        xa, ya, xb, yb = int(poly_x[i]), int(poly_y[i]), int(poly_x[(i + 1) % k]), int(poly_y[(i + 1) % k])
        cross = (xb - xa) * (py - ya) - (yb - ya) * (px - xa)
        on |= (cross == 0) & (px >= min(xa, xb)) & (px <= max(xa, xb)) & (py >= min(ya, yb)) & (py <= max(ya, yb))
        straddles = (ya > py) != (yb > py)
        # the edge crosses the pixel's row to the right of the centre
        right = (cross > 0) == (yb > ya)
        odd ^= straddles & right & (cross != 0)
    return odd | on if closed else odd & ~on


# ---- scenes ----------------------------------------------------------------------------------------------
IDENTITY_ROWS = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], F)


def grid_faces(ny, nx, alternate=False):
    """two triangles per cell of an ny x nx grid of vertices (row-major), int32 [2 (ny-1) (nx-1), 3]"""
    out = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i + 1, (j + 1) * nx + i
            out += [(a, b, c), (a, c, d)] if not (alternate and (i + j) & 1) else [(a, b, d), (b, c, d)]
    return np.array(out, np.int32)


def grid_outline(ny, nx):
    """the vertex indices along the border of the grid, in order"""
    top = list(range(nx))
    right = [j * nx + nx - 1 for j in range(1, ny)]
    bottom = [(ny - 1) * nx + i for i in range(nx - 2, -1, -1)]
    left = [j * nx for j in range(ny - 2, 0, -1)]
    return np.array(top + right + bottom + left)


def jittered_grid(H, W, intr, seed=3):
    """a 12 x 16 grid of vertices in front of the identity camera, 330 triangles facing it: spread
    over the image with a margin, each moved by up to 0.3 of a cell on the screen and 0.2 m in depth
    -> (vertices f32 [192,3], rgb u8, faces int32 [330,3])"""
    fx, fy, cx, cy = (float(a) for a in intr)
    rng = np.random.default_rng(seed)
    ny, nx = 12, 16
    du, dv = (W - 9.0) / (nx - 1), (H - 9.0) / (ny - 1)
    j, i = np.mgrid[:ny, :nx]
    u = 4.0 + du * (i + rng.uniform(-0.3, 0.3, i.shape))
    v = 4.0 + dv * (j + rng.uniform(-0.3, 0.3, j.shape))
    z = 2.0 + rng.uniform(-0.2, 0.2, i.shape)
    xyz = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], -1).reshape(-1, 3).astype(F)
    return xyz, rng.integers(0, 256, (ny * nx, 3), dtype=np.uint8), grid_faces(ny, nx)


TIE_INTR = (32.0, 32.0, 20.0, 14.0)


def tie_grid(seed=4):
    """an 8 x 10 grid whose vertices lie exactly on pixel centres of the identity camera with
    TIE_INTR (Z = 1, X and Y multiples of 1/32), cells 3 to 6 px wide, the diagonals alternating, so
    that vertices and many edges pass exactly through pixel centres; fits 37 x 53"""
    rng = np.random.default_rng(seed)
    ny, nx = 8, 10
    px = 2 + np.concatenate([[0], np.cumsum(rng.integers(3, 7, nx - 1))])
    py = 2 + np.concatenate([[0], np.cumsum(rng.integers(3, 6, ny - 1))])
    assert px[-1] <= 50 and py[-1] <= 34
    j, i = np.mgrid[:ny, :nx]
    xyz = np.stack([(px[i] - TIE_INTR[2]) / 32.0, (py[j] - TIE_INTR[3]) / 32.0, np.ones(i.shape)], -1)
    return (xyz.reshape(-1, 3).astype(F), rng.integers(0, 256, (ny * nx, 3), dtype=np.uint8),
            grid_faces(ny, nx, alternate=True))


WALL_CASES = [(0.05, 48, 64, 60.0), (0.04, 37, 53, 50.0), (0.02, 48, 64, 60.0)]
_WALLS = {}


def wall_scene(voxel, H, W, focal):
    """the tilted wall of mesh_ref seen by three cameras: dict(K, poses [3,4,4], depths, and the
    surface-nets mesh `mesh` = (vertices, rgb, faces) of their fusion by the restatement of
    bf_tsdf.hip); computed once per case, never changed"""
    key = (voxel, H, W, focal)
    if key not in _WALLS:
        n = np.array([0.2, 0.1, 1.0])
        plane = (n / np.sqrt((n * n).sum()), -1.2)
        K = np.array([[focal, 0, W / 2 - 0.5], [0, focal, H / 2 - 0.5], [0, 0, 1]], F)
        eyes = [(0.0, 0.0, 0.3), (0.25, -0.1, 0.35), (-0.2, 0.15, 0.25)]
        poses = [MR.look_at(e, (0.02 * i, 0.01, -1.2), up=(0.0, 1.0, 0.0)) for i, e in enumerate(eyes)]
        depths = [MR.render_depth(p, K, H, W, plane=plane) for p in poses]
        fused = MR.fuse(depths, poses, K, voxel, 4, 10.0)
        _WALLS[key] = dict(K=K, poses=np.stack(poses), depths=depths, plane=plane,
                           mesh=MR.surface(fused["key"], fused["state"], voxel))
    return _WALLS[key]


def inner(H, W, border=4):
    m = np.zeros((H, W), bool)
    m[border:H - border, border:W - border] = True
    return m
