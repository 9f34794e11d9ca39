"""Host restatements of bf_label_points (include/boxfusion_objects.h) for the object tests.

label_ref is the rule in numpy f32 with the kernel's operation order: every product and sum below is one
f32 ufunc, so each rounds on its own as the kernel's do with contraction off.  It returns what the kernel
writes, raw: labels, counts, the extents' uint32 keys and the stats without PAIR_TESTS.  label_f64 is the
same geometry by brute force in f64, with the distance of every point to the nearest box face."""
import numpy as np

_SIGNS = np.array([[sx, sy, sz] for sz in (-1, 1) for sy in (-1, 1) for sx in (-1, 1)], np.float64)


def random_rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def corners_of(centre, R, half):
    """centre [B,3], R [B,3,3] (columns = axes), half [B,3] -> corners f64 [B,8,3]"""
    centre, R, half = (np.asarray(a, np.float64) for a in (centre, R, half))
    return centre[:, None] + np.einsum("sk,bk,bjk->bsj", _SIGNS, half, R)


def random_boxes(rng, n, half_range=(0.05, 1.2), centre_range=3.0):
    half = rng.uniform(*half_range, size=(n, 3))
    return corners_of(rng.uniform(-centre_range, centre_range, size=(n, 3)), random_rotations(rng, n), half)


def axis_boxes(centres, halves):
    """axis-aligned boxes: corners f64 [B,8,3]"""
    centres = np.asarray(centres, np.float64).reshape(-1, 3)
    return corners_of(centres, np.tile(np.eye(3), (len(centres), 1, 1)), np.asarray(halves, np.float64).reshape(-1, 3))


def keys_of(values):
    """f32 -> the order-preserving uint32 keys, written out independently of the package"""
    bits = np.asarray(values, np.float32).view(np.uint32).astype(np.uint64)
    neg = bits >> 31 == 1
    return np.where(neg, bits ^ 0xFFFFFFFF, bits | 0x80000000).astype(np.uint32)


def label_ref(xyz, rows, margin=0.0):
    """xyz f32 [n,3], rows f32 [B,16] -> dict(labels int32 [n], counts int64 [B,2], keys uint32 [B,6],
    stats dict(points, nonfinite, labelled, shared), inside int [n])"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    rows = np.ascontiguousarray(rows, np.float32).reshape(-1, 16)
    margin = np.float32(margin)
    n, B = len(xyz), len(rows)
    fin = np.isfinite(xyz).all(1)
    labels = np.full(n, -1, np.int32)
    best_vol = np.zeros(n, np.float32)
    bt = np.zeros((n, 3), np.float32)
    inside = np.zeros(n, np.int64)
    counts = np.zeros((B, 2), np.int64)
    with np.errstate(all="ignore"):
        for b in range(B):
            r = rows[b]
            dx, dy, dz = xyz[:, 0] - r[0], xyz[:, 1] - r[1], xyz[:, 2] - r[2]
            t = [(dx * r[3 + 3 * k] + dy * r[4 + 3 * k]) + dz * r[5 + 3 * k] for k in range(3)]
            lim = [r[12 + k] + margin for k in range(3)]
            assert all(v.dtype == np.float32 for v in t) and all(v.dtype == np.float32 for v in lim)
            inn = fin & (np.abs(t[0]) <= lim[0]) & (np.abs(t[1]) <= lim[1]) & (np.abs(t[2]) <= lim[2])
            counts[b, 0] = inn.sum()
            inside += inn
            take = inn & ((labels < 0) | (r[15] < best_vol))
            labels[take] = b
            best_vol[take] = r[15]
            for k in range(3):
                bt[take, k] = t[k][take]
    keys = np.zeros((B, 6), np.uint32)
    keys[:, 0::2] = 0xFFFFFFFF
    k = keys_of(bt)
    for b in np.unique(labels[labels >= 0]):
        mine = labels == b
        counts[b, 1] = mine.sum()
        for a in range(3):
            keys[b, 2 * a], keys[b, 2 * a + 1] = k[mine, a].min(), k[mine, a].max()
    stats = dict(points=n, nonfinite=int((~fin).sum()), labelled=int((labels >= 0).sum()), shared=int((inside >= 2).sum()))
    return dict(labels=labels, counts=counts, keys=keys, stats=stats, inside=inside, finite=int(fin.sum()))


def label_f64(xyz, rows, margin=0.0):
    """the same rows (upcast) and points in f64 -> (labels int32 [n], member bool [n,B], face_dist f64
    [n]: over the boxes, the least | max_k (|t_k| - (h_k + margin)) |, the distance to a box's nearest face)"""
    p = np.asarray(xyz, np.float64).reshape(-1, 3)
    r = np.asarray(rows, np.float64).reshape(-1, 16)
    d = p[:, None, :] - r[None, :, 0:3]                                   # [n,B,3]
    t = np.einsum("nbj,bkj->nbk", d, r[:, 3:12].reshape(-1, 3, 3))        # [n,B,3]
    gap = np.abs(t) - (r[None, :, 12:15] + float(margin))
    member = (gap <= 0).all(2)
    vol = np.where(member, r[None, :, 15], np.inf)
    labels = np.where(member.any(1), np.argmin(vol, 1), -1).astype(np.int32)     # argmin: the first of equals
    # a point changes sides of box b where its largest gap crosses zero: that is how far it is from b's faces
    return labels, member, np.abs(gap.max(2)).min(1) if len(r) else np.full(len(p), np.inf)
