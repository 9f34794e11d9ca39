"""The scene mesh's rules, checked on the host: the numpy restatement of bf_tsdf.hip (tests/mesh_ref.py,
which test_gpu_mesh.py holds the kernels to bit for bit) against analytic geometry, the PLY writer, and
the two commands' argument errors.

The scene: a sphere of radius 8 voxels (voxel 5 cm) and a tilted wall inside a shell of radius 2 m, in
48x64 depth maps from six poses on a rotated octahedron 1.2 m from the sphere.  The shell is there
because a voxel is only known to be free where a ray passes it and ends on something."""
import numpy as np
import pytest

from tests import mesh_ref as R

T, MAX_DEPTH = 4, 3.5

# measured on the restatement ("Scene mesh"): the sphere's vertices are at most 0.573 voxels
# from the sphere, 0.094 voxels inside it on average, and the mesh encloses 4.90 % less than the sphere
SPHERE_MAX, SPHERE_BIAS, SPHERE_VOLUME = 0.573, 0.094, 0.0490
# and, seen from the camera that fares worst, 4.24 % of the wall's triangles, 0.70 % of its area, face away
WALL_FLIPPED_FACES, WALL_FLIPPED_AREA = 0.0424, 0.0070


@pytest.fixture(scope="module")
def fused():
    sc = R.Scene()
    depths = sc.depths()
    vol = R.fuse(depths, sc.poses, sc.K, sc.voxel, T, MAX_DEPTH)
    v, c, f = R.surface(vol["key"], vol["state"], sc.voxel)
    v64 = v.astype(np.float64)
    r = np.linalg.norm(v64 - sc.centre, axis=1)
    on_sphere = r < sc.radius + 3 * sc.voxel
    on_shell = r > sc.shell - 3 * sc.voxel
    plane = v64 @ sc.normal - sc.wall_at
    on_wall = ~on_sphere & ~on_shell & (np.abs(plane) < 3 * sc.voxel)
    assert on_sphere.sum() > 1000 and on_wall.sum() > 1000
    assert (on_sphere | on_shell | on_wall).all()            # nothing floats in between
    return dict(scene=sc, depths=depths, v=v64, f=f, r=r, on_sphere=on_sphere, on_wall=on_wall, plane=plane)


def _wall_pixels(sc, P, dm):
    """(the valid pixels of depth map dm that show the wall, the plane's depth and n_c . r as a function
    of (u, v), the pixel grids)"""
    fx, fy, cx, cy = [float(a) for a in R.intrinsics(sc.K)]
    P = P.astype(np.float64)
    nc = P[:3, :3].T @ sc.normal                             # the plane in camera coordinates: nc . x = dc
    dc = sc.wall_at - sc.normal @ P[:3, 3]
    v, u = np.mgrid[:sc.H, :sc.W].astype(np.float64)

    def plane_depth(u_, v_):
        nr = nc[0] * (u_ - cx) / fx + nc[1] * (v_ - cy) / fy + nc[2]
        return dc / nr, nr
    with np.errstate(all="ignore"):
        wall = (np.abs(plane_depth(u, v)[0] - dm) < 1e-4) & (dm > 0) & (dm < MAX_DEPTH)
    return wall, plane_depth, u, v


def _wall_bound(sc, depths):
    """see test_wall_distance"""
    e_perp, k = [], []
    for P, dm in zip(sc.poses, depths):
        wall, plane_depth, u, v = _wall_pixels(sc, P, dm)
        d0, nr = plane_depth(u, v)
        dev = np.max([np.abs(plane_depth(u + a, v + b)[0] - d0) for a in (-0.5, 0.5) for b in (-0.5, 0.5)], 0)
        e_perp.append((dev * np.abs(nr))[wall])
        k.append((1.0 / np.abs(nr))[wall])
    e_perp, k = np.concatenate(e_perp), np.concatenate(k)
    assert k.max() * (1.0 + e_perp.max() / sc.voxel) < T     # no sign-changing edge has a clamped or cut-off end
    interp = sc.voxel / 4 * (k.max() - k.min()) / np.sqrt(k.max() * k.min())
    quant = T * sc.voxel / 1024
    return e_perp.max() + interp + quant, e_perp.max(), interp


def test_wall_distance(fused):
    """Every wall vertex lies within a derived distance of the plane.

    A voxel at signed distance D from the plane, seen by camera c along the pixel ray r = ((u - cx) / fx,
    (v - cy) / fy, 1), stores sdf_c = k_c D + e_c: k_c = 1 / |n_c . r| turns a distance along the normal
    n_c into a difference of z-depths along the ray, and e_c is the error of reading the depth at the
    nearest pixel centre instead of at the voxel's own projection, at most the change of the plane's depth
    over half a pixel in u and in v.  That is the pixel footprint times the tangent of the incidence, and
    as a distance along the normal it is e_c / k_c, which the test evaluates exactly at the four corners of
    every wall pixel's square.  A voxel's value is the mean over the cameras that see it, s = K D + E with
    K = mean k_c and |E / K| <= max_c e_c / k_c (the mediant inequality).  On a sign-changing edge from a
    to b the crossing t = s_a / (s_a - s_b) is where the linear interpolant of s vanishes, so with one K
    for both ends the crossing is E / K from the plane; with K_a != K_b it moves by a further
    D_a D_b (K_a - K_b) / (K_a D_a - K_b D_b), which for D_a < 0 < D_b with D_b - D_a <= one voxel (an
    edge's length) is at most (voxel / 4) |K_a - K_b| / sqrt(K_a K_b); the k of all wall pixels bound K.
    Clamping and the cut-off at -trunc would break the linearity; the helper checks that no end of a
    sign-changing edge (at most a voxel and the pixel error from the plane) reaches them.  Rounding q to
    1 / 1024 of the truncation adds half a step per end, at most a step.  A vertex is the mean of its
    cell's crossings, so it is no further from the plane than they are."""
    sc = fused["scene"]
    bound, e_pix, interp = _wall_bound(sc, fused["depths"])
    got = np.abs(fused["plane"][fused["on_wall"]]).max()
    print(f"wall: max distance {got / sc.voxel:.4f} voxels; bound {bound / sc.voxel:.4f} = pixel "
          f"{e_pix / sc.voxel:.4f} + interpolation {interp / sc.voxel:.4f} + quantisation")
    assert bound < sc.voxel                                  # the bound says something
    assert got <= bound


def _sphere_faces(fused):
    f, on = fused["f"], fused["on_sphere"]
    mine = on[f].all(1)
    assert not on[f[~mine]].any()                            # no face joins the sphere to anything else
    return f[mine]


def test_sphere_accuracy(fused):
    sc, v = fused["scene"], fused["v"]
    err = (fused["r"][fused["on_sphere"]] - sc.radius) / sc.voxel
    fs = _sphere_faces(fused)
    a, b, c = v[fs[:, 0]] - sc.centre, v[fs[:, 1]] - sc.centre, v[fs[:, 2]] - sc.centre
    volume = (a * np.cross(b, c)).sum() / 6.0                # the divergence theorem; positive: outward normals
    rel = volume / (4.0 / 3.0 * np.pi * sc.radius ** 3) - 1.0
    print(f"sphere: max |error| {np.abs(err).max():.4f} voxels, mean {err.mean():+.4f} voxels, volume {rel:+.4%}")
    assert np.abs(err).max() <= min(1.5 * SPHERE_MAX, 1.0)
    assert abs(err.mean()) <= min(1.5 * SPHERE_BIAS, 0.25)
    assert abs(rel) <= 1.5 * SPHERE_VOLUME


def test_sphere_closed_and_oriented(fused):
    """every directed edge of the sphere's triangles appears once, and its reverse once"""
    fs = _sphere_faces(fused).astype(np.int64)
    e = np.concatenate([fs[:, [0, 1]], fs[:, [1, 2]], fs[:, [2, 0]]])
    n = len(fused["v"])
    fwd, rev = e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]
    assert len(np.unique(fwd)) == len(fwd)
    assert np.array_equal(np.sort(fwd), np.sort(rev))
    assert len(np.unique(fs)) - len(e) // 2 + len(fs) == 2   # Euler: one sphere


def test_wall_normals_face_the_cameras(fused):
    """The wall's faces look at the cameras that see it.  Where two neighbouring crossings are closer
    than the pixel error of test_wall_distance their order can reverse, and the strip between them folds
    over; such a strip is thin.  So: every triangle of at least half a regular one's area (a regular
    quad is a voxel square, its triangles 0.5 voxel^2) faces every such camera, and the folded strips
    are held to 1.5x the measured share of the wall's triangles and of its area ("Scene
    mesh"), as the sphere's figures are."""
    sc, v, f = fused["scene"], fused["v"], fused["f"]
    fw = f[fused["on_wall"][f].all(1)]
    assert len(fw) > 1000
    normal = np.cross(v[fw[:, 1]] - v[fw[:, 0]], v[fw[:, 2]] - v[fw[:, 0]]) / sc.voxel ** 2
    area = np.linalg.norm(normal, axis=1) / 2
    mid = v[fw].mean(1)
    fair = area >= 0.25
    assert area[fair].sum() > 0.8 * area.sum()                # most of the wall is such triangles
    seen_by = 0
    for P, dm in zip(sc.poses, fused["depths"]):
        if not _wall_pixels(sc, P, dm)[0].any():
            continue
        seen_by += 1
        facing = ((P[:3, 3].astype(np.float64) - mid) * normal).sum(1) > 0
        print(f"wall normals: {1 - facing.mean():.4%} of the faces, {area[~facing].sum() / area.sum():.4%} of the "
              "area face away")
        assert facing[fair].all()
        assert 1 - facing.mean() <= 1.5 * WALL_FLIPPED_FACES
        assert area[~facing].sum() <= 1.5 * WALL_FLIPPED_AREA * area.sum()
    assert seen_by == 3


def test_ply_round_trip(fused, tmp_path):
    from boxfusion_amd import evaluation, visualize
    v, f = fused["v"].astype(np.float32), fused["f"]
    rgb = (np.arange(len(v) * 3) % 251).astype(np.uint8).reshape(-1, 3)
    path = str(tmp_path / "sub" / "mesh.ply")
    visualize.mesh_to_ply(v, rgb, f, path)
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"]
    assert [h for h in head if h.startswith("property")] == [
        "property float x", "property float y", "property float z", "property uchar red", "property uchar green",
        "property uchar blue", "property list uchar int vertex_indices"]
    nv = int([h for h in head if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in head if h.startswith("element face")][0].split()[-1])
    vdt = np.dtype([("xyz", "<f4", (3,)), ("rgb", "u1", (3,))])
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    assert len(data) == end + nv * vdt.itemsize + nf * fdt.itemsize
    vert = np.frombuffer(data, vdt, nv, end)
    face = np.frombuffer(data, fdt, nf, end + nv * vdt.itemsize)
    assert np.array_equal(vert["xyz"], v) and np.array_equal(vert["rgb"], rgb)
    assert (face["n"] == 3).all() and np.array_equal(face["i"], f)
    xyz, col = visualize.read_ply_points(path)
    assert np.array_equal(xyz, v) and np.array_equal(col, rgb)
    assert np.array_equal(evaluation.read_ply_points(path), v.astype(np.float64))
    with pytest.raises(ValueError):
        visualize.mesh_to_ply(v, rgb, f + len(v), path)
    with pytest.raises(ValueError):
        visualize.mesh_to_ply(v, rgb[:-1], f, path)
    visualize.mesh_to_ply(v[:0], rgb[:0], f[:0], path)      # an empty mesh is a file too
    assert visualize.read_ply_points(path)[0].shape == (0, 3)


def _error(main, argv, capsys, text):
    with pytest.raises(SystemExit) as e:
        main(argv)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_sens_mesh_argument_errors(tmp_path, capsys):
    from boxfusion_amd import sens
    out = str(tmp_path / "o.ply")
    _error(sens.main, ["mesh", str(tmp_path / "none.sens"), out], capsys, "is missing")
    _error(sens.main, ["mesh", "x.sens", out, "--voxel", "0"], capsys, "--voxel must be positive")
    _error(sens.main, ["mesh", "x.sens", out, "--step", "0"], capsys, "--step must be at least 1")
    _error(sens.main, ["mesh", "x.sens", out, "--trunc-voxels", "0"], capsys, "--trunc-voxels")
    _error(sens.main, ["mesh", "x.sens", out, "--capacity", "1000"], capsys, "power of two")
    _error(sens.main, ["mesh", "x.sens"], capsys, "required")


def test_scene_mesh_argument_errors(tmp_path, capsys):
    from boxfusion_amd import scene_mesh
    seq = tmp_path / "seq"
    _error(scene_mesh.main, [str(seq)], capsys, "is not a directory")
    seq.mkdir()
    _error(scene_mesh.main, [str(seq), "--voxel", "0"], capsys, "--voxel must be positive")
    _error(scene_mesh.main, [str(seq), "--step", "0"], capsys, "--step must be at least 1")
    _error(scene_mesh.main, [str(seq), "--max-depth", "-1"], capsys, "--max-depth must be positive")
    _error(scene_mesh.main, [str(seq), "--depth-scale", "0"], capsys, "--depth-scale must be positive")
    _error(scene_mesh.main, [str(seq)], capsys, "K_depth.txt is missing")
    np.savetxt(seq / "K_depth.txt", np.eye(3))
    _error(scene_mesh.main, [str(seq)], capsys, "all_poses.npy is missing")
    np.save(seq / "all_poses.npy", np.eye(4)[None])
    _error(scene_mesh.main, [str(seq)], capsys, "holds no <i>.png")
    (seq / "depth").mkdir()
    (seq / "depth" / "0.png").write_bytes(b"")
    _error(scene_mesh.main, [str(seq)], capsys, "rgb/ holds 0 <i>.png and depth/ 1")


def test_volume_argument_errors():
    """TsdfVolume checks its arguments before it touches the device"""
    from boxfusion_amd.scene_mesh import TsdfVolume
    for kw in (dict(voxel=0.0), dict(trunc_voxels=0), dict(max_depth=0.0), dict(max_weight=0), dict(max_weight=1 << 21)):
        with pytest.raises(ValueError):
            TsdfVolume(device="cpu", **kw)
