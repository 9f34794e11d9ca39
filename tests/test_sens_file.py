"""boxfusion_amd.sens.SensFile on containers written by tests/sens_util.py (no GPU): header round
trip, the frame index, zero-copy payload views, the reference's pose filling, the refusals
(version, truncated payload / record header, a frame count the file cannot hold), the exported tree
and the `info` / `export` commands."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

from boxfusion_amd import sens as S
from tests import sens_util as U

HC, WC, HD, WD = 24, 32, 12, 16


def _frames(n, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:HC, 0:WC]
    colors, depths = [], []
    for i in range(n):
        rgb = np.stack([(8 * x + 3 * i) % 256, (5 * y + 40 * i) % 256, (x + y) * 4 % 256], -1).astype(np.uint8)
        colors.append(U.jpeg_bytes(rgb))
        depths.append(rng.integers(0, 65536, (HD, WD)).astype(np.uint16))
    return colors, depths


def _poses(valid):
    return [U.upright_pose((0.1 * i, 0.2, 1.0 + i)) if v else U.LOST for i, v in enumerate(valid)]


@pytest.fixture()
def scene(tmp_path):
    colors, depths = _frames(4)
    poses = _poses([True, False, False, True])
    Kc = np.eye(4, dtype=np.float32)
    Kc[:2, :3] = [[1170.1875, 0, 647.75], [0, 1170.1875, 483.75]]
    Kd = np.eye(4, dtype=np.float32)
    Kd[:2, :3] = [[577.87, 0, 319.5], [0, 577.87, 239.5]]
    Ed = np.arange(16, dtype=np.float32).reshape(4, 4) / 7
    path = tmp_path / "scene0000_00.sens"
    hdr = dict(sensor_name="StructureSensor", intrinsic_color=Kc, intrinsic_depth=Kd, extrinsic_depth=Ed)
    data, zblobs = U.write_sens(path, colors, depths, poses, (HC, WC), **hdr)
    return dict(path=path, data=data, colors=colors, depths=depths, zblobs=zblobs, poses=poses, Kc=Kc, Kd=Kd, Ed=Ed)


def test_header_round_trip(scene):
    with S.SensFile(scene["path"]) as f:
        assert f.sensor_name == "StructureSensor"
        np.testing.assert_array_equal(f.intrinsic_color, scene["Kc"])
        np.testing.assert_array_equal(f.intrinsic_depth, scene["Kd"])
        np.testing.assert_array_equal(f.extrinsic_color, np.eye(4, dtype=np.float32))
        np.testing.assert_array_equal(f.extrinsic_depth, scene["Ed"])
        assert f.intrinsic_depth.dtype == np.float32 and f.intrinsic_depth.shape == (4, 4)
        assert (f.color_compression, f.depth_compression) == (2, 1)
        assert (f.color_width, f.color_height, f.depth_width, f.depth_height) == (WC, HC, WD, HD)
        assert f.depth_shift == 1000.0
        assert f.num_frames == len(f) == 4


def test_index_and_payload_views(scene):
    data = scene["data"]
    with S.SensFile(scene["path"]) as f:
        assert f.poses.shape == (4, 4, 4) and f.poses.dtype == np.float32
        pos = len(U.header(4, (HC, WC), (HD, WD)))          # (same name length as the scene's)
        for i in range(4):
            pos += 64 + 32
            assert f.color_index[i].tolist() == [pos, len(scene["colors"][i])]
            pos += len(scene["colors"][i])
            assert f.depth_index[i].tolist() == [pos, len(scene["zblobs"][i])]
            pos += len(scene["zblobs"][i])
            c, d = f.color_bytes(i), f.depth_bytes(i)
            assert isinstance(c, memoryview) and isinstance(d, memoryview)
            assert c == scene["colors"][i] and d == scene["zblobs"][i]
            assert c.obj is d.obj                               # views of the one map, not copies
            np.testing.assert_array_equal(f.depth_u16(i), scene["depths"][i])
            np.testing.assert_array_equal(f.poses[i], scene["poses"][i])
            assert f.timestamps[i].tolist() == [1000 * i, 1000 * i + 7]
            del c, d
        assert pos == len(data)


def test_poses_filled(scene, tmp_path):
    with S.SensFile(scene["path"]) as f:           # valid, -inf, -inf, valid
        got = f.poses_filled()
        p = scene["poses"]
        for i, want in enumerate([p[0], p[0], p[0], p[3]]):
            np.testing.assert_array_equal(got[i], want)
        assert np.isinf(f.poses[1]).all()          # the poses as written stay
    colors, depths = _frames(3)
    poses = _poses([False, False, True])
    U.write_sens(tmp_path / "late.sens", colors, depths, poses, (HC, WC))
    with S.SensFile(tmp_path / "late.sens") as f:  # starts with -inf: the first valid pose
        got = f.poses_filled()
        for i in range(3):
            np.testing.assert_array_equal(got[i], poses[2])


def _refused(tmp_path, data, match):
    path = tmp_path / "bad.sens"
    path.write_bytes(data)
    with pytest.raises(ValueError, match=match) as e:
        S.SensFile(path)
    assert str(path) in str(e.value)


def test_refusals(scene, tmp_path):
    data = scene["data"]
    colors, depths = scene["colors"], scene["depths"]
    v3, _ = U.write_sens(tmp_path / "v3.sens", colors, depths, scene["poses"], (HC, WC), version=3)
    _refused(tmp_path, v3, "version 3")
    with S.SensFile(scene["path"]) as f:
        c2, d3 = f.color_index[2].tolist(), f.depth_index[3].tolist()
    _refused(tmp_path, data[:c2[0] + c2[1] // 2], "colour data of frame 2")       # cut inside a payload
    _refused(tmp_path, data[:d3[0] + d3[1] - 1], "depth data of frame 3")
    _refused(tmp_path, data[:c2[0] - 40], "record of frame 2")                     # cut inside a record header
    more, _ = U.write_sens(tmp_path / "more.sens", colors, depths, scene["poses"], (HC, WC), num_frames=5)
    _refused(tmp_path, more, "record of frame 4")                                  # more frames than records
    huge, _ = U.write_sens(tmp_path / "huge.sens", colors, depths, scene["poses"], (HC, WC), num_frames=1 << 40)
    _refused(tmp_path, huge, "do not fit")
    _refused(tmp_path, data[:50], "header")


def test_export_tree(scene, tmp_path):
    out = tmp_path / "tree"
    assert S.main(["export", str(scene["path"]), str(out), "--start", "1", "--stop", "4", "--step", "2"]) == 0
    assert sorted(p.name for p in (out / "color").iterdir()) == ["1.jpg", "3.jpg"]
    out = tmp_path / "all"
    assert S.main(["export", str(scene["path"]), str(out)]) == 0
    for i in range(4):
        assert (out / "color" / f"{i}.jpg").read_bytes() == scene["colors"][i]
        im = Image.open(out / "depth" / f"{i}.png")
        got = np.asarray(im)
        assert got.dtype == np.uint16 or im.mode.startswith("I;16")
        np.testing.assert_array_equal(got.astype(np.uint16), scene["depths"][i])
        lines = (out / "pose" / f"{i}.txt").read_text().splitlines()
        assert len(lines) == 4
        back = np.array([list(map(float, ln.split(" "))) for ln in lines])    # the reference's parse
        np.testing.assert_array_equal(back.astype(np.float32), scene["poses"][i])
    for name, want in (("intrinsic_depth", scene["Kd"]), ("intrinsic_color", scene["Kc"])):
        np.testing.assert_array_equal(np.loadtxt(out / "intrinsic" / f"{name}.txt").astype(np.float32), want)


def test_info_runs(scene, capsys):
    assert S.main(["info", str(scene["path"])]) == 0
    text = capsys.readouterr().out
    assert "StructureSensor" in text and "zlib_ushort" in text and "jpeg" in text
    assert "16 x 12" in text and "32 x 24" in text and "frames       4" in text
    assert "2 of 4" in text


def test_raw_depth_and_unsupported_kinds(scene, tmp_path):
    U.write_sens(tmp_path / "raw.sens", scene["colors"], scene["depths"], scene["poses"], (HC, WC), depth_compression=0)
    with S.SensFile(tmp_path / "raw.sens") as f:
        assert f.depth_index[0, 1] == 2 * HD * WD
        np.testing.assert_array_equal(np.array(f.depth_u16(2)), scene["depths"][2])
    U.write_sens(tmp_path / "occi.sens", scene["colors"], scene["depths"], scene["poses"], (HC, WC), depth_compression=2)
    with S.SensFile(tmp_path / "occi.sens") as f:
        with pytest.raises(ValueError, match="occi_ushort"):
            f.depth_u16(0)
    short = [zlib.compress(d.tobytes()[:-2]) for d in scene["depths"]]
    U.write_sens(tmp_path / "short.sens", scene["colors"], short, scene["poses"], (HC, WC), depth_hw=(HD, WD))
    with S.SensFile(tmp_path / "short.sens") as f:
        with pytest.raises(ValueError, match="expected"):
            f.depth_u16(0)
