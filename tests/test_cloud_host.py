"""Host side of the scene cloud (no GPU): the point-cloud PLY writer / reader, Pillow's bicubic
coefficient tables restated in _lib.pil_bicubic_coeffs, the `sens cloud` command line, and the
header's declarations."""
import os
import re

import numpy as np
import pytest

from boxfusion_amd import _lib
from boxfusion_amd import build as B
from boxfusion_amd.visualize import points_to_ply, read_ply_points

# (n_in, n_out) of every axis of the image size pairs the GPU test resizes
AXES = [(48, 24), (64, 32), (48, 12), (64, 16), (64, 48), (48, 32), (40, 13), (56, 19), (24, 48), (32, 64)]


def test_points_ply_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    xyz = rng.normal(0, 3, (257, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (257, 3), dtype=np.uint8)
    path = tmp_path / "sub" / "cloud.ply"
    points_to_ply(xyz, rgb, str(path))
    data = path.read_bytes()
    head = data[:data.index(b"end_header\n") + 11].decode("ascii")
    assert head == ("ply\nformat binary_little_endian 1.0\nelement vertex 257\n"
                    "property float x\nproperty float y\nproperty float z\n"
                    "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    assert len(data) == len(head) + 257 * 15
    got_xyz, got_rgb = read_ply_points(str(path))
    assert got_xyz.dtype == np.float32 and got_rgb.dtype == np.uint8
    np.testing.assert_array_equal(got_xyz, xyz)
    np.testing.assert_array_equal(got_rgb, rgb)


def test_points_ply_empty(tmp_path):
    path = str(tmp_path / "empty.ply")
    points_to_ply(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8), path)
    assert b"element vertex 0\n" in open(path, "rb").read()
    xyz, rgb = read_ply_points(path)
    assert xyz.shape == (0, 3) and rgb.shape == (0, 3)
    with pytest.raises(ValueError):
        points_to_ply(np.zeros((2, 3)), np.zeros((1, 3), np.uint8), path)


def apply_table(line, n_out):
    """one Pillow 8-bit resample pass along axis 0 of line u8 [n_in, c], in numpy"""
    bounds, coeffs = _lib.pil_bicubic_coeffs(line.shape[0], n_out)
    out = np.zeros((n_out,) + line.shape[1:], np.uint8)
    for i, (lo, n) in enumerate(bounds):
        acc = (line[lo:lo + n].astype(np.int64) * coeffs[i, :n, None]).sum(0) + (1 << 21)
        out[i] = np.clip(acc >> 22, 0, 255)
    return out


@pytest.mark.parametrize("n_in,n_out", AXES)
def test_pil_bicubic_coeffs_vs_pillow(n_in, n_out):
    from PIL import Image
    rng = np.random.default_rng(n_in * 1000 + n_out)
    bounds, coeffs = _lib.pil_bicubic_coeffs(n_in, n_out)
    assert bounds.dtype == np.int32 and coeffs.dtype == np.int32 and bounds.shape == (n_out, 2)
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= n_in).all()
    assert (bounds[:, 1] <= coeffs.shape[1]).all()
    for img in (rng.integers(0, 256, (1, n_in, 3), dtype=np.uint8), np.full((1, n_in, 3), 255, np.uint8),
                np.tile(np.array([0, 255], np.uint8).repeat(3).reshape(2, 3), (n_in // 2, 1))[None]):
        want = np.array(Image.fromarray(img).resize((n_out, 1)))
        np.testing.assert_array_equal(apply_table(img[0], n_out), want[0])


def test_sens_cloud_arguments(tmp_path, capsys):
    from boxfusion_amd.sens import main
    for bad in (["cloud"], ["cloud", "a.sens"], ["cloud", "a.sens", "o.ply", "--voxel", "x"],
                ["cloud", "a.sens", "o.ply", "--voxel", "0"], ["cloud", "a.sens", "o.ply", "--step", "0"],
                ["cloud", "a.sens", "o.ply", "--max-depth", "-1"], ["cloud", "a.sens", "o.ply", "--nope"]):
        with pytest.raises(SystemExit) as e:
            main(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
    with pytest.raises(FileNotFoundError):          # well-formed arguments reach the file
        main(["cloud", str(tmp_path / "missing.sens"), str(tmp_path / "o.ply"), "--voxel", "0.05", "--start", "1",
              "--stop", "9", "--step", "2", "--max-depth", "5"])


def test_header_declares_cloud_entry_points():
    src = open(os.path.join(os.path.dirname(B.HERE), "include", "boxfusion_hip.h")).read()
    for name in ("bf_resize_bicubic_u8", "bf_cloud_pack", "bf_cloud_integrate", "bf_cloud_extract"):
        assert re.search(rf"^int\s+{name}\s*\(", src, re.M), name
    assert "bf_cloud.hip" in B.SOURCES and B.SOURCES["bf_cloud.hip"] == B.EXACT
