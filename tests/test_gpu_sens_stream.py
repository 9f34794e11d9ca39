"""SensFrameStream on a container written by tests/sens_util.py yields the samples that
DecodedFrameStream yields for the tree `sens export` writes from it (GPU and host decode), frame
selection, raw-ushort depth, the refusal of other colour kinds, and one frame at ScanNet's sizes
through to DetectStage.preprocess_frames."""
import types

import numpy as np
import pytest
import torch
from PIL import Image

from tests import sens_util as U

pytestmark = pytest.mark.gpu

HC, WC, HD, WD = 96, 128, 48, 64
N, LOST_AT = 5, 2


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


def _scene_frames():
    from boxfusion_amd.synthetic import frame_rgbd
    colors, depths = [], []
    for i in range(N):
        colors.append(U.jpeg_bytes(frame_rgbd(i * 3, HC, WC)[0], quality=90))
        depths.append(np.clip(frame_rgbd(i * 3, HD, WD)[1] * 1000.0, 0, 65535).astype(np.uint16))
    poses = [U.LOST if i == LOST_AT else U.upright_pose((0.05 * i, 0.1, 1.2)) for i in range(N)]
    poses[3] = np.eye(4, dtype=np.float32)          # another orientation: the frame is rotated
    Kd = np.eye(4, dtype=np.float32)
    Kd[:2, :3] = [[57.8, 0, 31.5], [0, 57.8, 23.5]]
    return colors, depths, poses, Kd


@pytest.fixture(scope="module")
def scene(L, tmp_path_factory):
    """the container, its exported tree, and the tree's samples (GPU decode), computed once"""
    from boxfusion_amd import sens as S
    from boxfusion_amd.capture_stream import DecodedFrameStream
    tmp = tmp_path_factory.mktemp("sens")
    colors, depths, poses, Kd = _scene_frames()
    path = tmp / "scene0000_00.sens"
    U.write_sens(path, colors, depths, poses, (HC, WC), intrinsic_depth=Kd)
    tree = tmp / "tree"
    assert S.main(["export", str(path), str(tree)]) == 0
    f = S.SensFile(path)
    cps = [str(tree / "color" / f"{i}.jpg") for i in range(N)]
    dps = [str(tree / "depth" / f"{i}.png") for i in range(N)]
    args = (cps, dps, f.poses_filled(), Kd[:3, :3], f.depth_shift)
    want = list(DecodedFrameStream(*args, batch=3, color_decode="gpu"))
    yield dict(path=path, file=f, tree_args=args, want=want, colors=colors, depths=depths, poses=poses, Kd=Kd, tmp=tmp)
    f.close()


def assert_same_sample(got, want):
    for k in ("image", "depth"):
        assert got["wide"][k].dtype == want["wide"][k].dtype
        torch.testing.assert_close(got["wide"][k].cpu(), want["wide"][k].cpu(), rtol=0, atol=0)
    assert got["meta"] == want["meta"]
    g, w = got["sensor_info"], want["sensor_info"]
    torch.testing.assert_close(g.gt.RT, w.gt.RT, rtol=0, atol=0)
    torch.testing.assert_close(g.wide.T_gravity, w.wide.T_gravity, rtol=0, atol=0)
    torch.testing.assert_close(g.wide.RT, w.wide.RT, rtol=0, atol=0)
    torch.testing.assert_close(g.wide.image.K, w.wide.image.K, rtol=0, atol=0)
    torch.testing.assert_close(g.wide.depth.K, w.wide.depth.K, rtol=0, atol=0)
    assert g.wide.image.size == w.wide.image.size and g.wide.depth.size == w.wide.depth.size


def test_equals_exported_tree(scene):
    from boxfusion_amd.sens import SensFrameStream
    stream = SensFrameStream(scene["file"], batch=3)
    assert len(stream) == N
    got = list(stream)
    assert len(got) == len(scene["want"]) == N
    for g, w in zip(got, scene["want"]):
        assert_same_sample(g, w)
    # the lost pose was filled with the last valid one, the depth is the written one / depth_shift
    assert torch.equal(got[LOST_AT]["sensor_info"].gt.RT[0], torch.from_numpy(scene["poses"][LOST_AT - 1]))
    dep0 = scene["depths"][0].astype(np.float32) / np.float32(1000.0)
    np.testing.assert_array_equal(got[0]["wide"]["depth"].cpu().numpy().reshape(HD, WD), dep0)
    assert [s["meta"]["timestamp"] for s in got] == list(range(N))


def test_host_decode_equals_exported_tree(scene):
    from boxfusion_amd.capture_stream import DecodedFrameStream
    from boxfusion_amd.sens import SensFrameStream
    want = list(DecodedFrameStream(*scene["tree_args"], batch=3, color_decode="host", depth_decode="host"))
    got = list(SensFrameStream(str(scene["path"]), batch=3, color_decode="host", depth_decode="host"))
    assert len(got) == N
    for g, w in zip(got, want):
        assert_same_sample(g, w)
    for g, w in zip(got, scene["want"]):         # and the host decoders agree with the GPU ones
        assert_same_sample(g, w)


def test_start_step(scene):
    from boxfusion_amd.sens import SensFrameStream
    stream = SensFrameStream(scene["file"], batch=3, start=1, step=2)
    assert len(stream) == 2
    got = list(stream)
    assert [s["meta"]["timestamp"] for s in got] == [1, 3]
    for g, i in zip(got, (1, 3)):
        assert_same_sample(g, scene["want"][i])
    assert [s["meta"]["timestamp"] for s in SensFrameStream(scene["file"], start=2, stop=4, video_id=7)] == [2, 3]


def test_raw_ushort_depth(scene):
    from boxfusion_amd.sens import SensFile, SensFrameStream
    path = scene["tmp"] / "raw.sens"
    U.write_sens(path, scene["colors"], scene["depths"], scene["poses"], (HC, WC), intrinsic_depth=scene["Kd"],
                 depth_compression=0)
    with SensFile(path) as f:
        got = list(SensFrameStream(f, batch=2))
    assert len(got) == N
    for g, w in zip(got, scene["want"]):
        assert_same_sample(g, w)


def test_other_kinds_refused(scene):
    from boxfusion_amd.sens import SensFile, SensFrameStream
    for kw, name in ((dict(color_compression=1), "png"), (dict(color_compression=0), "raw"),
                     (dict(depth_compression=2), "occi_ushort")):
        path = scene["tmp"] / f"{name}.sens"
        U.write_sens(path, scene["colors"], scene["depths"], scene["poses"], (HC, WC), **kw)
        with SensFile(path) as f:
            with pytest.raises(ValueError, match=name) as e:
                SensFrameStream(f)
            assert str(path) in str(e.value)
    with pytest.raises(ValueError, match="depth_decode"):
        SensFrameStream(scene["file"], depth_decode="cpu")


def test_corrupt_depth_stream_raises(L, scene):
    from boxfusion_amd.sens import SensFile, SensFrameStream
    import zlib
    depths = [zlib.compress(d.tobytes()) for d in scene["depths"]]
    bad = bytearray(depths[1])
    bad[-1] ^= 1
    depths[1] = bytes(bad)
    path = scene["tmp"] / "corrupt.sens"
    U.write_sens(path, scene["colors"], depths, scene["poses"], (HC, WC), depth_hw=(HD, WD))
    with SensFile(path) as f:
        with pytest.raises(L.HipError, match="stream 1: Adler-32"):
            list(SensFrameStream(f, batch=4))


def test_scannet_sized_frame_reaches_preprocess(L, tmp_path):
    """1296 x 968 colour, 480 x 640 depth: the stream's sample and DetectStage.preprocess_frames on
    its depth (B = 1) -- shapes and dtypes only"""
    from boxfusion_amd.pipeline import DetectStage
    from boxfusion_amd.sens import SensFile, SensFrameStream
    from boxfusion_amd.synthetic import SCANNET_K, frame_rgbd
    rgb, d = frame_rgbd(0, 480, 640)
    color = U.jpeg_bytes(np.asarray(Image.fromarray(rgb).resize((1296, 968), Image.BILINEAR)), quality=90)
    d16 = np.clip(d * 1000.0, 0, 65535).astype(np.uint16)
    Kd = np.eye(4, dtype=np.float32)
    Kd[:3, :3] = SCANNET_K
    pose = U.upright_pose((0.0, 0.0, 1.5))
    U.write_sens(tmp_path / "one.sens", [color], [d16], [pose], (968, 1296), intrinsic_depth=Kd)
    with SensFile(tmp_path / "one.sens") as f:
        samples = list(SensFrameStream(f))
    assert len(samples) == 1
    img, dep = samples[0]["wide"]["image"], samples[0]["wide"]["depth"]
    assert tuple(img.shape) == (1, 3, 480, 640) and img.dtype == torch.uint8 and img.is_cuda
    assert tuple(dep.shape) == (1, 480, 640) and dep.dtype == torch.float32 and dep.is_cuda
    dev = dep.device
    for backproject in (False, True):
        stage = types.SimpleNamespace(backproject=backproject, dev=dev, last_frames=None,
                                      Kd_dev=torch.from_numpy(np.asarray(SCANNET_K, np.float32))[None].to(dev))
        out = DetectStage.preprocess_frames(stage, dep.contiguous(), pose[None])
        assert stage.last_frames is out
        assert tuple(out[0].shape) == (1, 480, 640) and out[0].dtype == torch.float32
        if backproject:
            assert out[2].shape[0] == 1 and out[2].dtype == torch.float32
