"""Host-side argument checks of the four batched decode wrappers (_lib.png_decode_u16,
zlib_decode_u16, png_decode_rgb, jpeg_decode_rgb).  They share one front end whose checks all run
before anything touches the device, so CPU tensors are enough here: a bad argument raises a HipError
that names the wrapper, and well-formed arguments get as far as the "need device tensors" error."""
import inspect

import pytest
import torch

from boxfusion_amd import build as B

H, W, N = 4, 6, 100
U16, U8, I = torch.uint16, torch.uint8, inspect.Parameter.empty
# name -> (output dtype, trailing output dims, the parameters after (data, offsets, H, W) with their defaults)
WRAPPERS = {
    "png_decode_u16": (U16, (), "files", dict(out=None, offsets_host=None, check=True, depth_scale=None, work=None)),
    "zlib_decode_u16": (U16, (), "streams", dict(out=None, offsets_host=None, check=True, depth_scale=None, work=None)),
    "png_decode_rgb": (U8, (3,), "files", dict(out=None, offsets_host=None, check=True, work=None)),
    "jpeg_decode_rgb": (U8, (3,), "files", dict(out=None, check=True, work=None, offsets_host=None)),
}


@pytest.fixture(scope="module")
def L():
    B.build()
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


def call(L, name, offs, **kw):
    """the wrapper on N CPU bytes, the offsets given both as the [F+1] tensor and on the host"""
    kw.setdefault("offsets_host", offs)
    return getattr(L, name)(torch.zeros(N, dtype=torch.uint8), torch.tensor(offs, dtype=torch.int64), H, W, **kw)


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_signature(L, name):
    _, _, data, tail = WRAPPERS[name]
    want = [(data, I), ("offsets", I), ("H", I), ("W", I)] + list(tail.items())
    assert [(p.name, p.default) for p in inspect.signature(getattr(L, name)).parameters.values()] == want


@pytest.mark.parametrize("name", sorted(WRAPPERS))
@pytest.mark.parametrize("offs,host,why", [
    ([0, 40, 100], [0, 100], r"offsets \[F\+1\]"),               # host offsets of another length
    ([0, 40, 100], [0], r"offsets \[F\+1\]"),
    ([-1, 40, 100], None, "offsets must not decrease"),          # negative first offset
    ([0, 60, 50], None, "offsets must not decrease"),            # a decreasing pair
    ([10, 5, 100], None, "offsets must not decrease"),
    ([0, 40, N + 1], None, "offsets run past"),                  # last offset past numel()
])
def test_bad_offsets(L, name, offs, host, why):
    with pytest.raises(L.HipError, match=f"{name}: {why}"):
        call(L, name, offs, offsets_host=offs if host is None else host)


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_bad_out(L, name):
    dt, tail, _, _ = WRAPPERS[name]
    shape = "F,H,W,3" if tail else "F,H,W"
    with pytest.raises(L.HipError, match=f"{name}: out: expected {dt}"):
        call(L, name, [0, 40, 100], out=torch.zeros((2, H, W, *tail), dtype=torch.int32))
    with pytest.raises(L.HipError, match=rf"{name}: out \[{shape}\]"):
        call(L, name, [0, 40, 100], out=torch.zeros((3, H, W, *tail), dtype=dt))
    if not tail:                                                 # depth_scale given: the output is f32
        with pytest.raises(L.HipError, match=f"{name}: out: expected torch.float32"):
            call(L, name, [0, 40, 100], out=torch.zeros((2, H, W), dtype=dt), depth_scale=1000.0)


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_bad_input_dtypes(L, name):
    fn = getattr(L, name)
    with pytest.raises(L.HipError, match=f"{name}: .*expected torch.uint8"):
        fn(torch.zeros(N, dtype=torch.int8), torch.tensor([0, N]), H, W, offsets_host=[0, N])
    with pytest.raises(L.HipError, match=f"{name}: offsets: expected torch.int64"):
        fn(torch.zeros(N, dtype=torch.uint8), torch.tensor([0, N], dtype=torch.int32), H, W, offsets_host=[0, N])


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_well_formed_arguments_reach_the_device_check(L, name):
    dt, tail, _, _ = WRAPPERS[name]
    for kw in (dict(), dict(out=torch.zeros((2, H, W, *tail), dtype=dt)),
               dict(work=torch.zeros(1, dtype=torch.uint8), check=False)):
        with pytest.raises(L.HipError, match="need device tensors"):
            call(L, name, [0, 40, 100], **kw)
    with pytest.raises(L.HipError, match="need device tensors"):        # offsets may start past 0
        call(L, name, [4, 40, 90])


@pytest.mark.parametrize("name", sorted(WRAPPERS))
def test_empty_batch_returns_without_a_launch(L, name):
    dt, tail, _, _ = WRAPPERS[name]
    out, st = call(L, name, [0])
    assert tuple(out.shape) == (0, H, W, *tail) and out.dtype == dt
    assert tuple(st.shape) == (0,) and st.dtype == torch.int32


def test_jpeg_without_host_offsets_reads_nothing_back(L):
    """bench.py calls jpeg_decode_rgb without host offsets inside timed regions: then the offsets'
    values are not looked at on the host (no device read-back), only their count"""
    files = torch.zeros(N, dtype=torch.uint8)
    with pytest.raises(L.HipError, match="need device tensors"):
        L.jpeg_decode_rgb(files, torch.tensor([0, 60, 50]), H, W)
    with pytest.raises(L.HipError, match=r"jpeg_decode_rgb: offsets \[F\+1\]"):
        L.jpeg_decode_rgb(files, torch.zeros(0, dtype=torch.int64), H, W)
