"""Direct tests of the decoder-tail kernels of bf_dec_native.hip: the predictor heads
(bf_row_heads_f32, all four modes), top-k, the proposal and the inference selection, and the edges
of ln_rows / groupnorm_cl / s2d / gemm_f32 that the engine's own shapes never reach.

Every reference is plain torch in float64 on the CPU, built from the same f32 inputs upcast; the
transform formulas are those of cubify_transformer.py (ScalePredictor, ClassPredictor,
DeltaBox2DTransform.apply_deltas + box_xyxy_to_cxcywh, AbsoluteBox3DPredictor,
Box2DPromptEncoderLearned, inference_single_image) written dtype-generic below.  Inputs are drawn
on the CPU from seeded generators, so they are the same on every machine.

Tolerances
  * linear outputs (class logits, box deltas, z_unscaled): the derivable bound
    |err| <= (K + 2) 2^-24 (sum_i |x_i| |w_ji| + |b_j|) that holds for any f32 summation order.
  * transformed outputs: 4 x the error of torch's own f32 evaluation of the same formula on the same
    inputs against the float64 reference (F32_ERR below; maxima over every parametrised case,
    measured once with torch on a CPU), with a floor of 4 ulp at the field's magnitude.  The margin
    covers the kernel's wave-tree sum and FMA contraction, which legitimately differ from torch's.
    Each test prints the kernel's figure and torch-f32's on the machine at hand before it asserts
    (the latter moves by a factor of about two with the CPU's matmul; the constants stay).
  * gathers and copies: bit for bit.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SENT = -777.25                 # sentinel of every output buffer: untouched memory keeps it
U24 = 2.0 ** -24
MAX_RATIO = float(torch.tensor(abs(math.log(0.016)), dtype=torch.float32))   # the engine's f32 value
CLAMP_WH = (96.0, 64.0)

# torch-f32 vs float64 on the inputs of this module, per output field (max over all cases).
# "rel" fields are max |a - b| / |b|, the others max |a - b|.
F32_ERR = {
    "box2d.boxes": 1.75e-4,       # cxcywh after apply_deltas + clamp, magnitudes <= 96
    "box3d.proj_xy": 4.67e-5,     # magnitudes <= 96
    "box3d.z_scaled": 6.08e-6,    # |z_scaled| <~ 25
    "box3d.dims": 4.09e-6,        # rel
    "box3d.R": 4.73e-6,           # cos / sin of the yaw, |yaw| <~ 12
    "scale.tokens": 6.55e-7,      # rel, exp of a logit with |logit| <~ 10
    "infer.scores": 8.59e-8,      # sigmoid, magnitude 1
    "infer.boxes": 3.82e-6,       # xyxy, magnitudes <= 96
    "infer.xyz": 9.08e-5,         # K^-1 (z u, z v, z), magnitudes <~ 1000
    "infer.R": 4.75e-7,           # T_gravity P, magnitudes <~ 8
}
REL_FIELDS = {"box3d.dims", "scale.tokens"}
# LayerNorm of rows with a large mean (x = 1000 + N(0, 1)): torch-f32's rel error against float64
LN_LARGE_MEAN_F32_REL = 9.79e-6


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from boxfusion_amd import _lib
    _lib.lib()
    return _lib


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def ulp32(m):
    """spacing of f32 at magnitude m"""
    return 2.0 ** (math.floor(math.log2(m)) - 23) if m > 0 else 2.0 ** -149


def field_err(field, got, ref):
    d = (got.double() - ref.double()).abs()
    if field in REL_FIELDS:
        d = d / ref.double().abs()
    return d.max().item()


def field_bound(field, ref):
    floor = 4 * 2.0 ** -23 if field in REL_FIELDS else 4 * ulp32(ref.abs().max().item())
    return max(4 * F32_ERR[field], floor)


def check_field(field, got, ref64, ref32):
    e, e32, bnd = field_err(field, got, ref64), field_err(field, ref32, ref64), field_bound(field, ref64)
    print(f"{field}: kernel {e:.3e}  torch-f32 {e32:.3e}  bound {bnd:.3e}")
    assert e <= bnd, f"{field}: {e:.3e} > {bnd:.3e}"


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a.cpu().float()), bits(b.cpu().float()))


# ------------------------------------------------------------------------------------------
# 1. row_heads
# ------------------------------------------------------------------------------------------
HEAD_K = [256, 512]
HEAD_FQ = [(1, 1), (1, 5), (1, 37), (3, 1), (3, 5), (3, 37)]     # rows = frames * nq: never a multiple of 4
HEAD_OFF = [0, 2]
CLASS_NOUT = [1, 3, 8]


def heads_inputs(mode, K, frames, nq, in_off, nout):
    """x ~ N(0, 1) as a column slice of a wider buffer, n = in_off + nq + 1 rows per frame; w, b scaled
    so the raw outputs have a standard deviation of about 3"""
    g = torch.Generator().manual_seed(1000 * K + 100 * frames + 10 * nq + in_off + 7 * nout)
    in_fs, rows = in_off + nq + 1, frames * nq
    xbuf = torch.randn(frames * in_fs, K + 8, generator=g)
    w = torch.randn(nout, K, generator=g) * (3.0 / math.sqrt(K))
    b = torch.randn(nout, generator=g) * 0.5
    cw, ch = CLAMP_WH
    prop = torch.cat((torch.rand(rows, 1, generator=g) * cw, torch.rand(rows, 1, generator=g) * ch,
                      2 + 28 * torch.rand(rows, 2, generator=g)), 1)
    params = torch.tensor([[0.3 + 0.4 * f, 0.7 + 0.5 * f] for f in range(frames)])
    xs = xbuf[:, 4:4 + K].reshape(frames, in_fs, K)[:, in_off:in_off + nq].reshape(rows, K)
    return dict(mode=mode, K=K, frames=frames, nq=nq, in_off=in_off, in_fs=in_fs, rows=rows, xbuf=xbuf,
                xs=xs.contiguous(), w=w, b=b, prop=prop, params=params)


def linear(inp, dtype):
    return inp["xs"].to(dtype) @ inp["w"].to(dtype).T + inp["b"].to(dtype)


def linear_bound(inp):
    """|f32 result - exact| of sum_i x_i w_ji + b_j in any summation order"""
    s = inp["xs"].double().abs() @ inp["w"].double().abs().T + inp["b"].double().abs()
    return (inp["K"] + 2) * U24 * s


def clamp_cols(b, cw, ch):
    return torch.stack([b[:, c].clamp(0, cw if c % 2 == 0 else ch) for c in range(b.shape[1])], 1)


def box2d_formula(d, prop, dtype):
    """DeltaBox2DTransform.apply_deltas + box_xyxy_to_cxcywh; also the unclamped xyxy"""
    d, prop = d.to(dtype), prop.to(dtype)
    dwh = d[:, 2:].clamp(min=-MAX_RATIO, max=MAX_RATIO)
    gxy = prop[:, :2] + prop[:, 2:] * d[:, :2]
    gwh = prop[:, 2:] * dwh.exp()
    raw = torch.cat((gxy - gwh * 0.5, gxy + gwh * 0.5), 1)
    x0, y0, x1, y1 = clamp_cols(raw, *CLAMP_WH).unbind(1)
    return torch.stack(((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0), 1), raw


def box2d_branches(d, raw):
    cw, ch = CLAMP_WH
    return {"d_w > max_ratio": (d[:, 2] > MAX_RATIO).any(), "d_w < -max_ratio": (d[:, 2] < -MAX_RATIO).any(),
            "d_h > max_ratio": (d[:, 3] > MAX_RATIO).any(), "d_h < -max_ratio": (d[:, 3] < -MAX_RATIO).any(),
            "x < 0": (raw[:, 0] < 0).any(), "x > W": (raw[:, 2] > cw).any(),
            "y < 0": (raw[:, 1] < 0).any(), "y > H": (raw[:, 3] > ch).any(),
            "inside": ((raw[:, :2] > 0).all(1) & (raw[:, 2] < cw) & (raw[:, 3] < ch)).any()}


def box3d_formula(o, inp, dtype):
    """AbsoluteBox3DPredictor: the 16 floats per row in the kernel's stored order"""
    o, prop = o.to(dtype), inp["prop"].to(dtype)
    par = inp["params"].to(dtype).repeat_interleave(inp["nq"], 0)     # row r = f * nq + q -> params[f]
    shift, scale = par[:, 0:1], par[:, 1:2]
    d2, z, dims, yaw = torch.split(o, (2, 1, 3, 1), 1)
    raw = prop[:, :2] + d2 * prop[:, 2:]
    c, s, zero, one = yaw.cos(), yaw.sin(), torch.zeros_like(yaw), torch.ones_like(yaw)
    return {"proj_xy": clamp_cols(raw, *CLAMP_WH), "z": z, "z_scaled": scale * z + shift,
            "dims": torch.exp(dims.clip(max=5)) * scale,
            "R": torch.cat((c, zero, s, zero, one, zero, -s, zero, c), 1), "raw_xy": raw}


def box3d_branches(o, raw):
    cw, ch = CLAMP_WH
    return {"dims logit > 5": (o[:, 3:6] > 5).any(), "dims logit < 5": (o[:, 3:6] < 5).any(),
            "yaw > pi": (o[:, 6] > math.pi).any(), "yaw < -pi": (o[:, 6] < -math.pi).any(),
            "x < 0": (raw[:, 0] < 0).any(), "x > W": (raw[:, 0] > cw).any(),
            "y < 0": (raw[:, 1] < 0).any(), "y > H": (raw[:, 1] > ch).any()}


def assert_branches(br):
    missed = [k for k, v in br.items() if not bool(v)]
    assert not missed, f"inputs never take the branches {missed}"


def dev_x(inp):
    xb = inp["xbuf"].cuda()
    return xb[:, 4:4 + inp["K"]]          # ldx = K + 8 > K, 16-byte aligned


def out_buf(rows, cols):
    return torch.full((rows + 3, cols), SENT, device="cuda")


def assert_untouched(buf, rows, cols):
    """everything of a sentinel-filled buffer outside [:rows, :cols] is as it was"""
    b = buf.cpu()
    assert (b[rows:] == SENT).all() and (b[:rows, cols:] == SENT).all()


@pytest.mark.parametrize("nout", CLASS_NOUT)
@pytest.mark.parametrize("in_off", HEAD_OFF)
@pytest.mark.parametrize("frames,nq", HEAD_FQ)
@pytest.mark.parametrize("K", HEAD_K)
def test_row_heads_class(L, K, frames, nq, in_off, nout):
    inp = heads_inputs("class", K, frames, nq, in_off, nout)
    rows = inp["rows"]
    out = out_buf(rows, nout + 3)
    L.row_heads(dev_x(inp), inp["in_fs"], in_off, rows, nq, inp["w"].cuda(), inp["b"].cuda(), "class", out=out)
    got = out.cpu()[:rows, :nout]
    assert ((got.double() - linear(inp, torch.float64)).abs() <= linear_bound(inp)).all()
    assert_untouched(out, rows, nout)


def run_box2d(L, inp, with_out=True, inplace=False):
    rows = inp["rows"]
    out = out_buf(rows, 6) if with_out else None
    boxes = torch.full((rows + 3, 4), SENT, device="cuda")
    if inplace:
        boxes[:rows] = inp["prop"].cuda()
        prop = boxes
    else:
        prop = inp["prop"].cuda()
    L.row_heads(dev_x(inp), inp["in_fs"], inp["in_off"], rows, inp["nq"], inp["w"].cuda(), inp["b"].cuda(),
                "box2d", out=out, prop=prop, boxes=boxes, clamp_wh=CLAMP_WH, max_ratio=MAX_RATIO)
    return out, boxes


@pytest.mark.parametrize("in_off", HEAD_OFF)
@pytest.mark.parametrize("frames,nq", HEAD_FQ)
@pytest.mark.parametrize("K", HEAD_K)
def test_row_heads_box2d(L, K, frames, nq, in_off):
    inp = heads_inputs("box2d", K, frames, nq, in_off, 4)
    rows = inp["rows"]
    d64 = linear(inp, torch.float64)
    ref, raw = box2d_formula(d64, inp["prop"], torch.float64)
    if rows >= 100:
        assert_branches(box2d_branches(d64, raw))
    out, boxes = run_box2d(L, inp)
    assert ((out.cpu()[:rows, :4].double() - d64).abs() <= linear_bound(inp)).all()
    ref32 = box2d_formula(linear(inp, torch.float32), inp["prop"], torch.float32)[0]
    check_field("box2d.boxes", boxes.cpu()[:rows], ref, ref32)
    assert_untouched(out, rows, 4)
    assert_untouched(boxes, rows, 4)


@pytest.mark.parametrize("K", HEAD_K)
def test_row_heads_box2d_no_deltas_and_in_place(L, K):
    """out=None emits the boxes alone; prop and boxes the same tensor (the decoder layers' REF)
    gives the out-of-place result bit for bit"""
    inp = heads_inputs("box2d", K, 3, 37, 2, 4)
    rows = inp["rows"]
    _, boxes = run_box2d(L, inp)
    out_n, boxes_n = run_box2d(L, inp, with_out=False)
    assert out_n is None and torch.equal(bits(boxes_n), bits(boxes))
    out_i, boxes_i = run_box2d(L, inp, inplace=True)
    assert torch.equal(bits(boxes_i), bits(boxes))
    assert_untouched(out_i, rows, 4)


@pytest.mark.parametrize("in_off", HEAD_OFF)
@pytest.mark.parametrize("frames,nq", HEAD_FQ)
@pytest.mark.parametrize("K", HEAD_K)
def test_row_heads_box3d(L, K, frames, nq, in_off):
    inp = heads_inputs("box3d", K, frames, nq, in_off, 7)
    rows = inp["rows"]
    o64 = linear(inp, torch.float64)
    ref = box3d_formula(o64, inp, torch.float64)
    if rows >= 100:
        assert_branches(box3d_branches(o64, ref["raw_xy"]))
    out = out_buf(rows, 20)
    L.row_heads(dev_x(inp), inp["in_fs"], in_off, rows, nq, inp["w"].cuda(), inp["b"].cuda(), "box3d", out=out,
                prop=inp["prop"].cuda(), params=inp["params"].cuda(), clamp_wh=CLAMP_WH)
    got = out.cpu()[:rows]
    ref32 = box3d_formula(linear(inp, torch.float32), inp, torch.float32)
    assert ((got[:, 2:3].double() - ref["z"]).abs() <= linear_bound(inp)[:, 2:3]).all()
    check_field("box3d.proj_xy", got[:, 0:2], ref["proj_xy"], ref32["proj_xy"])
    check_field("box3d.z_scaled", got[:, 3:4], ref["z_scaled"], ref32["z_scaled"])
    check_field("box3d.dims", got[:, 4:7], ref["dims"], ref32["dims"])
    check_field("box3d.R", got[:, 7:16], ref["R"], ref32["R"])
    # the constant entries of R_Y(yaw) = [c 0 s; 0 1 0; -s 0 c] are exact, and R[2,0] = -R[0,2]
    assert torch.equal(got[:, [8, 10, 12, 14]], torch.zeros(rows, 4)) and torch.equal(got[:, 11], torch.ones(rows))
    assert torch.equal(got[:, 13], -got[:, 9]) and torch.equal(got[:, 15], got[:, 7])
    assert_untouched(out, rows, 16)


def scale_formula(inp, dtype):
    """ScalePredictor: out[f] = (exp(shift(x[f, 0])), exp(scale(x[f, 1]))), W = [shift.w; scale.w]"""
    x = inp["xs"].to(dtype).view(inp["frames"], inp["nq"], -1)
    w, b = inp["w"].to(dtype), inp["b"].to(dtype)
    return torch.stack((torch.exp(x[:, 0] @ w[0] + b[0]), torch.exp(x[:, 1] @ w[1] + b[1])), 1)


SCALE_CASES = [(K, frames, n, in_off) for K in HEAD_K for frames in (1, 3) for n in (3, 5) for in_off in HEAD_OFF]


@pytest.mark.parametrize("K,frames,n,in_off", SCALE_CASES)
def test_row_heads_scale(L, K, frames, n, in_off):
    inp = heads_inputs("scale", K, frames, n, in_off, 2)
    out = torch.full((frames + 2, 2), SENT, device="cuda")
    L.row_heads(dev_x(inp), inp["in_fs"], in_off, frames * n, n, inp["w"].cuda(), inp["b"].cuda(), "scale", out=out)
    got = out.cpu()
    check_field("scale.tokens", got[:frames], scale_formula(inp, torch.float64), scale_formula(inp, torch.float32))
    assert (got[frames:] == SENT).all()


def test_row_heads_argument_checks(L):
    """refused on the host, before any launch"""
    z = lambda *s: torch.zeros(*s, device="cuda")
    x, out, b, prop = z(4, 256), z(4, 16), z(16), z(4, 4)
    with pytest.raises(L.HipError):       # K = 128
        L.row_heads(z(4, 128), 4, 0, 4, 4, z(3, 128), b, "class", out=out)
    with pytest.raises(L.HipError):       # nout = 9
        L.row_heads(x, 4, 0, 4, 4, z(9, 256), b, "class", out=out)
    with pytest.raises(L.HipError):       # box2d with nout != 4
        L.row_heads(x, 4, 0, 4, 4, z(3, 256), b, "box2d", out=out, prop=prop, boxes=z(4, 4))
    with pytest.raises(L.HipError):       # box3d with ldo < 16
        L.row_heads(x, 4, 0, 4, 4, z(7, 256), b, "box3d", out=z(4, 8), prop=prop, params=z(1, 2))
    with pytest.raises(L.HipError):       # x off the 16-byte alignment
        L.row_heads(z(4 * 256 + 4)[1:1 + 4 * 256].view(4, 256), 4, 0, 4, 4, z(3, 256), b, "class", out=out)


# ------------------------------------------------------------------------------------------
# 2. topk_rows
# ------------------------------------------------------------------------------------------
def stable_desc(v):
    """stable descending order of the float64 values along the last axis"""
    return torch.sort(v.double(), dim=-1, descending=True, stable=True)[1]


NAN = float("nan")


@pytest.mark.parametrize("vals,k,want", [
    ([1, NAN, 3, NAN, 2], 5, [2, 4, 0, 1, 3]),
    ([1, NAN, 3, NAN, 2], 4, [2, 4, 0, 1]),
    ([NAN, NAN, NAN, 7, NAN, NAN, NAN, NAN], 8, [3, 0, 1, 2, 4, 5, 6, 7]),
])
def test_topk_rows_nan_sorts_last_by_index(L, vals, k, want):
    """non-NaN first, then the NaN rows by ascending index; never a padding index (>= n).
    (Before the comparator was made a total order the first case gave [2, 4, 0, 10, 11].)"""
    v = torch.tensor([vals], dtype=torch.float32, device="cuda")
    got = torch.full((1, k), -1.0, device="cuda")
    idx = L.topk_rows(v, 1, len(vals), k, vals=got)
    assert idx[0].tolist() == want
    assert same_bits(got[0], v[0, want])


@pytest.mark.parametrize("n", [3, 100])
def test_topk_rows_infinities(L, n):
    g = torch.Generator().manual_seed(n)
    v = torch.randn(4, n, generator=g)
    v[:, 0], v[:, n - 1] = float("-inf"), float("inf")
    if n > 3:
        v[1, 5:9] = float("-inf")
        v[2, 20:23] = float("inf")
        v[3, 1::2] = float("-inf")
    for k in (n, max(1, n // 3)):
        idx = L.topk_rows(v.cuda(), 4, n, k).cpu().long()
        assert (idx >= 0).all() and (idx < n).all()
        assert torch.equal(idx, stable_desc(v)[:, :k])


@pytest.mark.parametrize("ldv", [1, 3])
@pytest.mark.parametrize("n", [3, 100, 2100, 4096])
def test_topk_rows_vals_output(L, n, ldv):
    g = torch.Generator().manual_seed(10 * n + ldv)
    frames = 3
    buf = torch.randn(frames, n, ldv, generator=g)
    v = buf[..., 0]
    for k in sorted({1, (n + 1) // 2, n}):
        vals = torch.full((frames, k), SENT, device="cuda")
        idx = L.topk_rows(buf.cuda(), frames, n, k, ldv=ldv, vals=vals).cpu().long()
        assert torch.equal(idx, stable_desc(v)[:, :k])
        assert same_bits(vals, torch.gather(v, 1, idx))


@pytest.mark.parametrize("n,k", [(600, 100), (37, 20), (64, 33)])
def test_topk_rows_equal_blocks(L, n, k):
    """runs of equal values that straddle the k cut: lower index first, as a stable sort"""
    g = torch.Generator().manual_seed(n + k)
    frames = 3
    v = torch.randint(0, 5, (frames, n), generator=g).float()            # 5 levels, ~n/5 of each
    v[1] = torch.randint(0, 3, (n // 8 + 1,), generator=g).float().repeat_interleave(8)[:n]   # contiguous blocks
    order = stable_desc(v)
    cut = torch.gather(v, 1, order[:, k - 1:k + 1])
    assert (cut[:, 0] == cut[:, 1]).any(), "no block of equal values straddles the cut"
    idx = L.topk_rows(v.cuda(), frames, n, k).cpu().long()
    assert torch.equal(idx, order[:, :k])


def test_topk_rows_argument_checks(L):
    v = torch.zeros(1, 4097, device="cuda")
    with pytest.raises(L.HipError):       # capacity
        L.topk_rows(v, 1, 4097, 10)
    with pytest.raises(L.HipError):       # k > n
        L.topk_rows(v, 1, 8, 9)


# ------------------------------------------------------------------------------------------
# 3. prop_select
# ------------------------------------------------------------------------------------------
MAX_E = 31.0


def prop_coords(count, g):
    """box coordinates cycling through every truncation case of clamp(c, 0, max_e).int()"""
    r = torch.rand(count, generator=g)
    whole = torch.randint(0, int(MAX_E), (count,), generator=g).float()
    kinds = [whole,                              # exact integers
             whole + 0.25 + 0.5 * r,             # fractional part in [0.25, 0.75]
             -0.25 - 40 * r,                     # negative
             MAX_E + 0.01 + 49.98 * r,           # in (max_e, max_e + 50)
             torch.full((count,), MAX_E)]        # exactly max_e
    return torch.stack(kinds, 1)[torch.arange(count), torch.arange(count) % len(kinds)]


PROP_CASES = [(frames, n, k, ed) for frames in (1, 3) for n, k in ((7, 1), (7, 5), (600, 1), (600, 5), (600, 300))
              for ed in (64, 40)]


@pytest.mark.parametrize("frames,n,k,ed", PROP_CASES)
def test_prop_select(L, frames, n, k, ed):
    g = torch.Generator().manual_seed(1000 * frames + n + 10 * k + ed)
    boxes = prop_coords(frames * n * 4, g)[torch.randperm(frames * n * 4, generator=g)].view(frames, n, 4)
    idx = torch.empty(frames, k, dtype=torch.int64)
    for f in range(frames):          # a random permutation prefix that holds index 0 and / or n - 1
        ends = [0, n - 1] if f % 2 == 0 else [n - 1, 0]
        order = torch.tensor(ends + (1 + torch.randperm(n - 2, generator=g)).tolist())[:k]
        idx[f] = order[torch.randperm(k, generator=g)]
    embs = [torch.randn(int(MAX_E) + 1, ed, generator=g) + 10 * t for t in range(4)]     # distinct tables
    qfs, qoff, ldq = k + 3, 2, 4 * ed + 8
    qbuf = torch.full((frames * qfs, ldq), SENT, device="cuda")
    ref = torch.full((frames * k + 1, 4), SENT, device="cuda")
    L.prop_select(boxes.cuda(), frames, n, k, idx.int().cuda(), ref, tuple(e.cuda() for e in embs), MAX_E,
                  qbuf[:, 4:4 + 4 * ed], qfs, qoff)
    want = torch.gather(boxes, 1, idx[:, :, None].expand(-1, -1, 4))                    # [frames, k, 4]
    assert same_bits(ref[:frames * k], want.view(-1, 4)) and (ref[frames * k:] == SENT).all()
    e = want.double().clamp(0, MAX_E).long()                                            # truncation
    if frames * k >= 15:             # every truncation case is among the selected coordinates
        c = want.flatten()
        assert (c < 0).any() and (c > MAX_E).any() and (c == MAX_E).any() and e.min() == 0 and e.max() == int(MAX_E)
        assert ((c > 0) & (c < MAX_E) & (c == c.floor())).any() and ((c > 0) & (c < MAX_E) & (c != c.floor())).any()
    qwant = torch.full((frames, qfs, ldq), SENT)
    qwant[:, qoff:qoff + k, 4:4 + 4 * ed] = torch.cat([embs[t][e[..., t]] for t in range(4)], -1)
    assert same_bits(qbuf, qwant.view(frames * qfs, ldq))


# ------------------------------------------------------------------------------------------
# 4. infer_select
# ------------------------------------------------------------------------------------------
INFER_SHAPES = [(300, 1, 100), (37, 3, 20), (64, 64, 100), (5, 7, 35), (5, 7, 1)]
INFER_VARIANTS = [(256, True), (24, False)]      # (C, with T_gravity)


def infer_inputs(nq, nc, k, frames, C, with_tg):
    g = torch.Generator().manual_seed(100000 * frames + 100 * nq + nc + 7 * k + C)
    n = nq * nc
    logits = torch.empty(frames, n)
    for f in range(frames):
        s = torch.linspace(8, -8, n, dtype=torch.float64).float()       # evenly spaced, descending
        s[1] = s[0]                                                     # exact duplicates: at the top,
        if k < n:
            s[k] = s[k - 1]                                             # across the k cut,
        s[n - 1] = s[n - 2]                                             # and at the bottom
        logits[f] = s[torch.randperm(n, generator=g)]
    wh = torch.tensor([[64.0 + 16 * f, 48.0 + 8 * f] for f in range(frames)])
    boxes = torch.empty(frames, nq, 4)
    for f in range(frames):
        W, H = wh[f].tolist()
        b = torch.stack((torch.rand(nq, generator=g) * W, torch.rand(nq, generator=g) * H,
                         2 + 20 * torch.rand(nq, generator=g), 2 + 20 * torch.rand(nq, generator=g)), 1)
        q = torch.arange(nq)
        b[q % 4 == 0, 0] = 0.5              # x0 < 0
        b[q % 4 == 1, 1] = 0.5              # y0 < 0
        b[q % 4 == 2, 0] = W - 0.5          # x1 > W
        b[q % 4 == 3, 1] = H - 0.5          # y1 > H
        boxes[f] = b
    b3 = torch.randn(frames * nq, 16, generator=g)
    b3[:, 0:2] = 60 * torch.rand(frames * nq, 2, generator=g)
    b3[:, 3] = 0.5 + 4.5 * torch.rand(frames * nq, generator=g)
    b3[:, 4:7] = 0.1 + 3 * torch.rand(frames * nq, 3, generator=g)
    desc_fs = nq + 3
    return dict(nq=nq, nc=nc, k=k, frames=frames, C=C, logits=logits, wh=wh, boxes=boxes.view(-1, 4), b3=b3,
                Kinv=torch.randn(frames, 3, 3, generator=g), desc_fs=desc_fs, desc_off=2,
                Tg=torch.randn(frames, 3, 3, generator=g) if with_tg else None,
                dbuf=torch.randn(frames * desc_fs, C + 8, generator=g))


def infer_formula(inp, sel_q, sel_logit, dtype):
    """inference_single_image on the selected (query, logit): scores, xyxy boxes, xyz, R"""
    frames, nq = inp["frames"], inp["nq"]
    fi = torch.arange(frames)[:, None]
    bx = inp["boxes"].to(dtype).view(frames, nq, 4)[fi, sel_q]                # [frames, k, 4]
    wh = inp["wh"].to(dtype)[:, None]
    hw, hh = 0.5 * bx[..., 2], 0.5 * bx[..., 3]
    raw = torch.stack((bx[..., 0] - hw, bx[..., 1] - hh, bx[..., 0] + hw, bx[..., 1] + hh), -1)
    lim = torch.cat((wh, wh), -1)
    xyxy = torch.minimum(raw.clamp(min=0), lim)
    bi = inp["b3"].to(dtype).view(frames, nq, 16)[fi, sel_q]
    z = bi[..., 3:4]
    uvz = torch.cat((z * bi[..., 0:2], z), -1)
    xyz = torch.einsum("frc,fkc->fkr", inp["Kinv"].to(dtype), uvz)
    P = bi[..., 7:16].reshape(frames, -1, 3, 3)
    R = P if inp["Tg"] is None else inp["Tg"].to(dtype)[:, None] @ P
    return {"scores": sel_logit.to(dtype).sigmoid(), "boxes": xyxy, "xyz": xyz, "R": R, "raw": raw, "lim": lim}


def infer_clamps(raw, lim):
    return {"x0 < 0": (raw[..., 0] < 0).any(), "y0 < 0": (raw[..., 1] < 0).any(),
            "x1 > W": (raw[..., 2] > lim[..., 2]).any(), "y1 > H": (raw[..., 3] > lim[..., 3]).any()}


@pytest.mark.parametrize("C,with_tg", INFER_VARIANTS)
@pytest.mark.parametrize("frames", [1, 3])
@pytest.mark.parametrize("nq,nc,k", INFER_SHAPES)
def test_infer_select(L, nq, nc, k, frames, C, with_tg):
    inp = infer_inputs(nq, nc, k, frames, C, with_tg)
    logits = inp["logits"]
    # the selection is exactly determined: f32 sigmoids of distinct logits are strictly ordered
    # (torch's sigmoid and the kernel's 1 / (1 + exp(-x)) alike), equal logits tie by index
    for f in range(frames):
        u = torch.unique(logits[f])                                      # sorted ascending
        assert (torch.diff(torch.sigmoid(u)) > 0).all() and (torch.diff(1 / (1 + torch.exp(-u))) > 0).all()
        assert u.numel() < logits[f].numel()
    order = stable_desc(logits)[:, :k]                                   # flat (query, class) index
    sel_q, sel_c = order // nc, order % nc
    sel_logit = torch.gather(logits, 1, order)
    ref = infer_formula(inp, sel_q, sel_logit, torch.float64)
    if k >= 20:
        assert_branches(infer_clamps(ref["raw"], ref["lim"]))

    dev = "cuda"
    outs = {"scores": torch.full((frames, k), NAN, device=dev),
            "classes": torch.full((frames, k), -1, dtype=torch.int64, device=dev),
            "logits": torch.full((frames, k, nc), NAN, device=dev), "boxes": torch.full((frames, k, 4), NAN, device=dev),
            "proj": torch.full((frames, k, 2), NAN, device=dev), "b3": torch.full((frames, k, 6), NAN, device=dev),
            "R": torch.full((frames, k, 3, 3), NAN, device=dev), "desc": torch.full((frames, k, C), NAN, device=dev)}
    dbuf = inp["dbuf"].cuda()
    L.infer_select(logits.view(frames * nq, nc).cuda(), frames, nq, nc, inp["boxes"].cuda(), inp["b3"].cuda(),
                   dbuf[:, 4:4 + C], inp["desc_fs"], inp["desc_off"], inp["Kinv"].cuda(),
                   None if inp["Tg"] is None else inp["Tg"].cuda(), inp["wh"].cuda(), k, outs)
    o = {name: t.cpu() for name, t in outs.items()}

    # gathers, bit for bit; every instance is checked
    fi = torch.arange(frames)[:, None]
    assert o["classes"].dtype == torch.int64 and torch.equal(o["classes"], sel_c)
    assert same_bits(o["logits"], logits.view(frames, nq, nc)[fi, sel_q])
    bi = inp["b3"].view(frames, nq, 16)[fi, sel_q]
    assert same_bits(o["proj"], bi[..., 0:2])
    assert same_bits(o["b3"][..., 3:6], bi[..., 4:7].flip(-1))
    desc = inp["dbuf"].view(frames, inp["desc_fs"], C + 8)[:, inp["desc_off"]:inp["desc_off"] + nq, 4:4 + C]
    assert same_bits(o["desc"], desc[fi, sel_q])
    if inp["Tg"] is None:
        assert same_bits(o["R"], bi[..., 7:16].reshape(frames, k, 3, 3))
    # arithmetic against float64
    r32 = infer_formula(inp, sel_q, sel_logit, torch.float32)
    check_field("infer.scores", o["scores"], ref["scores"], r32["scores"])
    check_field("infer.boxes", o["boxes"], ref["boxes"], r32["boxes"])
    check_field("infer.xyz", o["b3"][..., 0:3], ref["xyz"], r32["xyz"])
    if inp["Tg"] is not None:
        check_field("infer.R", o["R"], ref["R"], r32["R"])


def test_infer_select_argument_checks(L):
    z = lambda *s: torch.zeros(*s, device="cuda")
    outs = {"scores": z(1, 1), "classes": torch.zeros(1, 1, dtype=torch.int64, device="cuda"), "logits": z(1, 1, 1),
            "boxes": z(1, 1, 4), "proj": z(1, 1, 2), "b3": z(1, 1, 6), "R": z(1, 1, 3, 3), "desc": z(1, 1, 8)}
    args = lambda nq, nc, k: (z(nq, nc), 1, nq, nc, z(nq, 4), z(nq, 16), z(nq, 8), nq, 0, z(1, 3, 3), None,
                              z(1, 2), k, outs)
    with pytest.raises(L.HipError):       # capacity: nq * nc = 4097
        L.infer_select(*args(4097, 1, 1))
    with pytest.raises(L.HipError):       # k > nq * nc
        L.infer_select(*args(5, 7, 36))


# ------------------------------------------------------------------------------------------
# 5. edges of ln_rows, groupnorm_cl, s2d, gemm_f32
# ------------------------------------------------------------------------------------------
def ln_inputs(M, C, seed, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(M, C, generator=g) * (3 if mean == 0 else 1) + (1 if mean == 0 else mean),
            torch.randn(C, generator=g), torch.randn(C, generator=g), torch.randn(M, C, generator=g))


def col_view(t, lead, pad):
    """t's values as a column slice [:, lead:lead+C] of a sentinel-filled buffer with row stride C + pad"""
    M, C = t.shape
    buf = torch.full((M, C + pad), SENT, device="cuda")
    buf[:, lead:lead + C] = t.cuda()
    return buf, buf[:, lead:lead + C]


def pads_untouched(buf, lead, C):
    b = buf.cpu()
    return bool((b[:, :lead] == SENT).all() and (b[:, lead + C:] == SENT).all())


@pytest.mark.parametrize("M", [1, 5])
@pytest.mark.parametrize("C", [512, 768, 1024])
def test_ln_rows_widths_strides_in_place(L, C, M):
    x, gam, bet, pos = ln_inputs(M, C, C + M)
    ref = F.layer_norm(x.double(), (C,), gam.double(), bet.double(), 1e-5)
    gd, bd = gam.cuda(), bet.cuda()
    _, xv = col_view(x, 4, 8)                                  # ldx = C + 8
    obuf, ov = col_view(torch.zeros(M, C), 0, 4)
    _, pv = col_view(pos, 4, 12)
    o2buf, o2v = col_view(torch.zeros(M, C), 8, 16)
    L.ln_rows(xv, gd, bd, 1e-5, out=ov, pos=pv, out2=o2v)
    assert rel(ov.cpu(), ref) < 1e-6 and rel(o2v.cpu(), ref + pos.double()) < 1e-6
    assert pads_untouched(obuf, 0, C) and pads_untouched(o2buf, 8, C)
    yg = L.ln_rows(xv, gd, bd, 1e-6, gelu=True)
    assert rel(yg.cpu(), F.gelu(F.layer_norm(x.double(), (C,), gam.double(), bet.double(), 1e-6))) < 1e-6
    xbuf, xv = col_view(x, 4, 8)                               # in place, as the engine does
    L.ln_rows(xv, gd, bd, 1e-5, out=xv)
    assert rel(xv.cpu(), ref) < 1e-6 and pads_untouched(xbuf, 4, C)


def test_ln_rows_large_mean(L):
    """x = 1000 + N(0, 1): the two-pass variance keeps the result at the accuracy of the f32 mean
    (a one-pass E[x^2] - mean^2 would lose every digit); bound = 4 x torch-f32's own error"""
    M, C = 5, 512
    x, gam, bet, _ = ln_inputs(M, C, 99, mean=1000.0)
    ref = F.layer_norm(x.double(), (C,), gam.double(), bet.double(), 1e-5)
    e32 = rel(F.layer_norm(x, (C,), gam, bet, 1e-5), ref)
    e = rel(L.ln_rows(x.cuda(), gam.cuda(), bet.cuda(), 1e-5).cpu(), ref)
    print(f"ln_rows large mean: kernel {e:.3e}  torch-f32 {e32:.3e}  bound {4 * LN_LARGE_MEAN_F32_REL:.3e}")
    assert e <= 4 * LN_LARGE_MEAN_F32_REL


@pytest.mark.parametrize("B,P,C,G", [(1, 7, 64, 64), (2, 33, 96, 32), (1, 1600, 256, 1)])
def test_groupnorm_cl_shapes_and_strides(L, B, P, C, G):
    g = torch.Generator().manual_seed(P + C + G)
    x = torch.randn(B * P, C, generator=g) * 2 + 0.5
    gam, bet = torch.randn(C, generator=g), torch.randn(C, generator=g)
    pos = torch.randn(B * P, C, generator=g)
    ref = F.group_norm(x.double().view(B, P, C).permute(0, 2, 1), G, gam.double(), bet.double(), 1e-5)
    ref = ref.permute(0, 2, 1).reshape(B * P, C)
    _, xv = col_view(x, 1, 3)
    obuf, ov = col_view(torch.zeros(B * P, C), 2, 5)
    o2buf, o2v = col_view(torch.zeros(B * P, C), 1, 1)
    L.groupnorm_cl(xv, B, G, gam.cuda(), bet.cuda(), 1e-5, ov, pos=pos.cuda(), out2=o2v)
    assert rel(ov.cpu(), ref) < 1e-6 and rel(o2v.cpu(), ref + pos.double()) < 1e-6
    assert pads_untouched(obuf, 2, C) and pads_untouched(o2buf, 1, C)


@pytest.mark.parametrize("B,H,W,C,pad", [(3, 80, 80, 256, 0), (1, 2, 2, 4, 0), (1, 2, 2, 4, 4), (2, 6, 4, 12, 4)])
def test_s2d_grid_stride_and_views(L, B, H, W, C, pad):
    """(3, 80, 80, 256) is 1.23M elements, past the 4096 x 256 threads of the largest grid"""
    g = torch.Generator().manual_seed(H * W + C)
    x = torch.randn(B * H * W, C, generator=g)
    xv = col_view(x, pad // 2, pad)[1] if pad else x.cuda()
    got = L.s2d(xv, B, H, W)
    want = x.view(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B * (H // 2) * (W // 2), 4 * C)
    assert same_bits(got, want)


@pytest.mark.parametrize("act", [None, "relu", "gelu"])
@pytest.mark.parametrize("K", [37, 38, 39, 1])
def test_gemm_f32_k_tail_and_strided_residual(L, K, act):
    """K off the float4 width through column slices of buffers with a row stride of 40 (columns past
    K hold NaN: nothing beyond K may be read); out a strided view with resid aliasing it"""
    for M, N in ((1, 1), (65, 65), (1, 65), (65, 1)):
        g = torch.Generator().manual_seed(1000 * K + 10 * M + N)
        a, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.3
        bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        if M * N == 1:
            # one output element: the norm-wise error is that element's relative error, so keep it
            # away from the cancellation of resid + y and of GELU's 1 + erf at negative arguments
            a, w, bias, res = a.abs() + 0.25, w.abs() + 0.25, bias.abs(), res.abs()
        abuf = torch.full((M, 40), NAN)
        wbuf = torch.full((N, 40), NAN)
        abuf[:, :K], wbuf[:, :K] = a, w
        y = a.double() @ w.double().T + bias.double()
        y = F.relu(y) if act == "relu" else F.gelu(y) if act == "gelu" else y
        want = res.double() + y
        cbuf = torch.full((M + 2, N + 5), SENT, device="cuda")
        cv = cbuf[:M, 2:2 + N]
        cv.copy_(res)
        L.gemm_f32(abuf.cuda()[:, :K], wbuf.cuda()[:, :K], bias.cuda(), act=act, resid=cv, out=cv)
        err = rel(cv.cpu(), want)
        print("gemm_f32 tail", M, N, K, act, err)
        assert err < 2e-6
        assert pads_untouched(cbuf[:M], 2, N) and (cbuf[M:] == SENT).all()
