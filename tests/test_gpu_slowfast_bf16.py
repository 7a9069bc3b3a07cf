"""bf16 SlowFast / SlowOnly / FastOnly on the GPU: the frame-strided direct bf16 stem (ptx_conv_stem_bf16_strided_fwd) --
exact tap mapping, parity under the bf16 conv bound, bit equality of the two sources and with the plain entry point -- then
model parity calibrated against PyTorch's own bf16 arithmetic, uint8 frames / views, and the public API.  Every output
buffer is NaN-filled before a launch (pad channels included), so an element the kernel leaves unwritten fails."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import PtxError, _ptr
from pretorched_x_amd.testing import synth_state_dict
from oracle import functional as OF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, U8 = L.PTX_STEM_SRC_BF16_NCDHW, L.PTX_STEM_SRC_U8_NTHWC
N = 2

FAST = ((5, 7, 7), (1, 2, 2), (2, 3, 3))
SLOW = ((1, 7, 7), (1, 2, 2), (0, 3, 3))
R3D = ((7, 7, 7), (1, 2, 2), (3, 3, 3))
GEOMS = {
    # name: (filter, stride, pad), Co, (T_full, frame_step), (H, W)
    "fast_tiny": (FAST, 8, (9, 2), (5, 6)),            # every window touches both paddings; T_full no multiple of the step
    "fast_odd": (FAST, 8, (12, 3), (30, 33)),          # Wo = 17, rows of 66 / 99 bytes, pad channels at ldy = 8
    "fast_multi": (FAST, 8, (16, 2), (64, 72)),        # several workgroups per frame, a ragged last tile
    "slow_ragged": (SLOW, 64, (33, 16), (30, 34)),     # three used frames out of 33
    "co16": (FAST, 16, (9, 2), (30, 34)),              # one 16-channel tile ...
    "co17": (FAST, 17, (9, 2), (30, 34)),              # ... against two
    # the plain entry point's own cases (tests/test_gpu_bf16_stem.py), frame_step = 1
    "r3d_odd": (R3D, 64, (6, 1), (30, 33)),
    "r2p1d_83": (SLOW, 83, (4, 1), (30, 34)),
}
STRIDED = ["fast_tiny", "fast_odd", "fast_multi", "slow_ragged", "co16", "co17"]
IMAGENET_BGR255 = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], input_space="BGR", input_range=[0, 255])
PLAIN255 = dict(mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0], input_range=[0, 255])


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _r8(v):
    return (v + 7) // 8 * 8


def _used(geom):
    T_full, step = GEOMS[geom][2]
    return -(-T_full // step)


def _desc(geom, relu):
    (k, s, p), Co, _, (H, W) = GEOMS[geom]
    T = _used(geom)
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci = N, T, H, W, 3
    d.kT, d.kH, d.kW = k
    d.sT, d.sH, d.sW = s
    d.pT, d.pH, d.pW = p
    d.To, d.Ho, d.Wo = ((i + 2 * pp - kk) // ss + 1 for i, pp, kk, ss in zip((T, H, W), p, k, s))
    d.Co, d.ldy, d.Co_pad = Co, _r8(Co), (Co + 127) // 128 * 128
    d.flags = L.PTX_EPI_RELU if relu else 0
    return d


def _pack(w, bn):
    """w [Co][3][kT][kH][kW] bf16-exact fp32 (CPU); bn = (gamma, beta, mean, var) or None -> the stem's re-laid filter
    (ptx_pack_conv_weight of the (kh, kw)-folded filter, then ptx_pack_stem_bf16_weight), its fp32 bias, and the fp64
    reference filter / bias: the BN fold in fp32, ONE rounding to bf16."""
    Co, Ci, kT, kH, kW = w.shape
    K = kH * kW * Ci
    Kc, Co_pad = (K + 31) // 32 * 32, (Co + 127) // 128 * 128
    wr = w.permute(0, 3, 4, 1, 2).reshape(Co, K, kT, 1, 1).contiguous().to(DEV)
    dpk = L.PackDesc(Co, K, kT, 1, 1, Kc, Co_pad, 0, 0, 0, 0, 0, 0, L.PTX_PACK_BF16)
    lib = L.lib()
    wp = torch.full((lib.ptx_packed_weight_elems(C.byref(dpk)),), float("nan"), device=DEV, dtype=torch.bfloat16)
    bp = torch.full((Co_pad,), float("nan"), device=DEV, dtype=torch.float32)
    null = C.c_void_p(0)
    if bn is None:
        keep, args, eps = [], [null] * 4, 0.0
        scale = torch.ones(Co, dtype=torch.float64)
    else:
        keep = [t.to(DEV).contiguous() for t in bn]
        args, eps = [_ptr(t) for t in keep], 1e-5
        scale = (bn[0].float() / torch.sqrt(bn[3].float() + 1e-5)).double()
    L.check(lib.ptx_pack_conv_weight(C.byref(dpk), _ptr(wr), null, *args, C.c_float(eps), _ptr(wp), _ptr(bp), _st()), "pack")
    dw = L.ConvDesc()
    dw.Ci, dw.kT, dw.kH, dw.kW, dw.Co, dw.Co_pad = 3, kT, kH, kW, Co, Co_pad
    ws = torch.full((lib.ptx_stem_bf16_weight_elems(C.byref(dw)),), float("nan"), device=DEV, dtype=torch.bfloat16)
    L.check(lib.ptx_pack_stem_bf16_weight(C.byref(dw), _ptr(wp), _ptr(ws), _st()), "ptx_pack_stem_bf16_weight")
    torch.cuda.synchronize()
    wf = (w.double() * scale.view(-1, 1, 1, 1, 1)).float().to(torch.bfloat16).double()
    return ws, bp, wf, bp[:Co].cpu().double()


def _norm(opts):
    return L.NormDesc.make(opts["mean"], opts["std"], opts.get("input_space", "RGB"), opts["input_range"])


def _at_offset(t, offset):
    """A copy of the contiguous tensor t that starts `offset` elements into a fresh device buffer."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t.to(DEV))
    return view


def _run(geom, d, x, src, norm, ws, bp, plain=False):
    """One launch into a NaN-filled buffer -> ([N][Co][To][Ho][Wo] fp64 on the CPU, the pad channels).  x holds T_full frames."""
    T_full, step = GEOMS[geom][2]
    lib = L.lib()
    y = torch.full((d.N, d.To, d.Ho, d.Wo, d.ldy), float("nan"), device=DEV, dtype=torch.bfloat16)
    nd = C.byref(norm) if norm is not None else None
    if plain:
        assert step == 1
        L.check(lib.ptx_conv_stem_bf16_fwd(C.byref(d), _ptr(x), src, nd, _ptr(ws), _ptr(bp), _ptr(y), _st()), "ptx_conv_stem_bf16_fwd")
    else:
        L.check(lib.ptx_conv_stem_bf16_strided_fwd(C.byref(d), _ptr(x), src, nd, step, T_full, _ptr(ws), _ptr(bp), _ptr(y), _st()),
                "ptx_conv_stem_bf16_strided_fwd")
    torch.cuda.synchronize()
    g = y.cpu().float()
    return g[..., :d.Co].permute(0, 4, 1, 2, 3).double(), g[..., d.Co:]


def _frames(geom, seed):
    (T_full, _), (H, W) = GEOMS[geom][2], GEOMS[geom][3]
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, T_full, H, W, 3), dtype=torch.uint8, generator=g)


def _frames_operand(frames, opts):
    """The operand the uint8 source defines: ptx_frames_u8_to_ncdhw (fp32, the project's normalisation) rounded to bf16."""
    n, T, H, W, _ = frames.shape
    out = torch.full((n, 3, T, H, W), float("nan"), device=DEV, dtype=torch.float32)
    fd = frames.to(DEV).contiguous()
    norm = _norm(opts)
    L.check(L.lib().ptx_frames_u8_to_ncdhw(_ptr(fd), _ptr(out), n, T, H, W, 3, C.byref(norm), _st()), "ptx_frames_u8_to_ncdhw")
    torch.cuda.synchronize()
    return out.to(torch.bfloat16)


def _tap_filter(geom, taps_per_channel, seed):
    """+-1 on `taps_per_channel` seeded taps per output channel; the first channels sit on the corner taps (kt, kh, kw in
    {0, last}) of each input channel."""
    (k, _, _), Co = GEOMS[geom][0], GEOMS[geom][1]
    g = torch.Generator().manual_seed(seed)
    w = torch.zeros(Co, 3, *k)
    corners = [(c, kt, kh, kw) for kt in sorted({0, k[0] - 1}) for kh in (0, k[1] - 1) for kw in (0, k[2] - 1) for c in range(3)]
    for co in range(Co):
        picks = [corners[co]] if co < len(corners) else []
        while len(picks) < taps_per_channel:
            t = (int(torch.randint(0, 3, (1,), generator=g)),) + tuple(int(torch.randint(0, kk, (1,), generator=g)) for kk in k)
            if t not in picks:
                picks.append(t)
        for t in picks[:taps_per_channel]:
            w[(co,) + t] = 1.0 if int(torch.randint(0, 2, (1,), generator=g)) else -1.0
    return w


# ------------------------------------------------------------------------------------------------ 1. exact tap mapping
@pytest.mark.parametrize("geom", STRIDED)
def test_exact_tap_mapping_bf16_clip(geom):
    """Integers in [-8, 8] times four +-1 taps: every product and every sum (|sum| <= 32) is exact in bf16."""
    (k, s, p), Co, (T_full, step), (H, W) = GEOMS[geom]
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-8, 9, (N, 3, T_full, H, W), generator=g).float()
    w = _tap_filter(geom, 4, 12)
    d = _desc(geom, relu=False)
    ws, bp, wf, _ = _pack(w, None)
    assert torch.equal(wf, w.double())
    ref = F.conv3d(x[:, :, ::step].double(), w.double(), None, s, p)
    for offset in (0, 3):
        got, pad = _run(geom, d, _at_offset(x.to(torch.bfloat16), offset), BF16, None, ws, bp)
        assert torch.equal(got, ref), (geom, offset, float((got - ref).abs().max()))
        assert torch.all(pad == 0), (geom, offset)


@pytest.mark.parametrize("geom", STRIDED)
def test_exact_tap_mapping_uint8_frames(geom):
    """mean 0, std 1, range 255: the operands are the integers 0..255; one +-1 tap per channel keeps |sum| <= 255."""
    (k, s, p), Co, (T_full, step), (H, W) = GEOMS[geom]
    frames = _frames(geom, 21)
    w = _tap_filter(geom, 1, 22)
    d = _desc(geom, relu=False)
    ws, bp, _, _ = _pack(w, None)
    for space in ("RGB", "BGR"):
        opts = dict(PLAIN255, input_space=space)
        x = frames.permute(0, 4, 1, 2, 3).double()
        if space == "BGR":
            x = x.flip(1)
        assert torch.equal(_frames_operand(frames, opts).cpu().double(), x)
        ref = F.conv3d(x[:, :, ::step], w.double(), None, s, p)
        for offset in (0, 1):
            got, pad = _run(geom, d, _at_offset(frames, offset), U8, _norm(opts), ws, bp)
            assert torch.equal(got, ref), (geom, space, offset, float((got - ref).abs().max()))
            assert torch.all(pad == 0), (geom, space, offset)


# ------------------------------------------------------------------------------------------------ 2. random data
def _random_problem(geom, seed):
    (k, s, p), Co = GEOMS[geom][0], GEOMS[geom][1]
    torch.manual_seed(seed)
    w = (torch.randn(Co, 3, *k) * (2.0 / (3 * k[0] * k[1] * k[2])) ** 0.5).to(torch.bfloat16).float()
    bn = (torch.rand(Co) + 0.5, torch.randn(Co) * 0.1, torch.randn(Co) * 0.1, torch.rand(Co) + 0.5)
    return w, bn


def _check_bound(got, x16, wf, bias, s, p, what):
    """The project's bound for bf16 convs: |got - ref| <= 2^-8 |ref| + 2^-20 conv(|x|, |w|), ref in fp64 on the same operands."""
    x = x16.cpu().double()
    ref = F.conv3d(x, wf, bias, s, p).clamp_min(0)
    absref = F.conv3d(x.abs(), wf.abs(), None, s, p)
    bar = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * absref + 1e-30
    err = (got - ref).abs()
    print("%s: max err %.3e, max err / bar %.3f" % (what, float(err.max()), float((err / bar).max())))
    assert torch.all(err <= bar), (what, float((err - bar).max()))


@pytest.mark.parametrize("geom", STRIDED)
def test_parity_random_and_sources_bit_identical(geom):
    """Both sources under the bound around one fp64 reference on x[:, :, ::step]; uint8 frames under a non-trivial norm ==
    the bf16 clip ptx_frames_u8_to_ncdhw(f).to(bfloat16), bit for bit: same operands, same kernel arithmetic."""
    (k, s, p), Co, (T_full, step), (H, W) = GEOMS[geom]
    w, bn = _random_problem(geom, 31)
    d = _desc(geom, relu=True)
    ws, bp, wf, bias = _pack(w, bn)
    x16 = torch.randn(N, 3, T_full, H, W, generator=torch.Generator().manual_seed(33)).to(torch.bfloat16)
    got, pad = _run(geom, d, x16.to(DEV).contiguous(), BF16, None, ws, bp)
    assert torch.all(pad == 0)
    _check_bound(got, x16[:, :, ::step], wf, bias, s, p, geom + "/bf16")
    frames = _frames(geom, 32)
    f16 = _frames_operand(frames, IMAGENET_BGR255)
    from_u8, pad8 = _run(geom, d, frames.to(DEV).contiguous(), U8, _norm(IMAGENET_BGR255), ws, bp)
    assert torch.all(pad8 == 0)
    _check_bound(from_u8, f16[:, :, ::step], wf, bias, s, p, geom + "/u8")
    from_clip, pad16 = _run(geom, d, f16.contiguous(), BF16, None, ws, bp)
    assert torch.equal(from_u8, from_clip) and torch.all(pad16 == 0)


# ------------------------------------------------------------------------------------------------ 3. the plain entry point
@pytest.mark.parametrize("geom", ["r3d_odd", "r2p1d_83"])
def test_step_one_is_the_plain_entry_point(geom):
    (k, s, p), Co, (T_full, step), (H, W) = GEOMS[geom]
    w, bn = _random_problem(geom, 41)
    d = _desc(geom, relu=True)
    ws, bp, wf, bias = _pack(w, bn)
    x16 = torch.randn(N, 3, T_full, H, W, generator=torch.Generator().manual_seed(43)).to(torch.bfloat16).to(DEV).contiguous()
    frames = _frames(geom, 42).to(DEV).contiguous()
    for x, src, norm in ((x16, BF16, None), (frames, U8, _norm(IMAGENET_BGR255))):
        strided, pad_s = _run(geom, d, x, src, norm, ws, bp)
        plain, pad_p = _run(geom, d, x, src, norm, ws, bp, plain=True)
        assert not torch.isnan(plain).any() and torch.equal(strided, plain) and torch.all(pad_s == 0) and torch.all(pad_p == 0)
    _check_bound(plain, _frames_operand(frames.cpu(), IMAGENET_BGR255), wf, bias, s, p, geom + "/plain u8")


# ------------------------------------------------------------------------------------------------ 4. model parity
CASES = {
    # name: (factory, mode, constructor extras, clip shape)
    "resnet50_sf": ("resnet50", "SF", {}, (2, 3, 32, 64, 64)),
    "resnet50_s": ("resnet50", "S", {}, (2, 3, 32, 64, 64)),
    "resnet50_f": ("resnet50", "F", {}, (2, 3, 32, 64, 64)),
    "resnet18_sf": ("resnet18", "SF", {}, (3, 3, 32, 48, 80)),
    "resnet50_sf_8x1": ("resnet50", "SF", dict(slow_stride=8, fast_stride=1), (2, 3, 16, 64, 64)),
    "resnet50_sf_ragged_t": ("resnet50", "SF", {}, (2, 3, 35, 64, 64)),
}
LAYERS = {"resnet50": ("bottleneck", [3, 4, 6, 3]), "resnet18": ("basic", [2, 2, 2, 2])}


def _build(arch, mode, kw, stem="direct"):
    """(bf16 model on the device, its bf16-exact fp32 state dict)."""
    m = ptx.slowfast.__dict__[arch](mode=mode, num_classes=51, **kw)
    sd = synth_state_dict(m.state_dict(), 1234)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    m.load_state_dict(sd)
    m = m.eval().to(torch.bfloat16).to(DEV)
    m.engine().lanes = 1
    m.engine().bf16_stem = stem
    return m, sd


def _clip(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)


@pytest.mark.parametrize("case", list(CASES))
def test_model_parity(case):
    arch, mode, kw, shape = CASES[case]
    m, sd = _build(arch, mode, kw)
    x = _clip(shape)
    block, layers = LAYERS[arch]
    okw = dict(mode=mode.lower(), slow_stride=kw.get("slow_stride", 16), fast_stride=kw.get("fast_stride", 2))
    ref = OF.slowfast_forward(sd, x.float(), block, layers, **okw)
    sd16 = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in sd.items()}
    err_torch = float((OF.slowfast_forward(sd16, x, block, layers, **okw).float() - ref).abs().max())
    bar = 2 * err_torch + 1e-3 * float(ref.abs().max())
    top2 = ref.topk(2, 1).values
    margin = top2[:, 0] - top2[:, 1]
    with torch.no_grad():
        out = m(x.to(DEV))
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and out.shape == (shape[0], 51)
    o = out.float().cpu()
    err = float((o - ref).abs().max())
    print("%s: max|ref| %.3f  err_torch %.4f  bar %.4f  err %.4f  smallest margin %.3f" % (
        case, float(ref.abs().max()), err_torch, bar, err, float(margin.min())))
    assert torch.all(margin > 2 * bar), (margin, bar)         # the inputs are well chosen: the argmax check covers every clip
    assert err <= bar, (err, bar)
    assert torch.equal(o.argmax(1), ref.argmax(1))


# ------------------------------------------------------------------------------------------------ 5. frames and views
def _video(n, t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, t, h, w, 3), dtype=torch.uint8, generator=g).to(DEV)


def test_frames_and_views():
    TF = ptx.transforms
    opts = dict(IMAGENET_BGR255, input_size=[3, 64, 64])
    m, _ = _build("resnet50", "SF", {})
    with torch.no_grad():
        frames = _video(2, 32, 64, 64, 61)
        got = m.forward_frames(frames, opts)
        want = m(TF.FramesToTensor(opts)(frames).to(torch.bfloat16))
        assert got.dtype == torch.bfloat16 and got.shape == (2, 51)
        assert torch.equal(got, want), float((got.float() - want.float()).abs().max())
        big = _video(2, 32, 90, 120, 62)
        tf = TF.TransformFrames(opts, out="frames")
        assert torch.equal(m.forward_frames(big, opts, transform=tf), m.forward_frames(tf(big), opts))
        video = _video(2, 80, 90, 120, 63)
        vs = TF.SampleViews(opts, num_frames=32, frame_stride=2, clips=2, crops=1)
        views = vs(video)                                                            # [2,2,32,64,64,3]
        assert tuple(views.shape) == (2, 2, 32, 64, 64, 3)
        per_view = m.forward_frames(views.reshape((4,) + tuple(views.shape[2:])), opts).reshape(2, 2, 51)
        probs = m.forward_views(video, opts, views=vs)
        assert probs.dtype == torch.float32 and probs.shape == (2, 51)
        assert torch.allclose(probs, torch.softmax(per_view.float(), -1).mean(1), rtol=1e-5, atol=1e-7)
        assert torch.equal(m.forward_views(video, opts, views=vs, reduce=None), per_view)
        assert torch.equal(probs, ptx.engine.views_mean(per_view, 2, 2, "softmax"))
        # a tensor-out bf16 sampler goes through forward(): the sampler's own clips, view by view
        vt = TF.SampleViews(opts, num_frames=32, frame_stride=2, clips=2, crops=1, out="tensor", dtype=torch.bfloat16)
        clips = vt(video)                                                            # [2,2,3,32,64,64]
        assert tuple(clips.shape) == (2, 2, 3, 32, 64, 64) and clips.dtype == torch.bfloat16
        from_tensor = m.forward_views(video, views=vt, reduce=None)
        assert from_tensor.dtype == torch.bfloat16
        assert torch.equal(from_tensor, m(clips.reshape(4, 3, 32, 64, 64)).reshape(2, 2, 51))
        # under "fold" the same model refuses clips and frames
        m.engine().bf16_stem = "fold"
        with pytest.raises(PtxError, match="bf16"):
            m(TF.FramesToTensor(opts)(frames).to(torch.bfloat16))
        with pytest.raises(PtxError):
            m.forward_frames(frames, opts)


# ------------------------------------------------------------------------------------------------ 6. API
def test_api():
    m, _ = _build("resnet50", "SF", {})
    x = _clip((2, 3, 32, 64, 64)).to(DEV)
    with torch.no_grad():
        out = m(x)
        again = m(x)
        assert out.dtype == torch.bfloat16 and out.shape == (2, 51) and not torch.isnan(out.float()).any()
        assert torch.equal(out, again)
        with pytest.raises(PtxError, match="bfloat16"):
            m(x.float())
        # an in-place update (version counter) is noticed on the next call: a lateral conv, then the bias-free classifier
        m.fast.lateral_res3.weight.mul_(1.5)
        out2 = m(x)
        assert not torch.equal(out2, out)
        m.last_linear.weight.mul_(0.5)
        out3 = m(x)
        assert not torch.equal(out3, out2)
        # a .data edit bumps no version counter: refresh() re-reads the parameters
        m.slow.res5[2].bn3.weight.data.mul_(1.5)
        m.refresh()
        out4 = m(x)
        assert not torch.equal(out4, out3)
        assert torch.equal(m(x), out4)
