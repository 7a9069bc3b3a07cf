"""The patch-resident bf16 stem on the GPU (ptx_conv_stem_bf16_fwd, Engine.bf16_stem = "direct"): exact tap mapping on data
whose every product and sum is exact in bf16, parity against fp64 on random data under the bf16 conv bound, bit equality
of the two sources, the fold path under the same bound, and bf16 models fed from uint8 frames.  Every output buffer is
NaN-filled before a launch (pad channels included), so an element the kernel leaves unwritten fails."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import PtxError, _ptr
from pretorched_x_amd.testing import synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16, U8 = L.PTX_STEM_SRC_BF16_NCDHW, L.PTX_STEM_SRC_U8_NTHWC
N = 2

R3D = ((7, 7, 7), (1, 2, 2), (3, 3, 3))
R2P1D = ((1, 7, 7), (1, 2, 2), (0, 3, 3))
GEOMS = {
    # name: (filter, stride, pad), Co, (T, H, W)
    "r3d_tiny": (R3D, 64, (2, 5, 6)),          # every temporal / vertical window touches both paddings; W < kW
    "r3d_odd": (R3D, 64, (6, 30, 33)),         # Wo = 17; rows of 99 bytes (uint8) / 66 bytes (bf16)
    "r3d_multi": (R3D, 64, (9, 64, 72)),       # several workgroups per frame, a ragged last tile, T > kT
    "r2p1d_83": (R2P1D, 83, (4, 30, 34)),      # odd Co, two channel tiles, pad channels
    "r2p1d_110": (R2P1D, 110, (4, 30, 34)),
}
IMAGENET_BGR255 = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], input_space="BGR", input_range=[0, 255])
PLAIN255 = dict(mean=[0.0, 0.0, 0.0], std=[1.0, 1.0, 1.0], input_range=[0, 255])


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _r8(v):
    return (v + 7) // 8 * 8


def _desc(geom, relu):
    (k, s, p), Co, (T, H, W) = GEOMS[geom]
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
    """w [Co][3][kT][kH][kW] bf16-exact fp32 (CPU); bn = (gamma, beta, mean, var) or None -> the fold path's packed filter
    ([kT][Co_pad][Kc] bf16, k = (kh*kW + kw)*3 + c, ptx_pack_conv_weight), its fp32 bias, and the fp64 reference filter /
    bias: the BN fold in fp32, ONE rounding to bf16 (as _pack_bf16 of tests/test_gpu_bf16.py)."""
    Co, Ci, kT, kH, kW = w.shape
    K = kH * kW * Ci
    Kc, Co_pad = (K + 31) // 32 * 32, (Co + 127) // 128 * 128
    wr = w.permute(0, 3, 4, 1, 2).reshape(Co, K, kT, 1, 1).contiguous().to(DEV)
    dpk = L.PackDesc(Co, K, kT, 1, 1, Kc, Co_pad, 0, 0, 0, 0, 0, 0, L.PTX_PACK_BF16)
    wp = torch.full((L.lib().ptx_packed_weight_elems(C.byref(dpk)),), float("nan"), device=DEV, dtype=torch.bfloat16)
    bp = torch.full((Co_pad,), float("nan"), device=DEV, dtype=torch.float32)
    null = C.c_void_p(0)
    if bn is None:
        keep, args, eps = [], [null] * 4, 0.0
        scale, bias = torch.ones(Co, dtype=torch.float64), torch.zeros(Co, dtype=torch.float64)
    else:
        keep = [t.to(DEV).contiguous() for t in bn]
        args, eps = [_ptr(t) for t in keep], 1e-5
        g, b, m, v = [t.double() for t in bn]
        scale = (g.float() / torch.sqrt(v.float() + 1e-5)).double()
        bias = b - m * scale
    L.check(L.lib().ptx_pack_conv_weight(C.byref(dpk), _ptr(wr), null, *args, C.c_float(eps), _ptr(wp), _ptr(bp), _st()), "pack")
    torch.cuda.synchronize()
    wf = (w.double() * scale.view(-1, 1, 1, 1, 1)).float().to(torch.bfloat16).double()
    return wp, bp, wf, bp[:Co].cpu().double(), Kc


def _relay(d, wp):
    lib = L.lib()
    ws = torch.full((lib.ptx_stem_bf16_weight_elems(C.byref(d)),), float("nan"), device=DEV, dtype=torch.bfloat16)
    L.check(lib.ptx_pack_stem_bf16_weight(C.byref(d), _ptr(wp), _ptr(ws), _st()), "ptx_pack_stem_bf16_weight")
    return ws


def _norm(opts):
    return L.NormDesc.make(opts["mean"], opts["std"], opts.get("input_space", "RGB"), opts["input_range"])


def _at_offset(t, offset):
    """A copy of the contiguous tensor t that starts `offset` elements into a fresh device buffer."""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
    view = buf[offset:offset + t.numel()].view(t.shape)
    view.copy_(t.to(DEV))
    return view


def _run(d, x, src, norm, ws, bp):
    """One launch into a NaN-filled buffer -> ([N][Co][To][Ho][Wo] fp64 on the CPU, the pad channels)."""
    y = torch.full((d.N, d.To, d.Ho, d.Wo, d.ldy), float("nan"), device=DEV, dtype=torch.bfloat16)
    L.check(L.lib().ptx_conv_stem_bf16_fwd(C.byref(d), _ptr(x), src, C.byref(norm) if norm is not None else None, _ptr(ws),
                                           _ptr(bp), _ptr(y), _st()), "ptx_conv_stem_bf16_fwd")
    torch.cuda.synchronize()
    g = y.cpu().float()
    return g[..., :d.Co].permute(0, 4, 1, 2, 3).double(), g[..., d.Co:]


def _frames(geom, seed):
    T, H, W = GEOMS[geom][2]
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, T, H, W, 3), dtype=torch.uint8, generator=g)


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
    (k, _, _), Co, _ = GEOMS[geom]
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
@pytest.mark.parametrize("geom", list(GEOMS))
def test_exact_tap_mapping_bf16_clip(geom):
    """Integers in [-8, 8] times four +-1 taps: every product and every sum (|sum| <= 32) is exact in bf16."""
    (k, s, p), Co, (T, H, W) = GEOMS[geom]
    g = torch.Generator().manual_seed(11)
    x = torch.randint(-8, 9, (N, 3, T, H, W), generator=g).float()
    w = _tap_filter(geom, 4, 12)
    d = _desc(geom, relu=False)
    wp, bp, wf, _, _ = _pack(w, None)
    assert torch.equal(wf, w.double())
    ws = _relay(d, wp)
    ref = F.conv3d(x.double(), w.double(), None, s, p)
    for offset in (0, 3):
        got, pad = _run(d, _at_offset(x.to(torch.bfloat16), offset), BF16, None, ws, bp)
        assert torch.equal(got, ref), (geom, offset, float((got - ref).abs().max()))
        assert torch.all(pad == 0), (geom, offset)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_exact_tap_mapping_uint8_frames(geom):
    """mean 0, std 1, range 255: the operands are the integers 0..255; one +-1 tap per channel keeps |sum| <= 255."""
    (k, s, p), Co, (T, H, W) = GEOMS[geom]
    frames = _frames(geom, 21)
    w = _tap_filter(geom, 1, 22)
    d = _desc(geom, relu=False)
    wp, bp, _, _, _ = _pack(w, None)
    ws = _relay(d, wp)
    for space in ("RGB", "BGR"):
        opts = dict(PLAIN255, input_space=space)
        x = frames.permute(0, 4, 1, 2, 3).double()
        if space == "BGR":
            x = x.flip(1)
        assert torch.equal(_frames_operand(frames, opts).cpu().double(), x)
        ref = F.conv3d(x, w.double(), None, s, p)
        for offset in (0, 1):
            got, pad = _run(d, _at_offset(frames, offset), U8, _norm(opts), ws, bp)
            assert torch.equal(got, ref), (geom, space, offset, float((got - ref).abs().max()))
            assert torch.all(pad == 0), (geom, space, offset)


# ------------------------------------------------------------------------------------------------ 2. - 4. parity
def _random_problem(geom, seed):
    (k, s, p), Co, (T, H, W) = GEOMS[geom]
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


@pytest.mark.parametrize("src", ["bf16", "u8"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_parity_random(geom, src):
    (k, s, p), Co, (T, H, W) = GEOMS[geom]
    w, bn = _random_problem(geom, 31)
    d = _desc(geom, relu=True)
    wp, bp, wf, bias, _ = _pack(w, bn)
    ws = _relay(d, wp)
    if src == "bf16":
        x16 = torch.randn(N, 3, T, H, W).to(torch.bfloat16)
        got, pad = _run(d, x16.to(DEV).contiguous(), BF16, None, ws, bp)
    else:
        frames = _frames(geom, 32)
        x16 = _frames_operand(frames, IMAGENET_BGR255)
        got, pad = _run(d, frames.to(DEV).contiguous(), U8, _norm(IMAGENET_BGR255), ws, bp)
    assert torch.all(pad == 0)
    _check_bound(got, x16, wf, bias, s, p, "%s/%s" % (geom, src))


@pytest.mark.parametrize("geom", list(GEOMS))
def test_sources_are_bit_identical(geom):
    """uint8 frames under a non-trivial norm == the bf16 clip ptx_frames_u8_to_ncdhw(f).to(bfloat16): same operands, same
    kernel arithmetic."""
    w, bn = _random_problem(geom, 41)
    d = _desc(geom, relu=True)
    wp, bp, _, _, _ = _pack(w, bn)
    ws = _relay(d, wp)
    frames = _frames(geom, 42)
    norm = _norm(IMAGENET_BGR255)
    from_u8, pad8 = _run(d, frames.to(DEV).contiguous(), U8, norm, ws, bp)
    from_clip, pad16 = _run(d, _frames_operand(frames, IMAGENET_BGR255).contiguous(), BF16, None, ws, bp)
    assert torch.equal(from_u8, from_clip) and torch.all(pad8 == 0) and torch.all(pad16 == 0)


@pytest.mark.parametrize("geom", ["r3d_odd", "r2p1d_83"])
def test_direct_and_fold_inside_the_same_bound(geom):
    """ptx_im2col_hw_bf16 + the picked bf16 tile on the SAME packed filter: both stems sit inside the bound around one
    fp64 reference (they may differ from each other: another summation order)."""
    (k, s, p), Co, (T, H, W) = GEOMS[geom]
    lib = L.lib()
    w, bn = _random_problem(geom, 51)
    d = _desc(geom, relu=True)
    wp, bp, wf, bias, Kc = _pack(w, bn)
    ws = _relay(d, wp)
    torch.manual_seed(52)
    x16 = torch.randn(N, 3, T, H, W).to(torch.bfloat16)
    xd = x16.to(DEV).contiguous()
    direct, _ = _run(d, xd, BF16, None, ws, bp)
    _check_bound(direct, x16, wf, bias, s, p, geom + "/direct")
    fold = torch.full((N, T, d.Ho, d.Wo, Kc), float("nan"), device=DEV, dtype=torch.bfloat16)
    L.check(lib.ptx_im2col_hw_bf16(_ptr(xd), _ptr(fold), N, 3, T, H, W, k[1], k[2], s[1], s[2], p[1], p[2], d.Ho, d.Wo, Kc, _st()), "im2col")
    K = k[1] * k[2] * 3
    df = L.ConvDesc()
    df.N, df.Ti, df.Hi, df.Wi, df.Ci, df.ldx = N, T, d.Ho, d.Wo, (K + 1) // 2, Kc // 2
    df.To, df.Ho, df.Wo, df.Co, df.ldy = d.To, d.Ho, d.Wo, Co + Co % 2, d.ldy
    df.kT, df.kH, df.kW, df.sT, df.sH, df.sW, df.pT, df.pH, df.pW = k[0], 1, 1, s[0], 1, 1, p[0], 0, 0
    df.Kc, df.Co_pad, df.groups = Kc // 2, d.Co_pad, 1
    df.flags = L.PTX_F16_OPERANDS | L.PTX_BF16_OPERANDS | L.PTX_EPI_OUT_F16 | L.PTX_EPI_RELU
    y = torch.full((N, d.To, d.Ho, d.Wo, d.ldy), float("nan"), device=DEV, dtype=torch.bfloat16)
    sk = C.c_int(1)
    cfg = lib.ptx_conv3d_pick_config(C.byref(df), C.byref(sk))
    assert lib.ptx_conv3d_config_name(cfg).decode().endswith("/bf16")
    L.check(lib.ptx_conv3d_fused_fwd(C.byref(df), _ptr(fold), _ptr(wp), _ptr(bp), None, _ptr(y), None, None, 0, cfg, 1, _st()), "fold stem")
    torch.cuda.synchronize()
    folded = y.cpu().float()[..., :Co].permute(0, 4, 1, 2, 3).double()
    _check_bound(folded, x16, wf, bias, s, p, geom + "/fold")


# ------------------------------------------------------------------------------------------------ 5. - 6. models
OPTS = dict(input_size=[3, 64, 64], input_space="RGB", input_range=[0, 1], mean=[0.45, 0.40, 0.35], std=[0.2, 0.25, 0.3])


def _zoo(name):
    try:
        return ptx.__dict__[name](num_classes=400, pretrained=None)
    except TypeError:
        return ptx.__dict__[name](num_classes=400)


def _models(name):
    """(bf16 model under "direct", its fp32 twin with the same bf16-exact weights)."""
    m = _zoo(name)
    sd = synth_state_dict(m.state_dict(), 1234)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    m.load_state_dict(sd)
    m16 = m.eval().to(torch.bfloat16).to(DEV)
    m16.engine().lanes = 1
    m16.engine().bf16_stem = "direct"
    m32 = _zoo(name)
    m32.load_state_dict(sd)
    m32 = m32.eval().to(DEV)
    m32.engine().lanes = 1
    return m16, m32


def _video(n, t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, t, h, w, 3), dtype=torch.uint8, generator=g).to(DEV)


@pytest.mark.parametrize("name", ["resnet3d18", "r2plus1d18"])
def test_models_from_frames_under_direct(name):
    TF = ptx.transforms
    m16, _ = _models(name)
    eng = m16.engine()
    to_tensor = TF.FramesToTensor(OPTS)
    with torch.no_grad():
        for hw in ((64, 64), (62, 70)):
            frames = _video(2, 4, hw[0], hw[1], 61)
            clip16 = to_tensor(frames).to(torch.bfloat16)
            got = m16.forward_frames(frames, OPTS)
            want = m16(clip16)
            assert got.dtype == torch.bfloat16 and got.shape == (2, 400)
            assert torch.equal(got, want), (name, hw, float((got.float() - want.float()).abs().max()))
            assert torch.equal(m16.logits(m16.features(clip16)), want)
        frames = _video(2, 4, 64, 64, 61)
        # the transform hook, and a frames-out sampler through forward_views
        big = _video(2, 4, 90, 120, 62)
        tf = TF.TransformFrames(OPTS, out="frames")
        assert torch.equal(m16.forward_frames(big, OPTS, transform=tf), m16.forward_frames(tf(big), OPTS))
        video = _video(2, 24, 90, 120, 63)
        vs = TF.SampleViews(OPTS, num_frames=4, frame_stride=2, clips=2, crops=3)
        views = vs(video)                                                            # [2,6,4,64,64,3]
        got = m16.forward_views(video, OPTS, views=vs, reduce=None)
        assert got.dtype == torch.bfloat16 and got.shape == (2, 6, 400)
        assert torch.equal(got, m16.forward_frames(views.reshape((12,) + tuple(views.shape[2:])), OPTS).reshape(2, 6, 400))
        # an in-place update of the stem filter reaches the re-laid copy
        before = m16.forward_frames(frames, OPTS)
        conv1 = next(mod for mod in m16.modules() if isinstance(mod, nn.Conv3d))
        conv1.weight.mul_(1.25)
        after = m16.forward_frames(frames, OPTS)
        assert not torch.equal(after, before)
        fresh = _zoo(name)
        fresh.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in m16.state_dict().items()})
        fresh = fresh.eval().to(torch.bfloat16).to(DEV)
        fresh.engine().lanes = 1
        fresh.engine().bf16_stem = "direct"
        assert torch.equal(fresh.forward_frames(frames, OPTS), after)
        # back under "fold" the same model object refuses frames again, in both entry points
        eng.bf16_stem = "fold"
        with pytest.raises(PtxError, match="float32 models only"):
            m16.forward_frames(frames, OPTS)
        with pytest.raises(PtxError, match="bfloat16"):
            m16.forward_views(video, OPTS, views=vs)


@pytest.mark.parametrize("name", ["resnet3d18", "r2plus1d18"])
def test_direct_accuracy_not_worse_than_fold(name):
    """Against the fp32 twin (same weights, fp32 forward_frames): e_direct <= 1.5 e_fold -- two independent bf16 roundings
    of the same quantities; 1.5 leaves room for sampling noise on 2 clips."""
    TF = ptx.transforms
    m16, m32 = _models(name)
    frames = _video(2, 4, 64, 64, 71)
    with torch.no_grad():
        ref = m32.forward_frames(frames, OPTS).float()
        direct = m16.forward_frames(frames, OPTS).float()
        m16.engine().bf16_stem = "fold"
        fold = m16(TF.FramesToTensor(OPTS)(frames).to(torch.bfloat16)).float()
    e_fold, e_direct = float((fold - ref).abs().max()), float((direct - ref).abs().max())
    print("%s: e_fold %.4e  e_direct %.4e  (max |logit| %.3f)" % (name, e_fold, e_direct, float(ref.abs().max())))
    assert e_fold > 0 and e_direct <= 1.5 * e_fold, (e_direct, e_fold)
