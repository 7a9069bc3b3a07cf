"""bf16 inference on the GPU: kernel parity of the bf16 conv tiles / stem fold / pools against CPU fp64 references, model
parity calibrated against PyTorch's own bf16 arithmetic, and the public API of a bf16 model.  Every output buffer is
NaN-filled before a launch (pad columns included), so a kernel that leaves anything unwritten fails."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import Engine, PtxError, _ptr
from pretorched_x_amd.testing import synth_clips, synth_state_dict
from oracle import functional as OF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _r8(v):
    return (v + 7) // 8 * 8


def _bf(t):
    return t.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ kernel parity
def _pack_bf16(w, bn):
    """w [Co][Ci][kT][kH][kW] bf16-exact fp32 (CPU); bn = (gamma, beta, mean, var) fp32 or None -> packed bf16 filter, fp32 bias,
    and the folded fp64 reference filter / bias the kernel must reproduce."""
    Co, Ci, kT, kH, kW = w.shape
    Kc, Co_pad = _r8(Ci), (Co + 127) // 128 * 128
    d = L.PackDesc(Co, Ci, kT, kH, kW, Kc, Co_pad, 0, 0, 0, 0, 0, 0, L.PTX_PACK_BF16)
    n = L.lib().ptx_packed_weight_elems(C.byref(d))
    wp = torch.full((n,), float("nan"), device=DEV, dtype=torch.bfloat16)
    bp = torch.full((Co_pad,), float("nan"), device=DEV, dtype=torch.float32)
    wd = w.to(DEV).contiguous()
    null = C.c_void_p(0)
    if bn is None:
        args, eps = [null] * 4, 0.0
        keep = []
    else:
        keep = [t.to(DEV).contiguous() for t in bn]
        args, eps = [_ptr(t) for t in keep], 1e-5
    L.check(L.lib().ptx_pack_conv_weight(C.byref(d), _ptr(wd), null, *args, C.c_float(eps), _ptr(wp), _ptr(bp), _st()), "pack")
    torch.cuda.synchronize()
    if bn is None:
        scale, bias = torch.ones(Co, dtype=torch.float64), torch.zeros(Co, dtype=torch.float64)
    else:
        g, b, m, v = [t.double() for t in bn]
        scale = (g.float() / torch.sqrt(v.float() + 1e-5)).double()
        bias = b - m * scale
    # the kernel multiplies with the ONE bf16 rounding of the folded filter
    wf = (w.double() * scale.view(-1, 1, 1, 1, 1)).float().to(torch.bfloat16).double()
    return wp, bp, Kc, Co_pad, wf, (bp[:Co].cpu().double())


GEOMS = [
    # name, Ci, Co, k, stride, pad, residual kind
    ("pw_s1", 64, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), None),
    ("pw_s2", 64, 128, (1, 1, 1), (2, 2, 2), (0, 0, 0), None),
    ("k3_s1_res", 64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), "add"),
    ("k3_s2", 64, 128, (3, 3, 3), (2, 2, 2), (1, 1, 1), None),
    ("spatial_1kk", 64, 144, (1, 3, 3), (1, 1, 1), (0, 1, 1), None),
    ("temporal_k11", 144, 64, (3, 1, 1), (1, 1, 1), (1, 0, 0), "add"),
    ("ragged_45", 45, 110, (1, 3, 3), (1, 2, 2), (0, 1, 1), None),
    ("ragged_in_110", 110, 45, (3, 1, 1), (2, 1, 1), (1, 0, 0), None),
    ("shortcutA", 64, 128, (3, 3, 3), (1, 1, 1), (1, 1, 1), "padA"),
]


@pytest.mark.parametrize("name,Ci,Co,k,s,p,res", GEOMS)
def test_bf16_conv_kernel_parity(name, Ci, Co, k, s, p, res):
    torch.manual_seed(7)
    N, T, H, W = 2, 4, 10, 12
    x = _bf(torch.randn(N, Ci, T, H, W)).float()
    w = _bf(torch.randn(Co, Ci, *k) * (2.0 / (Ci * k[0] * k[1] * k[2])) ** 0.5).float()
    bn = (torch.rand(Co) + 0.5, torch.randn(Co) * 0.1, torch.randn(Co) * 0.1, torch.rand(Co) + 0.5)
    wp, bp, Kc, Co_pad, wf, bias = _pack_bf16(w, bn)
    ldx, ldy = _r8(Ci), _r8(Co)
    xc = torch.zeros(N, T, H, W, ldx, dtype=torch.bfloat16)
    xc[..., :Ci] = _bf(x.permute(0, 2, 3, 4, 1))
    xd = xc.to(DEV)
    To, Ho, Wo = [(e + 2 * pp - kk) // ss + 1 for e, pp, kk, ss in zip((T, H, W), p, k, s)]
    ref = F.conv3d(x.double(), wf, bias, s, p)                 # [N][Co][To][Ho][Wo]
    absref = F.conv3d(x.double().abs(), wf.abs(), None, s, p)
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, (Ci + 1) // 2, ldx // 2
    d.To, d.Ho, d.Wo, d.Co, d.ldy = To, Ho, Wo, Co + Co % 2, ldy
    d.kT, d.kH, d.kW = k
    d.sT, d.sH, d.sW = s
    d.pT, d.pH, d.pW = p
    d.Kc, d.Co_pad, d.groups = Kc // 2, Co_pad, 1
    flags = L.PTX_F16_OPERANDS | L.PTX_BF16_OPERANDS | L.PTX_EPI_OUT_F16 | L.PTX_EPI_RELU
    resd = None
    if res == "add":
        r = _bf(torch.randn(N, Co, To, Ho, Wo)).float()
        rc = torch.zeros(N, To, Ho, Wo, ldy, dtype=torch.bfloat16)
        rc[..., :Co] = _bf(r.permute(0, 2, 3, 4, 1))
        resd = rc.to(DEV)
        flags |= L.PTX_EPI_RES_ADD | L.PTX_RES_F16
        d.ldr = ldy
        ref = ref + r.double()
        absref = absref + r.double().abs()
    elif res == "padA":        # shortcut A: the block input itself, strided by 1, zero channels above its own width
        rc = xc
        resd = xd
        flags |= L.PTX_EPI_RES_PADA | L.PTX_RES_F16
        d.ldr, d.res_C, d.res_T, d.res_H, d.res_W = ldx, Ci, T, H, W
        d.res_sT = d.res_sH = d.res_sW = 1
        add = torch.zeros(N, Co, To, Ho, Wo, dtype=torch.float64)
        add[:, :Ci] = x.double()[:, :, :To, :Ho, :Wo]
        ref = ref + add
        absref = absref + add.abs()
    ref = ref.clamp_min(0)
    d.flags = flags
    y = torch.full((N, To, Ho, Wo, ldy), float("nan"), device=DEV, dtype=torch.bfloat16)
    lib = L.lib()
    seen = 0
    for cfg in range(lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16()):
        cname = lib.ptx_conv3d_config_name(cfg).decode()
        if not cname.endswith("/bf16") or not lib.ptx_conv3d_config_supported(C.byref(d), cfg):
            continue
        for split in (1, 3):
            y.fill_(float("nan"))
            ws_bytes = lib.ptx_conv3d_workspace_bytes(C.byref(d), split)
            ws = torch.zeros(max(ws_bytes // 4, 4), device=DEV, dtype=torch.float32)
            st = lib.ptx_conv3d_fused_fwd(C.byref(d), _ptr(xd), _ptr(wp), _ptr(bp), _ptr(resd) if resd is not None else None,
                                          _ptr(y), None, _ptr(ws), ws_bytes, cfg, split, _st())
            if st != 0:
                continue
            torch.cuda.synchronize()
            got = y.cpu().float()
            assert torch.all(got[..., Co:] == 0), (cname, split, "pad channels")
            g = got[..., :Co].permute(0, 4, 1, 2, 3).double()
            bar = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * absref + 1e-30
            err = (g - ref).abs()
            assert torch.all(err <= bar), (cname, split, float((err - bar).max()))
            seen += 1
    assert seen >= 4, "too few bf16 tiles ran %s" % name


@pytest.mark.parametrize("kind", ["resnet3d", "r2plus1d"])
@pytest.mark.parametrize("offset", [0, 3])
def test_bf16_stem_fold_and_conv(kind, offset):
    """ptx_im2col_hw_bf16 on the caller's bf16 NCDHW clip (any 2-byte alignment) + the stem conv on the bf16 tiles."""
    torch.manual_seed(3)
    N, Cin, T, H, W = 2, 3, 6, 30, 34
    Co, k, s, p = (64, (7, 7, 7), (1, 2, 2), (3, 3, 3)) if kind == "resnet3d" else (83, (1, 7, 7), (1, 2, 2), (0, 3, 3))
    x = _bf(torch.randn(N, Cin, T, H, W)).float()
    buf = torch.zeros(x.numel() + 16, dtype=torch.bfloat16, device=DEV)
    view = buf[offset:offset + x.numel()].view(N, Cin, T, H, W)
    view.copy_(_bf(x).to(DEV))
    kT, kH, kW = k
    Ho, Wo = (H + 2 * p[1] - kH) // s[1] + 1, (W + 2 * p[2] - kW) // s[2] + 1
    K = kH * kW * Cin
    ld = (K + 31) // 32 * 32
    fold = torch.full((N, T, Ho, Wo, ld), float("nan"), device=DEV, dtype=torch.bfloat16)
    lib = L.lib()
    L.check(lib.ptx_im2col_hw_bf16(_ptr(view), _ptr(fold), N, Cin, T, H, W, kH, kW, s[1], s[2], p[1], p[2], Ho, Wo, ld, _st()),
            "im2col")
    torch.cuda.synchronize()
    ref = F.unfold(F.pad(x.permute(0, 2, 1, 3, 4).reshape(N * T, Cin, H, W), (p[2], p[2], p[1], p[1])), (kH, kW), stride=s[1:])
    ref = ref.view(N, T, Cin, kH * kW, Ho * Wo).permute(0, 1, 4, 3, 2).reshape(N, T, Ho, Wo, K)   # k = (kh*kW + kw)*C + c
    got = fold.cpu().float()
    assert torch.equal(got[..., :K], ref) and torch.all(got[..., K:] == 0)
    # the stem conv over the folded channels
    w = _bf(torch.randn(Co, Cin, *k) * 0.05).float()
    wr = w.permute(0, 3, 4, 1, 2).reshape(Co, K, kT, 1, 1)
    wp, bp, Kc, Co_pad, wf, bias = _pack_bf16(wr, None)
    Kc = ld
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, Ho, Wo, (K + 1) // 2, ld // 2
    d.To, d.Ho, d.Wo, d.Co, d.ldy = T, Ho, Wo, Co + Co % 2, _r8(Co)
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = kT, 1, 1, 1, 1, 1, p[0], 0, 0
    # repack with the stem's 160-wide rows
    dpk = L.PackDesc(Co, K, kT, 1, 1, ld, Co_pad, 0, 0, 0, 0, 0, 0, L.PTX_PACK_BF16)
    wp = torch.full((lib.ptx_packed_weight_elems(C.byref(dpk)),), float("nan"), device=DEV, dtype=torch.bfloat16)
    wrd = wr.contiguous().to(DEV)
    L.check(lib.ptx_pack_conv_weight(C.byref(dpk), _ptr(wrd), None, None, None, None, None, C.c_float(0), _ptr(wp), _ptr(bp), _st()), "pack")
    d.Kc, d.Co_pad, d.groups = ld // 2, Co_pad, 1
    d.flags = L.PTX_F16_OPERANDS | L.PTX_BF16_OPERANDS | L.PTX_EPI_OUT_F16
    y = torch.full((N, T, Ho, Wo, _r8(Co)), float("nan"), device=DEV, dtype=torch.bfloat16)
    sk = C.c_int(1)
    cfg = lib.ptx_conv3d_pick_config(C.byref(d), C.byref(sk))
    assert lib.ptx_conv3d_config_name(cfg).decode().endswith("/bf16")
    L.check(lib.ptx_conv3d_fused_fwd(C.byref(d), _ptr(fold), _ptr(wp), _ptr(bp), None, _ptr(y), None, None, 0, cfg, 1, _st()), "stem")
    torch.cuda.synchronize()
    refc = F.conv3d(x.double(), w.double(), None, s, p)
    absc = F.conv3d(x.double().abs(), w.double().abs(), None, s, p)
    g = y.cpu().float()
    assert torch.all(g[..., Co:] == 0)
    g = g[..., :Co].permute(0, 4, 1, 2, 3).double()
    assert torch.all((g - refc).abs() <= 2.0 ** -8 * refc.abs() + 2.0 ** -20 * absc + 1e-30)


def test_bf16_maxpool_bit_exact():
    torch.manual_seed(5)
    N, Cc, T, H, W = 2, 64, 5, 13, 15
    x = _bf(torch.randn(N, Cc, T, H, W))
    ld = _r8(Cc)
    xc = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    To, Ho, Wo = (T - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.full((N, To, Ho, Wo, ld), float("nan"), device=DEV, dtype=torch.bfloat16)
    d = L.PoolDesc(N, T, H, W, Cc, ld, To, Ho, Wo, 3, 3, 3, 2, 2, 2, 1, 1, 1, ld, L.PTX_POOL_BF16)
    L.check(L.lib().ptx_maxpool3d_fwd(C.byref(d), _ptr(xc), _ptr(y), _st()), "maxpool")
    torch.cuda.synchronize()
    ref = F.max_pool3d(x, 3, 2, 1)
    assert torch.equal(y.cpu().permute(0, 4, 1, 2, 3), ref)


def test_bf16_avgpool_and_head():
    torch.manual_seed(6)
    N, Cc, S = 3, 2048, 98
    x = _bf(torch.randn(N, S, Cc))
    pooled = torch.full((N, Cc), float("nan"), device=DEV)
    L.check(L.lib().ptx_global_avgpool_bf16(_ptr(x.to(DEV)), _ptr(pooled), N, Cc, S, Cc, _st()), "avgpool")
    torch.cuda.synchronize()
    ref = x.double().mean(1)
    assert torch.allclose(pooled.cpu().double(), ref, rtol=1e-5, atol=1e-6)
    # the head: fp32 linear on the fp32 pooled vector, one bf16 rounding
    lin = torch.nn.Linear(Cc, 339).to(torch.bfloat16)
    logits32 = F.linear(pooled.cpu().double(), lin.weight.double(), lin.bias.double())
    m = ptx.__dict__["resnet3d50"](num_classes=339, pretrained=None).eval().to(torch.bfloat16).to(DEV)
    m.last_linear.weight.data.copy_(lin.weight)
    m.last_linear.bias.data.copy_(lin.bias)
    out = m.engine()._head_bf16(m, pooled)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16
    # before the final rounding: within 1e-5 relative; after it, within one bf16 ulp
    assert torch.all((out.cpu().double() - logits32).abs() <= 2.0 ** -8 * logits32.abs() + 1e-5 * logits32.abs().max())


def test_bf16_layout_roundtrip_and_checksum():
    torch.manual_seed(8)
    N, Cc, S = 2, 45, 77
    x = _bf(torch.randn(N, Cc, S)).to(DEV)
    ld = _r8(Cc)
    cl = torch.full((N, S, ld), float("nan"), device=DEV, dtype=torch.bfloat16)
    back = torch.full((N, Cc, S), float("nan"), device=DEV, dtype=torch.bfloat16)
    lib = L.lib()
    L.check(lib.ptx_ncdhw_to_ndhwc_bf16(_ptr(x), _ptr(cl), N, Cc, S, ld, _st()), "to cl")
    L.check(lib.ptx_ndhwc_to_ncdhw_bf16(_ptr(cl), _ptr(back), N, Cc, S, ld, _st()), "to cf")
    torch.cuda.synchronize()
    assert torch.equal(cl[..., :Cc].cpu(), x.cpu().permute(0, 2, 1)) and torch.all(cl[..., Cc:].cpu() == 0)
    assert torch.equal(back.cpu(), x.cpu())
    t = torch.tensor([[x.data_ptr(), x.numel()]], dtype=torch.int64, device=DEV)

    def cs():
        out = torch.zeros(1, dtype=torch.int64, device=DEV)
        L.check(lib.ptx_checksum_b16(_ptr(t), 1, _ptr(out), _st()), "checksum")
        return int(out.item())
    a = cs()
    x.view(-1)[17] = x.view(-1)[17] + 1
    assert cs() != a


# ------------------------------------------------------------------------------------------------ model parity
def _shortcut_a_fp32_pool(x, planes, stride):
    out = F.avg_pool3d(x.float(), kernel_size=1, stride=stride).to(x.dtype)    # CPU torch has no bf16 avg_pool3d
    pad = torch.zeros(out.size(0), planes - out.size(1), *out.shape[2:], dtype=out.dtype)
    return torch.cat([out, pad], dim=1)


def _zoo(name, **kw):
    try:
        return ptx.__dict__[name](num_classes=339, pretrained=None, **kw)
    except TypeError:         # the (2+1)D factories take no `pretrained` (and never download)
        return ptx.__dict__[name](num_classes=339, **kw)


def _setup(name, shape, seed=3, shortcut=None):
    """A zoo model with synth_state_dict weights rounded to bf16 (then cast to bf16), a bf16 clip batch, the oracle config."""
    kw = {} if shortcut is None else {"shortcut_type": shortcut}
    m = _zoo(name, **kw)
    sd = synth_state_dict(m.state_dict(), 1234)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    m.load_state_dict(sd)
    m = m.eval().to(torch.bfloat16).to(DEV)
    x = synth_clips(shape[0], shape[2], shape[3], seed).to(torch.bfloat16)
    return m, sd, x, (_cfg_with_shortcut(name, shortcut) if shortcut is not None else OF.ARCHS[name])


def _bars(cfg, sd, x, monkeypatch):
    ref = OF.forward(cfg, sd, x.float())
    monkeypatch.setattr(OF, "shortcut_a", _shortcut_a_fp32_pool)
    sd16 = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in sd.items()}
    torch_bf16 = OF.forward(cfg, sd16, x).float()
    err_torch = float((torch_bf16 - ref).abs().max())
    return ref, err_torch, 2 * err_torch + 1e-3 * float(ref.abs().max())


def _check_parity(out, ref, bar):
    assert out.dtype == torch.bfloat16
    o = out.float().cpu()
    err = float((o - ref).abs().max())
    assert err <= bar, (err, bar)
    top2 = ref.topk(2, 1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * bar
    assert torch.equal(o.argmax(1)[sure], ref.argmax(1)[sure])
    return err


MODELS = [("resnet3d18", "A"), ("resnet3d18", "B"), ("resnet3d50", None), ("r2plus1d18", None)]


@pytest.mark.parametrize("name,shortcut", MODELS)
def test_bf16_model_parity(name, shortcut, monkeypatch):
    m, sd, x, cfg = _setup(name, (2, 3, 8, 64, 64), shortcut=shortcut)
    if shortcut is not None:
        assert m.arch.shortcut == shortcut
    ref, err_torch, bar = _bars(cfg, sd, x, monkeypatch)
    with torch.no_grad():
        out = m(x.to(DEV))
    torch.cuda.synchronize()
    _check_parity(out, ref, bar)


def _cfg_with_shortcut(name, shortcut):
    import dataclasses
    c = OF.ARCHS[name]
    return dataclasses.replace(c, shortcut=shortcut) if dataclasses.is_dataclass(c) else c._replace(shortcut=shortcut)


def test_bf16_model_parity_full_config2(monkeypatch):
    m, sd, x, cfg = _setup("resnet3d50", (8, 3, 16, 224, 224))
    ref, err_torch, bar = _bars(cfg, sd, x, monkeypatch)
    with torch.no_grad():
        out = m(x.to(DEV))
    torch.cuda.synchronize()
    _check_parity(out, ref, bar)


# ------------------------------------------------------------------------------------------------ API
def test_bf16_api(monkeypatch):
    m, sd, x, cfg = _setup("resnet3d50", (2, 3, 8, 64, 64))
    xd = x.to(DEV)
    eng = m.engine()
    eng.lanes = 1
    with torch.no_grad():
        out = m(xd)
        feats = m.features(xd)
        lg = m.logits(feats)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and out.shape == (2, 339)
    assert feats.dtype == torch.bfloat16 and feats.dim() == 5 and feats.shape[:2] == (2, 2048) and feats.is_contiguous()
    assert torch.equal(lg, out)
    ref, err_torch, bar = _bars(cfg, sd, x, monkeypatch)
    # two clip lanes: within the bar of the parity test
    eng.lanes = 2
    with torch.no_grad():
        out2 = m(xd)
    _check_parity(out2, ref, bar)
    eng.lanes = 1
    # graph replay equals eager bitwise
    eng.use_graph = True
    with torch.no_grad():
        g1 = m(xd)
        g2 = m(xd)
    eng.use_graph = False
    torch.cuda.synchronize()
    assert torch.equal(g1, out) and torch.equal(g2, out)
    # an in-place bf16 BN update changes the output
    with torch.no_grad():
        m.layer4[2].bn3.weight.mul_(1.5)
        out3 = m(xd)
    assert not torch.equal(out3, out)
    # a .data edit is seen under check_weights = "checksum"
    eng.check_weights = "checksum"
    with torch.no_grad():
        base = m(xd)
        m.layer4[2].bn3.bias.data.add_(0.25)
        out4 = m(xd)
    assert not torch.equal(out4, base)
    # dtype mismatches raise both ways; out-of-scope families raise
    with pytest.raises(PtxError):
        m(xd.float())
    m32 = ptx.__dict__["resnet3d18"](num_classes=339, pretrained=None).eval().to(DEV)
    with pytest.raises(PtxError):
        m32(xd)
    nl = ptx.__dict__["nonlocalresnet3d50"](num_classes=339, pretrained=None).eval().to(torch.bfloat16).to(DEV)
    with pytest.raises(PtxError, match="bf16"):
        nl(xd)
    with pytest.raises(PtxError):
        eng.forward_frames(m, torch.zeros(1, 8, 64, 64, 3, dtype=torch.uint8, device=DEV), opts=dict(
            mean=[0.5] * 3, std=[0.5] * 3, input_space="RGB", input_range=[0, 1]))
