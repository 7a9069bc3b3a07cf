"""bf16 BigGAN-deep generator on the GPU: parity of the bf16 patch kernels and of the generic bf16 tiles on every fused
generator-stage flag combination the plan uses (against fp64 on the same bf16 operands, NaN-prefilled outputs), the
PTX_ACT_OUT_BF16 affine pass, generator parity calibrated against PyTorch's own bf16 arithmetic on the fp32 stand-in, the
adversarial-table weights that need a guard in fp16, weight refresh, and the errors."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import PtxError, _ptr
from pretorched_x_amd.testing import BIGGAN_RECIPE, synth_state_dict
from oracle import biggan_standin as BG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = L.PTX_F16_OPERANDS | L.PTX_BF16_OPERANDS | L.PTX_EPI_OUT_F16


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _r8(v):
    return (v + 7) // 8 * 8


def _bfx(t):
    """bf16-exact fp32 copy"""
    return t.to(torch.bfloat16).float()


def _nhwc(x, ld):
    """[N][C][H][W] -> bf16 [N][1][H][W][ld], pad channels zero"""
    N, C_, H, W = x.shape
    out = torch.zeros(N, 1, H, W, ld, dtype=torch.bfloat16)
    out[:, 0, ..., :C_] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
    return out.to(DEV)


def _bar(ref, absref):
    """one bf16 rounding of the fp64 result (2^-8 relative covers round-to-nearest with room for the fp32 accumulation)"""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -20 * absref + 1e-30


def _close(got, ref, absref, what):
    err = (got.double() - ref).abs()
    bar = _bar(ref, absref)
    assert torch.isfinite(got).all(), what
    assert torch.all(err <= bar), (what, float((err - bar).max()), float(err.max()))


# ----------------------------------------------------------------------------------------------------- kernel parity
def _problem(k, N, H, W, K, Co, up2=False, skip=None, affine=False, relu=False, dual=False, tanh=False, seed=0):
    """One generator-stage conv on bf16 operands: inputs on the device, descriptor, ext, and the fp64 reference
    (raw = conv + bias + skip, act = relu?/tanh?(raw * scale + shift))."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = _bfx(torch.randn(N, K, H, W, generator=g))
    w = _bfx(torch.randn(Co, K, k, k, generator=g) * (K * k * k) ** -0.5)
    bias = torch.randn(Co, generator=g) * 0.2
    Ho, Wo = (2 * H, 2 * W) if up2 else (H, W)
    xin = F.interpolate(x, scale_factor=2, mode="nearest") if up2 else x
    raw = F.conv2d(xin.double(), w.double(), bias.double(), 1, k // 2)
    absraw = F.conv2d(xin.double().abs(), w.double().abs(), bias.double().abs(), 1, k // 2)
    d = L.ConvDesc()
    flags = BF | (L.PTX_PRO_UP2 if up2 else 0)
    res_d = None
    if skip is not None:
        up = skip == "up"
        Cr = Co if skip == "same" else Co + 64
        rh, rw = (-(-Ho // 2), -(-Wo // 2)) if up else (Ho, Wo)
        r = _bfx(torch.randn(N, Cr, rh, rw, generator=g))
        rr = F.interpolate(r[:, :Co], scale_factor=2, mode="nearest")[:, :, :Ho, :Wo] if up else r[:, :Co]
        raw, absraw = raw + rr.double(), absraw + rr.double().abs()
        ldr = _r8(Cr) + 8
        res_d = _nhwc(r, ldr)
        d.ldr = ldr
        if skip == "same":
            flags |= L.PTX_EPI_RES_ADD
        else:
            flags |= L.PTX_EPI_RES_PADA | L.PTX_EPI_RES_UP
            d.res_C, d.res_T, d.res_H, d.res_W = Cr, 1, rh, rw
            d.res_sT, d.res_sH, d.res_sW = 0, int(up), int(up)
        flags |= L.PTX_RES_F16
    ld_aff = _r8(Co) + 4
    sc = torch.rand(N, ld_aff, generator=g) + 0.5
    sh = torch.randn(N, ld_aff, generator=g) * 0.3
    act, absact = raw, absraw
    if affine:
        act = raw * sc[:, :Co, None, None].double() + sh[:, :Co, None, None].double()
        absact = absraw * sc[:, :Co, None, None].double() + sh[:, :Co, None, None].double().abs()
        flags |= L.PTX_EPI_AFFINE
    if relu:
        act = act.clamp_min(0)
        flags |= L.PTX_EPI_RELU
    if tanh:
        act = torch.tanh(act)
        flags |= L.PTX_EPI_TANH
    if dual:
        flags |= L.PTX_EPI_DUAL_RAW
    ldx = _r8(K) + 8
    Cp = Co + Co % 2
    pd = L.PackDesc(Co, K, 1, k, k, ldx, (Co + 127) // 128 * 128, 0, 0, 0, 0, 0, 0, L.PTX_PACK_BF16)
    lib = L.lib()
    wp = torch.full((lib.ptx_packed_weight_elems(C.byref(pd)),), float("nan"), device=DEV, dtype=torch.bfloat16)
    bp = torch.full((pd.Co_pad,), float("nan"), device=DEV, dtype=torch.float32)
    wd, bd = w.view(Co, K, 1, k, k).to(DEV), bias.to(DEV)
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), _ptr(wd), _ptr(bd), None, None, None, None, C.c_float(0), _ptr(wp), _ptr(bp),
                                     _st()), "pack bf16")
    ldy, ld_raw = _r8(Cp) + 8, _r8(Cp) + 16
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, 1, Ho, Wo, K // 2, ldx // 2
    d.To, d.Ho, d.Wo, d.Co, d.ldy = 1, Ho, Wo, Cp, ldy
    d.kT, d.kH, d.kW = 1, k, k
    d.sT = d.sH = d.sW = 1
    d.pT, d.pH, d.pW = 0, k // 2, k // 2
    d.Kc, d.Co_pad, d.groups = ldx // 2, pd.Co_pad, 1
    d.flags = flags
    scd, shd = sc.to(DEV), sh.to(DEV)
    y = torch.full((N, 1, Ho, Wo, ldy), float("nan"), device=DEV, dtype=torch.bfloat16)
    yraw = torch.full((N, 1, Ho, Wo, ld_raw), float("nan"), device=DEV, dtype=torch.bfloat16)
    ext = L.ConvFusedExt()
    ext.scale, ext.shift, ext.ld_affine = scd.data_ptr(), shd.data_ptr(), ld_aff
    ext.y_raw, ext.ld_raw = yraw.data_ptr(), ld_raw
    pr = dict(x=_nhwc(x, ldx), wp=wp, bp=bp, res=res_d, y=y, yraw=yraw, d=d, ext=ext, keep=(scd, shd, wd, bd), Co=Co)
    return pr, (act, absact), (raw, absraw)


def _check_outputs(pr, want, raw, what):
    Co = pr["Co"]
    torch.cuda.synchronize()
    got = pr["y"].cpu().float()[:, 0]
    _close(got[..., :Co].permute(0, 3, 1, 2), want[0], want[1], what + " y")
    assert torch.isfinite(got[..., Co:pr["d"].Co]).all(), what + " pad channel"
    if pr["d"].flags & L.PTX_EPI_DUAL_RAW:
        gr = pr["yraw"].cpu().float()[:, 0]
        _close(gr[..., :Co].permute(0, 3, 1, 2), raw[0], raw[1], what + " y_raw")


def _launch_patch(pr):
    lib, d = L.lib(), pr["d"]
    x, wp, bp, y = [C.c_void_p(pr[k].data_ptr()) for k in ("x", "wp", "bp", "y")]
    if d.kH == 3:
        assert lib.ptx_conv3x3_bf16_supported(C.byref(d)) and not lib.ptx_conv3x3_f16_supported(C.byref(d))
        L.check(lib.ptx_conv3x3_bf16_fwd(C.byref(d), x, wp, bp, y, C.byref(pr["ext"]), _st()), "conv3x3_bf16")
    else:
        assert lib.ptx_conv1x1_skip_bf16_supported(C.byref(d)) and not lib.ptx_conv1x1_skip_f16_supported(C.byref(d))
        res = C.c_void_p(pr["res"].data_ptr()) if pr["res"] is not None else None
        L.check(lib.ptx_conv1x1_skip_bf16_fwd(C.byref(d), x, wp, bp, res, y, C.byref(pr["ext"]), _st()), "conv1x1_skip_bf16")


def _run_tiles(pr, want, raw, what, min_runs=2):
    """Every bf16 tile that takes the descriptor, with split-K 1 and 2 (the split-K reduce has its own fused epilogue)."""
    lib, d = L.lib(), pr["d"]
    seen = 0
    for cfg in range(lib.ptx_conv3d_num_configs(), lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16()):
        if not lib.ptx_conv3d_config_supported(C.byref(d), cfg):
            continue
        name = lib.ptx_conv3d_config_name(cfg).decode()
        for split in (1, 2):
            pr["y"].fill_(float("nan"))
            pr["yraw"].fill_(float("nan"))
            ws_bytes = lib.ptx_conv3d_workspace_bytes(C.byref(d), split)
            ws = torch.zeros(max(ws_bytes // 4, 4), device=DEV, dtype=torch.float32)
            rc = lib.ptx_conv3d_fused_fwd(C.byref(d), C.c_void_p(pr["x"].data_ptr()), C.c_void_p(pr["wp"].data_ptr()),
                                          C.c_void_p(pr["bp"].data_ptr()),
                                          C.c_void_p(pr["res"].data_ptr()) if pr["res"] is not None else None,
                                          C.c_void_p(pr["y"].data_ptr()), C.byref(pr["ext"]), _ptr(ws), ws_bytes, cfg, split, _st())
            if rc != 0:
                continue
            _check_outputs(pr, want, raw, "%s %s split %d" % (what, name, split))
            seen += 1
    assert seen >= min_runs, (what, seen)


C3 = [  # N, H, W, C, up2, affine, relu
    (2, 8, 32, 64, False, True, True),
    (1, 12, 20, 128, True, False, True),       # upsampling loader, bias only, ragged
    (1, 8, 16, 256, True, True, True),         # four input chunks, output channels over blockIdx.y
    (1, 19, 45, 64, True, True, True),         # ragged + upsampled
    (2, 16, 32, 128, False, True, True),       # 128 channels, plain loader (the <2, 4, false> kernel)
    (1, 16, 64, 256, False, True, True),       # 256 channels, plain loader (<4, 4, false>), two output-channel parts
]


@pytest.mark.parametrize("N,H,W,Cc,up2,affine,relu", C3)
@pytest.mark.parametrize("path", ["patch", "tile"])
def test_bf16_conv3x3_stage_parity(path, N, H, W, Cc, up2, affine, relu):
    pr, want, raw = _problem(3, N, H, W, Cc, Cc, up2=up2, affine=affine, relu=relu, seed=Cc + H)
    if path == "patch":
        _launch_patch(pr)
        _check_outputs(pr, want, raw, "conv3x3_bf16")
    else:
        _run_tiles(pr, want, raw, "3x3 tile")


C1 = [  # N, H, W, K, Co, skip, affine, dual, relu
    (2, 16, 32, 64, 128, "up", True, True, True),       # upsampled, channel-truncated skip, both outputs
    (2, 16, 64, 64, 256, "same", True, True, True),     # same-shape skip, two output-channel parts
    (1, 19, 45, 128, 128, "up", True, True, True),      # ragged tiles
    (1, 8, 32, 256, 256, "chan", True, True, False),    # channel truncation only
    (2, 8, 32, 64, 128, "up", False, False, False),     # raw output only (attention next)
    (1, 12, 40, 128, 128, "same", True, False, True),   # the last block: output BN + ReLU, no raw
]


@pytest.mark.parametrize("N,H,W,K,Co,skip,affine,dual,relu", C1)
@pytest.mark.parametrize("path", ["patch", "tile"])
def test_bf16_conv1x1_skip_stage_parity(path, N, H, W, K, Co, skip, affine, dual, relu):
    pr, want, raw = _problem(1, N, H, W, K, Co, skip=skip, affine=affine, relu=relu, dual=dual, seed=K + H)
    if path == "patch":
        _launch_patch(pr)
        _check_outputs(pr, want, raw, "conv1x1_skip_bf16")
    else:
        _run_tiles(pr, want, raw, "1x1 tile")


@pytest.mark.parametrize("case", ["conv1_affine", "small_map_dual", "image_tanh"])
def test_bf16_generic_tile_stage_parity(case):
    """Shapes only the generic bf16 tiles take in the plan: a GBlock's first 1x1 conv (affine + ReLU), the 4 x 4 / 8 x 8
    stages (upsampling 3x3, dual output over an fp32-free bf16 skip), and the 3-channel image conv with tanh."""
    if case == "conv1_affine":
        pr, want, raw = _problem(1, 2, 8, 8, 256, 64, affine=True, relu=True, seed=1)
    elif case == "small_map_dual":
        pr, want, raw = _problem(1, 3, 8, 8, 128, 256, skip="up", affine=True, relu=True, dual=True, seed=2)
    else:
        pr, want, raw = _problem(3, 2, 16, 16, 64, 3, tanh=True, seed=3)
    _run_tiles(pr, want, raw, case)


def test_bf16_affine_pass():
    """ptx_affine_act_upsample with PTX_ACT_OUT_BF16: the fp32 affine + ReLU (+ nearest 2x) rounded to bf16 once."""
    lib = L.lib()
    g = torch.Generator().manual_seed(9)
    N, H, W, C_, up = 3, 4, 4, 42, 2                  # C % 4 != 0: the kernel zeroes channels [C, round4(C))
    ldx, ldy, lds = 48, 56, 52
    x = torch.randn(N, H, W, ldx, generator=g) * 30.0
    sc, sh = torch.randn(N, lds, generator=g) * 5.0, torch.randn(N, lds, generator=g) * 5.0
    ref = (x[..., :C_].double() * sc[:, None, None, :C_].double() + sh[:, None, None, :C_].double())
    ref = ref.float().clamp_min(0)          # the kernel's fp32 FMA result, then one rounding
    ref = ref.repeat_interleave(up, 1).repeat_interleave(up, 2)
    xd, scd, shd = x.to(DEV), sc.to(DEV), sh.to(DEV)
    y = torch.full((N, H * up, W * up, ldy), float("nan"), device=DEV, dtype=torch.bfloat16)
    L.check(lib.ptx_affine_act_upsample(_ptr(xd), C.c_void_p(y.data_ptr()), _ptr(scd), _ptr(shd), lds, N, H, W, C_, ldx, ldy,
                                        up, 1 | L.PTX_ACT_OUT_BF16, _st()), "affine bf16")
    torch.cuda.synchronize()
    got = y.cpu().float()
    c4 = (C_ + 3) // 4 * 4
    assert torch.all(got[..., C_:c4] == 0) and torch.isnan(got[..., c4:]).all()     # (plan buffers start zeroed)
    err = (got[..., :C_].double() - ref.double()).abs()
    assert torch.all(err <= 2.0 ** -8 * ref.double().abs() + 1e-30), float(err.max())
    # both 16-bit output bits at once: refused
    assert lib.ptx_affine_act_upsample(_ptr(xd), C.c_void_p(y.data_ptr()), _ptr(scd), _ptr(shd), lds, N, H, W, C_, ldx, ldy,
                                       up, 1 | L.PTX_ACT_OUT_BF16 | L.PTX_ACT_OUT_F16, _st()) != 0


# ------------------------------------------------------------------------------------------------- generator parity
def _generator(res, ch, sd=None, seed=1234):
    G = ptx.biggan_deep(res, ch=ch)
    if sd is None:
        sd = synth_state_dict(G.state_dict(), seed, **BIGGAN_RECIPE)
        sd = {k: (_bfx(v) if v.is_floating_point() else v) for k, v in sd.items()}      # bf16-exact weights
    G.load_state_dict(sd)
    return G.eval().to(torch.bfloat16).to(DEV), sd


def _inputs(batch, sd, seed=3):
    g = torch.Generator().manual_seed(seed)
    z = _bfx(torch.randn(batch, 128, generator=g))
    lab = torch.randint(0, 1000, (batch,), generator=g)
    return z, lab


def _torch_bar(sd, z, yemb):
    """fp32 stand-in on the bf16-exact weights / inputs, PyTorch's own bf16 run of it, and the bar 2 x that error + 1e-3."""
    ref = BG.forward(sd, z, yemb)
    sd16 = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in sd.items()}
    err_torch = float((BG.forward(sd16, z.to(torch.bfloat16), yemb.to(torch.bfloat16)).float() - ref).abs().max())
    return ref, err_torch, 2 * err_torch + 1e-3


@pytest.mark.parametrize("res,ch,batch,check", [(128, 32, 3, None), (256, 128, 3, None), (256, 128, 64, (0, 21, 42, 63))])
def test_bf16_generator_parity(res, ch, batch, check):
    G, sd = _generator(res, ch)
    z, lab = _inputs(batch, sd)
    zd = z.to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        yd = G.shared(lab.to(DEV))
        assert yd.dtype == torch.bfloat16
        img = G(zd, yd)
        img2 = G(zd, yd)
    torch.cuda.synchronize()
    assert img.dtype == torch.bfloat16 and tuple(img.shape) == (batch, 3, res, res)
    assert torch.equal(img, img2)                                        # repeated calls: bit-identical
    idx = list(check) if check is not None else list(range(batch))      # (samples are independent: a subset at batch 64)
    ref, err_torch, bar = _torch_bar(sd, z[idx], sd["shared.weight"][lab[idx]])
    err = float((img[idx].float().cpu() - ref).abs().max())
    print("biggan-deep-%d ch %d batch %d bf16: max|d image| %.3e, torch bf16 %.3e, bar %.3e" % (res, ch, batch, err, err_torch, bar))
    assert err <= bar, (err, bar)


def _pre_output_bn(sd, z, yemb, depth=2, bottom_width=4, eps=1e-5):
    """oracle/biggan_standin.pre_tanh up to the output layer's BatchNorm: the raw last feature map (fp32)."""
    with torch.no_grad():
        y = torch.cat([yemb, z], 1)
        h = F.linear(y, sd["linear.weight"], sd["linear.bias"]).view(z.size(0), -1, bottom_width, bottom_width)
        i = 0
        while ("blocks.%d.0.conv1.weight" % i) in sd:
            for j in range(depth):
                h = BG.gblock(sd, h, y, "blocks.%d.%d" % (i, j), eps, upsample=(j == depth - 1))
            if ("blocks.%d.%d.theta.weight" % (i, depth)) in sd:
                h = BG.attention(sd, h, "blocks.%d.%d" % (i, depth))
            i += 1
        return h


def _output_layer(sd, h, eps=1e-5):
    p = "output_layer.0"
    h = F.batch_norm(h, sd[p + ".stored_mean"], sd[p + ".stored_var"], sd[p + ".gain"], sd[p + ".bias"], False, 0.1, eps)
    return torch.tanh(BG.conv(sd, F.relu(h), "output_layer.2", 1))


def test_bf16_generator_adversarial_tables():
    """The output-BN table that overflows / cancels in packed fp16 (tests/test_gpu_models.py's adversarial case): channel 0 at
    scale 7e4, every other channel at |mean| = 1e3 sigma.  In bf16 the same weights must come out within the bar of the
    UNMODIFIED generator on the same inputs -- the output BN runs in the last conv's fp32 epilogue on the unrounded sum.
    (PyTorch's own bf16 run of these weights loses the image to the cancellation, so its error is no yardstick here.)  The
    bar is shown to be able to fail: rounding the raw last feature map to bf16 BEFORE the output BN -- the failure this case
    rules out -- lands far above it."""
    G0 = ptx.biggan_deep(128, ch=32)
    clean = synth_state_dict(G0.state_dict(), 1234, **BIGGAN_RECIPE)
    sd = {k: v.clone() for k, v in clean.items()}
    clean = {k: (_bfx(v) if v.is_floating_point() else v) for k, v in clean.items()}
    eps = float(G0.bn_eps)
    bw2 = G0.bottom_width ** 2
    for k in list(sd):
        if k.endswith((".conv4.weight", ".conv4.bias", ".o.weight", ".o.bias")):
            sd[k][0] = 0.0
    sd["linear.weight"][:bw2] = 0.0
    sd["linear.bias"][:bw2] = 0.0
    last = max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    sigma = (sd["output_layer.0.stored_var"] + eps).sqrt()
    sd["output_layer.0.stored_mean"] = 1e3 * sigma
    sd["blocks.%d.1.conv4.bias" % last] = sd["blocks.%d.1.conv4.bias" % last] + sd["output_layer.0.stored_mean"]
    sd["blocks.%d.1.conv4.bias" % last][0] = 0.0
    sd["output_layer.0.stored_mean"][0] = 0.0
    sd["output_layer.0.stored_var"][0] = 0.0
    sd["output_layer.0.gain"][0] = 7e4 * eps ** 0.5
    sd = {k: (_bfx(v) if v.is_floating_point() else v) for k, v in sd.items()}
    z, lab = _inputs(2, sd, seed=5)
    _, err_clean, bar = _torch_bar(clean, z, clean["shared.weight"][lab])     # the bar of the unmodified generator
    assert bar < 0.2, bar
    ref = BG.forward(sd, z, sd["shared.weight"][lab])
    assert torch.isfinite(ref).all() and ref.std().item() > 1e-2
    # the control: the raw last feature map rounded to bf16 ahead of the output BN fails this bar
    h = _pre_output_bn(sd, z, sd["shared.weight"][lab], eps=eps)
    assert float((_output_layer(sd, h, eps) - ref).abs().max()) < 1e-5
    err_rounded = float((_output_layer(sd, _bfx(h), eps) - ref).abs().max())
    assert err_rounded > 2 * bar, (err_rounded, bar)
    G, _ = _generator(128, 32, sd)
    with torch.no_grad():
        img = G(z.to(DEV).to(torch.bfloat16), G.shared(lab.to(DEV)))
    torch.cuda.synchronize()
    err = float((img.float().cpu() - ref).abs().max())
    print("biggan bf16, adversarial output-BN tables: max|d image| %.3e (bar of the unmodified generator %.3e; raw map rounded "
          "before the BN %.3e)" % (err, bar, err_rounded))
    assert err <= bar, (err, bar)
    # the output BN + ReLU is the last conv4's fp32 epilogue (no packed-fp16 consumer kernel, no range guard)
    plan = list(G.engine()._plans.values())[-1]
    byl = {getattr(s_, "label", ""): s_ for s_ in plan.steps}
    f = byl["blocks.%d.1.conv4" % last].d.flags
    assert f & L.PTX_EPI_AFFINE and f & L.PTX_EPI_RELU and f & L.PTX_BF16_OPERANDS
    assert byl["output_layer.2"].d.flags & L.PTX_EPI_TANH


def test_bf16_generator_pad8_attention():
    """ch = 16: the attention's theta / phi are 4 channels wide, so phi and g start on the 8-channel boundaries of the pad8
    projection (8 and 16) with zero channels between the slices -- what the bf16 attention contracts over.  Parity, and the
    pad channels of the projection's output are zero after a run."""
    G, sd = _generator(128, 16)
    z, lab = _inputs(3, sd)
    with torch.no_grad():
        img = G(z.to(DEV).to(torch.bfloat16), G.shared(lab.to(DEV)))
    torch.cuda.synchronize()
    ref, err_torch, bar = _torch_bar(sd, z, sd["shared.weight"][lab])
    err = float((img.float().cpu() - ref).abs().max())
    print("biggan-deep-128 ch 16 bf16: max|d image| %.3e, torch bf16 %.3e, bar %.3e" % (err, err_torch, bar))
    assert err <= bar, (err, bar)
    plan = list(G.engine()._plans.values())[-1]
    (th, ph, g, y), = plan.attn_operands
    assert th.C == 4 and g.C == 16
    tpg = th.t._base                                   # the projection's whole output [N, 1, H, W, 32]
    assert tpg is not None and tpg.shape[-1] == 32 and th.t.storage_offset() == 0
    out = tpg.float().cpu()
    assert torch.all(out[..., 4:8] == 0) and torch.all(out[..., 12:16] == 0)    # theta's and phi's pad channels
    assert out[..., 0:4].abs().max() > 0 and out[..., 8:12].abs().max() > 0 and out[..., 16:32].abs().max() > 0


def test_bf16_generator_graph_capture():
    """A bf16 generator call, once its plan is built and tuned, captures into a CUDA graph (torch.cuda.graph) and replays
    bit-identically to the eager call."""
    G, sd = _generator(128, 32)
    z, lab = _inputs(2, sd)
    zd = z.to(DEV).to(torch.bfloat16)
    with torch.no_grad():
        yd = G.shared(lab.to(DEV))
        eager = G(zd, yd)
        G(zd, yd)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = G(zd, yd)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager)
        z2, y2 = zd.flip(0).contiguous(), yd.flip(0).contiguous()
        eager2 = G(z2, y2)
        zd.copy_(z2)                                     # new inputs in the captured buffers
        yd.copy_(y2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static_out, eager2)


def test_bf16_generator_refresh_and_api():
    G, sd = _generator(128, 32)
    z, lab = _inputs(2, sd)
    zd = z.to(DEV).to(torch.bfloat16)
    eng = G.engine()
    with torch.no_grad():
        yd = G.shared(lab.to(DEV))
        base = G(zd, yd)
        # an in-place update bumps _version: picked up on the next call
        G.blocks[1][0].conv2.weight.mul_(1.5)
        out1 = G(zd, yd)
        assert not torch.equal(out1, base)
        # a .data edit is invisible to _version: picked up after refresh()
        G.output_layer[0].bias.data.add_(0.5)
        G.refresh()
        out2 = G(zd, yd)
        assert not torch.equal(out2, out1)
        # the same under check_weights = "checksum", without refresh()
        saved, eng.check_weights = eng.check_weights, "checksum"
        G.blocks[3][2].gamma.data.mul_(0.25)
        out3 = G(zd, yd)
        assert not torch.equal(out3, out2)
        eng.check_weights = saved
        assert torch.equal(G(zd, yd), out3)
    # errors: fp32 inputs into a bf16 generator, bf16 into an fp32 one, CPU tensors
    with pytest.raises(PtxError):
        G(z.to(DEV), yd)
    with pytest.raises(PtxError):
        G(zd, yd.float())
    with pytest.raises(PtxError):
        G(zd.cpu(), yd.cpu())
    G32 = ptx.biggan_deep(128, ch=32).eval().to(DEV)
    with pytest.raises(PtxError):
        G32(zd, yd)
    G16 = ptx.biggan_deep(128, ch=32).eval().half().to(DEV)
    with pytest.raises(PtxError):
        G16(z.to(DEV), yd.float())
