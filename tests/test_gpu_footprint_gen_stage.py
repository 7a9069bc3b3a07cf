"""Footprint tests of the 16-bit generator-stage kernels (gen_stage_f16.hip) at the smallest rows of their tests, with those
tests' bars: fp16 from tests/test_gpu_kernels.py (4e-3 absolute for the RGB conv, 2e-3 / 3e-3 x scale for the others), bf16
from tests/test_gpu_biggan_bf16.py (2^-8 |ref| + 2^-20 conv(|x|, |w|): one bf16 rounding of the fp32 sum).  Operands sit in a
guarded arena (tests/arena.py) at 16 bytes -- "rgb_conv3x3_f16: pointers must be 16-byte aligned", "%s: misaligned pointer"
of the other entries, and the PTX_EPI_AFFINE tables as below; the RGB conv's three biases are read one float at a time: 4
bytes -- once under each fill.  Guards and inputs intact, nothing non-finite written, columns [Co, ldy) still holding the
fill, float64 references on the rounded operands, bit-identical outputs under the two fills (no atomics: none excused).

Found while reading the kernels for this module: conv3x3_kernel and the 1x1 skip kernel read the PTX_EPI_AFFINE tables four
channels per load, and ptx_conv3x3_f16/bf16_fwd, ptx_conv1x1_skip_f16/bf16_fwd and (for its OUTPUT tables)
ptx_conv1x1_pro_f16_fwd checked only ld_affine % 4, not the tables' own alignment.  They now refuse with PTX_ERR_INVALID like
ptx_conv3d_fused_fwd; each of the five refusals (a host-side return, nothing launched) is asserted below, status and message."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from arena import FILLS
from footprint import DEV, P, ST, judge, repack, rnd, run

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def _kind(L, kind):
    """(torch dtype, operand flags, pack code, entry-name infix)"""
    if kind == "bf16":
        return BF16, L.PTX_F16_OPERANDS | L.PTX_BF16_OPERANDS | L.PTX_EPI_OUT_F16, L.PTX_PACK_BF16, "bf16"
    return F16, L.PTX_F16_OPERANDS | L.PTX_EPI_OUT_F16, 1, "f16"


def _check(res, name, want, absref, kind, Co, ldy, tol16):
    """fp16: judge at tol16 x scale.  bf16: the derived bar of tests/test_gpu_biggan_bf16.py, then judge's other parts."""
    live, rest = (Ellipsis, slice(0, Co)), [(Ellipsis, slice(Co, ldy))]
    if kind == "bf16":
        for out in res:
            err = (out[name][live].double() - want).abs()
            assert bool((err <= 2.0 ** -8 * want.abs() + 2.0 ** -20 * absref + 1e-30).all()), (name, float(err.max()))
        judge(res, name, want, None, live, untouched=rest)
    else:
        judge(res, name, want, tol16, live, untouched=rest)


def _refusals(lib, call, v, ext, names=("sc", "sh")):
    """The entry with either table 4 bytes off: PTX_ERR_INVALID and the message; host-side, nothing is launched."""
    for off_sc, off_sh in ((4, 0), (0, 4)):
        ext.scale, ext.shift = v[names[0]].data_ptr() + off_sc, v[names[1]].data_ptr() + off_sh
        assert call(ext) == 1
        assert b"16-byte aligned scale / shift tables" in lib.ptx_last_error()
    ext.scale, ext.shift = v[names[0]].data_ptr(), v[names[1]].data_ptr()


def test_rgb_conv3x3_f16(ptx):
    """(1, 8, 32, 32) of test_rgb_conv3x3_f16, 4e-3 absolute; channel 3 of every output position is written as zero."""
    L, lib = ptx._lib, ptx._lib.lib()
    N, H, W, Cc = 1, 8, 32, 32
    g_ = torch.Generator().manual_seed(7 + H + Cc)
    ldx, lda = Cc + 8, Cc + 4
    x = (torch.randn(N, H, W, ldx, generator=g_) * 1.5).half()
    scale = torch.rand(N, lda, generator=g_) + 0.5
    shift = torch.randn(N, lda, generator=g_) * 0.3
    w = torch.randn(3, Cc, 3, 3, generator=g_) * (1.0 / (9 * Cc)) ** 0.5
    b = torch.randn(3, generator=g_) * 0.1
    act = F.relu((x[..., :Cc].float() * scale[:, None, None, :Cc].half().float() + shift[:, None, None, :Cc].half().float()).half().float())
    want = torch.tanh(F.conv2d(act.permute(0, 3, 1, 2).double(), w.half().double(), b.double(), padding=1)).permute(0, 2, 3, 1)
    # the filter pack runs in the arena too (w [3][C][3][3] fp32 in, the half layout out); its output is what the conv reads
    wp = repack(lambda a, b: L.check(lib.ptx_pack_rgb_conv_weight(a, Cc, b, ST()), "pack"), w.contiguous(),
                int(lib.ptx_rgb_conv_weight_elems(Cc)), F16)
    d = L.RgbConvDesc(N, H, W, Cc, ldx, 4, lda, L.PTX_EPI_TANH)
    assert lib.ptx_rgb_conv3x3_f16_supported(C.byref(d))

    def launch(v, ar):
        L.check(lib.ptx_rgb_conv3x3_f16_fwd(C.byref(d), P(v["x"]), P(v["scale"]), P(v["shift"]), P(v["wp"]), P(v["b"]), P(v["y"]), ST()),
                "rgb conv")

    res = run([("x", x, None, 16, "in"), ("scale", scale, None, 16, "in"), ("shift", shift, None, 16, "in"), ("wp", wp, None, 16, "in"),
               ("b", b, None, 4, "in"), ("y", (N, H, W, 4), F32, 16, "out")], launch)
    judge(res, "y", want, 4e-3, (Ellipsis, slice(0, 3)), written=Ellipsis, zero=[(Ellipsis, slice(3, 4))], absolute=True)


def _operands(L, lib, kind, N, H, W, K, Co, k, seed):
    """x [N][1][H][W][K + 8] and the packed [Co][K] (k x k) filter in the 16-bit type, bias fp32; values exact in that type."""
    dt, flags, code, _ = _kind(L, kind)
    x = rnd(N, K, 1, H, W, seed=seed).to(dt).float()
    w = rnd(Co, K, 1, k, k, seed=seed + 1, scale=(K * k * k) ** -0.5).to(dt).float()
    bias = rnd(Co, seed=seed + 2)
    ldh = K + 8
    xh = torch.zeros(N, 1, H, W, ldh, dtype=dt)
    xh[..., :K] = x.permute(0, 2, 3, 4, 1).to(dt)
    pd = L.PackDesc(Co, K, 1, k, k, ldh, (Co + 127) // 128 * 128, 0, 0, 0, 0, 0, 0, code)
    wp = torch.empty(lib.ptx_packed_weight_elems(C.byref(pd)), device=DEV, dtype=dt)
    bp = torch.empty(pd.Co_pad, device=DEV)
    wd, bd = w.to(DEV), bias.to(DEV)
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), P(wd), P(bd), None, None, None, None, C.c_float(0), P(wp), P(bp), ST()), "pack 16-bit")
    torch.cuda.synchronize()
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, 1, H, W, K // 2, ldh // 2
    d.To, d.Ho, d.Wo, d.Co = 1, H, W, Co
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = 1, k, k, 1, 1, 1, 0, k // 2, k // 2
    d.Kc, d.Co_pad, d.groups, d.flags = ldh // 2, pd.Co_pad, 1, flags
    return x, w, bias, xh, wp.cpu(), bp.cpu(), d


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_conv3x3(ptx, kind, affine):
    """ptx_conv3x3_f16_fwd / ptx_conv3x3_bf16_fwd at (3, 8, 32, 64) of test_conv3x3_f16_patch_kernel (one tile per image), plain
    and with the per-sample affine; y is 16-bit with ldy = C + 16."""
    L, lib = ptx._lib, ptx._lib.lib()
    dt, _, _, nm = _kind(L, kind)
    N, H, W, Cc = 3, 8, 32, 64
    x, w, bias, xh, wp, bp, d = _operands(L, lib, kind, N, H, W, Cc, Cc, 3, 400 + Cc + H)
    ld_aff, ldy = Cc + 4, Cc + 16
    sc = torch.rand(N, ld_aff, generator=torch.Generator().manual_seed(405)) + 0.5
    sh = rnd(N, ld_aff, seed=406, scale=0.3)
    v = F.conv3d(x.double(), w.double(), bias.double(), 1, (0, 1, 1))
    a = F.conv3d(x.double().abs(), w.double().abs(), bias.double().abs(), 1, (0, 1, 1))
    if affine:
        s_, t_ = sc.double()[:, :Cc, None, None, None], sh.double()[:, :Cc, None, None, None]
        v, a = v * s_ + t_, a * s_.abs() + t_.abs()
    d.ldy = ldy
    d.flags |= L.PTX_EPI_AFFINE if affine else 0
    fwd = getattr(lib, "ptx_conv3x3_%s_fwd" % nm)
    assert getattr(lib, "ptx_conv3x3_%s_supported" % nm)(C.byref(d))

    def launch(v_, ar):
        ext = L.ConvFusedExt()
        ext.scale, ext.shift, ext.ld_affine = v_["sc"].data_ptr(), v_["sh"].data_ptr(), ld_aff
        args = (C.byref(d), P(v_["x"]), P(v_["wp"]), P(v_["bp"]), P(v_["y"]))
        L.check(fwd(*args, C.byref(ext) if affine else None, ST()), "conv3x3_%s" % nm)
        if affine:
            _refusals(lib, lambda e: fwd(*args, C.byref(e), ST()), v_, ext)

    res = run([("x", xh, None, 16, "in"), ("wp", wp, None, 16, "in"), ("bp", bp, None, 16, "in"), ("sc", sc, None, 16, "in"),
               ("sh", sh, None, 16, "in"), ("y", (N, 1, H, W, ldy), dt, 16, "out")], launch)
    _check(res, "y", v[:, :, 0].permute(0, 2, 3, 1).unsqueeze(1), a[:, :, 0].permute(0, 2, 3, 1).unsqueeze(1), kind, Cc, ldy, 2e-3)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_conv1x1_skip(ptx, kind):
    """ptx_conv1x1_skip_f16_fwd / _bf16_fwd at the smallest row of test_conv1x1_skip_f16_kernel that has every operand
    ((2, 16, 32, 64, 128): upsampled, channel-truncated 16-bit skip, affine + ReLU, raw AND activated output).  res and y_raw
    are placed too (16 bytes: "%s: misaligned pointer")."""
    L, lib = ptx._lib, ptx._lib.lib()
    dt, _, _, nm = _kind(L, kind)
    N, H, W, K, Co = 2, 16, 32, 64, 128
    x, w, bias, xh, wp, bp, d = _operands(L, lib, kind, N, H, W, K, Co, 1, 500 + K + H)
    Cr, rh, rw = Co + 64, H // 2, W // 2
    r = rnd(N, Cr, 1, rh, rw, seed=503).to(dt).float()
    rr = F.interpolate(r[:, :Co, 0].double(), scale_factor=2, mode="nearest").unsqueeze(2)
    v = F.conv3d(x.double(), w.double(), bias.double()) + rr
    a = F.conv3d(x.double().abs(), w.double().abs(), bias.double().abs()) + rr.abs()
    ldr = Cr + 8
    rt = torch.zeros(N, 1, rh, rw, ldr, dtype=dt)
    rt[..., :Cr] = r.permute(0, 2, 3, 4, 1).to(dt)
    ld_aff, ldy, ld_raw = Co + 4, Co + 8, Co + 16
    sc = torch.rand(N, ld_aff, generator=torch.Generator().manual_seed(505)) + 0.5
    sh = rnd(N, ld_aff, seed=506, scale=0.3)
    s_, t_ = sc.double()[:, :Co, None, None, None], sh.double()[:, :Co, None, None, None]
    act, act_abs = F.relu(v * s_ + t_), a * s_.abs() + t_.abs()
    d.ldy, d.ldr = ldy, ldr
    d.res_C, d.res_T, d.res_H, d.res_W, d.res_sT, d.res_sH, d.res_sW = Cr, 1, rh, rw, 0, 1, 1
    d.flags |= L.PTX_EPI_RES_PADA | L.PTX_EPI_RES_UP | L.PTX_RES_F16 | L.PTX_EPI_AFFINE | L.PTX_EPI_RELU | L.PTX_EPI_DUAL_RAW
    fwd = getattr(lib, "ptx_conv1x1_skip_%s_fwd" % nm)
    assert getattr(lib, "ptx_conv1x1_skip_%s_supported" % nm)(C.byref(d))

    def launch(v_, ar):
        ext = L.ConvFusedExt()
        ext.scale, ext.shift, ext.ld_affine = v_["sc"].data_ptr(), v_["sh"].data_ptr(), ld_aff
        ext.y_raw, ext.ld_raw = v_["raw"].data_ptr(), ld_raw
        args = (C.byref(d), P(v_["x"]), P(v_["wp"]), P(v_["bp"]), P(v_["res"]), P(v_["y"]))
        L.check(fwd(*args, C.byref(ext), ST()), "conv1x1_skip_%s" % nm)
        _refusals(lib, lambda e: fwd(*args, C.byref(e), ST()), v_, ext)

    res = run([("x", xh, None, 16, "in"), ("wp", wp, None, 16, "in"), ("bp", bp, None, 16, "in"), ("res", rt, None, 16, "in"),
               ("sc", sc, None, 16, "in"), ("sh", sh, None, 16, "in"), ("y", (N, 1, H, W, ldy), dt, 16, "out"),
               ("raw", (N, 1, H, W, ld_raw), dt, 16, "out")], launch)
    nhwc = lambda t: t[:, :, 0].permute(0, 2, 3, 1).unsqueeze(1)                                      # noqa: E731
    _check(res, "y", nhwc(act), nhwc(act_abs), kind, Co, ldy, 2e-3)
    _check(res, "raw", nhwc(v), nhwc(a), kind, Co, ld_raw, 2e-3)


def test_conv1x1_pro_f16(ptx):
    """ptx_conv1x1_pro_f16_fwd at the smallest row of test_conv1x1_pro_f16_kernel ((2, 16, 16, 256, 64), input and output
    affine, ReLU), 3e-3 x scale; all four tables at 16 bytes: the input tables were checked with the other pointers, the output
    tables (read four channels per load like the rest) only for ld_affine % 4 until this change; all refusals asserted."""
    L, lib = ptx._lib, ptx._lib.lib()
    N, H, W, K, Co = 2, 16, 16, 256, 64
    x, w, bias, xh, wp, bp, d = _operands(L, lib, "f16", N, H, W, K, Co, 1, 600 + K)
    ld1, ld2, ldy = K + 4, Co + 4, Co + 8
    g_ = torch.Generator().manual_seed(603)
    s1, t1 = torch.rand(N, ld1, generator=g_) + 0.5, torch.randn(N, ld1, generator=g_) * 0.3
    s2, t2 = torch.rand(N, ld2, generator=g_) + 0.5, torch.randn(N, ld2, generator=g_) * 0.3
    act = F.relu((x * s1[:, :K, None, None, None].half().float() + t1[:, :K, None, None, None].half().float()).half().float())
    v = F.conv3d(act.double(), w.double(), bias.double())
    v = F.relu(v * s2.double()[:, :Co, None, None, None] + t2.double()[:, :Co, None, None, None])
    d.ldy = ldy
    d.flags |= L.PTX_EPI_AFFINE | L.PTX_EPI_RELU
    assert lib.ptx_conv1x1_pro_f16_supported(C.byref(d))

    def launch(v_, ar):
        ext_in, ext = L.ConvFusedExt(), L.ConvFusedExt()
        ext_in.scale, ext_in.shift, ext_in.ld_affine = v_["s1"].data_ptr(), v_["t1"].data_ptr(), ld1
        ext.scale, ext.shift, ext.ld_affine = v_["s2"].data_ptr(), v_["t2"].data_ptr(), ld2
        L.check(lib.ptx_conv1x1_pro_f16_fwd(C.byref(d), P(v_["x"]), C.byref(ext_in), P(v_["wp"]), P(v_["bp"]), P(v_["y"]), C.byref(ext),
                                            ST()), "conv1x1_pro_f16")
        call = lambda e: lib.ptx_conv1x1_pro_f16_fwd(C.byref(d), P(v_["x"]), C.byref(ext_in), P(v_["wp"]), P(v_["bp"]), P(v_["y"]),   # noqa: E731
                                                     C.byref(e), ST())
        _refusals(lib, call, v_, ext, names=("s2", "t2"))              # the OUTPUT tables 4 bytes off: refused since this change
        for off_s, off_t in ((4, 0), (0, 4)):                           # the INPUT tables: "conv1x1_pro_f16: misaligned pointer"
            ext_in.scale, ext_in.shift = v_["s1"].data_ptr() + off_s, v_["t1"].data_ptr() + off_t
            assert call(ext) == 1 and b"misaligned pointer" in lib.ptx_last_error()

    res = run([("x", xh, None, 16, "in"), ("wp", wp, None, 16, "in"), ("bp", bp, None, 16, "in"), ("s1", s1, None, 16, "in"),
               ("t1", t1, None, 16, "in"), ("s2", s2, None, 16, "in"), ("t2", t2, None, 16, "in"), ("y", (N, 1, H, W, ldy), F16, 16, "out")],
              launch)
    judge(res, "y", v[:, :, 0].permute(0, 2, 3, 1).unsqueeze(1), 3e-3, (Ellipsis, slice(0, Co)), untouched=[(Ellipsis, slice(Co, ldy))])
    assert len(res) == len(FILLS)
