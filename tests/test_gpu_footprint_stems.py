"""Footprint tests of the stem kernels and of their filter re-packs: ptx_conv_stem_f32_fwd (conv_stem_f32.hip),
ptx_conv_stem_x3_fwd / ptx_conv_stem_x3p_fwd (conv_stem_x3.hip), ptx_conv_stem_bf16_fwd and its frame-strided form
(conv_stem_bf16.hip), each at a small ragged row of its own test with that test's bar.  Operands sit in a guarded arena
(tests/arena.py), once under each fill: guards and inputs intact, nothing non-finite written, pad channels zero,
bit-identical outputs under the two fills (no atomics: nothing is excused).  The re-packs (ptx_pack_stem_f32_weight,
ptx_pack_stem_x3p_weight, ptx_pack_stem_bf16_weight) run in the arena too, and their OUTPUT is the filter the stem then reads,
so a wrong or fill-dependent re-pack fails the stem's float64 comparison.

Alignment (all refusals, no switch): "conv_stem_f32 / conv_stem_x3 / conv_stem_x3p: pointers must be 16-byte aligned" (x, filter,
y; conv_stem_f32.hip:177, conv_stem_x3.hip:546, :634); conv_stem_bf16.hip:356-357: the bf16 clip at any 2-byte alignment
(placed exactly 2 bytes off), uint8 frames at any byte (placed at an odd byte), filter and y 16; :334 ptx_pack_stem_bf16_weight:
the packed filter 2 bytes, the stem filter 16.  The biases and the re-packs' inputs sit at 16 bytes (not examined further)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from footprint import DEV, P, ST, judge, r4, repack, rnd, run
from test_gpu_bf16_stem import GEOMS, PLAIN255, _desc, _norm, _pack, _tap_filter
from test_gpu_kernels import make_bn, ref_conv

pytestmark = pytest.mark.gpu

F32, F16, BF16, U8 = torch.float32, torch.float16, torch.bfloat16, torch.uint8


def _dbl(bn):
    return tuple(t.double() for t in bn[:4]) + (bn[4],)


def _pack_folded(L, lib, w, bn, Kc, x3):
    """ptx_pack_conv_weight with the kW taps folded into the K axis, on plain allocations (set-up; its own footprint case is
    in test_gpu_footprint_layout.py)."""
    Co, Ci, kT, kH, kW = w.shape
    Co_pad = (Co + 127) // 128 * 128
    pd = L.PackDesc(Co, Ci, kT, kH, kW, Kc, Co_pad, 1)
    pd.f16 = 2 if x3 else 0
    wp = torch.empty(lib.ptx_packed_weight_elems(C.byref(pd)), device=DEV)
    bp = torch.empty(Co_pad, device=DEV)
    ts = [t.to(DEV) for t in bn[:4]]
    wd = w.contiguous().to(DEV)
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), P(wd), None, P(ts[0]), P(ts[1]), P(ts[2]), P(ts[3]), C.c_float(bn[4]), P(wp), P(bp), ST()),
            "pack folded")
    torch.cuda.synchronize()
    return wp.cpu(), bp.cpu(), Co_pad


@pytest.mark.parametrize("step", [1, 2], ids=["contiguous", "every_second_frame"])
def test_conv_stem_f32(ptx, step):
    """(2, 4, 20, 20) -> 110 channels, (1,7,7) stride (1,2,2) of test_conv_stem_f32_direct (two channel tiles, ragged), read from
    the NCDHW clip and from a frame-strided view of it passed as strides; 2e-5 x scale as there."""
    L, lib = ptx._lib, ptx._lib.lib()
    N, T, H, W, Co, k, s_, p_ = 2, 4, 20, 20, 110, (1, 7, 7), (1, 2, 2), (0, 3, 3)
    full = rnd(N, 3, T * step, H, W, seed=180)
    x = full[:, :, ::step]
    w = rnd(Co, 3, *k, seed=181, scale=(3 * k[0] * k[1] * k[2]) ** -0.5)
    bn = make_bn(Co, 182)
    want = ref_conv(x.double(), w.double(), s_, p_, bn=_dbl(bn), relu=True)
    To, Ho, Wo = want.shape[2:]
    Kc = 24
    wf, bp, Co_pad = _pack_folded(L, lib, w, bn, Kc, False)
    ldy = r4(Co)
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, 3, 0
    d.To, d.Ho, d.Wo, d.Co, d.ldy = To, Ho, Wo, Co, ldy
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = *k, *s_, *p_
    d.Kc, d.Co_pad, d.flags = Kc, Co_pad, L.PTX_EPI_RELU
    plane = H * W
    sn, sc, st = 3 * T * step * plane, T * step * plane, step * plane
    assert lib.ptx_conv_stem_f32_supported(C.byref(d), sn, sc, st)
    ws = repack(lambda a, b: L.check(lib.ptx_pack_stem_f32_weight(C.byref(d), a, Kc, b, ST()), "pack stem f32"), wf,
                 lib.ptx_stem_f32_weight_elems(C.byref(d)))

    def launch(v, ar):
        L.check(lib.ptx_conv_stem_f32_fwd(C.byref(d), P(v["x"]), sn, sc, st, P(v["ws"]), P(v["bp"]), P(v["y"]), ST()), "stem f32")
        assert lib.ptx_conv_stem_f32_fwd(C.byref(d), P(v["x"], 1), sn, sc, st, P(v["ws"]), P(v["bp"]), P(v["y"]), ST()) == 1
        assert b"pointers must be 16-byte aligned" in lib.ptx_last_error()           # host-side return, nothing launched

    out = run([("x", full.contiguous(), None, 16, "in"), ("ws", ws, None, 16, "in"), ("bp", bp, None, 16, "in"),
               ("y", (N, To, Ho, Wo, ldy), F32, 16, "out")], launch)
    judge(out, "y", want.permute(0, 2, 3, 4, 1), 2e-5, (Ellipsis, slice(0, Co)), written=Ellipsis, zero=[(Ellipsis, slice(Co, ldy))])


def test_conv_stem_x3_and_planar(ptx):
    """(2, 3, 2, 40, 48) -> 110 channels, (1,7,7) stride (1,2,2) of test_conv_stem_x3_direct (the row both kernels take): the
    16-byte-position kernel on ptx_ncdhw_to_split4's format and the planar kernel on ptx_ncdhw_to_split_planes' (both built
    on the host with the same fp32 operations; their own footprint cases are in test_gpu_footprint_layout.py); 2e-5 x scale."""
    L, lib = ptx._lib, ptx._lib.lib()
    N, Ci, T, H, W, Co, k, s_, p_ = 2, 3, 2, 40, 48, 110, (1, 7, 7), (1, 2, 2), (0, 3, 3)
    x = rnd(N, Ci, T, H, W, seed=80)
    w = rnd(Co, Ci, *k, seed=81, scale=(Ci * k[0] * k[1] * k[2]) ** -0.5)
    bn = make_bn(Co, 82)
    want = ref_conv(x.double(), w.double(), s_, p_, bn=_dbl(bn), relu=True).permute(0, 2, 3, 4, 1)
    To, Ho, Wo = want.shape[1:4]
    v4 = torch.zeros(N, T, H, W, 4)
    v4[..., :Ci] = x.permute(0, 2, 3, 4, 1)
    hi = v4.to(F16)
    x4 = torch.cat([hi, ((v4 - hi.float()) * 4096.0).to(F16)], -1)                       # [N][T][H][W] positions of 8 halfs
    v3 = x.permute(0, 2, 1, 3, 4).contiguous()
    h3 = v3.to(F16)
    xpl = torch.cat([h3, ((v3 - h3.float()) * 4096.0).to(F16)], 2)                       # [N][T][6][H][W]
    w4 = torch.zeros(Co, 4, *k)
    w4[:, :Ci] = w
    wp, bp, Co_pad = _pack_folded(L, lib, w4, bn, 32, True)
    ldy = r4(Co)
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, Ci, 4
    d.To, d.Ho, d.Wo, d.Co, d.ldy = To, Ho, Wo, Co, ldy
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = *k, *s_, *p_
    d.Kc, d.Co_pad, d.flags = 32, Co_pad, L.PTX_EPI_RELU | L.PTX_F16X3_OPERANDS
    assert lib.ptx_conv_stem_x3_supported(C.byref(d)) and lib.ptx_conv_stem_x3p_supported(C.byref(d))
    wq = repack(lambda a, b: L.check(lib.ptx_pack_stem_x3p_weight(C.byref(d), a, b, ST()), "pack planar stem"), wp,
                 lib.ptx_stem_x3p_weight_elems(C.byref(d)))

    def launch(v, ar):
        L.check(lib.ptx_conv_stem_x3_fwd(C.byref(d), P(v["x4"]), P(v["wp"]), P(v["bp"]), P(v["y"]), ST()), "stem x3")
        L.check(lib.ptx_conv_stem_x3p_fwd(C.byref(d), P(v["xpl"]), P(v["wq"]), P(v["bp"]), P(v["yq"]), ST()), "stem x3 planar")
        for fn, xs, ws_, ys in ((lib.ptx_conv_stem_x3_fwd, "x4", "wp", "y"), (lib.ptx_conv_stem_x3p_fwd, "xpl", "wq", "yq")):
            assert fn(C.byref(d), P(v[xs]), P(v[ws_]), P(v["bp"]), P(v[ys], 1), ST()) == 1      # host-side return, nothing launched
            assert b"pointers must be 16-byte aligned" in lib.ptx_last_error()

    out = run([("x4", x4, None, 16, "in"), ("xpl", xpl, None, 16, "in"), ("wp", wp, None, 16, "in"), ("wq", wq, None, 16, "in"),
               ("bp", bp, None, 16, "in"), ("y", (N, To, Ho, Wo, ldy), F32, 16, "out"), ("yq", (N, To, Ho, Wo, ldy), F32, 16, "out")], launch)
    for name in ("y", "yq"):
        judge(out, name, want, 2e-5, (Ellipsis, slice(0, Co)), written=Ellipsis, zero=[(Ellipsis, slice(Co, ldy))])


@pytest.mark.parametrize("step", [1, 2], ids=["every_frame", "every_second_frame"])
@pytest.mark.parametrize("src", ["bf16", "u8"])
@pytest.mark.parametrize("geom", ["r3d_tiny", "r2p1d_83"])
def test_conv_stem_bf16(ptx, geom, src, step):
    """The exact-tap problems of tests/test_gpu_bf16_stem.py (integer operands, +-1 taps: every product and sum is exact in
    bf16, so the comparison is exact) on "r3d_tiny" (every window touches both paddings) and "r2p1d_83" (odd Co, two channel
    tiles, pad channels), from a bf16 clip exactly 2 bytes off a 4-byte boundary and from uint8 frames at an odd byte, through
    ptx_conv_stem_bf16_fwd and ptx_conv_stem_bf16_strided_fwd (every second frame of a longer source)."""
    L, lib = ptx._lib, ptx._lib.lib()
    (k, s, p), Co, (T, H, W) = GEOMS[geom]
    N = 2
    T_full = T * step - (step - 1)                                   # ceil(T_full / step) == T
    g = torch.Generator().manual_seed(11)
    d = _desc(geom, relu=False)
    if src == "bf16":
        full = torch.randint(-8, 9, (N, 3, T_full, H, W), generator=g).float()
        w = _tap_filter(geom, 4, 12)
        xin, norm, code, align = full.to(BF16), None, L.PTX_STEM_SRC_BF16_NCDHW, 2
        used = full[:, :, ::step]
    else:
        frames = torch.randint(0, 256, (N, T_full, H, W, 3), dtype=U8, generator=g)
        w = _tap_filter(geom, 1, 22)
        xin, norm, code, align = frames, _norm(dict(PLAIN255, input_space="RGB")), L.PTX_STEM_SRC_U8_NTHWC, 1
        used = frames.permute(0, 4, 1, 2, 3).float()[:, :, ::step]
    assert used.shape[2] == T
    wp, bp, wf, _, _ = _pack(w, None)
    assert torch.equal(wf, w.double())
    want = F.conv3d(used.double(), w.double(), None, s, p).permute(0, 2, 3, 4, 1)
    ws = repack(lambda a, b: L.check(lib.ptx_pack_stem_bf16_weight(C.byref(d), a, b, ST()), "pack stem bf16"), wp.cpu(),
                 lib.ptx_stem_bf16_weight_elems(C.byref(d)), BF16, a_in=2)
    nref = C.byref(norm) if norm is not None else None

    def launch(v, ar):
        if step == 1:
            L.check(lib.ptx_conv_stem_bf16_fwd(C.byref(d), P(v["x"]), code, nref, P(v["ws"]), P(v["bp"]), P(v["y"]), ST()), "stem bf16")
        else:
            assert lib.ptx_conv_stem_bf16_strided_supported(C.byref(d), code, step, T_full), lib.ptx_last_error()
            L.check(lib.ptx_conv_stem_bf16_strided_fwd(C.byref(d), P(v["x"]), code, nref, step, T_full, P(v["ws"]), P(v["bp"]), P(v["y"]),
                                                       ST()), "stem bf16 strided")
        assert lib.ptx_conv_stem_bf16_fwd(C.byref(d), P(v["x"]), code, nref, P(v["ws"]), P(v["bp"]), P(v["y"], 1), ST()) == 1
        assert b"filter and output must be 16-byte aligned" in lib.ptx_last_error()      # host-side return, nothing launched

    out = run([("x", xin.contiguous(), None, align, "in"), ("ws", ws, None, 16, "in"), ("bp", bp.cpu(), None, 16, "in"),
               ("y", (N, d.To, d.Ho, d.Wo, d.ldy), BF16, 16, "out")], launch)
    judge(out, "y", want, 0, (Ellipsis, slice(0, Co)), written=Ellipsis, zero=[(Ellipsis, slice(Co, d.ldy))])
