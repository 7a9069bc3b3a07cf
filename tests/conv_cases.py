"""Run ONE convolution problem given as a filled descriptor ({field: int}, tests/tuned_cases.py) on a named tile with a given
split, next to its float64 reference on the CPU.  The driver of test_gpu_tuned_table.py: the entry point is the one the
descriptor calls for (ptx_conv3d_fwd, ptx_conv3d_dual_fwd with a second source, ptx_conv3d_fused_fwd under a fused
generator-stage flag, ptx_conv3d_chain_fwd for a (conv, tail) pair), tiles are looked up by NAME, the workspace is sized
by ptx_conv3d_workspace_bytes.

Operands.  Activations are seeded Gaussians; filters are Gaussians scaled by (Ci / groups * taps) ** -0.5, so outputs are
O(1).  fp32 and split-operand ("/x3") problems fold an eval-mode BatchNorm into the filter (ptx_pack_conv_weight) and the
reference applies it in float64 to the UNROUNDED operands.  fp16-operand problems round activations and filter to half
first and carry a bias instead (a folded filter would be rounded a second time), as _fused_stage_case of
test_gpu_kernels.py does; a half skip operand is rounded the same way.

Layout contract checked on every run: the output is pre-filled with NaN; columns [Co, round_up(Co, 4)) come back zero and
the columns from there to ldy are still NaN; the result is finite in [0, Co).  Input columns [Ci, Kc) are zero (the
project's contract for pad channels), input columns [Kc, ldx) -- which no filter column multiplies -- hold NaN and must not
reach the result.
"""
import ctypes as C

import torch
import torch.nn.functional as F

from tuned_cases import fill

DEV = "cuda:0"
FUSED_FLAGS = 0x200 | 0x400 | 0x800 | 0x1000 | 0x2000 | 0x4000     # OUT_F16, AFFINE, DUAL_RAW, RES_F16, PRO_UP2, TANH
NAN = float("nan")


def _r4(v):
    return (v + 3) // 4 * 4


def _r8(v):
    return (v + 7) // 8 * 8


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=_gen(seed))


def _bn(c, seed):
    g = _gen(seed)
    return (torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.1, torch.randn(c, generator=g) * 0.1,
            torch.rand(c, generator=g) + 0.5, 1e-5)


def _bn_affine64(bn):
    gamma, beta, mean, var, eps = bn
    scale = gamma.double() / torch.sqrt(var.double() + eps)
    return scale, beta.double() - mean.double() * scale


def tile_index(lib, name, chain=False):
    """Index of a tile by NAME in this build's table (KeyError if the build has no such tile)."""
    if chain:
        names = {lib.ptx_conv3d_chain_config_name(i).decode(): i for i in range(lib.ptx_conv3d_chain_num_configs())}
    else:
        names = {lib.ptx_conv3d_config_name(i).decode(): i
                 for i in range(lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16())}
    return names[name]


def _channels_last(t, ld, dtype, live_end, nan_from):
    """NCDHW fp32 -> [N][T][H][W][ld] of `dtype`: columns [C, live_end) zero, [nan_from, ld) NaN."""
    n, c = t.shape[:2]
    y = torch.zeros(n, *t.shape[2:], ld, dtype=dtype)
    y[..., :c] = t.permute(0, 2, 3, 4, 1).to(dtype)
    if nan_from < ld:
        assert nan_from >= max(c, live_end)
        y[..., nan_from:] = NAN
    return y


def conv64(x, w, d, groups=1):
    """float64 conv3d of x [N][C][Ti][Hi][Wi] under the descriptor's geometry, symmetric or SAME: the front pad is p, the
    back pad whatever the last output needs; positions beyond the descriptor's output extent are cut."""
    pads = []
    for n_in, n_out, k, s, p in ((d["Wi"], d["Wo"], d["kW"], d["sW"], d["pW"]), (d["Hi"], d["Ho"], d["kH"], d["sH"], d["pH"]),
                                 (d["Ti"], d["To"], d["kT"], d["sT"], d["pT"])):
        pads += [p, max((n_out - 1) * s + k - n_in - p, 0)]
    y = F.conv3d(F.pad(x.double(), pads), w.double(), None, (d["sT"], d["sH"], d["sW"]), 0, 1, groups)
    return y[:, :, :d["To"], :d["Ho"], :d["Wo"]]


def _pack(L, lib, w, Kc, Co_pad, bn=None, bias=None, f16=0, ld_k=0, k_off=0, accumulate=0, out=None):
    """ptx_pack_conv_weight of w [Co][Ci][kT][kH][kW] (BatchNorm folded when given) -> (w_packed, bias) on the device."""
    Co, Ci, kT, kH, kW = w.shape
    pd = L.PackDesc(Co, Ci, kT, kH, kW, Kc, Co_pad, 0, ld_k, k_off, accumulate, 0, 0, f16)
    if out is None:
        n = lib.ptx_packed_weight_elems(C.byref(pd))
        wp = torch.zeros(n, device=DEV, dtype=torch.float16 if f16 == 1 else torch.float32)
        bp = torch.zeros(Co_pad, device=DEV)
    else:
        wp, bp = out
    wd = w.contiguous().to(DEV)
    bnd = [t.contiguous().to(DEV) for t in bn[:4]] if bn is not None else [None] * 4
    bd = bias.to(DEV) if bias is not None else None
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), _vp(wd), _vp(bd), *[_vp(t) for t in bnd],
                                     C.c_float(bn[4] if bn is not None else 0.0), _vp(wp), _vp(bp), _st()), "pack")
    torch.cuda.synchronize()
    return wp, bp


def _check_layout(yd, Co, what):
    """Pad columns zero, columns beyond untouched (NaN), live columns finite."""
    live, pad, beyond = yd[..., :Co], yd[..., Co:_r4(Co)], yd[..., _r4(Co):]
    assert bool(torch.isfinite(live).all()), "%s: non-finite values in the live columns" % what
    assert pad.numel() == 0 or bool((pad == 0).all()), "%s: pad columns [Co, round_up(Co, 4)) must be written as zero" % what
    assert beyond.numel() == 0 or bool(torch.isnan(beyond).all()), "%s: columns beyond round_up(Co, 4) must stay untouched" % what


def _ncdhw(yd, Co):
    return yd[..., :Co].permute(0, 4, 1, 2, 3).double().cpu()


def run_conv(ptx, d, tile, split, seed=0, mutate=None):
    """One launch of the conv problem `d` on `tile` with `split`.  Returns a list of (got, want, bar) -- float64 CPU
    tensors in NCDHW and the RELATIVE tolerance of that output (the main output; the raw halfs of PTX_EPI_DUAL_RAW) -- the
    layout contract already asserted.  mutate: "no_residual" / "drop_tap" falsify the REFERENCE (the tests of the tests)."""
    L, lib = ptx._lib, ptx._lib.lib()
    fl = d["flags"]
    f16, x3 = bool(fl & L.PTX_F16_OPERANDS), bool(fl & L.PTX_F16X3_OPERANDS)
    fused = bool(fl & FUSED_FLAGS)
    up2, out16, res16 = bool(fl & L.PTX_PRO_UP2), bool(fl & L.PTX_EPI_OUT_F16), bool(fl & L.PTX_RES_F16)
    words = 2 if f16 else 1                                   # 16-bit operands: Ci / ldx / Kc count channel pairs
    adt = torch.float16 if f16 else torch.float32
    rnd16 = (lambda t: t.half().float()) if f16 else (lambda t: t)
    N, Co, groups = d["N"], d["Co"], max(d["groups"], 1)
    Ci = d["Ci"] * words
    cig = Ci // groups
    taps = d["kT"] * d["kH"] * d["kW"]
    what = "%s split %d on %s" % (tile, split, {k: v for k, v in d.items() if v})

    # ---- operands and the float64 reference
    Hs, Ws = (d["Hi"] // 2, d["Wi"] // 2) if up2 else (d["Hi"], d["Wi"])              # stored extents
    x = rnd16(_randn(seed + 1, N, Ci, d["Ti"], Hs, Ws))
    w = rnd16(_randn(seed + 2, Co, cig, d["kT"], d["kH"], d["kW"]) * (cig * taps) ** -0.5)
    xin = x.repeat_interleave(2, 3).repeat_interleave(2, 4) if up2 else x
    w_ref = w
    if mutate == "drop_tap":
        w_ref = w.clone()
        w_ref[:, :, d["kT"] // 2, d["kH"] // 2, d["kW"] // 2] = 0        # the centre tap: live at every output
    v = conv64(xin, w_ref, d, groups)
    bn = bias = None
    if f16:
        bias = _randn(seed + 3, Co)
        v = v + bias.double()[None, :, None, None, None]
    else:
        bn = _bn(Co, seed + 3)
        sc, sh = _bn_affine64(bn)
        v = v * sc[None, :, None, None, None] + sh[None, :, None, None, None]
    x2 = w2 = bn2 = None
    if d["x2_C"] > 0:
        x2 = _randn(seed + 4, N, d["x2_C"], d["x2_T"], d["x2_H"], d["x2_W"])
        w2 = _randn(seed + 5, Co, d["x2_C"], 1, 1, 1) * d["x2_C"] ** -0.5
        bn2 = _bn(Co, seed + 6)
        sc2, sh2 = _bn_affine64(bn2)
        g = x2[:, :, ::d["x2_sT"], ::d["x2_sH"], ::d["x2_sW"]][:, :, :d["To"], :d["Ho"], :d["Wo"]]
        v2 = F.conv3d(g.double(), w2.double())
        v = v + v2 * sc2[None, :, None, None, None] + sh2[None, :, None, None, None]
    res = None
    rdt = torch.float16 if res16 else torch.float32
    if fl & L.PTX_EPI_RES_ADD:
        res = _randn(seed + 7, N, Co, d["To"], d["Ho"], d["Wo"])
        res = res.half().float() if res16 else res
        add = res.double()
    elif fl & L.PTX_EPI_RES_PADA:
        res = _randn(seed + 7, N, d["res_C"], d["res_T"], d["res_H"], d["res_W"])
        res = res.half().float() if res16 else res
        up = bool(fl & L.PTX_EPI_RES_UP)
        # shortcut A: index = out * res_s*, zero channels above res_C; PTX_EPI_RES_UP: the nearest-upsampled, channel-truncated
        # skip, index = out >> res_s*
        it, ih, iw = [(torch.arange(n) >> s) if up else (torch.arange(n) * s)
                      for n, s in ((d["To"], d["res_sT"]), (d["Ho"], d["res_sH"]), (d["Wo"], d["res_sW"]))]
        sub = res.double()[:, :, it][:, :, :, ih][:, :, :, :, iw]
        add = torch.zeros_like(v)
        add[:, :min(Co, d["res_C"])] = sub[:, :Co]
    if res is not None and mutate != "no_residual":
        v = v + add
    raw_want = v
    ld_aff = _r4(Co) + 4
    aff_s = torch.rand(N, ld_aff, generator=_gen(seed + 8)) + 0.5
    aff_b = _randn(seed + 9, N, ld_aff) * 0.3
    if fl & L.PTX_EPI_AFFINE:
        v = v * aff_s.double()[:, :Co, None, None, None] + aff_b.double()[:, :Co, None, None, None]
    if fl & L.PTX_EPI_RELU:
        v = F.relu(v)
    if fl & L.PTX_EPI_TANH:
        v = torch.tanh(v)

    # ---- the device side
    ldx, Kc = d["ldx"] * words, d["Kc"] * words
    if groups > 1:
        xd = _channels_last(x, ldx, adt, ldx, ldx)
    else:
        xd = _channels_last(x, ldx, adt, min(Kc, ldx), min(Kc, ldx))
    xd = xd.to(DEV)
    x2d = None
    kind = 1 if f16 else 2 if x3 else 0
    if x2 is not None:
        kc2 = _r8(d["x2_C"]) if x3 else _r4(d["x2_C"])
        ld_k = d["Kc"] + kc2
        out = (torch.zeros(d["Co_pad"] * ld_k, device=DEV), torch.zeros(d["Co_pad"], device=DEV))
        wp, bp = _pack(L, lib, w, d["Kc"], d["Co_pad"], bn=bn, f16=kind, ld_k=ld_k, out=out)
        _pack(L, lib, w2, kc2, d["Co_pad"], bn=bn2, f16=kind, ld_k=ld_k, k_off=d["Kc"], accumulate=1, out=out)
        x2d = _channels_last(x2, d["x2_ld"], torch.float32, d["x2_ld"], d["x2_ld"]).to(DEV)
    else:
        wp, bp = _pack(L, lib, w, Kc, d["Co_pad"], bn=bn, bias=bias, f16=kind)
    rd = None
    if res is not None:
        rd = _channels_last(res, d["ldr"], rdt, d["ldr"], d["ldr"]).to(DEV)
    ydt = torch.float16 if out16 else torch.float32
    yd = torch.full((N, d["To"], d["Ho"], d["Wo"], d["ldy"]), NAN, device=DEV, dtype=ydt)
    cd = fill(d)
    cfg = tile_index(lib, tile)
    ws_bytes = int(lib.ptx_conv3d_workspace_bytes(C.byref(cd), split))
    assert (ws_bytes > 0) == (split > 1)
    ws = torch.empty(max(ws_bytes // 4, 4), device=DEV)
    rawd = None
    if d["x2_C"] > 0:
        st = lib.ptx_conv3d_dual_fwd(C.byref(cd), _vp(xd), _vp(x2d), _vp(wp), _vp(bp), _vp(yd), _vp(ws), ws_bytes, cfg,
                                     split, _st())
    elif fused:
        ext = L.ConvFusedExt()
        sd, bd = aff_s.to(DEV), aff_b.to(DEV)
        ext.scale, ext.shift, ext.ld_affine = sd.data_ptr(), bd.data_ptr(), ld_aff
        ld_raw = _r8(_r4(Co))
        rawd = torch.full((N, d["To"], d["Ho"], d["Wo"], ld_raw), NAN, device=DEV, dtype=torch.float16)
        ext.y_raw, ext.ld_raw = rawd.data_ptr(), ld_raw
        st = lib.ptx_conv3d_fused_fwd(C.byref(cd), _vp(xd), _vp(wp), _vp(bp), _vp(rd), _vp(yd), C.byref(ext), _vp(ws),
                                      ws_bytes, cfg, split, _st())
    else:
        st = lib.ptx_conv3d_fwd(C.byref(cd), _vp(xd), _vp(wp), _vp(bp), _vp(rd), _vp(yd), _vp(ws), ws_bytes, cfg, split, _st())
    assert st == 0, "%s: status %d: %s" % (what, st, lib.ptx_last_error().decode())
    torch.cuda.synchronize()
    _check_layout(yd, Co, what)
    # the project's own bars: close() for fp32 tiles, test_conv_x3_split_operands for x3, _fused_stage_case for f16
    bar = (2e-3 if out16 else 2e-4) if f16 else 2e-5 if x3 else 2e-4
    outs = [(_ncdhw(yd, Co), v, bar)]
    if fl & L.PTX_EPI_DUAL_RAW:
        assert bool(torch.isfinite(rawd[..., :Co]).all()), what
        outs.append((_ncdhw(rawd, Co), raw_want, 2e-3))
    return outs


def run_chain(ptx, d, t, tile, seed=0, mutate=None):
    """One ptx_conv3d_chain_fwd launch of the pair (d, t) on the chained `tile`: [(got, want, bar)] as run_conv, the bar
    test_conv_chain's (2e-5 of the output scale, fp32 and split operands alike)."""
    L, lib = ptx._lib, ptx._lib.lib()
    x3 = bool(d["flags"] & L.PTX_F16X3_OPERANDS)
    N, N1, Co2 = d["N"], d["Co"], t["Co"]
    taps = d["kT"] * d["kH"] * d["kW"]
    what = "%s on %s -> %s" % (tile, {k: v for k, v in d.items() if v}, {k: v for k, v in t.items() if v})
    x = _randn(seed + 1, N, d["Ci"], d["Ti"], d["Hi"], d["Wi"])
    w1 = _randn(seed + 2, N1, d["Ci"], d["kT"], d["kH"], d["kW"]) * (d["Ci"] * taps) ** -0.5
    w2 = _randn(seed + 3, Co2, N1, 1, 1, 1) * N1 ** -0.5
    bn1, bn2 = _bn(N1, seed + 4), _bn(Co2, seed + 5)
    w1_ref = w1
    if mutate == "drop_tap":
        w1_ref = w1.clone()
        w1_ref[:, :, d["kT"] // 2, d["kH"] // 2, d["kW"] // 2] = 0
    sc, sh = _bn_affine64(bn1)
    mid = conv64(x, w1_ref, d) * sc[None, :, None, None, None] + sh[None, :, None, None, None]
    mid = F.relu(mid) if d["flags"] & L.PTX_EPI_RELU else mid
    sc, sh = _bn_affine64(bn2)
    v = F.conv3d(mid, w2.double()) * sc[None, :, None, None, None] + sh[None, :, None, None, None]
    res = None
    if t["flags"] & L.PTX_EPI_RES_ADD:
        res = _randn(seed + 6, N, Co2, d["To"], d["Ho"], d["Wo"])
        if mutate != "no_residual":
            v = v + res.double()
    v = F.relu(v) if t["flags"] & L.PTX_EPI_RELU else v
    kind = 2 if x3 else 0
    wp1, bp1 = _pack(L, lib, w1, d["Kc"], d["Co_pad"], bn=bn1, f16=kind)
    wp2, bp2 = _pack(L, lib, w2, t["Kc"], t["Co_pad"], bn=bn2, f16=kind)
    live = min(d["Kc"], d["ldx"])
    xd = _channels_last(x, d["ldx"], torch.float32, live, live).to(DEV)
    rd = _channels_last(res, t["ldr"], torch.float32, t["ldr"], t["ldr"]).to(DEV) if res is not None else None
    yd = torch.full((N, d["To"], d["Ho"], d["Wo"], t["ldy"]), NAN, device=DEV)
    st = lib.ptx_conv3d_chain_fwd(C.byref(fill(d)), C.byref(fill(t)), _vp(xd), _vp(wp1), _vp(bp1), _vp(wp2), _vp(bp2),
                                  _vp(rd), _vp(yd), tile_index(lib, tile, chain=True), _st())
    assert st == 0, "%s: status %d: %s" % (what, st, lib.ptx_last_error().decode())
    torch.cuda.synchronize()
    _check_layout(yd, Co2, what)
    return [(_ncdhw(yd, Co2), v, 2e-5)]


def error_over_bar(got, want, bar):
    """max|got - want| over the project's tolerance bar * max(1, max|want|) (close() of test_gpu_kernels.py)."""
    assert got.shape == want.shape
    return (got - want).abs().max().item() / (bar * max(1.0, want.abs().max().item()))
