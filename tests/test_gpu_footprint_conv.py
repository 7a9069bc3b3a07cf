"""Footprint tests of the dense implicit-GEMM convolution (ptx_conv3d_fwd: conv_igemm.hip / conv_igemm_kernel.h): x, the packed
filter, the bias, the residual, y and the split-K workspace all carved out of one guarded arena (tests/arena.py) at 16-byte
alignment -- the weakest ptx_conv3d_fwd accepts ("conv3d: pointers must be 16-byte aligned", "conv3d: bias must be 16-byte
aligned") -- once under each fill.  Per case: guards and inputs intact, nothing non-finite written, pad channels
[Co, round_up(Co, 4)) zero and the columns beyond still holding the fill, a float64 reference at the 2e-4 of
test_gpu_kernels.py::test_conv_every_config_and_split (`close`; 2e-5 for the split-operand tiles, as
test_conv_x3_split_operands), bit-identical outputs under the two fills.

Excused from bit-equality: nothing.  The only atomics these launches reach are the integer tile counters of
PTX_SPLITK_FUSED (conv_igemm_kernel.h, `__hip_atomic_fetch_add(p.counters + tile, 1u, ...)`); the partial sums are added in
split order by the last arriver or by splitk_reduce_kernel, never with floating-point atomics.

The buffer resources of these kernels clamp at host-computed byte counts such as M * ldy * 4, which over-count when y is a
channel slice of a wider row: the slice cases here are the ones where only the per-lane selects stand between a tile's
ragged edge and the neighbouring columns."""
import ctypes as C

import pytest
import torch

from footprint import DEV, P, ST, cl, judge, r4, rnd, run
from test_gpu_kernels import GEOMS, fp32_configs, make_bn, ref_conv, x3_configs

pytestmark = pytest.mark.gpu

F32 = torch.float32
TOL = 2e-4                                  # fp32 tiles: test_conv_every_config_and_split (`close`)
TOL_X3 = 2e-5                               # split-operand tiles: test_conv_x3_split_operands, same scaling
NPART = 8                                   # the tile configurations are spread over this many test cases


def _lib(ptx):
    return ptx._lib.lib()


_PACKED = {}


def _pack(ptx, key, w, bn, bias, x3):
    """ptx_pack_conv_weight as tests/test_gpu_kernels.py::hip_conv calls it; the packed filter and bias come back to the host
    (they are `in` operands of the arena), once per distinct filter."""
    if key in _PACKED:
        return _PACKED[key]
    L, lib = ptx._lib, _lib(ptx)
    Co, Ci, kT, kH, kW = w.shape
    pd = L.PackDesc(Co, Ci, kT, kH, kW, (Ci + 7) // 8 * 8 if x3 else r4(Ci), (Co + 127) // 128 * 128, 0)
    pd.f16 = 2 if x3 else 0
    wp = torch.empty(lib.ptx_packed_weight_elems(C.byref(pd)), device=DEV)
    bp = torch.empty(pd.Co_pad, device=DEV)
    wd = w.contiguous().to(DEV)
    null = C.c_void_p(0)
    bnargs, eps, keep = [null] * 4, 0.0, []
    if bn is not None:
        keep = [t.contiguous().to(DEV) for t in bn[:4]]
        bnargs, eps = [P(t) for t in keep], bn[4]
    bd = bias.to(DEV) if bias is not None else None
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), P(wd), P(bd) if bd is not None else null, *bnargs, C.c_float(eps), P(wp), P(bp),
                                     ST()), "pack")
    torch.cuda.synchronize()
    _PACKED[key] = (wp.cpu(), bp.cpu(), pd.Kc, pd.Co_pad)
    return _PACKED[key]


def conv_case(ptx, key, x, w, stride, padding, bn=None, bias=None, relu=False, res=None, res_pad=None, res_stride=1, cfg=-1,
              split=0, x3=False, fused=False, x_cols=None, y_cols=None, must_support=False):
    """x_cols = (first column, row stride): x is a channel slice of a wider row whose other columns hold NaN;
    y_cols likewise for y, whose other columns must keep the fill."""
    L, lib = ptx._lib, _lib(ptx)
    Co, Ci, kT, kH, kW = w.shape
    N, _, T, H, W = x.shape
    (sT, sH, sW), (pT, pH, pW) = stride, padding
    To, Ho, Wo = (T + 2 * pT - kT) // sT + 1, (H + 2 * pH - kH) // sH + 1, (W + 2 * pW - kW) // sW + 1
    wp, bp, Kc, Co_pad = _pack(ptx, key, w, bn, bias, x3)
    x0, ldx = x_cols or (0, r4(Ci))
    xd = torch.full((N, T, H, W, ldx), float("nan"))
    xd[..., x0:x0 + r4(Ci)] = cl(x)
    y0, ldy = y_cols or (0, r4(Co))
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, Ci, ldx
    d.To, d.Ho, d.Wo, d.Co, d.ldy = To, Ho, Wo, Co, ldy
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = kT, kH, kW, sT, sH, sW, pT, pH, pW
    d.Kc, d.Co_pad = Kc, Co_pad
    flags = (L.PTX_EPI_RELU if relu else 0) | (L.PTX_F16X3_OPERANDS if x3 else 0) | (L.PTX_SPLITK_FUSED if fused else 0)
    specs = [("x", xd, None, 16, "in"), ("wp", wp, None, 16, "in"), ("bp", bp, None, 16, "in")]
    if res is not None:
        rd = cl(res)
        d.ldr = rd.shape[-1]
        flags |= L.PTX_EPI_RES_ADD
        specs.append(("res", rd, None, 16, "in"))
    if res_pad is not None:
        rd = cl(res_pad)
        d.ldr = rd.shape[-1]
        d.res_C, d.res_T, d.res_H, d.res_W = res_pad.shape[1:]
        d.res_sT = d.res_sH = d.res_sW = res_stride
        flags |= L.PTX_EPI_RES_PADA
        specs.append(("res", rd, None, 16, "in"))
    d.flags = flags
    assert not must_support or lib.ptx_conv3d_config_supported(C.byref(d), cfg) == 1, lib.ptx_conv3d_config_name(cfg)
    ws_bytes = lib.ptx_conv3d_workspace_bytes(C.byref(d), split if split > 0 else 8)
    specs.append(("y", (N, To, Ho, Wo, ldy), F32, 16, "out"))
    # the fused reduction's contract: the caller zeroes the workspace once (its tile counters return to zero after a launch)
    specs.append(("ws", (max(ws_bytes // 4, 4),), F32, 16, "scratch", fused))
    want = ref_conv(x.double(), w.double(), stride, padding, bias=None if bias is None else bias.double(),
                    bn=None if bn is None else tuple(t.double() for t in bn[:4]) + (bn[4],), relu=relu,
                    res=None if res is None else res.double(), res_pad=None if res_pad is None else res_pad.double(),
                    res_stride=res_stride)

    def launch(v, ar):
        L.check(lib.ptx_conv3d_fwd(C.byref(d), P(v["x"], x0), P(v["wp"]), P(v["bp"]), P(v["res"]) if "res" in v else None,
                                   P(v["y"], y0), P(v["ws"]), ws_bytes, cfg, split, ST()), "conv %s" % (key,))

    res_ = run(specs, launch)
    c4 = r4(Co)
    judge(res_, "y", want.permute(0, 2, 3, 4, 1), TOL_X3 if x3 else TOL, (Ellipsis, slice(y0, y0 + Co)), written=(Ellipsis, slice(y0, y0 + c4)),
          zero=[(Ellipsis, slice(y0 + Co, y0 + c4))], untouched=[(Ellipsis, slice(0, y0)), (Ellipsis, slice(y0 + c4, ldy))])


def _ragged():
    """N,T,H,W,Ci,Co = 2,3,9,10,64,160, 3x3x3, pad 1 (test_conv_every_config_and_split): M = 540 against 64 / 128 / 256-row
    tiles, Co ragged against 128; BN + residual + ReLU."""
    N, T, H, W, Ci, Co = 2, 3, 9, 10, 64, 160
    x, w = rnd(N, Ci, T, H, W, seed=4), rnd(Co, Ci, 3, 3, 3, seed=5, scale=0.03)
    return x, w, make_bn(Co, 6), rnd(N, Co, T, H, W, seed=7)


@pytest.mark.parametrize("part", range(NPART))
@pytest.mark.parametrize("kind", ["fp32", "x3"])
def test_every_tile_configuration_split_1_and_2(ptx, kind, part):
    lib = _lib(ptx)
    x, w, bn, res = _ragged()
    x3 = kind == "x3"
    cfgs = (x3_configs(lib) if x3 else fp32_configs(lib))[part::NPART]
    for cfg in cfgs:
        for split in (1, 2):
            conv_case(ptx, ("ragged", kind), x, w, (1, 1, 1), (1, 1, 1), bn=bn, relu=True, res=res, cfg=cfg, split=split, x3=x3)


def test_splitk_fused(ptx):
    """PTX_SPLITK_FUSED once (test_splitk_fused_reduction's shape): the zeroed workspace sits in the arena as well."""
    lib = _lib(ptx)
    names = [lib.ptx_conv3d_config_name(i).decode() for i in range(lib.ptx_conv3d_num_configs())]
    x, w, bn, res = _ragged()
    cfg = [c for c in fp32_configs(lib) if not names[c].endswith("/direct")][0]
    conv_case(ptx, ("ragged", "fp32"), x, w, (1, 1, 1), (1, 1, 1), bn=bn, relu=True, res=res, cfg=cfg, split=2, fused=True)


@pytest.mark.parametrize("name", ["spatial_odd", "c5_generic"])
def test_auto_configuration(ptx, name):
    _, N, T, H, W, Ci, Co, k, s, p = [g for g in GEOMS if g[0] == name][0]
    x, w = rnd(N, Ci, T, H, W, seed=1), rnd(Co, Ci, *k, seed=2, scale=(Ci * k[0] * k[1] * k[2]) ** -0.5)
    conv_case(ptx, (name, "fp32"), x, w, s, p, bn=make_bn(Co, 3), relu=True)


def test_y_and_x_as_channel_slices(ptx):
    """y a channel slice of a wider row (slowfast's torch.cat(dim=1) of branch outputs), then x a slice with ldx > Ci whose
    other columns hold NaN: "columns [Kc, ldx) of a wider row meet no filter column, so they are not read at all"."""
    x, w, bn, res = _ragged()
    for split in (1, 2):
        conv_case(ptx, ("ragged", "fp32"), x, w, (1, 1, 1), (1, 1, 1), bn=bn, relu=True, res=res, split=split, y_cols=(8, 160 + 24))
        conv_case(ptx, ("ragged", "fp32"), x, w, (1, 1, 1), (1, 1, 1), bn=bn, relu=True, res=res, split=split, x_cols=(0, 64 + 12))


def test_shortcut_a_residual(ptx):
    """Stride-2 conv with the subsampled, channel-padded shortcut-A residual (test_conv_epilogues' last case), split 3."""
    x, w3 = rnd(2, 64, 4, 8, 8, seed=11), rnd(128, 64, 3, 3, 3, seed=16, scale=0.03)
    conv_case(ptx, ("shortcut_a", "fp32"), x, w3, (2, 2, 2), (1, 1, 1), bn=make_bn(128, 13), relu=True,
              res_pad=rnd(2, 48, 4, 8, 8, seed=17), res_stride=2, split=3)


def test_bias_alignment_is_refused(ptx):
    """The row-major epilogues, the direct kernel and the split-K reduction read four biases with one 16-byte load; a bias that
    is only 4-byte aligned used to be launched as it was.  Now it is PTX_ERR_INVALID with a message (a host-side return:
    nothing is launched) -- for ptx_conv3d_fwd and for bias2 of ptx_conv3d_chain_fwd.  (An aligned bias is what every other case
    of this module passes.)"""
    L, lib = ptx._lib, _lib(ptx)
    buf = torch.zeros(128 * 64 + 4096 + 256, device=DEV)
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = 1, 1, 4, 4, 64, 64
    d.To, d.Ho, d.Wo, d.Co, d.ldy = 1, 4, 4, 4, 4
    d.kT = d.kH = d.kW = d.sT = d.sH = d.sW = 1
    d.Kc, d.Co_pad = 64, 128
    st = lib.ptx_conv3d_fwd(C.byref(d), P(buf), P(buf), P(buf, 1), None, P(buf, 4096), None, 0, 2, 1, ST())
    assert st == 1 and b"bias must be 16-byte aligned" in lib.ptx_last_error()
    t = L.ConvDesc()
    t.N, t.Ti, t.Hi, t.Wi, t.Ci, t.ldx = 1, 1, 4, 4, 4, 4
    t.To, t.Ho, t.Wo, t.Co, t.ldy = 1, 4, 4, 4, 4
    t.kT = t.kH = t.kW = t.sT = t.sH = t.sW = 1
    t.Kc, t.Co_pad = 4, 128
    args = (C.byref(d), C.byref(t), P(buf), P(buf), P(buf))
    st = lib.ptx_conv3d_chain_fwd(*args, P(buf), P(buf, 1), None, P(buf, 4096), -1, ST())
    assert st == 1 and b"bias2 must be 16-byte aligned" in lib.ptx_last_error()
    torch.cuda.synchronize()


def _pack_plain(ptx, pd, w, bn, wp=None, bp=None):
    """One ptx_pack_conv_weight call on plain allocations (a K window of an existing buffer when wp / bp are given)."""
    L, lib = ptx._lib, _lib(ptx)
    wp = torch.full((lib.ptx_packed_weight_elems(C.byref(pd)),), float("nan"), device=DEV) if wp is None else wp
    bp = torch.full((pd.Co_pad,), float("nan"), device=DEV) if bp is None else bp
    ts = [t.contiguous().to(DEV) for t in bn[:4]]
    wd = w.contiguous().to(DEV)
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), P(wd), None, P(ts[0]), P(ts[1]), P(ts[2]), P(ts[3]), C.c_float(bn[4]), P(wp), P(bp),
                                     ST()), "pack")
    torch.cuda.synchronize()
    return wp, bp


def test_dual_source(ptx):
    """ptx_conv3d_dual_fwd at the smallest (and ragged) row of test_dual_source_conv: 20 + 36 input channels, 72 outputs, the second
    source a stride-2 gather; x2 is "conv3d_dual: x2 must be 16-byte aligned" like the rest.  2e-4 (`close`)."""
    L, lib = ptx._lib, _lib(ptx)
    N, T, H, W, C1, C2, Co, s_ = 1, 1, 5, 6, 20, 36, 72, 2
    T2, H2, W2 = (T - 1) * s_ + 1, (H - 1) * s_ + 1 + (s_ - 1), (W - 1) * s_ + 1
    o, x = rnd(N, C1, T, H, W, seed=60), rnd(N, C2, T2, H2, W2, seed=61)
    w3, wd = rnd(Co, C1, 1, 1, 1, seed=62, scale=C1 ** -0.5), rnd(Co, C2, 1, 1, 1, seed=63, scale=C2 ** -0.5)
    bn3, bnd = make_bn(Co, 64), make_bn(Co, 65)
    dbl = lambda bn: tuple(t.double() for t in bn[:4]) + (bn[4],)                          # noqa: E731
    want = torch.relu(ref_conv(o.double(), w3.double(), (1, 1, 1), (0, 0, 0), bn=dbl(bn3)) +
                      ref_conv(x.double(), wd.double(), (s_, s_, s_), (0, 0, 0), bn=dbl(bnd)))
    Kc, Kc2, Co_pad = r4(C1), r4(C2), (Co + 127) // 128 * 128
    ld = Kc + Kc2
    wp, bp = None, None
    for (wt, bn, Ci_, kc, koff, acc) in ((w3, bn3, C1, Kc, 0, 0), (wd, bnd, C2, Kc2, Kc, 1)):
        pd = L.PackDesc(Co, Ci_, 1, 1, 1, kc, Co_pad, 0, ld, koff, acc)
        if wp is None:
            wp, bp = torch.full((Co_pad * ld,), float("nan"), device=DEV), torch.full((Co_pad,), float("nan"), device=DEV)
        _pack_plain(ptx, pd, wt, bn, wp, bp)
    od, xd = cl(o), cl(x)
    ldy = r4(Co) + 4
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, C1, od.shape[-1]
    d.To, d.Ho, d.Wo, d.Co, d.ldy = T, H, W, Co, ldy
    d.kT = d.kH = d.kW = d.sT = d.sH = d.sW = 1
    d.Kc, d.Co_pad, d.flags = Kc, Co_pad, L.PTX_EPI_RELU
    d.x2_C, d.x2_ld, d.x2_T, d.x2_H, d.x2_W = C2, xd.shape[-1], T2, H2, W2
    d.x2_sT = d.x2_sH = d.x2_sW = s_
    ws_bytes = lib.ptx_conv3d_workspace_bytes(C.byref(d), 8)

    def launch(v, ar):
        L.check(lib.ptx_conv3d_dual_fwd(C.byref(d), P(v["o"]), P(v["x2"]), P(v["wp"]), P(v["bp"]), P(v["y"]), P(v["ws"]), ws_bytes, -1, 0,
                                        ST()), "dual conv")

    out = run([("o", od, None, 16, "in"), ("x2", xd, None, 16, "in"), ("wp", wp.cpu(), None, 16, "in"), ("bp", bp.cpu(), None, 16, "in"),
               ("y", (N, T, H, W, ldy), F32, 16, "out"), ("ws", (max(ws_bytes // 4, 4),), F32, 16, "scratch")], launch)
    judge(out, "y", want.permute(0, 2, 3, 4, 1), TOL, (Ellipsis, slice(0, Co)), untouched=[(Ellipsis, slice(Co, ldy))])


def test_grouped(ptx):
    """Grouped 3x3x3 conv on the direct tiles at the smallest row of test_grouped_conv (64 channels in 4 groups, 1 x 3 x 6 x 7),
    library's own choice of tile.  2e-4 (`close`)."""
    import torch.nn.functional as F
    L, lib = ptx._lib, _lib(ptx)
    N, T, H, W, Cin, Co, G, s = 1, 3, 6, 7, 64, 64, 4, (1, 1, 1)
    cig = Cin // G
    x, w = rnd(N, Cin, T, H, W, seed=140), rnd(Co, cig, 3, 3, 3, seed=141, scale=(cig * 27) ** -0.5)
    bn = make_bn(Co, 142)
    want = torch.relu(F.batch_norm(F.conv3d(x.double(), w.double(), None, s, 1, 1, G), bn[2].double(), bn[3].double(), bn[0].double(),
                                   bn[1].double(), False, 0.1, bn[4]))
    pd = L.PackDesc(Co, cig, 3, 3, 3, r4(cig), (Co + 127) // 128 * 128, 0)
    wp, bp = _pack_plain(ptx, pd, w, bn)
    ldy = Co + 8
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, Cin, Cin
    d.To, d.Ho, d.Wo, d.Co, d.ldy = T, H, W, Co, ldy
    d.kT = d.kH = d.kW = 3
    d.sT, d.sH, d.sW = s
    d.pT = d.pH = d.pW = 1
    d.Kc, d.Co_pad, d.flags, d.groups = pd.Kc, pd.Co_pad, L.PTX_EPI_RELU, G

    def launch(v, ar):
        L.check(lib.ptx_conv3d_fwd(C.byref(d), P(v["x"]), P(v["wp"]), P(v["bp"]), None, P(v["y"]), None, 0, -1, 1, ST()), "grouped conv")

    out = run([("x", cl(x), None, 16, "in"), ("wp", wp.cpu(), None, 16, "in"), ("bp", bp.cpu(), None, 16, "in"),
               ("y", (N, T, H, W, ldy), F32, 16, "out")], launch)
    judge(out, "y", want.permute(0, 2, 3, 4, 1), TOL, (Ellipsis, slice(0, Co)), untouched=[(Ellipsis, slice(Co, ldy))])


@pytest.mark.parametrize("workers", ["2", "5", None], ids=["two_tiles_per_worker", "a_worker_without_a_tile", "default_grid"])
def test_weight_stationary_tile(ptx, workers, monkeypatch):
    """The persistent weight-stationary tile (".../ws", conv_ws_kernel.h) at the smallest ragged case of tests/test_gpu_conv_ws.py:
    a pointwise conv with M = 105 = 3 x 32 + 9 rows (four row tiles, the last ragged), K = 64, Co = 100 (ragged column blocks),
    ReLU + residual, ldx = Ci + 8 with NaN in the foreign columns, ldy = Co + 12.  2e-4 x scale, that module's bar."""
    lib = _lib(ptx)
    names = [lib.ptx_conv3d_config_name(i).decode() for i in range(lib.ptx_conv3d_num_configs())]
    tiles = [i for i, n in enumerate(names) if n.endswith("/ws")]
    assert tiles
    if workers is None:
        monkeypatch.delenv("PTX_WS_WORKERS", raising=False)
    else:
        monkeypatch.setenv("PTX_WS_WORKERS", workers)
    N, T, H, W, Ci, Co = 1, 1, 7, 15, 64, 100
    x, w = rnd(N, Ci, T, H, W, seed=100), rnd(Co, Ci, 1, 1, 1, seed=101, scale=Ci ** -0.5)
    bn, res = make_bn(Co, 102), rnd(N, Co, T, H, W, seed=103)
    for cfg in tiles:
        conv_case(ptx, ("ws", "fp32"), x, w, (1, 1, 1), (0, 0, 0), bn=bn, relu=True, res=res, cfg=cfg, split=1,
                  x_cols=(0, Ci + 8), y_cols=(0, Co + 12), must_support=True)
