"""Footprint tests of the patch-resident fp32 body kernels (conv_body_f32.hip: ptx_conv_body_f32_fwd on its tall / square
tiles and on the T-stacked tile of (kT,1,1) convs) at the smallest and the ragged rows of test_gpu_kernels.py::
test_conv_body_f32 / test_conv_tstack_f32, tolerance 2e-4 x scale (`close`) as there.  x, the body-layout filter, the bias, the
residual and y (ldy > round_up(Co, 4): a channel slice of a wider row) sit in a guarded arena (tests/arena.py) at 16 bytes
("conv_body_f32: pointers must be 16-byte aligned"; the bias is read one float at a time: 4 bytes), once under each fill.
Guards and inputs intact, nothing non-finite written, pad channels zero, the columns beyond still holding the fill,
bit-identical outputs under the two fills (no atomics: nothing is excused).  The kernels clamp y and res through buffer
resources of M * ldy * 4 and M * ldr * 4 bytes."""
import ctypes as C

import pytest
import torch

from footprint import DEV, P, ST, cl, judge, r4, repack, rnd, run
from test_gpu_kernels import make_bn, ref_conv

pytestmark = pytest.mark.gpu

F32 = torch.float32

CASES = [
    # id, N, C, Co, T, H, W, (kT, kH, kW), shape
    ("square_smallest", 1, 16, 64, 1, 19, 30, (3, 3, 3), 1),      # one chunk, T = 1: both outer temporal taps pruned
    ("tall_ragged", 1, 32, 48, 3, 17, 23, (3, 3, 3), 0),          # odd extents, 48 of 64 columns live, 2 chunks
    ("tstack_smallest", 1, 16, 100, 3, 6, 6, (7, 1, 1), 0),       # T < kT: most taps outside the clip; 100 of 128 columns
    ("tstack_ragged", 2, 32, 48, 11, 5, 5, (5, 1, 1), 0),         # a 3-frame last tile, 25 positions, 48 of 64 columns
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_conv_body(ptx, case):
    L = ptx._lib
    lib = L.lib()
    _, N, Ci, Co, T, H, W, (kT, kH, kW), shape = case
    x = rnd(N, Ci, T, H, W, seed=1)
    w = rnd(Co, Ci, kT, kH, kW, seed=2, scale=(2.0 / (Ci * kT * kH * kW)) ** 0.5)
    bn, res = make_bn(Co, 3), rnd(N, Co, T, H, W, seed=4)
    pad = (kT // 2, kH // 2, kW // 2)
    pd = L.PackDesc(Co, Ci, kT, kH, kW, r4(Ci), (Co + 127) // 128 * 128, 0)
    wp = torch.empty(lib.ptx_packed_weight_elems(C.byref(pd)), device=DEV)
    bp = torch.empty(pd.Co_pad, device=DEV)
    wd = w.contiguous().to(DEV)
    keep = [t.contiguous().to(DEV) for t in bn[:4]]
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), P(wd), None, *[P(t) for t in keep], C.c_float(bn[4]), P(wp), P(bp), ST()), "pack")
    xd, rd = cl(x), cl(res)
    c4 = r4(Co)
    ldy = c4 + 8
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, Ci, xd.shape[-1]
    d.To, d.Ho, d.Wo, d.Co, d.ldy = T, H, W, Co, ldy
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = kT, kH, kW, 1, 1, 1, *pad
    d.Kc, d.Co_pad = pd.Kc, pd.Co_pad
    d.flags = L.PTX_EPI_RELU | L.PTX_EPI_RES_ADD
    d.ldr = rd.shape[-1]
    assert lib.ptx_conv_body_f32_supported(C.byref(d), shape), lib.ptx_last_error()
    torch.cuda.synchronize()
    # the body-layout re-pack runs in the arena too; its output is the filter the kernel below reads
    wb = repack(lambda a, b: L.check(lib.ptx_pack_conv_body_f32_weight(C.byref(d), a, b, ST()), "pack body"), wp.cpu(),
                lib.ptx_conv_body_f32_weight_elems(C.byref(d)))
    want = ref_conv(x.double(), w.double(), (1, 1, 1), pad, bn=tuple(t.double() for t in bn[:4]) + (bn[4],), relu=True, res=res.double())

    def launch(v, ar):
        L.check(lib.ptx_conv_body_f32_fwd(C.byref(d), P(v["x"]), P(v["wb"]), P(v["bp"]), P(v["res"]), P(v["y"]), shape, ST()), "conv body")

    out = run([("x", xd, None, 16, "in"), ("wb", wb, None, 16, "in"), ("bp", bp.cpu(), None, 4, "in"), ("res", rd, None, 16, "in"),
               ("y", (N, T, H, W, ldy), F32, 16, "out")], launch)
    judge(out, "y", want.permute(0, 2, 3, 4, 1), 2e-4, (Ellipsis, slice(0, Co)), written=(Ellipsis, slice(0, c4)),
          zero=[(Ellipsis, slice(Co, c4))], untouched=[(Ellipsis, slice(c4, ldy))])


BODY_CHAIN = [
    # id, N, Cin, N1, N2, T, H, W, shape, residual
    ("ragged_tall_no_residual", 1, 32, 48, 100, 2, 17, 23, 0, False),      # 48 intermediate channels, 100 output columns
    ("square_residual", 2, 64, 64, 128, 2, 14, 14, 1, True),
]


@pytest.mark.parametrize("case", BODY_CHAIN, ids=[c[0] for c in BODY_CHAIN])
def test_conv_body_chain(ptx, case):
    """ptx_conv_body_chain_f32_fwd (conv3x3x3 -> ReLU -> conv1x1x1 (+ residual) -> ReLU in one launch) at the two smallest rows
    of test_conv_body_chain_f32, 2e-4 x scale (`close`) as there.  x, w_body, w_tail, res, y at 16 bytes ("conv_body_chain_f32:
    pointers must be 16-byte aligned"); bias and bias2 are read one float at a time: 4 bytes.  ldy = round_up(N2, 4) + 8."""
    L = ptx._lib
    lib = L.lib()
    _, N, Cin, N1, N2, T, H, W, shape, with_res = case
    x = rnd(N, Cin, T, H, W, seed=11)
    w1 = rnd(N1, Cin, 3, 3, 3, seed=12, scale=(2.0 / (Cin * 27)) ** 0.5)
    w2 = rnd(N2, N1, 1, 1, 1, seed=13, scale=(2.0 / N1) ** 0.5)
    bn1, bn2 = make_bn(N1, 14), make_bn(N2, 15)
    res = rnd(N, N2, T, H, W, seed=16) if with_res else None

    def pack(w, bn):
        Co, Ci, kT, kH, kW = w.shape
        pd = L.PackDesc(Co, Ci, kT, kH, kW, r4(Ci), (Co + 127) // 128 * 128, 0)
        wp = torch.empty(lib.ptx_packed_weight_elems(C.byref(pd)), device=DEV)
        bp = torch.empty(pd.Co_pad, device=DEV)
        ts = [t.contiguous().to(DEV) for t in bn[:4]]
        wd = w.contiguous().to(DEV)
        L.check(lib.ptx_pack_conv_weight(C.byref(pd), P(wd), None, *[P(t) for t in ts], C.c_float(bn[4]), P(wp), P(bp), ST()), "pack")
        torch.cuda.synchronize()
        return pd, wp, bp
    pd1, wp1, bp1 = pack(w1, bn1)
    pd2, wp2, bp2 = pack(w2, bn2)
    xd = cl(x)
    c4 = r4(N2)
    ldy = c4 + 8
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, Cin, xd.shape[-1]
    d.To, d.Ho, d.Wo, d.Co, d.ldy = T, H, W, N1, r4(N1)
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = 3, 3, 3, 1, 1, 1, 1, 1, 1
    d.Kc, d.Co_pad, d.flags = pd1.Kc, pd1.Co_pad, L.PTX_EPI_RELU
    t = L.ConvDesc()
    t.N, t.Ti, t.Hi, t.Wi, t.Ci, t.ldx = N, T, H, W, N1, r4(N1)
    t.To, t.Ho, t.Wo, t.Co, t.ldy = T, H, W, N2, ldy
    t.kT = t.kH = t.kW = t.sT = t.sH = t.sW = 1
    t.Kc, t.Co_pad = pd2.Kc, pd2.Co_pad
    t.flags = L.PTX_EPI_RELU | (L.PTX_EPI_RES_ADD if with_res else 0)
    rd = cl(res) if with_res else None
    t.ldr = rd.shape[-1] if with_res else 0
    assert lib.ptx_conv_body_chain_f32_supported(C.byref(d), C.byref(t), shape), lib.ptx_last_error()
    wb = repack(lambda a, b: L.check(lib.ptx_pack_conv_body_f32_weight(C.byref(d), a, b, ST()), "pack body"), wp1.cpu(),
                lib.ptx_conv_body_f32_weight_elems(C.byref(d)))
    wt = repack(lambda a, b: L.check(lib.ptx_pack_conv_body_tail_f32_weight(C.byref(t), a, b, ST()), "pack tail"), wp2.cpu(),
                lib.ptx_conv_body_tail_f32_weight_elems(C.byref(t)))
    dbl = lambda bn: tuple(v.double() for v in bn[:4]) + (bn[4],)                                  # noqa: E731
    mid = ref_conv(x.double(), w1.double(), (1, 1, 1), (1, 1, 1), bn=dbl(bn1), relu=True)
    want = ref_conv(mid, w2.double(), (1, 1, 1), (0, 0, 0), bn=dbl(bn2), relu=True, res=res.double() if with_res else None)
    specs = [("x", xd, None, 16, "in"), ("wb", wb, None, 16, "in"), ("bp1", bp1.cpu(), None, 4, "in"),
             ("wt", wt, None, 16, "in"), ("bp2", bp2.cpu(), None, 4, "in")]
    if with_res:
        specs.append(("res", rd, None, 16, "in"))
    specs.append(("y", (N, T, H, W, ldy), F32, 16, "out"))

    def launch(v, ar):
        L.check(lib.ptx_conv_body_chain_f32_fwd(C.byref(d), C.byref(t), P(v["x"]), P(v["wb"]), P(v["bp1"]), P(v["wt"]), P(v["bp2"]),
                                                P(v["res"]) if with_res else None, P(v["y"]), shape, ST()), "body chain")

    out = run(specs, launch)
    judge(out, "y", want.permute(0, 2, 3, 4, 1), 2e-4, (Ellipsis, slice(0, N2)), written=(Ellipsis, slice(0, c4)),
          zero=[(Ellipsis, slice(N2, c4))], untouched=[(Ellipsis, slice(c4, ldy))])
