"""Footprint tests of the chained convolution (ptx_conv3d_chain_fwd, conv_chain.hip: conv -> ReLU -> 1x1x1 conv (+ residual)
-> ReLU in one launch, the intermediate tile in LDS) on EVERY chained tile that takes the case, fp32 and split operands,
at the smallest and the ragged rows of test_gpu_kernels.py::CHAIN_CASES with that test's 2e-5 x scale (`close`).  x, both
packed filters, bias2, the residual and y (ldy = round_up(Co2, 4) + 8) sit in a guarded arena (tests/arena.py) at 16 bytes
("conv3d_chain: pointers must be 16-byte aligned", "conv3d_chain: bias2 must be 16-byte aligned"); the first conv's bias is
read one float at a time and sits at 4 bytes.  Once under each fill: guards and inputs intact, nothing non-finite written, pad
channels zero, the columns beyond still holding the fill, bit-identical outputs under the two fills (no atomics: nothing
is excused).  The kernels clamp y and res through buffer resources of M * ldy * 4 and M * ldr * 4 bytes."""
import ctypes as C

import pytest
import torch

from footprint import P, ST, cl, judge, r4, rnd, run
from test_gpu_kernels import CHAIN_CASES, _pack_plain, make_bn, ref_conv

pytestmark = pytest.mark.gpu

F32 = torch.float32
ROWS = [c for c in CHAIN_CASES if c[0].startswith(("narrow mid", "(2+1)D pointwise pair", "(1,3,3) conv"))]


def _dbl(bn):
    return tuple(t.double() for t in bn[:4]) + (bn[4],)


@pytest.mark.parametrize("kind", ["fp32", "x3"])
@pytest.mark.parametrize("case", ROWS, ids=["narrow_mid_64_32_64", "pair_64_51_256_res", "k133_144_100_36_ragged"])
def test_conv_chain(ptx, case, kind):
    x3 = kind == "x3"
    L = ptx._lib
    lib = L.lib()
    _, N, T, H, W, Ci, N1, Co2, k, s_, p_, relu1, relu2, with_res = case
    x = rnd(N, Ci, T, H, W, seed=400 + Ci)
    w1 = rnd(N1, Ci, *k, seed=401, scale=(Ci * k[0] * k[1] * k[2]) ** -0.5)
    w2 = rnd(Co2, N1, 1, 1, 1, seed=402, scale=N1 ** -0.5)
    bn1, bn2 = make_bn(N1, 403), make_bn(Co2, 404)
    mid = ref_conv(x.double(), w1.double(), s_, p_, bn=_dbl(bn1), relu=relu1)
    To, Ho, Wo = mid.shape[2:]
    res = rnd(N, Co2, To, Ho, Wo, seed=405) if with_res else None
    want = ref_conv(mid, w2.double(), (1, 1, 1), (0, 0, 0), bn=_dbl(bn2), relu=relu2, res=res.double() if with_res else None)
    pd1, wp1, bp1 = _pack_plain(ptx, w1, bn1, x3=x3)
    pd2, wp2, bp2 = _pack_plain(ptx, w2, bn2, x3=x3)
    fx3 = L.PTX_F16X3_OPERANDS if x3 else 0
    xd = cl(x, pd1.Kc)
    rd = cl(res) if with_res else None
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, Ci, xd.shape[-1]
    d.To, d.Ho, d.Wo, d.Co, d.ldy = To, Ho, Wo, N1, r4(N1)
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = k[0], k[1], k[2], s_[0], s_[1], s_[2], p_[0], p_[1], p_[2]
    d.Kc, d.Co_pad, d.flags = pd1.Kc, pd1.Co_pad, (L.PTX_EPI_RELU if relu1 else 0) | fx3
    c4 = r4(Co2)
    ldy = c4 + 8
    d2 = L.ConvDesc()
    d2.N, d2.Ti, d2.Hi, d2.Wi, d2.Ci, d2.ldx = N, To, Ho, Wo, N1, r4(N1)
    d2.To, d2.Ho, d2.Wo, d2.Co, d2.ldy = To, Ho, Wo, Co2, ldy
    d2.kT = d2.kH = d2.kW = d2.sT = d2.sH = d2.sW = 1
    d2.Kc, d2.Co_pad = pd2.Kc, pd2.Co_pad
    d2.flags = (L.PTX_EPI_RELU if relu2 else 0) | (L.PTX_EPI_RES_ADD if with_res else 0) | fx3
    d2.ldr = rd.shape[-1] if with_res else 0
    specs = [("x", xd, None, 16, "in"), ("wp1", wp1.cpu(), None, 16, "in"), ("bp1", bp1.cpu(), None, 4, "in"),
             ("wp2", wp2.cpu(), None, 16, "in"), ("bp2", bp2.cpu(), None, 16, "in")]
    if with_res:
        specs.append(("res", rd, None, 16, "in"))
    specs.append(("y", (N, To, Ho, Wo, ldy), F32, 16, "out"))
    cfgs = [c for c in range(lib.ptx_conv3d_chain_num_configs()) if lib.ptx_conv3d_chain_supported(C.byref(d), C.byref(d2), c)]
    assert cfgs, "no chained tile takes %s" % (case[0],)
    for cfg in cfgs + [-1]:
        def launch(v, ar, cfg=cfg):
            L.check(lib.ptx_conv3d_chain_fwd(C.byref(d), C.byref(d2), P(v["x"]), P(v["wp1"]), P(v["bp1"]), P(v["wp2"]), P(v["bp2"]),
                                             P(v["res"]) if with_res else None, P(v["y"]), cfg, ST()), "chain cfg %d" % cfg)

        out = run(specs, launch)
        judge(out, "y", want.permute(0, 2, 3, 4, 1), 2e-5, (Ellipsis, slice(0, Co2)), written=(Ellipsis, slice(0, c4)),
              zero=[(Ellipsis, slice(Co2, c4))], untouched=[(Ellipsis, slice(c4, ldy))])
