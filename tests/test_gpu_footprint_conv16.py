"""Footprint tests of the 16-bit-operand tiles of the implicit GEMM (conv_igemm.hip: ".../f16" through ptx_conv3d_fwd, ".../bf16"
through ptx_conv3d_fused_fwd), every tile configuration that takes the case, split 1 and 3, at the smallest ragged cases of
their tests: tests/test_gpu_kernels.py::test_conv_f16_operands (1e-4 x scale against float64 on the half-rounded operands) and
tests/test_gpu_bf16.py::test_bf16_conv_kernel_parity (2^-8 |ref| + 2^-20 conv(|x|, |w|): one bf16 rounding of the fp32 sum).
Everything at 16 bytes ("conv3d: pointers must be 16-byte aligned", "conv3d: bias must be 16-byte aligned", and the
PTX_EPI_OUT_F16 / PTX_RES_F16 checks of make_conv_args), in a guarded arena (tests/arena.py), once under each fill: guards and
inputs intact, nothing non-finite written, pad channels zero, columns beyond the written width still holding the fill,
bit-identical outputs under the two fills (integer tile counters are the only atomics: nothing is excused)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from footprint import DEV, P, ST, cl, judge, r4, rnd, run
from test_gpu_bf16 import _pack_bf16

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16


def test_f16_operand_tiles(ptx):
    """(3, 9, 9, 40, 24), 1x1: Ci = 40 and Co = 24 ragged against every tile, M = 243; fp32 bias / output."""
    L, lib = ptx._lib, ptx._lib.lib()
    names = [lib.ptx_conv3d_config_name(i).decode() for i in range(lib.ptx_conv3d_num_configs())]
    cfgs = [i for i, n in enumerate(names) if n.endswith("/f16") and "/kwr/" not in n]
    N, H, W, Ci, Co = 3, 9, 9, 40, 24
    x = rnd(N, Ci, 1, H, W, seed=160).half().float()
    w = rnd(Co, Ci, 1, 1, 1, seed=161, scale=Ci ** -0.5).half().float()
    bias, res = rnd(Co, seed=162), rnd(N, Co, 1, H, W, seed=163)
    want = F.relu(F.conv3d(x.double(), w.double(), bias.double()) + res.double())
    ldh = (Ci + 7) // 8 * 8
    xh = torch.zeros(N, 1, H, W, ldh, dtype=F16)
    xh[..., :Ci] = x.permute(0, 2, 3, 4, 1).half()
    pd = L.PackDesc(Co, Ci, 1, 1, 1, ldh, (Co + 127) // 128 * 128, 0, 0, 0, 0, 0, 0, 1)
    wp = torch.empty(lib.ptx_packed_weight_elems(C.byref(pd)), device=DEV, dtype=F16)
    bp = torch.empty(pd.Co_pad, device=DEV)
    wd, bd = w.to(DEV), bias.to(DEV)
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), P(wd), P(bd), None, None, None, None, C.c_float(0), P(wp), P(bp), ST()), "pack f16")
    torch.cuda.synchronize()
    rd = cl(res)
    c4 = r4(Co)
    ldy = c4 + 8
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, 1, H, W, Ci // 2, ldh // 2
    d.To, d.Ho, d.Wo, d.Co, d.ldy = 1, H, W, Co, ldy
    d.kT = d.kH = d.kW = d.sT = d.sH = d.sW = 1
    d.Kc, d.Co_pad, d.groups = ldh // 2, pd.Co_pad, 1
    d.flags = L.PTX_F16_OPERANDS | L.PTX_EPI_RELU | L.PTX_EPI_RES_ADD
    d.ldr = rd.shape[-1]
    ran = 0
    for cfg, split in [(-1, 0)] + [(c, s) for c in cfgs for s in (1, 3)]:
        if cfg >= 0 and not lib.ptx_conv3d_config_supported(C.byref(d), cfg):
            continue
        ws_bytes = lib.ptx_conv3d_workspace_bytes(C.byref(d), split if split else 8)

        def launch(v, ar, cfg=cfg, split=split, ws_bytes=ws_bytes):
            L.check(lib.ptx_conv3d_fwd(C.byref(d), P(v["x"]), P(v["wp"]), P(v["bp"]), P(v["res"]), P(v["y"]), P(v["ws"]), ws_bytes, cfg, split,
                                       ST()), "conv f16 cfg %d" % cfg)

        out = run([("x", xh, None, 16, "in"), ("wp", wp.cpu(), None, 16, "in"), ("bp", bp.cpu(), None, 16, "in"), ("res", rd, None, 16, "in"),
                   ("y", (N, 1, H, W, ldy), F32, 16, "out"), ("ws", (max(ws_bytes // 4, 4),), F32, 16, "scratch")], launch)
        judge(out, "y", want.permute(0, 2, 3, 4, 1), 1e-4, (Ellipsis, slice(0, Co)), written=(Ellipsis, slice(0, c4)),
              zero=[(Ellipsis, slice(Co, c4))], untouched=[(Ellipsis, slice(c4, ldy))])
        ran += 1
    assert ran >= 7, ran


@pytest.mark.parametrize("name,Ci,Co,k,s,p,with_res", [("ragged_45", 45, 110, (1, 3, 3), (1, 2, 2), (0, 1, 1), False),
                                                      ("k3_s1_res", 64, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), True)])
def test_bf16_operand_tiles(ptx, name, Ci, Co, k, s, p, with_res):
    """Two rows of test_bf16_conv_kernel_parity at a smaller clip (1 x 3 x 10 x 12): odd Ci (the last channel pair half pad) and
    Co ragged against every tile; a 3x3x3 conv with a bf16 residual.  bf16 in, bf16 out, BN folded into the filter."""
    L, lib = ptx._lib, ptx._lib.lib()
    g = torch.Generator().manual_seed(7)
    N, T, H, W = 1, 3, 10, 12
    x = torch.randn(N, Ci, T, H, W, generator=g).to(BF16).float()
    w = (torch.randn(Co, Ci, *k, generator=g) * (2.0 / (Ci * k[0] * k[1] * k[2])) ** 0.5).to(BF16).float()
    bn = (torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.1, torch.randn(Co, generator=g) * 0.1,
          torch.rand(Co, generator=g) + 0.5)
    wp, bp, Kc, Co_pad, wf, bias = _pack_bf16(w, bn)
    ldx, c8 = (Ci + 7) // 8 * 8, (Co + 7) // 8 * 8
    ldy = c8 + 8
    xc = torch.zeros(N, T, H, W, ldx, dtype=BF16)
    xc[..., :Ci] = x.permute(0, 2, 3, 4, 1).to(BF16)
    To, Ho, Wo = [(e + 2 * pp - kk) // ss + 1 for e, pp, kk, ss in zip((T, H, W), p, k, s)]
    ref = F.conv3d(x.double(), wf, bias, s, p)
    absref = F.conv3d(x.double().abs(), wf.abs(), None, s, p)
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, (Ci + 1) // 2, ldx // 2
    d.To, d.Ho, d.Wo, d.Co, d.ldy = To, Ho, Wo, Co + Co % 2, ldy
    d.kT, d.kH, d.kW = k
    d.sT, d.sH, d.sW = s
    d.pT, d.pH, d.pW = p
    d.Kc, d.Co_pad, d.groups = Kc // 2, Co_pad, 1
    flags = L.PTX_F16_OPERANDS | L.PTX_BF16_OPERANDS | L.PTX_EPI_OUT_F16 | L.PTX_EPI_RELU
    specs = [("x", xc, None, 16, "in"), ("wp", wp.cpu(), None, 16, "in"), ("bp", bp.cpu(), None, 16, "in")]
    if with_res:
        r = torch.randn(N, Co, To, Ho, Wo, generator=g).to(BF16).float()
        rc = torch.zeros(N, To, Ho, Wo, c8, dtype=BF16)
        rc[..., :Co] = r.permute(0, 2, 3, 4, 1).to(BF16)
        flags |= L.PTX_EPI_RES_ADD | L.PTX_RES_F16
        d.ldr = c8
        ref, absref = ref + r.double(), absref + r.double().abs()
        specs.append(("res", rc, None, 16, "in"))
    ref = ref.clamp_min(0).permute(0, 2, 3, 4, 1)
    absref = absref.permute(0, 2, 3, 4, 1)
    d.flags = flags
    specs.append(("y", (N, To, Ho, Wo, ldy), BF16, 16, "out"))
    live = (Ellipsis, slice(0, Co))
    seen = 0
    for cfg in range(lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16()):
        if not lib.ptx_conv3d_config_name(cfg).decode().endswith("/bf16") or not lib.ptx_conv3d_config_supported(C.byref(d), cfg):
            continue
        for split in (1, 3):
            ws_bytes = lib.ptx_conv3d_workspace_bytes(C.byref(d), split)
            status = []

            def launch(v, ar, cfg=cfg, split=split, ws_bytes=ws_bytes, status=status):
                status.append(lib.ptx_conv3d_fused_fwd(C.byref(d), P(v["x"]), P(v["wp"]), P(v["bp"]), P(v["res"]) if with_res else None,
                                                       P(v["y"]), None, P(v["ws"]), ws_bytes, cfg, split, ST()))

            out = run(specs + [("ws", (max(ws_bytes // 4, 4),), F32, 16, "scratch", True)], launch)
            assert status[0] == status[1]
            if status[0] != 0:                     # (a tile that does not take this split: reported, nothing launched)
                continue
            for o in out:
                err = (o["y"][live].double() - ref).abs()
                assert bool((err <= 2.0 ** -8 * ref.abs() + 2.0 ** -20 * absref + 1e-30).all()), (cfg, split, float(err.max()))
            judge(out, "y", ref, None, live, written=(Ellipsis, slice(0, c8)), zero=[(Ellipsis, slice(Co, c8))],
                  untouched=[(Ellipsis, slice(c8, ldy))])
            seen += 1
    assert seen >= 4, "too few bf16 tiles ran %s" % name
