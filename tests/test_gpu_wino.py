"""GPU parity tests of the Winograd F(2x2,3x3) execution of stride-1 (kT,3,3) fp32 convs (csrc/conv_wino_f32.hip): the full
path pack -> ptx_wino_in_f32 -> grouped ptx_conv3d_fwd -> ptx_wino_out_f32 against F.conv3d + F.batch_norm + ReLU on the CPU,
the refusals of ptx_conv_wino_f32_supported, and one model run with the Winograd launches forced."""
import ctypes as C

import pytest
import torch

from conftest import GOLDEN_CASES, golden_input, golden_recipe, load_golden
from test_gpu_kernels import DEV, _lib, _p, _r4, _st, close, from_cl, hip_conv, make_bn, ref_conv, rnd, to_cl

pytestmark = pytest.mark.gpu


def wino_desc(L, N, Ci, Co, T, H, W, kT, ldx=None, ldy=None, relu=True, res_ld=0):
    """The DIRECT conv's descriptor, as the Winograd entry points take it."""
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, Ci, _r4(Ci) if ldx is None else ldx
    d.To, d.Ho, d.Wo, d.Co, d.ldy = T, H, W, Co, _r4(Co) if ldy is None else ldy
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = kT, 3, 3, 1, 1, 1, kT // 2, 1, 1
    d.Kc, d.Co_pad = _r4(Ci), (Co + 127) // 128 * 128
    d.flags = (L.PTX_EPI_RELU if relu else 0) | (L.PTX_EPI_RES_ADD if res_ld else 0)
    d.ldr = res_ld
    return d


def hip_conv_wino(ptx, x, w, bn, relu=True, res=None, reps=1, ldx=None, ldy=None):
    """x NCDHW cpu, w [Co,Ci,kT,3,3] cpu -> (NCDHW cpu output, the raw [N,T,H,W,ldy] device tensor) of the three launches.
    The filter goes through ptx_pack_conv_weight (BN fold), then ptx_pack_wino_f32_weight."""
    L, lib = ptx._lib, _lib(ptx)
    Co, Ci, kT = w.shape[:3]
    N, _, T, H, W = x.shape
    pd = L.PackDesc(Co, Ci, kT, 3, 3, _r4(Ci), (Co + 127) // 128 * 128, 0)
    wp = torch.empty(lib.ptx_packed_weight_elems(C.byref(pd)), device=DEV)
    bp = torch.empty(pd.Co_pad, device=DEV)
    wd = w.contiguous().to(DEV)
    null = C.c_void_p(0)
    keep = [t.contiguous().to(DEV) for t in bn[:4]]
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), _p(wd), null, *[_p(t) for t in keep], C.c_float(bn[4]), _p(wp), _p(bp), _st()), "pack")
    xd = to_cl(x, ldx)
    if ldx is not None:
        xd[..., Ci:] = 7.0          # a padded pitch may hold anything past the conv's own channels
    rd = to_cl(res) if res is not None else None
    d = wino_desc(L, N, Ci, Co, T, H, W, kT, xd.shape[-1], ldy, relu, rd.shape[-1] if rd is not None else 0)
    assert lib.ptx_conv_wino_f32_supported(C.byref(d)), lib.ptx_last_error()
    yd = torch.full((N, T, H, W, d.ldy), float("nan"), device=DEV)
    gd = L.ConvDesc()
    L.check(lib.ptx_conv_wino_f32_gemm_desc(C.byref(d), C.byref(gd)), "gemm desc")
    assert (gd.groups, gd.kT, gd.kH, gd.kW, gd.Ci, gd.Co, gd.Kc) == (16, kT, 1, 1, 16 * _r4(Ci), 16 * _r4(Co), _r4(Ci))
    u = torch.full((lib.ptx_wino_f32_weight_elems(C.byref(d)),), float("nan"), device=DEV)
    L.check(lib.ptx_pack_wino_f32_weight(C.byref(d), _p(wp), _p(u), _st()), "pack wino")
    nbytes = lib.ptx_conv_wino_f32_workspace_bytes(C.byref(d))
    v_bytes = (4 * gd.N * gd.Ti * gd.Hi * gd.Wi * gd.ldx + 255) // 256 * 256
    assert nbytes == v_bytes + 4 * gd.N * gd.To * gd.Ho * gd.Wo * gd.ldy
    arena = torch.full((nbytes // 4,), float("nan"), device=DEV)
    for _ in range(reps):
        L.check(lib.ptx_wino_in_f32(C.byref(d), _p(xd), _p(arena), _st()), "wino in")
        L.check(lib.ptx_conv3d_fwd(C.byref(gd), _p(arena), _p(u), null, null, _p(arena, v_bytes // 4), null, 0, -1, 1, _st()), "wino gemm")
        L.check(lib.ptx_wino_out_f32(C.byref(d), _p(arena, v_bytes // 4), _p(bp), _p(rd) if rd is not None else null, _p(yd), _st()),
                "wino out")
    torch.cuda.synchronize()
    return from_cl(yd, Co), yd


WINO_SHAPES = [
    # N, Ci, Co, T, H, W, kT
    (2, 8, 12, 3, 4, 6, 3),            # ragged Co inside one column tile, all three temporal taps, 2 x 3 tiles per frame
    (1, 16, 64, 1, 2, 2, 3),           # one tile per frame, every patch mostly halo, T = 1: both outer temporal taps pruned
    (1, 12, 20, 5, 6, 2, 3),           # W = 2 (one tile column), Ci and Co no multiples of 8
    (2, 64, 64, 2, 14, 14, 1),         # the (1,3,3) form
    (2, 128, 128, 4, 28, 28, 3),       # layer2 of config 2: crosses M-tile and column-tile boundaries
    (3, 256, 256, 2, 14, 14, 3),       # layer3
]


@pytest.mark.parametrize("N,Ci,Co,T,H,W,kT", WINO_SHAPES)
def test_conv_wino_f32(ptx, N, Ci, Co, T, H, W, kT):
    """The three launches against F.conv3d + F.batch_norm + ReLU on the CPU (resnet3D.py:129-131), with and without the
    same-shape residual of a BasicBlock (resnet3D.py:101-104): the project's 2e-4 x scale bar, bit-equal across repeated
    launches, and 2e-5 against the generic implicit-GEMM tile -- the two bars of test_conv_body_f32."""
    x = rnd(N, Ci, T, H, W, seed=1)
    w = rnd(Co, Ci, kT, 3, 3, seed=2, scale=(2.0 / (Ci * 9 * kT)) ** 0.5)
    bn = make_bn(Co, 3)
    res = rnd(N, Co, T, H, W, seed=4)
    pre = ref_conv(x, w, (1, 1, 1), (kT // 2, 1, 1), bn=bn)           # the CPU reference, computed once
    got, _ = hip_conv_wino(ptx, x, w, bn)
    close(got, torch.relu(pre))
    got, _ = hip_conv_wino(ptx, x, w, bn, res=res)
    close(got, torch.relu(pre + res))
    again, _ = hip_conv_wino(ptx, x, w, bn, res=res, reps=2)
    assert torch.equal(got, again)
    close(got, hip_conv(ptx, x, w, (1, 1, 1), (kT // 2, 1, 1), bn=bn, relu=True, res=res), tol=2e-5)


def test_conv_wino_f32_padded_pitch_and_channel_slice(ptx):
    """ldx > round_up(Ci, 4) with foreign data past the conv's channels, ldy > round_up(Co, 4): the output is a channel slice
    of a wider row -- columns [Co, round_up(Co, 4)) are written as zero, the columns beyond keep what they held."""
    N, Ci, Co, T, H, W, kT = 2, 10, 18, 3, 6, 4, 3
    x = rnd(N, Ci, T, H, W, seed=1)
    w = rnd(Co, Ci, kT, 3, 3, seed=2, scale=(2.0 / (Ci * 9 * kT)) ** 0.5)
    bn = make_bn(Co, 3)
    got, yd = hip_conv_wino(ptx, x, w, bn, ldx=20, ldy=28)
    close(got, ref_conv(x, w, (1, 1, 1), (kT // 2, 1, 1), bn=bn, relu=True))
    assert bool((yd[..., Co:_r4(Co)] == 0).all()) and bool(torch.isnan(yd[..., _r4(Co):]).all())


def test_conv_wino_f32_refusals(ptx):
    L, lib = ptx._lib, _lib(ptx)

    def ok(edit=None, **kw):
        a = dict(N=2, Ci=16, Co=16, T=4, H=8, W=8, kT=3)
        a.update(kw)
        d = wino_desc(L, **a)
        if edit is not None:
            edit(d)
        return bool(lib.ptx_conv_wino_f32_supported(C.byref(d)))

    def stride2(d):
        d.sH = d.sW = 2
        d.Ho, d.Wo = 4, 4

    def pad0(d):
        d.pH = d.pW = 0
        d.Ho, d.Wo = 6, 6

    def k1(d):
        d.kH, d.pH = 1, 0

    def pad_a(d):
        d.flags |= L.PTX_EPI_RES_PADA

    assert ok() and ok(kT=1)
    assert not ok(H=7) and not ok(W=9)
    assert not ok(stride2) and not ok(pad0) and not ok(k1) and not ok(pad_a)
    assert not ok(lambda d: setattr(d, "groups", 2))
    assert not ok(lambda d: setattr(d, "flags", L.PTX_F16X3_OPERANDS))
    # V of one launch: frames x 256 x 256 tiles x 16 x 128 floats = frames x 512 MiB -- 3 frames fit, 4 are exactly 2 GiB
    assert ok(N=1, Ci=128, Co=16, T=3, H=512, W=512) and not ok(N=1, Ci=128, Co=16, T=4, H=512, W=512)
    assert b"2 GiB" in lib.ptx_last_error()
    d = wino_desc(L, 1, 128, 16, 4, 512, 512, 3)
    assert lib.ptx_conv_wino_f32_workspace_bytes(C.byref(d)) == 0 and lib.ptx_wino_f32_weight_elems(C.byref(d)) == 0
    assert lib.ptx_wino_in_f32(C.byref(d), C.c_void_p(16), C.c_void_p(16), _st()) == 2          # refused before any launch


def test_engine_runs_winograd_steps(ptx, monkeypatch):
    """resnet3d18_small with the Winograd launches forced (PTX_CONV_WINO=1) against the golden at the model tests' plain 1e-3
    bar with argmax equality, and against the same model with them compiled out (PTX_CONV_WINO=0) within 3e-5 of the logits'
    scale."""
    from pretorched_x_amd.steps import WinoStep
    from pretorched_x_amd.testing import synth_state_dict
    case = "resnet3d18_small"
    arch, kw = GOLDEN_CASES[case]
    blob = load_golden(case)
    x = golden_input(blob).to(DEV)
    ref = torch.from_numpy(blob["logits"])
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("PTX_CONV_WINO", mode)
        model = ptx.__dict__[arch](**kw)
        model.load_state_dict(synth_state_dict(model.state_dict(), **golden_recipe(blob)))
        model = model.to(DEV).eval()
        outs[mode] = model(x).cpu()
        torch.cuda.synchronize()
        plan = list(model.engine()._plans.values())[-1]
        wino = [s for s in plan.wino_steps if s.use_wino]
        if mode == "1":
            assert wino and all(len(s.active()) == 3 and s.active()[1] is s.gemm for s in wino)
            assert any(isinstance(s, WinoStep) for s in plan.steps) or any(isinstance(p, WinoStep) for a in plan.alt_steps for p in a.pair)
        else:
            assert not plan.wino_steps
    err = (outs["1"] - ref).abs().max().item()
    assert err <= 1e-3, "forced Winograd vs golden: max abs err %.3e" % err
    assert torch.equal(outs["1"].argmax(1), ref.argmax(1))
    assert (outs["1"] - outs["0"]).abs().max().item() <= 3e-5 * max(1.0, ref.abs().max().item())
