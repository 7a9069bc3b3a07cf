"""GPU parity tests of the Winograd F(4x4,3x3) execution of stride-1 (kT,3,3) fp32 convs (csrc/conv_wino_f32.hip): the full
path pack -> ptx_wino4_in_f32 -> 36-group ptx_conv3d_fwd -> ptx_wino4_out_f32 against F.conv3d + F.batch_norm + ReLU on the
CPU, partial tiles and padded pitches, the refusals, and two model runs with the F(4x4) launches forced."""
import ctypes as C

import pytest
import torch

from conftest import GOLDEN_CASES, golden_input, golden_recipe, load_golden
from test_gpu_kernels import DEV, _lib, _p, _r4, _st, close, from_cl, hip_conv, make_bn, ref_conv, rnd, to_cl
from test_gpu_wino import wino_desc

pytestmark = pytest.mark.gpu


def report(what, got, want):
    """Print the figure an assertion is about to judge (pytest -s shows it)."""
    scale = max(1.0, want.abs().max().item())
    print("%s: max err %.3e at scale %.3f = %.2e x scale" % (what, (got - want).abs().max().item(), scale,
                                                             (got - want).abs().max().item() / scale))


def hip_conv_wino4(ptx, x, w, bn, relu=True, res=None, reps=1, ldx=None, ldy=None):
    """x NCDHW cpu, w [Co,Ci,kT,3,3] cpu -> (NCDHW cpu output, the raw [N,T,H,W,ldy] device tensor) of the three launches.
    The filter goes through ptx_pack_conv_weight (BN fold), then ptx_pack_wino4_f32_weight."""
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
    assert lib.ptx_conv_wino4_f32_supported(C.byref(d)), lib.ptx_last_error()
    yd = torch.full((N, T, H, W, d.ldy), float("nan"), device=DEV)
    gd = L.ConvDesc()
    L.check(lib.ptx_conv_wino4_f32_gemm_desc(C.byref(d), C.byref(gd)), "gemm desc")
    assert (gd.groups, gd.kT, gd.kH, gd.kW, gd.Ci, gd.Co, gd.Kc) == (36, kT, 1, 1, 36 * _r4(Ci), 36 * _r4(Co), _r4(Ci))
    assert (gd.Hi, gd.Wi) == (-(-H // 4), -(-W // 4))
    u = torch.full((lib.ptx_wino4_f32_weight_elems(C.byref(d)),), float("nan"), device=DEV)
    L.check(lib.ptx_pack_wino4_f32_weight(C.byref(d), _p(wp), _p(u), _st()), "pack wino4")
    nbytes = lib.ptx_conv_wino4_f32_workspace_bytes(C.byref(d))
    v_bytes = (4 * gd.N * gd.Ti * gd.Hi * gd.Wi * gd.ldx + 255) // 256 * 256
    assert nbytes == v_bytes + 4 * gd.N * gd.To * gd.Ho * gd.Wo * gd.ldy
    arena = torch.full((nbytes // 4,), float("nan"), device=DEV)
    for _ in range(reps):
        L.check(lib.ptx_wino4_in_f32(C.byref(d), _p(xd), _p(arena), _st()), "wino4 in")
        L.check(lib.ptx_conv3d_fwd(C.byref(gd), _p(arena), _p(u), null, null, _p(arena, v_bytes // 4), null, 0, -1, 1, _st()), "wino4 gemm")
        L.check(lib.ptx_wino4_out_f32(C.byref(d), _p(arena, v_bytes // 4), _p(bp), _p(rd) if rd is not None else null, _p(yd), _st()),
                "wino4 out")
    torch.cuda.synchronize()
    return from_cl(yd, Co), yd


WINO4_SHAPES = [
    # N, Ci, Co, T, H, W, kT
    (2, 8, 12, 3, 4, 8, 3),            # ragged Co, 1 x 2 tiles per frame
    (1, 16, 64, 1, 2, 2, 3),           # one partial tile, T = 1: both outer temporal taps pruned
    (2, 12, 20, 2, 6, 10, 3),          # an overhang of 2 in both axes
    (1, 8, 8, 2, 7, 5, 1),             # odd extents, the (1,3,3) form
    (2, 128, 128, 4, 28, 28, 3),       # layer2 of config 2: 392 GEMM rows per group, crosses M-tile and column-tile boundaries
    (3, 256, 256, 2, 14, 14, 3),       # layer3: 14 padded to 16
]


@pytest.mark.parametrize("N,Ci,Co,T,H,W,kT", WINO4_SHAPES)
def test_conv_wino4_f32(ptx, N, Ci, Co, T, H, W, kT):
    """The three launches against F.conv3d + F.batch_norm + ReLU on the CPU, with and without the same-shape residual of a
    BasicBlock: the project's 2e-4 x scale bar, bit-equal across repeated launches, and 1e-4 x scale against the generic
    implicit-GEMM tile (F(4x4) in fp32 measures <= 1e-5 x scale against fp64 at these channel counts)."""
    x = rnd(N, Ci, T, H, W, seed=1)
    w = rnd(Co, Ci, kT, 3, 3, seed=2, scale=(2.0 / (Ci * 9 * kT)) ** 0.5)
    bn = make_bn(Co, 3)
    res = rnd(N, Co, T, H, W, seed=4)
    pre = ref_conv(x, w, (1, 1, 1), (kT // 2, 1, 1), bn=bn)           # the CPU reference, computed once
    got, _ = hip_conv_wino4(ptx, x, w, bn)
    report("wino4 vs cpu", got, torch.relu(pre))
    close(got, torch.relu(pre))
    got, _ = hip_conv_wino4(ptx, x, w, bn, res=res)
    report("wino4 + res vs cpu", got, torch.relu(pre + res))
    close(got, torch.relu(pre + res))
    again, _ = hip_conv_wino4(ptx, x, w, bn, res=res, reps=2)
    assert torch.equal(got, again)
    tile = hip_conv(ptx, x, w, (1, 1, 1), (kT // 2, 1, 1), bn=bn, relu=True, res=res)
    report("wino4 vs generic tile", got, tile)
    close(got, tile, tol=1e-4)


def test_conv_wino4_f32_padded_pitch_and_channel_slice(ptx):
    """ldx > round_up(Ci, 4) with foreign data past the conv's channels, ldy > round_up(Co, 4), partial tiles in both axes:
    columns [Co, round_up(Co, 4)) are written as zero, the columns beyond keep what they held."""
    N, Ci, Co, T, H, W, kT = 2, 10, 18, 3, 6, 5, 3
    x = rnd(N, Ci, T, H, W, seed=1)
    w = rnd(Co, Ci, kT, 3, 3, seed=2, scale=(2.0 / (Ci * 9 * kT)) ** 0.5)
    bn = make_bn(Co, 3)
    got, yd = hip_conv_wino4(ptx, x, w, bn, ldx=20, ldy=28)
    close(got, ref_conv(x, w, (1, 1, 1), (kT // 2, 1, 1), bn=bn, relu=True))
    assert bool((yd[..., Co:_r4(Co)] == 0).all()) and bool(torch.isnan(yd[..., _r4(Co):]).all())


def test_conv_wino4_f32_refusals(ptx):
    L, lib = ptx._lib, _lib(ptx)

    def ok(edit=None, **kw):
        a = dict(N=2, Ci=16, Co=16, T=4, H=8, W=8, kT=3)
        a.update(kw)
        d = wino_desc(L, **a)
        if edit is not None:
            edit(d)
        return bool(lib.ptx_conv_wino4_f32_supported(C.byref(d)))

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

    assert ok() and ok(kT=1) and ok(H=7) and ok(W=9)
    assert not ok(stride2) and not ok(pad0) and not ok(k1) and not ok(pad_a)
    assert not ok(lambda d: setattr(d, "groups", 2))
    assert not ok(lambda d: setattr(d, "flags", L.PTX_F16X3_OPERANDS))
    # V of one launch: frames x 128 x 128 tiles x 36 x 128 floats = frames x 288 MiB -- 7 frames fit, 8 do not
    assert ok(N=1, Ci=128, Co=16, T=7, H=512, W=512) and not ok(N=1, Ci=128, Co=16, T=8, H=512, W=512)
    assert b"2 GiB" in lib.ptx_last_error()
    d = wino_desc(L, 1, 128, 16, 8, 512, 512, 3)
    assert lib.ptx_conv_wino4_f32_workspace_bytes(C.byref(d)) == 0 and lib.ptx_wino4_f32_weight_elems(C.byref(d)) == 0
    # refused before any launch: the pointers below are never dereferenced
    assert lib.ptx_wino4_in_f32(C.byref(d), C.c_void_p(16), C.c_void_p(16), _st()) == 2
    assert lib.ptx_wino4_out_f32(C.byref(d), C.c_void_p(16), None, None, C.c_void_p(16), _st()) == 2
    assert lib.ptx_pack_wino4_f32_weight(C.byref(d), C.c_void_p(16), C.c_void_p(16), _st()) == 2
    d = wino_desc(L, 2, 16, 16, 4, 8, 8, 3)
    assert lib.ptx_wino4_in_f32(C.byref(d), C.c_void_p(16), C.c_void_p(8), _st()) == 1          # misaligned V: PTX_ERR_INVALID
    assert lib.ptx_wino4_in_f32(C.byref(d), None, C.c_void_p(16), _st()) == 1
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["resnet3d18_small", "resnet3d50_small"])
def test_engine_runs_wino4_steps(ptx, monkeypatch, case):
    """A golden model with the F(4x4) launches forced (PTX_CONV_WINO=4) against the golden at the model tests' plain 1e-3 bar
    with argmax equality, and against the same model with the Winograd forms compiled out (PTX_CONV_WINO=0) within 3e-5 of
    the logits' scale; the F(4x4) steps must actually be what ran."""
    from pretorched_x_amd.testing import synth_state_dict
    arch, kw = GOLDEN_CASES[case]
    blob = load_golden(case)
    x = golden_input(blob).to(DEV)
    ref = torch.from_numpy(blob["logits"])
    outs = {}
    for mode in ("4", "0"):
        monkeypatch.setenv("PTX_CONV_WINO", mode)
        model = ptx.__dict__[arch](**kw)
        model.load_state_dict(synth_state_dict(model.state_dict(), **golden_recipe(blob)))
        model = model.to(DEV).eval()
        outs[mode] = model(x).cpu()
        torch.cuda.synchronize()
        plan = list(model.engine()._plans.values())[-1]
        if mode == "4":
            assert plan.wino4_steps and all(w.use_wino4 and not w.use_wino and w.need_u4 is None for w in plan.wino4_steps)
            assert all(len(w.active()) == 3 and w.active()[1] is w.gemm4 and w.gemm4.d.groups == 36 for w in plan.wino4_steps)
            ran = [t for t in plan.all_convs() if getattr(t, "label", "").endswith(".wino4_gemm")]
            assert len(ran) == len(plan.wino4_steps)                   # every one of them is on the forward's launch list
            # ... and a forward writes the arena through them: V and M of the last step, whole
            last = plan.wino4_steps[-1]
            plan.wino_arena.fill_(float("nan"))
            again = model(x).cpu()
            torch.cuda.synchronize()
            g = last.gemm4.d
            n_m = g.N * g.To * g.Ho * g.Wo * g.ldy
            assert bool(torch.isfinite(plan.wino_arena[:g.N * g.Ti * g.Hi * g.Wi * g.ldx]).all())
            assert bool(torch.isfinite(plan.wino_arena[last.v4_bytes // 4:last.v4_bytes // 4 + n_m]).all())
            assert torch.equal(again, outs[mode])
        else:
            assert not plan.wino_steps and not plan.wino4_steps
    scale = max(1.0, ref.abs().max().item())
    err = (outs["4"] - ref).abs().max().item()
    print("%s: forced F(4x4) vs golden %.3e, vs PTX_CONV_WINO=0 %.3e, scale %.3f" % (
        case, err, (outs["4"] - outs["0"]).abs().max().item(), scale))
    assert err <= 1e-3, "forced F(4x4) vs golden: max abs err %.3e" % err
    assert torch.equal(outs["4"].argmax(1), ref.argmax(1))
    assert (outs["4"] - outs["0"]).abs().max().item() <= 3e-5 * scale
