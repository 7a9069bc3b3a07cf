"""Host-side tests of the Winograd F(2x2,3x3) execution (no GPU): the eligibility rule, the "wino:" entries of the tuned table,
the plan compiler's Winograd steps on a dry plan, and the three-step decomposition restated in torch."""
import ctypes as C
import json

import pytest
import torch
import torch.nn.functional as F


def _desc(L, N=2, Ci=16, Co=16, T=4, H=8, W=8, kT=3, flags=1):
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, Ci, (Ci + 3) // 4 * 4
    d.To, d.Ho, d.Wo, d.Co, d.ldy = T, H, W, Co, (Co + 3) // 4 * 4
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = kT, 3, 3, 1, 1, 1, kT // 2, 1, 1
    d.Kc, d.Co_pad, d.flags = d.ldx, (Co + 127) // 128 * 128, flags
    return d


def test_eligibility_rule(ptx):
    L, lib = ptx._lib, ptx._lib.lib()

    def ok(**edits):
        shape = {k: edits.pop(k) for k in list(edits) if k in ("N", "Ci", "Co", "T", "H", "W", "kT", "flags")}
        d = _desc(L, **shape)
        for k, v in edits.items():
            setattr(d, k, v)
        return bool(lib.ptx_conv_wino_f32_supported(C.byref(d)))

    assert ok() and ok(kT=1) and ok(Ci=10, Co=18) and ok(flags=L.PTX_EPI_RELU | L.PTX_EPI_RES_ADD, ldr=16)
    assert not ok(H=7) and not ok(W=6 + 1)
    assert not ok(sH=2, sW=2, Ho=4, Wo=4) and not ok(sT=2, To=2)
    assert not ok(pH=0, pW=0, Ho=6, Wo=6) and not ok(pT=0, To=2)
    assert not ok(groups=2) and not ok(kH=1, pH=0) and not ok(kT=5, pT=2)
    for flag in (L.PTX_EPI_RES_PADA, L.PTX_F16X3_OPERANDS, L.PTX_F16_OPERANDS, L.PTX_F16_OPERANDS | L.PTX_BF16_OPERANDS):
        assert not ok(flags=flag)
    assert not ok(flags=L.PTX_EPI_RES_ADD, ldr=8)                        # a residual row shorter than Co
    # every operand of one launch below 2 GiB: V = frames x 256 x 256 tiles x 16 x 128 floats = frames x 512 MiB
    assert ok(N=1, Ci=128, T=3, H=512, W=512) and not ok(N=1, Ci=128, T=4, H=512, W=512)
    assert b"2 GiB" in lib.ptx_last_error()
    # the grouped descriptor and the sizes that go with it
    d, g = _desc(L, N=8, Ci=128, Co=128, T=4, H=28, W=28), L.ConvDesc()
    assert lib.ptx_conv_wino_f32_gemm_desc(C.byref(d), C.byref(g)) == 0
    assert (g.N, g.Ti, g.Hi, g.Wi, g.To, g.Ho, g.Wo) == (8, 4, 14, 14, 4, 14, 14)
    assert (g.Ci, g.ldx, g.Co, g.ldy, g.Kc, g.Co_pad, g.groups, g.flags) == (2048, 2048, 2048, 2048, 128, 2048, 16, 0)
    assert (g.kT, g.kH, g.kW, g.pT, g.pH, g.pW, g.sT, g.sH, g.sW) == (3, 1, 1, 1, 0, 0, 1, 1, 1)
    tiles = 8 * 4 * 14 * 14
    assert lib.ptx_conv_wino_f32_workspace_bytes(C.byref(d)) == 2 * tiles * 2048 * 4
    assert lib.ptx_wino_f32_weight_elems(C.byref(d)) == 3 * 2048 * 128
    assert any(lib.ptx_conv3d_config_supported(C.byref(g), i) for i in range(lib.ptx_conv3d_num_configs()))


def test_wino_keys_round_trip(ptx, tmp_path):
    from pretorched_x_amd import tuned
    lib = ptx._lib.lib()
    keep = tuned.tuned_snapshot()
    try:
        key = json.dumps(_desc(ptx._lib, N=8).key())
        assert tuned.wino_lookup(key) is None
        name = lib.ptx_conv3d_config_name(0).decode()
        tuned.wino_store(key, True, 0)
        tuned.wino_store("chain:" + key, False, 0)
        assert tuned.wino_lookup(key) is True and tuned.wino_lookup("chain:" + key) is False
        path = str(tmp_path / "table.json")
        tuned.save_tuned_table(path)
        saved = json.load(open(path))
        assert saved["wino:" + key] == [name, 1] and saved["wino:chain:" + key] == [name, 2]
        tuned.tuned_replace(saved)
        assert tuned.wino_lookup(key) is True and tuned.wino_lookup("chain:" + key) is False
        # a verdict measured for 8 clips says nothing about 4
        assert tuned.wino_lookup(json.dumps(_desc(ptx._lib, N=4).key())) is None
    finally:
        tuned.tuned_replace(keep)


def test_dry_plan_compiles_winograd_steps(ptx, monkeypatch):
    """Config 2: layer1..3 hold the eligible stride-1 3x3x3 convs (layer4's 7 x 7 frames are odd, the stride-2 convs and the
    stem are not Winograd problems); without a verdict every one of them runs its direct execution."""
    from pretorched_x_amd import tuned
    from pretorched_x_amd.steps import ConvStep, WinoStep
    keep = tuned.tuned_snapshot()
    try:
        tuned.tuned_replace({k: v for k, v in keep.items() if not k.startswith("wino:")})
        m = ptx.resnet3d50(num_classes=339, pretrained=None)
        plan = m.engine().dry_plan(m, (8, 3, 16, 224, 224))
        labels = [w.label for w in plan.wino_steps]
        assert labels == ["layer1.%d.conv2" % i for i in range(3)] + ["layer2.%d.conv2" % i for i in (1, 2, 3)] + \
            ["layer3.%d.conv2" % i for i in (1, 2, 3, 4, 5)]
        assert not any(w.use_wino for w in plan.wino_steps)
        n_convs = len(plan.all_convs())
        for w in plan.wino_steps:
            assert len(w.direct) == 1 and isinstance(w.direct[0], ConvStep) and w.direct[0] in plan.conv_steps
            assert w.gemm not in plan.conv_steps and w.gemm.d.groups == 16 and w.gemm.split == 1 and w.gemm.macs == w.direct[0].macs
            assert [getattr(s, "label", None) for s in w.wino] == ["wino_in", w.label + ".wino_gemm", "wino_out"]
            assert w.wino[0].hbm_bytes > 0 and w.wino[2].hbm_bytes > 0 and w.arena_bytes <= plan.wino_bytes
            # inside a bottleneck tail the verdict is the pair's: keyed by the chain, and the AltStep is known
            assert (w.alt is not None) == w.key.startswith("chain:") and (w.alt is None or w.alt.pair[0] is w)
            assert w.gemm.issued_flop() < 2.0 * w.direct[0].macs            # fewer multiplies issued than direct convolution
        assert sum(w.alt is not None for w in plan.wino_steps) == 5 and sum(isinstance(s, WinoStep) for s in plan.steps) == 6
        # a stored verdict switches the step at compile time -- and the pair it opens away from the chained launch
        for w in plan.wino_steps[1:4]:
            tuned.wino_store(w.key, True, w.gemm.cfg)
        plan2 = m.engine().dry_plan(m, (8, 3, 16, 224, 224))
        assert [w.use_wino for w in plan2.wino_steps] == [False] + [True] * 5 + [False] * 5      # identical problems share a key
        assert not plan2.wino_steps[1].alt.use_chain and plan2.wino_steps[0].alt is None
        assert len(plan2.all_convs()) == n_convs + 2       # layer1.{1,2}: the chained launch became conv2 (Winograd) + conv3
        assert abs(sum(s.macs for s in plan2.all_convs()) - sum(s.macs for s in plan.all_convs())) < 1
        # PTX_CONV_WINO=0 compiles no Winograd step; =1 runs every one of them
        monkeypatch.setenv("PTX_CONV_WINO", "0")
        assert not m.engine().dry_plan(m, (8, 3, 16, 224, 224)).wino_steps
        monkeypatch.setenv("PTX_CONV_WINO", "1")
        plan1 = m.engine().dry_plan(m, (8, 3, 16, 224, 224))
        assert len(plan1.wino_steps) == 11 and all(w.use_wino for w in plan1.wino_steps)
        assert not any(a.use_chain for a in plan1.alt_steps)
    finally:
        tuned.tuned_replace(keep)


Bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float32)
G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float32)
At = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float32)


def wino_torch(x, w, b):
    """The three steps in the layout the kernels use: V [N, 16 Cg, T, H/2, W/2] with transform position xi = 4 a + b major
    over channels, a 16-group (kT,1,1) conv with the filter rows U[xi][co], and the output transform + bias."""
    N, Ci, T, H, W = x.shape
    Co, _, kT = w.shape[:3]
    U = torch.einsum("ai,octij,bj->abotc", G, w, G)                                      # 4,4,Co,kT,Ci
    d = F.pad(x, (1, 1, 1, 1)).unfold(3, 4, 2).unfold(4, 4, 2)                           # N,Ci,T,H/2,W/2,4,4
    V = torch.einsum("ai,ncthwij,bj->nabcthw", Bt, d, Bt).reshape(N, 16 * Ci, T, H // 2, W // 2)
    Wg = U.permute(0, 1, 2, 4, 3).reshape(16 * Co, Ci, kT, 1, 1).contiguous()
    M = F.conv3d(V, Wg, None, padding=(kT // 2, 0, 0), groups=16).reshape(N, 4, 4, Co, T, H // 2, W // 2)
    Y = torch.einsum("ia,nabcthw,jb->ncthiwj", At, M, At).reshape(N, Co, T, H, W)
    return Y + b.view(1, -1, 1, 1, 1)


@pytest.mark.parametrize("N,Ci,Co,T,H,W,kT", [(2, 8, 12, 3, 4, 6, 3), (1, 12, 20, 2, 6, 2, 1)])
def test_three_step_decomposition_in_torch(N, Ci, Co, T, H, W, kT):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, Ci, T, H, W, generator=g)
    w = torch.randn(Co, Ci, kT, 3, 3, generator=g) * (2.0 / (Ci * 9 * kT)) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    want = F.conv3d(x.double(), w.double(), b.double(), padding=(kT // 2, 1, 1))
    got = wino_torch(x, w, b)
    direct = F.conv3d(x, w, b, padding=(kT // 2, 1, 1))
    scale = max(1.0, want.abs().max().item())
    # fp32 against an fp64 reference: the same class of error as direct fp32 convolution (a few ulp of the output scale)
    assert (got.double() - want).abs().max().item() <= 2e-5 * scale
    assert (direct.double() - want).abs().max().item() <= 2e-5 * scale
