"""Host-side tests of the Winograd F(4x4,3x3) execution (no GPU): the eligibility rule (any H and W), the 36-group descriptor
and its sizes, the "wino4:" entries of the tuned table, the plan compiler's F(4x4) steps on a dry plan, and the three-step
decomposition restated in torch in the kernels' layouts."""
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


def test_header_binding_and_library_agree(ptx):
    """The seven F(4x4) calls live in include/ptx_amd_wino4.h: that header, _lib.SIGNATURES_WINO4 and the library's exports name
    the same functions, each mirrors its F(2x2) counterpart's signature, and ptx_amd.h's own census is untouched."""
    import re
    L = ptx._lib
    text = re.sub(r"/\*.*?\*/", "", open(L.WINO4_HEADER_PATH).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ptx_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(L.SIGNATURES_WINO4) and len(declared) == 7
    assert declared == sorted(["ptx_conv_wino4_f32_supported", "ptx_conv_wino4_f32_workspace_bytes", "ptx_conv_wino4_f32_gemm_desc",
                               "ptx_wino4_f32_weight_elems", "ptx_pack_wino4_f32_weight", "ptx_wino4_in_f32", "ptx_wino4_out_f32"])
    assert not set(declared) & set(L.SIGNATURES) and not set(declared) & set(L.header_symbols())
    assert '#include "ptx_amd.h"' in text
    lib = L.lib()
    for name in declared:
        fn = getattr(lib, name)
        twin = L.SIGNATURES[name.replace("wino4", "wino")]
        assert (fn.restype, list(fn.argtypes)) == (twin[0], list(twin[1])) == (L.SIGNATURES_WINO4[name][0], list(L.SIGNATURES_WINO4[name][1]))
    integ = open(L.HEADER_PATH.replace("include/ptx_amd.h", "INTEGRATION.md")).read()
    assert "ptx_amd_wino4.h" in integ and all(n in integ for n in declared)


def test_eligibility_rule(ptx):
    L, lib = ptx._lib, ptx._lib.lib()

    def ok(**edits):
        shape = {k: edits.pop(k) for k in list(edits) if k in ("N", "Ci", "Co", "T", "H", "W", "kT", "flags")}
        d = _desc(L, **shape)
        for k, v in edits.items():
            setattr(d, k, v)
        return bool(lib.ptx_conv_wino4_f32_supported(C.byref(d)))

    assert ok() and ok(kT=1) and ok(Ci=10, Co=18) and ok(flags=L.PTX_EPI_RELU | L.PTX_EPI_RES_ADD, ldr=16)
    # the F(2x2) rule without "H and W even": odd and ragged extents, frames smaller than one tile
    assert ok(H=7) and ok(W=7) and ok(H=7, W=5) and ok(H=6, W=10) and ok(H=1, W=1) and ok(H=2, W=3)
    assert not ok(H=0)
    assert not ok(sH=2, sW=2, Ho=4, Wo=4) and not ok(sT=2, To=2)
    assert not ok(pH=0, pW=0, Ho=6, Wo=6) and not ok(pT=0, To=2)
    assert not ok(groups=2) and not ok(kH=1, pH=0) and not ok(kT=5, pT=2)
    for flag in (L.PTX_EPI_RES_PADA, L.PTX_F16X3_OPERANDS, L.PTX_F16_OPERANDS, L.PTX_F16_OPERANDS | L.PTX_BF16_OPERANDS):
        assert not ok(flags=flag)
    assert not ok(flags=L.PTX_EPI_RES_ADD, ldr=8)                        # a residual row shorter than Co
    # every operand of one launch below 2 GiB: x = frames x 512 x 512 x 128 floats = frames x 128 MiB, V = 2.25 x that
    # (128 x 128 tiles x 36 x 128 floats = 288 MiB per frame): 7 frames of V are 2016 MiB, 8 are 2304 MiB
    assert ok(N=1, Ci=128, T=7, H=512, W=512) and not ok(N=1, Ci=128, T=8, H=512, W=512)
    assert b"2 GiB" in lib.ptx_last_error()
    d = _desc(L, N=1, Ci=128, T=8, H=512, W=512)
    assert lib.ptx_conv_wino4_f32_workspace_bytes(C.byref(d)) == 0 and lib.ptx_wino4_f32_weight_elems(C.byref(d)) == 0
    # on even frames the two rules agree, refusal by refusal
    def both(**edits):
        d = _desc(L)
        for k, v in edits.items():
            setattr(d, k, v)
        return bool(lib.ptx_conv_wino_f32_supported(C.byref(d))), bool(lib.ptx_conv_wino4_f32_supported(C.byref(d)))

    for edits in (dict(), dict(sH=2, sW=2, Ho=4, Wo=4), dict(groups=2), dict(flags=L.PTX_EPI_RES_PADA), dict(ldx=18), dict(Kc=8),
                  dict(pT=0, To=2), dict(flags=L.PTX_EPI_RES_ADD, ldr=8), dict(flags=L.PTX_EPI_RES_ADD, ldr=16)):
        two, four = both(**edits)
        assert two == four, edits


def test_grouped_descriptor_and_sizes(ptx):
    L, lib = ptx._lib, ptx._lib.lib()
    d, g = _desc(L, N=8, Ci=128, Co=128, T=4, H=28, W=28), L.ConvDesc()
    assert lib.ptx_conv_wino4_f32_gemm_desc(C.byref(d), C.byref(g)) == 0
    assert (g.N, g.Ti, g.Hi, g.Wi, g.To, g.Ho, g.Wo) == (8, 4, 7, 7, 4, 7, 7)
    assert (g.Ci, g.ldx, g.Co, g.ldy, g.Kc, g.Co_pad, g.groups, g.flags) == (4608, 4608, 4608, 4608, 128, 4608, 36, 0)
    assert (g.kT, g.kH, g.kW, g.pT, g.pH, g.pW, g.sT, g.sH, g.sW) == (3, 1, 1, 1, 0, 0, 1, 1, 1)
    tiles = 8 * 4 * 7 * 7
    assert lib.ptx_conv_wino4_f32_workspace_bytes(C.byref(d)) == 2 * tiles * 4608 * 4
    assert lib.ptx_wino4_f32_weight_elems(C.byref(d)) == 3 * 4608 * 128
    assert any(lib.ptx_conv3d_config_supported(C.byref(g), i) for i in range(lib.ptx_conv3d_num_configs()))
    # partial tiles and ragged channels: ceil(H/4) x ceil(W/4) tiles, Cg / Cog round up to 4, rows to 128, V to 256 bytes
    d = _desc(L, N=1, Ci=10, Co=18, T=2, H=7, W=5, kT=1)
    assert lib.ptx_conv_wino4_f32_gemm_desc(C.byref(d), C.byref(g)) == 0
    assert (g.Hi, g.Wi, g.Ci, g.Co, g.Kc, g.Co_pad, g.groups, g.kT, g.pT) == (2, 2, 36 * 12, 36 * 20, 12, 768, 36, 1, 0)
    v = (8 * 36 * 12 * 4 + 255) // 256 * 256
    assert lib.ptx_conv_wino4_f32_workspace_bytes(C.byref(d)) == v + 8 * 36 * 20 * 4
    assert lib.ptx_wino4_f32_weight_elems(C.byref(d)) == 768 * 12
    assert lib.ptx_conv_wino4_f32_gemm_desc(C.byref(_desc(L, kT=5)), C.byref(g)) == 2       # PTX_ERR_UNSUPPORTED


def test_wino4_keys_round_trip(ptx, tmp_path):
    from pretorched_x_amd import tuned
    lib = ptx._lib.lib()
    keep = tuned.tuned_snapshot()
    try:
        key = json.dumps(_desc(ptx._lib, N=8).key())
        assert tuned.wino4_lookup(key) is None and tuned.wino_lookup(key) is None
        name = lib.ptx_conv3d_config_name(0).decode()
        tuned.wino_store(key, True, 0)
        tuned.wino4_store(key, False, 0)
        tuned.wino4_store("chain:" + key, True, 0)
        assert tuned.wino4_lookup(key) is False and tuned.wino4_lookup("chain:" + key) is True
        assert tuned.wino_lookup(key) is True and tuned.wino_lookup("chain:" + key) is None     # the two families are apart
        path = str(tmp_path / "table.json")
        tuned.save_tuned_table(path)
        saved = json.load(open(path))
        assert saved["wino4:" + key] == [name, 2] and saved["wino4:chain:" + key] == [name, 1] and saved["wino:" + key] == [name, 1]
        assert {k: v for k, v in saved.items() if k.startswith("wino:")} == \
            {k: list(v) for k, v in dict(keep, **{"wino:" + key: (name, 1)}).items() if k.startswith("wino:")}
        tuned.tuned_replace(saved)
        assert tuned.wino4_lookup(key) is False and tuned.wino4_lookup("chain:" + key) is True and tuned.wino_lookup(key) is True
        assert tuned.wino4_lookup(json.dumps(_desc(ptx._lib, N=4).key())) is None
    finally:
        tuned.tuned_replace(keep)


ELEVEN = ["layer1.%d.conv2" % i for i in range(3)] + ["layer2.%d.conv2" % i for i in (1, 2, 3)] + \
    ["layer3.%d.conv2" % i for i in (1, 2, 3, 4, 5)]


def test_dry_plan_compiles_wino4_steps(ptx, monkeypatch):
    """Config 2: the eleven convs with an F(2x2) form carry an F(4x4) form too, and layer4.{1,2}.conv2 (7 x 7 frames) are
    F(4x4)-only candidates; without a verdict everything runs direct, a "wino4:" verdict switches the step (and opens the
    chained pair), PTX_CONV_WINO=4 selects F(4x4) wherever it exists."""
    from pretorched_x_amd import tuned
    from pretorched_x_amd.steps import ConvStep, Wino4Step, WinoStep
    monkeypatch.delenv("PTX_CONV_WINO", raising=False)
    keep = tuned.tuned_snapshot()
    try:
        tuned.tuned_replace({k: v for k, v in keep.items() if not k.startswith(("wino:", "wino4:"))})
        m = ptx.resnet3d50(num_classes=339, pretrained=None)
        plan = m.engine().dry_plan(m, (8, 3, 16, 224, 224))
        assert [w.label for w in plan.wino_steps] == ELEVEN
        assert [w.label for w in plan.wino4_steps] == ELEVEN + ["layer4.1.conv2", "layer4.2.conv2"]
        assert plan.wino4_steps[:11] == plan.wino_steps
        assert not any(w.use_wino or w.use_wino4 for w in plan.wino4_steps)
        n_convs = len(plan.all_convs())
        for w in plan.wino4_steps:
            only4 = w.label.startswith("layer4")
            assert isinstance(w, Wino4Step if only4 else WinoStep) and (w.wino is None) == only4 and (w.gemm is None) == only4
            assert w.active() == w.direct and len(w.direct) == 1 and isinstance(w.direct[0], ConvStep)
            g = w.gemm4
            assert g not in plan.conv_steps and g.d.groups == 36 and g.split == 1 and g.macs == w.direct[0].macs
            d = w.direct[0].d
            assert (g.d.Hi, g.d.Wi, g.d.Kc, g.d.Ci) == (-(-d.Hi // 4), -(-d.Wi // 4), d.Ci, 36 * d.Ci)
            assert [getattr(s, "label", None) for s in w.wino4] == ["wino4_in", w.label + ".wino4_gemm", "wino4_out"]
            assert w.wino4[0].hbm_bytes > 0 and w.wino4[2].hbm_bytes > 0 and w.arena_bytes <= plan.wino_bytes
            assert w.need_u4 is not None                       # no verdict: U4 is neither allocated nor packed
            if not only4:
                assert w.gemm.d.groups == 16 and w.wino4[0].hbm_bytes < w.wino[0].hbm_bytes      # V is 2.25x, not 4x
                assert g.issued_flop() < w.gemm.issued_flop()
        # a stored wino4: verdict switches the step at compile time -- and the pair it opens away from the chained launch
        for w in plan.wino4_steps[1:4]:
            tuned.wino4_store(w.key, True, w.gemm4.cfg)
        tuned.wino4_store(plan.wino4_steps[11].key, True, plan.wino4_steps[11].gemm4.cfg)
        tuned.wino_store(plan.wino_steps[3].key, True, plan.wino_steps[3].gemm.cfg)       # F(4x4) goes first where both say yes
        tuned.wino_store(plan.wino_steps[6].key, True, plan.wino_steps[6].gemm.cfg)
        plan2 = m.engine().dry_plan(m, (8, 3, 16, 224, 224))
        assert [w.use_wino4 for w in plan2.wino4_steps] == [False] + [True] * 5 + [False] * 5 + [True] * 2
        assert [w.use_wino for w in plan2.wino4_steps] == [False] * 6 + [True] * 5 + [False] * 2
        assert not any(w.use_wino and w.use_wino4 for w in plan2.wino4_steps)
        assert not plan2.wino4_steps[1].alt.use_chain and plan2.wino4_steps[0].alt is None
        for w in plan2.wino4_steps:
            assert (w.need_u4 is None) == w.use_wino4
            if w.use_wino4:
                assert w.active() == w.wino4 and w.active()[1] is w.gemm4
        assert len(plan2.all_convs()) == n_convs + 2       # layer1.{1,2}: the chained launch became conv2 (F(4x4)) + conv3
        assert abs(sum(s.macs for s in plan2.all_convs()) - sum(s.macs for s in plan.all_convs())) < 1
        # PTX_CONV_WINO=4: F(4x4) wherever it is supported; =1 leaves the F(4x4)-only convs on their auto behaviour
        monkeypatch.setenv("PTX_CONV_WINO", "4")
        plan4 = m.engine().dry_plan(m, (8, 3, 16, 224, 224))
        assert len(plan4.wino4_steps) == 13 and all(w.use_wino4 and not w.use_wino for w in plan4.wino4_steps)
        assert not any(a.use_chain for a in plan4.alt_steps if isinstance(a.pair[0], WinoStep))
        monkeypatch.setenv("PTX_CONV_WINO", "1")
        plan1 = m.engine().dry_plan(m, (8, 3, 16, 224, 224))
        assert all(w.use_wino and not w.use_wino4 for w in plan1.wino_steps)
        assert [w.use_wino4 for w in plan1.wino4_steps[11:]] == [True, True]          # their stored verdict, as under auto
        monkeypatch.setenv("PTX_CONV_WINO", "0")
        plan0 = m.engine().dry_plan(m, (8, 3, 16, 224, 224))
        assert not plan0.wino_steps and not plan0.wino4_steps
    finally:
        tuned.tuned_replace(keep)


Bt = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                   [0, 4, 0, -5, 0, 1]], dtype=torch.float32)
G = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                  [0, 0, 1]], dtype=torch.float32)
At = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float32)


def wino4_torch(x, w, b):
    """The three steps in the layout the kernels use: V [N, 36 Cg, T, H4, W4] with transform position xi = 6 a + b major over
    channels (reads past the frame are zero, the overhang of a partial tile included), a 36-group (kT,1,1) conv with the
    filter rows U[xi][co], and the output transform + bias with the outputs past the frame cut off."""
    N, Ci, T, H, W = x.shape
    Co, _, kT = w.shape[:3]
    H4, W4 = -(-H // 4), -(-W // 4)
    U = torch.einsum("ai,octij,bj->abotc", G, w, G)                                      # 6,6,Co,kT,Ci
    d = F.pad(x, (1, 4 * W4 + 1 - W, 1, 4 * H4 + 1 - H)).unfold(3, 6, 4).unfold(4, 6, 4)  # N,Ci,T,H4,W4,6,6
    V = torch.einsum("ai,ncthwij,bj->nabcthw", Bt, d, Bt).reshape(N, 36 * Ci, T, H4, W4)
    Wg = U.permute(0, 1, 2, 4, 3).reshape(36 * Co, Ci, kT, 1, 1).contiguous()
    M = F.conv3d(V, Wg, None, padding=(kT // 2, 0, 0), groups=36).reshape(N, 6, 6, Co, T, H4, W4)
    Y = torch.einsum("ia,nabcthw,jb->ncthiwj", At, M, At).reshape(N, Co, T, 4 * H4, 4 * W4)[..., :H, :W]
    return Y + b.view(1, -1, 1, 1, 1)


@pytest.mark.parametrize("N,Ci,Co,T,H,W,kT", [(2, 8, 12, 3, 4, 8, 3), (1, 12, 20, 2, 6, 10, 1), (1, 8, 8, 2, 7, 5, 3)])
def test_three_step_decomposition_in_torch(N, Ci, Co, T, H, W, kT):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, Ci, T, H, W, generator=g)
    w = torch.randn(Co, Ci, kT, 3, 3, generator=g) * (2.0 / (Ci * 9 * kT)) ** 0.5
    b = torch.randn(Co, generator=g) * 0.1
    want = F.conv3d(x.double(), w.double(), b.double(), padding=(kT // 2, 1, 1))
    got = wino4_torch(x, w, b)
    scale = max(1.0, want.abs().max().item())
    # fp32 F(4x4) against an fp64 reference: measured <= 9e-6 x scale at C = 64..256, so 1e-4 keeps about 10x margin
    err = (got.double() - want).abs().max().item()
    print("F(4x4) in torch, max err %.3e at scale %.3f" % (err, scale))
    assert err <= 1e-4 * scale
