"""The patch-resident bf16 stem (Engine.bf16_stem = "direct"), host side (no GPU): the switch, plans compiled on the 'meta'
device under both settings, the kernel's geometry table and the ABI."""
import ctypes as C

import pytest
import torch

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import ConvStep, Engine, PtxError, StemBf16Step

SHAPE_FULL = (8, 3, 16, 224, 224)
SHAPE_SMALL = (2, 3, 8, 64, 64)
DIRECT_CASES = [("resnet3d50", SHAPE_FULL), ("resnet3d50", SHAPE_SMALL), ("r2plus1d18", SHAPE_SMALL)]


def _bf16(name):
    try:
        m = ptx.__dict__[name](num_classes=339, pretrained=None)
    except TypeError:
        m = ptx.__dict__[name](num_classes=339)
    return m.eval().to(torch.bfloat16)


def _direct_engine():
    eng = Engine()
    eng.bf16_stem = "direct"
    return eng


def test_switch_default_bad_value_and_plan_drop():
    eng = Engine()
    assert eng.bf16_stem == "fold"
    with pytest.raises(PtxError, match="bf16_stem"):
        eng.bf16_stem = "patch"
    assert eng.bf16_stem == "fold"
    eng._plans["sentinel"] = object()
    eng.bf16_stem = "fold"                      # unchanged value: the plans stay
    assert "sentinel" in eng._plans
    epoch = eng._epoch
    eng.bf16_stem = "direct"
    assert eng.bf16_stem == "direct" and not eng._plans and eng._epoch == epoch + 1


def test_switch_reads_the_environment(monkeypatch):
    monkeypatch.setenv("PTX_BF16_STEM", "direct")
    assert Engine().bf16_stem == "direct"
    monkeypatch.setenv("PTX_BF16_STEM", "nonsense")
    with pytest.raises(PtxError, match="bf16_stem"):
        Engine()


@pytest.mark.parametrize("name", ["resnet3d50", "r2plus1d18"])
def test_default_plans_hold_no_direct_stem(name):
    plan = Engine().dry_plan(_bf16(name), SHAPE_SMALL)
    assert plan.bf16_stem == "fold"
    assert not any(isinstance(s, StemBf16Step) for s in plan.steps)
    assert plan.stem_bf16_step is plan.conv_steps[0]
    assert any(getattr(s, "label", "") == "im2col_hw_bf16" for s in plan.steps)


def _steps_in_clip(d):
    """(kt, kh) steps the kernel walks, summed over the output frames: temporal taps outside the clip are skipped."""
    n = 0
    for to in range(d.To):
        t0 = to * d.sT - d.pT
        n += sum(1 for kt in range(d.kT) if 0 <= t0 + kt < d.Ti) * d.kH
    return n


@pytest.mark.parametrize("name,shape", DIRECT_CASES)
def test_direct_plans(name, shape):
    lib = L.lib()
    model = _bf16(name)
    fold = Engine().dry_plan(model, shape)
    plan = _direct_engine().dry_plan(model, shape)
    assert plan.bf16 and plan.bf16_stem == "direct"
    stems = [s for s in plan.steps if isinstance(s, StemBf16Step)]
    assert len(stems) == 1 and plan.steps[0] is stems[0]
    assert not any(getattr(s, "label", "") == "im2col_hw_bf16" for s in plan.steps)
    assert plan.stem_bf16_step is None and plan.stem_steps == 1
    # every remaining conv is what _check_bf16_plan (tests/test_bf16_host.py) asks of a bf16 plan's convs
    assert plan.conv_steps and len(plan.conv_steps) == len(fold.conv_steps) - 1
    for st in plan.conv_steps:
        assert isinstance(st, ConvStep)
        assert st.d.flags & L.PTX_BF16_OPERANDS and st.d.flags & L.PTX_F16_OPERANDS and st.d.flags & L.PTX_EPI_OUT_F16, st.label
        assert lib.ptx_conv3d_config_name(st.cfg).decode().endswith("/bf16"), st.label
    for a in plan.acts:
        assert a.t.element_size() == 2 and a.bf16 and a.ld % 8 == 0
    # the stem's output is the fold plan's: same shape, same row stride (its consumers are unchanged)
    st, fst = stems[0], fold.stem_bf16_step
    d = st.d
    assert st.kernel == "conv_stem_bf16" and st.src == L.PTX_STEM_SRC_BF16_NCDHW and st.norm is None
    assert (d.N, d.To, d.Ho, d.Wo, d.Co, d.ldy) == (fst.d.N, fst.d.To, fst.d.Ho, fst.d.Wo, fst.d.Co, fst.d.ldy)
    assert [c.d.key() for c in plan.conv_steps] == [c.d.key() for c in fold.conv_steps[1:]]
    assert st.macs == fst.macs and st.hbm_bytes > 0
    # issued work, closed form: a tile = 256 consecutive outputs of a frame (the full-width patch of these shapes fits);
    # per (kt, kh) step inside the clip its 4 waves issue, for each of their 4 position tiles, one
    # v_mfma_f32_16x16x32_bf16 (16 * 16 * 32 * 2 FLOP) per 16-channel tile below ldy
    assert (min(d.Ho, (255 + d.Wo - 1) // d.Wo + 1) - 1) * d.sH + d.kH <= 40960 // (((d.Wo - 1) * 2 + 8) * 8)
    tiles = d.N * -(-(d.Ho * d.Wo) // 256)
    want = tiles * _steps_in_clip(d) * 4 * 4 * -(-d.ldy // 16) * 16384
    assert st.issued_flop() == float(want)
    ratio = st.issued_flop() / (2.0 * st.macs)
    assert 0.5 < ratio <= 1.6, ratio


def test_direct_plan_from_uint8_frames():
    norm = L.NormDesc.make([0.485, 0.456, 0.406], [0.229, 0.224, 0.225], "BGR", (0, 255))
    model = _bf16("resnet3d50")
    plan = ptx.engine.Plan(_direct_engine(), model, SHAPE_SMALL, torch.device("meta"), norm)
    stems = [s for s in plan.steps if isinstance(s, StemBf16Step)]
    assert len(stems) == 1 and stems[0].src == L.PTX_STEM_SRC_U8_NTHWC and stems[0].norm is norm
    assert not any(getattr(s, "label", "") in ("im2col_hw_bf16", "frames_u8_to_ncdhw") for s in plan.steps)
    # under "fold" the same request keeps raising, with the same words
    with pytest.raises(PtxError, match="uint8 frames / frame sub-sampling are fp32 only"):
        ptx.engine.Plan(Engine(), model, SHAPE_SMALL, torch.device("meta"), norm)


@pytest.mark.parametrize("name", ["resnet3d50", "r2plus1d18"])
def test_max_batch_not_smaller_under_direct(name):
    model = _bf16(name)
    assert _direct_engine().max_batch(model, SHAPE_FULL[1:]) >= Engine().max_batch(model, SHAPE_FULL[1:])


def _desc(N, T, H, W, k, s, p, Co, Ci=3):
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci = N, T, H, W, Ci
    d.kT, d.kH, d.kW = k
    d.sT, d.sH, d.sW = s
    d.pT, d.pH, d.pW = p
    d.To, d.Ho, d.Wo = ((i + 2 * pp - kk) // ss + 1 for i, pp, kk, ss in zip((T, H, W), p, k, s))
    d.Co, d.ldy, d.Co_pad = Co, (Co + 7) // 8 * 8, (Co + 127) // 128 * 128
    return d


def test_supported_table():
    lib = L.lib()
    ok = [_desc(8, 16, 224, 224, (7, 7, 7), (1, 2, 2), (3, 3, 3), 64),
          _desc(2, 8, 64, 64, (7, 7, 7), (1, 2, 2), (3, 3, 3), 64),
          _desc(2, 8, 64, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), 83),
          _desc(2, 8, 64, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), 110),
          _desc(1, 3, 1080, 1920, (3, 7, 7), (1, 2, 2), (1, 3, 3), 64),       # wide frames: row-segment tiles
          _desc(1, 2, 80, 400, (2, 61, 5), (1, 2, 2), (0, 30, 2), 40)]        # a filter taller than the patch buffer
    for d in ok:
        for src in (L.PTX_STEM_SRC_BF16_NCDHW, L.PTX_STEM_SRC_U8_NTHWC):
            assert lib.ptx_conv_stem_bf16_supported(C.byref(d), src) == 1, lib.ptx_last_error()
    base = dict(N=2, T=8, H=64, W=64, k=(7, 7, 7), s=(1, 2, 2), p=(3, 3, 3), Co=64)
    bad = {"Ci == 3": _desc(**dict(base, Ci=4)),
           "filter width": _desc(**dict(base, k=(7, 7, 9), p=(3, 3, 4))),
           "stride_w": _desc(**dict(base, s=(1, 2, 3)))}
    same = _desc(**base)
    same.Ho, same.Wo, same.pH, same.pW = 32, 32, 2, 2                         # TF-SAME extents: front pad 2, back pad 3
    bad["SAME"] = same
    huge = _desc(1, 1, 30000, 30000, (1, 7, 7), (1, 2, 2), (0, 3, 3), 64)     # one input frame past 2^31 elements
    bad["2^31"] = huge
    for why, d in bad.items():
        for src in (L.PTX_STEM_SRC_BF16_NCDHW, L.PTX_STEM_SRC_U8_NTHWC):
            assert lib.ptx_conv_stem_bf16_supported(C.byref(d), src) == 0, why
            msg = lib.ptx_last_error().decode()
            assert msg and why in msg, (why, msg)
    assert lib.ptx_conv_stem_bf16_supported(C.byref(ok[0]), 2) == 0 and lib.ptx_last_error()
    # the re-laid filter: one 4 KiB block per (kt, kh) step and 64-channel tile
    assert lib.ptx_stem_bf16_weight_elems(C.byref(ok[0])) == 7 * 7 * 2 * 2048
    assert lib.ptx_stem_bf16_weight_elems(C.byref(ok[2])) == 1 * 7 * 2 * 2048


def test_abi():
    text = open(L.HEADER_PATH).read()
    lib = L.lib()
    for sym in ("ptx_conv_stem_bf16_supported", "ptx_stem_bf16_weight_elems", "ptx_pack_stem_bf16_weight", "ptx_conv_stem_bf16_fwd"):
        assert sym in L.header_symbols() and sym in L.SIGNATURES and hasattr(lib, sym), sym
        assert sym not in L.EXPERIMENTAL
    assert "#define PTX_STEM_SRC_BF16_NCDHW %d\n" % L.PTX_STEM_SRC_BF16_NCDHW in text
    assert "#define PTX_STEM_SRC_U8_NTHWC %d\n" % L.PTX_STEM_SRC_U8_NTHWC in text
    # host-side argument checks need no device
    d = _desc(2, 8, 64, 64, (7, 7, 7), (1, 2, 2), (3, 3, 3), 64)
    assert lib.ptx_conv_stem_bf16_fwd(C.byref(d), None, 0, None, None, None, None, None) == 1
