"""bf16 inference, host side (no GPU): plans of bf16 models compiled on the 'meta' device, the families that raise, and the
ABI pieces (flags, pack mode, tuner / lanes keys)."""
import json

import pytest
import torch

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd import engine as E
from pretorched_x_amd.engine import (AltStep, ChainStep, ConvStep, Engine, Plan, ProgramStep, PtxError, StemF32Step,
                                     StemStep, issued_conv_flop)

SHAPE_FULL = (8, 3, 16, 224, 224)
SHAPE_SMALL = (2, 3, 8, 64, 64)


def _zoo(name, **kw):
    try:
        return ptx.__dict__[name](num_classes=339, pretrained=None, **kw)
    except TypeError:
        return ptx.__dict__[name](num_classes=339, **kw)


def _bf16(name):
    return _zoo(name).eval().to(torch.bfloat16)


def _check_bf16_plan(plan):
    lib = L.lib()
    assert plan.bf16 and plan.precision == "bf16"
    assert plan.conv_steps, "no conv launches"
    for st in plan.steps:
        assert not isinstance(st, (ChainStep, AltStep, ProgramStep, StemStep, StemF32Step)), type(st).__name__
        assert getattr(st, "body", None) is None
    assert not plan.chain_steps and not plan.alt_steps and not plan.program_steps
    for st in plan.conv_steps:
        assert st.d.flags & L.PTX_BF16_OPERANDS and st.d.flags & L.PTX_F16_OPERANDS, st.label
        assert st.d.flags & L.PTX_EPI_OUT_F16, st.label
        assert lib.ptx_conv3d_config_name(st.cfg).decode().endswith("/bf16"), st.label
        assert st.x2 is None and not st.d.x2_C, st.label          # shortcut B unfused
    for a in plan.acts:
        assert a.t.element_size() == 2 and a.bf16 and a.ld % 8 == 0, (a.C, a.ld, a.t.dtype)
    stem = plan.stem_bf16_step
    assert stem is plan.conv_steps[0] and stem.label.startswith("conv1")
    ratio = stem.issued_flop() / (2.0 * stem.macs)
    assert 0.5 < ratio <= 1.6, ratio          # (below 1: temporal padding taps are skipped, the MAC count prices them)
    assert plan.feat.bf16 and plan.pooled.dtype == torch.float32


@pytest.mark.parametrize("name,shape", [("resnet3d50", SHAPE_FULL), ("resnet3d50", SHAPE_SMALL), ("r2plus1d18", SHAPE_FULL),
                                        ("r2plus1d18", SHAPE_SMALL), ("resnet3d18", SHAPE_SMALL), ("resnet3d10", SHAPE_SMALL),
                                        ("r2plus1d50", SHAPE_SMALL)])
def test_dry_plan_bf16(name, shape):
    plan = Engine().dry_plan(_bf16(name), shape)
    _check_bf16_plan(plan)
    flags = [st.d.flags for st in plan.conv_steps]
    if name == "resnet3d18":          # shortcut A: strided, zero-padded residual fused into the epilogue
        assert any(f & L.PTX_EPI_RES_PADA for f in flags)
        assert all(f & L.PTX_RES_F16 for f in flags if f & (L.PTX_EPI_RES_PADA | L.PTX_EPI_RES_ADD))
    if name in ("resnet3d50", "r2plus1d18", "resnet3d10"):    # shortcut B: its own conv, then a residual add
        assert any(".downsample" in st.label for st in plan.conv_steps)
        assert any(f & L.PTX_EPI_RES_ADD for f in flags)
    if name.startswith("r2plus1d"):   # ragged mid channels: odd widths ride on 16-byte padded rows
        assert any(a.C % 2 for a in plan.acts)


@pytest.mark.parametrize("name,shortcut", [("resnet3d18", "B"), ("resnet3d50", "A"), ("r2plus1d18", "A")])
def test_dry_plan_bf16_shortcut_override(name, shortcut):
    m = _zoo(name, shortcut_type=shortcut).eval().to(torch.bfloat16)
    assert m.arch.shortcut == shortcut
    plan = Engine().dry_plan(m, SHAPE_SMALL)
    _check_bf16_plan(plan)
    flags = [st.d.flags for st in plan.conv_steps]
    assert any(f & (L.PTX_EPI_RES_PADA if shortcut == "A" else L.PTX_EPI_RES_ADD) for f in flags)


def test_fp32_plan_unchanged_by_bf16_support():
    """The fp32 plan of the same model keeps its own kernels: no bf16 flag anywhere, fp32 activations."""
    m = ptx.__dict__["resnet3d50"](num_classes=339, pretrained=None).eval()
    plan = Engine().dry_plan(m, SHAPE_SMALL)
    assert not plan.bf16 and plan.precision == "fp32"
    assert all(not (st.d.flags & L.PTX_BF16_OPERANDS) for st in plan.conv_steps)
    assert all(a.t.dtype == torch.float32 for a in plan.acts)


def _make(name):
    if name.startswith("slowfast."):
        return ptx.slowfast.__dict__[name.split(".")[1]](num_classes=339)
    if name == "i3d":
        return ptx.i3d(num_classes=339, pretrained=None)
    try:
        return ptx.__dict__[name](num_classes=339, pretrained=None)
    except TypeError:
        return ptx.__dict__[name](num_classes=339)


OUT_OF_SCOPE = [("nonlocalresnet3d50", (1, 3, 8, 64, 64)), ("nonlocal_r2plus1d50", (1, 3, 8, 64, 64)),
                ("resnext3d50", (1, 3, 8, 64, 64)), ("wideresnet3d50", (1, 3, 8, 64, 64)), ("resneti3d50", (1, 3, 8, 64, 64)),
                ("preact_resnet3d50", (1, 3, 8, 64, 64)), ("mvresnet18", (1, 3, 8, 64, 64)), ("resnet50", (1, 3, 224, 224)),
                ("slowfast.resnet50", (1, 3, 32, 64, 64)), ("i3d", (1, 3, 16, 224, 224))]


@pytest.mark.parametrize("name,shape", OUT_OF_SCOPE)
def test_dry_plan_bf16_out_of_scope_raises(name, shape):
    m = _make(name).eval().to(torch.bfloat16)
    with pytest.raises(PtxError, match="bf16"):
        Engine().dry_plan(m, shape)


def test_adopted_bf16_raises():
    """An adopted instance (adopt.py names it "adopted:<class>") is not one of the bf16 families."""
    m = ptx.__dict__["resnet3d18"](num_classes=339, pretrained=None).eval().to(torch.bfloat16)
    m.arch_name = "adopted:ResNet"
    with pytest.raises(PtxError, match="bf16"):
        Engine().dry_plan(m, (1, 3, 8, 64, 64))


def test_dry_plan_half_raises():
    m = ptx.__dict__["resnet3d50"](num_classes=339, pretrained=None).eval().half()
    with pytest.raises(PtxError, match="fp16"):
        Engine().dry_plan(m, SHAPE_SMALL)
    m = _zoo("r2plus1d18").eval().half()
    with pytest.raises(PtxError, match="fp16"):
        Engine().dry_plan(m, SHAPE_SMALL)


def test_header_flags_and_pack_mode_bound():
    text = open(L.HEADER_PATH).read()
    assert "#define PTX_BF16_OPERANDS 0x%xu" % L.PTX_BF16_OPERANDS in text
    assert "#define PTX_POOL_BF16 %du" % L.PTX_POOL_BF16 in text
    assert L.PTX_PACK_BF16 == 3
    used = (L.PTX_EPI_RELU | L.PTX_EPI_RES_ADD | L.PTX_EPI_RES_PADA | L.PTX_PRO_RELU | L.PTX_EPI_ACCUM | L.PTX_EPI_RES_UP |
            L.PTX_F16_OPERANDS | L.PTX_F16X3_OPERANDS | L.PTX_SPLITK_FUSED | L.PTX_EPI_OUT_F16 | L.PTX_EPI_AFFINE |
            L.PTX_EPI_DUAL_RAW | L.PTX_RES_F16 | L.PTX_PRO_UP2 | L.PTX_EPI_TANH)
    assert not (L.PTX_BF16_OPERANDS & used)
    assert not (L.PTX_POOL_BF16 & (L.PTX_POOL_SAME | L.PTX_POOL_PAD_ZERO))
    lib = L.lib()
    for sym in ("ptx_conv3d_num_configs_bf16", "ptx_checksum_b16", "ptx_ncdhw_to_ndhwc_bf16", "ptx_ndhwc_to_ncdhw_bf16", "ptx_im2col_hw_bf16",
                "ptx_f32_to_bf16", "ptx_global_avgpool_bf16"):
        assert sym in L.SIGNATURES and hasattr(lib, sym)
    names = [lib.ptx_conv3d_config_name(i).decode() for i in range(lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16())]
    bf = [n for n in names if n.endswith("/bf16")]
    assert bf and all(E._tile_kind(n) == "bf16" for n in bf)
    # the bf16 tiles close the table, outside the range ptx_conv3d_num_configs() enumerates
    n0 = lib.ptx_conv3d_num_configs()
    assert len(bf) == lib.ptx_conv3d_num_configs_bf16() and names[n0:] == bf
    assert not any(n.endswith("/bf16") for n in names[:n0])
    assert E._flags_kind(L.PTX_F16_OPERANDS | L.PTX_BF16_OPERANDS) == "bf16"
    assert E._flags_kind(L.PTX_F16_OPERANDS) == "f16" and E._flags_kind(0) == ""


def test_pack_desc_bf16_elems():
    d = L.PackDesc(64, 64, 3, 3, 3, 64, 128, 0, 0, 0, 0, 0, 0, L.PTX_PACK_BF16)
    assert L.lib().ptx_packed_weight_elems(d) == 27 * 128 * 64


def test_tuner_and_lanes_keys_do_not_collide():
    m32 = ptx.__dict__["resnet3d50"](num_classes=339, pretrained=None).eval()
    m16 = ptx.__dict__["resnet3d50"](num_classes=339, pretrained=None).eval().to(torch.bfloat16)
    eng = Engine()
    p32, p16 = eng.dry_plan(m32, SHAPE_SMALL), eng.dry_plan(m16, SHAPE_SMALL)
    k32 = {json.dumps(s.d.key()) for s in p32.conv_steps}
    k16 = {json.dumps(s.d.key()) for s in p16.conv_steps}
    assert not (k32 & k16)
    assert eng.precision_of(m16) == "bf16" and eng.precision_of(m32) == "fp32"
    eng.precision = "x3"
    assert eng.precision_of(m16) == "bf16"         # Engine.precision governs fp32 models only
    assert E.lanes_key(m16, SHAPE_FULL, "bf16") != E.lanes_key(m32, SHAPE_FULL, "fp32")
    # a bf16 problem never takes an fp32 / f16 / x3 tuned entry (and the other way round)
    for s in p16.conv_steps:
        t = E.tuned_lookup(json.dumps(s.d.key()), E._flags_kind(s.d.flags))
        assert t is None or L.lib().ptx_conv3d_config_name(t[0]).decode().endswith("/bf16")


def test_bf16_max_batch_counts_two_byte_activations():
    eng = Engine()
    m16 = _bf16("resnet3d50")
    one = eng.dry_plan(m16, (1,) + SHAPE_FULL[1:])
    assert all(a.t.element_size() == 2 for a in one.acts)
    per_clip = max(a.t.numel() * 2 for a in one.acts)
    assert eng.max_batch(m16, SHAPE_FULL[1:]) == eng.LIMIT_BYTES // per_clip


def test_stem_issued_work_accounting():
    """The bf16 stem's issued FLOP follows the tile walk: 160 folded channels for 147 live ones."""
    plan = Engine().dry_plan(_bf16("resnet3d50"), SHAPE_FULL)
    st = plan.stem_bf16_step
    assert st.d.kH == 1 and st.d.kW == 1 and st.d.kT == 7 and st.d.Kc * 2 == 160 and st.d.ldx * 2 == 160
    name = L.lib().ptx_conv3d_config_name(st.cfg).decode()
    tile = E._tile_dims(name)
    assert st.issued_flop() == issued_conv_flop(st.d, tile, 2)
