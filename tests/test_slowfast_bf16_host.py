"""bf16 SlowFast / SlowOnly / FastOnly on the frame-strided direct bf16 stem, host side (no GPU): the ABI of
include/ptx_amd_stem_strided.h, the strided kernel's geometry table, plans compiled on the 'meta' device under
Engine.bf16_stem = "direct" (clips and uint8 frames), and what keeps raising."""
import ctypes as C
import os
import re

import pytest
import torch

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import AltStep, ChainStep, ConvStep, Engine, ProgramStep, PtxError, StemBf16Step

BF16, U8 = L.PTX_STEM_SRC_BF16_NCDHW, L.PTX_STEM_SRC_U8_NTHWC
FAST = ((5, 7, 7), (1, 2, 2), (2, 3, 3))
SLOW = ((1, 7, 7), (1, 2, 2), (0, 3, 3))
SHAPE = (1, 3, 32, 64, 64)
NAMES = ["ptx_conv_stem_bf16_strided_fwd", "ptx_conv_stem_bf16_strided_supported"]


def _direct_engine():
    eng = Engine()
    eng.bf16_stem = "direct"
    return eng


def _model(arch, mode, **kw):
    return ptx.slowfast.__dict__[arch](mode=mode, num_classes=51, **kw).eval().to(torch.bfloat16)


# --------------------------------------------------------------------------------------------- the C ABI
def test_header_bindings_and_exports_agree():
    text = open(L.STEM_STRIDED_HEADER_PATH).read()
    declared = L.header_symbols(L.STEM_STRIDED_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_STEM_STRIDED) == NAMES
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.SIGNATURES_YUV16, L.SIGNATURES_COLOR,
                  L.SIGNATURES_RANDAUG, L.SIGNATURES_RESAMPLE, L.SIGNATURES_MIX, L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_STEM_STRIDED[name][0], list(L.SIGNATURES_STEM_STRIDED[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_STEM_STRIDED[name][1]), name
    # each is its plain twin's signature with (frame_step, T_full) added: after `src` / after `norm`
    sup, fwd = L.SIGNATURES["ptx_conv_stem_bf16_supported"], L.SIGNATURES["ptx_conv_stem_bf16_fwd"]
    i32 = C.c_int32
    assert list(L.SIGNATURES_STEM_STRIDED[NAMES[1]][1]) == list(sup[1]) + [i32, i32]
    assert list(L.SIGNATURES_STEM_STRIDED[NAMES[0]][1]) == list(fwd[1][:4]) + [i32, i32] + list(fwd[1][4:])
    root = os.path.dirname(os.path.dirname(L.HEADER_PATH))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "ptx_amd_stem_strided.h" in integ and all(n in integ for n in declared)
    # the build: the header is hashed into the version and is a dependency of the object that holds the kernel
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert len(build.SOURCES) == 10 and any(h.endswith("ptx_amd_stem_strided.h") for h in build.HEADERS)
    assert any(p.endswith("ptx_amd_stem_strided.h") for p in build.tu_files("pack_layout.hip"))
    assert L.binary_source_hash() == L.source_hash()
    # host-side argument checks need no device
    assert lib.ptx_conv_stem_bf16_strided_fwd(C.byref(_desc(FAST, 8, 32, 64, 64)), None, 0, None, 2, 64, None, None, None, None) == 1


def _desc(geom, Co, Ti, H, W, N=2):
    k, s, p = geom
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci = N, Ti, H, W, 3
    d.kT, d.kH, d.kW = k
    d.sT, d.sH, d.sW = s
    d.pT, d.pH, d.pW = p
    d.To, d.Ho, d.Wo = ((i + 2 * pp - kk) // ss + 1 for i, pp, kk, ss in zip((Ti, H, W), p, k, s))
    d.Co, d.ldy, d.Co_pad = Co, (Co + 7) // 8 * 8, (Co + 127) // 128 * 128
    return d


STEPS = [(2, 64), (16, 64), (1, None), (2, 9), (16, 33)]


def test_strided_supported_table():
    lib = L.lib()
    sup = lib.ptx_conv_stem_bf16_strided_supported
    for geom, Co in ((FAST, 8), (SLOW, 64)):
        for step, T_full in STEPS:
            T_full = 7 if T_full is None else T_full
            Ti = -(-T_full // step)
            d = _desc(geom, Co, Ti, 64, 64)
            for src in (BF16, U8):
                assert sup(C.byref(d), src, step, T_full) == 1, (Co, step, T_full, lib.ptx_last_error())
    d = _desc(FAST, 8, 32, 64, 64)
    assert sup(C.byref(d), BF16, 2, 64) == 1 and sup(C.byref(d), BF16, 2, 63) == 1       # ceil(63 / 2) == 32
    for why, args in {"frame_step": (0, 64), "ceil": (2, 62)}.items():
        assert sup(C.byref(d), BF16, *args) == 0, why
        assert why in lib.ptx_last_error().decode(), (why, lib.ptx_last_error())
    assert sup(C.byref(d), BF16, -1, 64) == 0 and sup(C.byref(d), BF16, 2, 66) == 0 and sup(C.byref(d), BF16, 1, 64) == 0
    assert sup(C.byref(d), BF16, 2, 0) == 0 and sup(C.byref(d), 2, 2, 64) == 0
    same = _desc(FAST, 8, 32, 64, 64)
    same.Ho, same.Wo, same.pH, same.pW = 32, 32, 2, 2                         # TF-SAME extents: front pad 2, back pad 3
    bad_sw = _desc((FAST[0], (1, 2, 3), FAST[2]), 8, 32, 64, 64)
    for why, bad in (("SAME", same), ("stride_w", bad_sw)):
        for src in (BF16, U8):
            assert sup(C.byref(bad), src, 2, 64) == 0, why
            assert why in lib.ptx_last_error().decode(), (why, lib.ptx_last_error())
    # (1, Ti) is the plain entry point's rule, refusal by refusal
    sample = [_desc(FAST, 8, 32, 64, 64), _desc(SLOW, 64, 2, 64, 64), _desc(SLOW, 83, 4, 30, 34), same, bad_sw,
              _desc(((7, 7, 7), (1, 2, 2), (3, 3, 3)), 64, 16, 224, 224, N=8), _desc(FAST, 8, 3, 1080, 1920, N=1),
              _desc(SLOW, 64, 1, 30000, 30000, N=1), _desc(((1, 7, 9), (1, 2, 2), (0, 3, 4)), 64, 4, 64, 64)]
    for d in sample:
        for src in (BF16, U8, 2):
            assert sup(C.byref(d), src, 1, d.Ti) == lib.ptx_conv_stem_bf16_supported(C.byref(d), src)


# --------------------------------------------------------------------------------------------- plans on the meta device
CASES = [("resnet50", "SF", 2), ("resnet50", "S", 1), ("resnet50", "F", 1), ("resnet18", "SF", 2)]


def _stems(plan):
    return [s for s in plan.steps if isinstance(s, StemBf16Step)]


def _expected_stems(mode, T):
    """[(label, frame_step, used frames, Co, kT)] in plan order: the fast pathway is compiled first."""
    fast, slow = ("fast.conv1", 2, -(-T // 2), 8, 5), ("slow.conv1", 16, -(-T // 16), 64, 1)
    return {"SF": [fast, slow], "S": [slow], "F": [fast]}[mode]


@pytest.mark.parametrize("arch,mode,n_stems", CASES)
def test_dry_plan_under_direct(arch, mode, n_stems):
    lib = L.lib()
    model = _model(arch, mode)
    plan = _direct_engine().dry_plan(model, SHAPE)
    N, _, T, H, W = SHAPE
    assert plan.bf16 and plan.bf16_stem == "direct"
    for a in plan.acts:
        assert a.bf16 and a.t.dtype == torch.bfloat16 and a.ld % 8 == 0
    stems = _stems(plan)
    assert len(stems) == n_stems and plan.stem_steps == n_stems and plan.stem_bf16_step is None
    want = _expected_stems(mode, T)
    for st, (label, step, used, Co, kT) in zip(stems, want):
        d = st.d
        assert (st.label, st.frame_step, st.T_full, d.Ti, d.Co, d.ldy, d.kT) == (label, step, T, used, Co, Co, kT)
        assert (d.N, d.To, d.Ho, d.Wo) == (N, used, H // 2, W // 2)
        assert st.src == BF16 and st.norm is None and st.kernel == "conv_stem_bf16"
        assert lib.ptx_conv_stem_bf16_strided_supported(C.byref(d), st.src, st.frame_step, st.T_full) == 1
        # compulsory traffic: ceil(T / step) frames of the clip in, the bf16 activation out, the re-laid filter
        w_elems = lib.ptx_stem_bf16_weight_elems(C.byref(d))
        assert st.hbm_bytes == 2 * N * 3 * used * H * W + 2 * N * used * (H // 2) * (W // 2) * d.ldy + 2 * w_elems
        assert st.macs == N * used * (H // 2) * (W // 2) * Co * 3 * kT * 49
    labels = [getattr(s, "label", "") for s in plan.steps]
    assert "im2col_hw_bf16" not in labels and "fold_kw" not in labels and "frames_u8_to_ncdhw" not in labels
    assert not plan.chain_steps and not plan.alt_steps and not plan.program_steps and not plan.wino_steps and not plan.wino4_steps
    assert not any(isinstance(s, (AltStep, ChainStep, ProgramStep)) for s in plan.steps)
    for st in plan.conv_steps:
        assert isinstance(st, ConvStep) and st.x2 is None
        assert st.d.flags & L.PTX_BF16_OPERANDS and st.d.flags & L.PTX_F16_OPERANDS and st.d.flags & L.PTX_EPI_OUT_F16, st.label
        assert lib.ptx_conv3d_config_name(st.cfg).decode().endswith("/bf16"), st.label
    # shortcut B: its own conv, then a fused residual add in the block's last conv
    tail = "conv3" if arch == "resnet50" else "conv2"
    by_label = {s.label: s for s in plan.conv_steps}
    path = "fast" if mode == "F" else "slow"
    assert path + ".res2.0.downsample" in by_label
    assert by_label["%s.res2.0.%s" % (path, tail)].d.flags & L.PTX_EPI_RES_ADD
    laterals = [s for s in plan.conv_steps if s.label.startswith("fast.lateral")]
    assert len(laterals) == (4 if mode == "SF" else 0)
    if mode == "SF":
        exp = 4 if arch == "resnet50" else 1
        mains = [64, 64 * exp, 128 * exp, 256 * exp]
        seen = set()
        for lat, main_C in zip(laterals, mains):
            # the lateral conv writes [main_C, main_C + Co) of its stage's concatenated buffer: base + main_C bf16 elements
            # (on the meta device a buffer's base is 0 and a view's pointer is its byte offset)
            dims = (lat.d.N, lat.d.To, lat.d.Ho, lat.d.Wo)
            cats = [a for a in plan.acts if (a.N, a.T, a.H, a.W, a.C) == dims + (main_C + lat.d.Co,) and id(a) not in seen]
            assert len(cats) >= 1, lat.label                   # (resnet18: stages 0 and 1 have equal shapes; plan order)
            cat = cats[0]
            seen.add(id(cat))
            base = (cat.t.data_ptr() or 0)
            assert (lat.y.value or 0) == base + 2 * main_C and lat.d.ldy == cat.ld == main_C + lat.d.Co and main_C % 8 == 0
            assert (lat.d.kT, lat.d.sT) == (5, 8)
        # ... and the slow pathway's stage outputs write [0, main_C) of the same rows (the max pool writes the first buffer's)
        wide = [s for s in plan.conv_steps if s not in laterals and s.d.ldy != (s.d.Co + 7) // 8 * 8]
        assert [(s.label, s.d.Co, s.d.ldy, s.y.value or 0) for s in wide] == [
            ("slow.res%d.%d.%s" % (i + 2, n - 1, tail), mains[i + 1], mains[i + 1] + laterals[i + 1].d.Co, 0)
            for i, n in enumerate(model.slow.layers[:3])]
        assert plan.head is not None and tuple(plan.pooled.shape) == (N, 512 * exp + 64 * exp)
    else:
        assert plan.head is None and tuple(plan.pooled.shape) == (N, (512 if mode == "S" else 64) * (4 if arch == "resnet50" else 1))
    assert plan.pooled.dtype == torch.float32


def test_dry_plan_other_strides_and_ragged_t():
    model = _model("resnet50", "SF", slow_stride=8, fast_stride=1)
    stems = _stems(_direct_engine().dry_plan(model, (2, 3, 16, 64, 64)))
    assert [(s.frame_step, s.T_full, s.d.Ti) for s in stems] == [(1, 16, 16), (8, 16, 2)]
    stems = _stems(_direct_engine().dry_plan(_model("resnet50", "SF"), (2, 3, 35, 64, 64)))
    assert [(s.frame_step, s.T_full, s.d.Ti) for s in stems] == [(2, 35, 18), (16, 35, 3)]


def test_plan_from_uint8_frames():
    norm = L.NormDesc.make([0.485, 0.456, 0.406], [0.229, 0.224, 0.225], "BGR", (0, 255))
    model = _model("resnet50", "SF")
    plan = ptx.engine.Plan(_direct_engine(), model, SHAPE, torch.device("meta"), norm)
    stems = _stems(plan)
    N, _, T, H, W = SHAPE
    assert len(stems) == 2 and all(s.src == U8 and s.norm is norm for s in stems)
    assert [(s.frame_step, s.T_full) for s in stems] == [(2, T), (16, T)]
    labels = [getattr(s, "label", "") for s in plan.steps]
    assert "frames_u8_to_ncdhw" not in labels and "im2col_hw_bf16" not in labels and "fold_kw" not in labels
    for s in stems:           # one byte per sample of the frames that are read
        w_elems = L.lib().ptx_stem_bf16_weight_elems(C.byref(s.d))
        assert s.hbm_bytes == N * 3 * s.d.Ti * H * W + 2 * N * s.d.Ti * (H // 2) * (W // 2) * s.d.ldy + 2 * w_elems
    with pytest.raises(PtxError, match="bf16"):
        ptx.engine.Plan(Engine(), model, SHAPE, torch.device("meta"), norm)


# --------------------------------------------------------------------------------------------- what keeps raising
@pytest.mark.parametrize("arch,mode", [("resnet50", "SF"), ("resnet50", "S"), ("resnet50", "F"), ("resnet18", "SF")])
def test_default_engine_refuses_every_mode(arch, mode):
    eng = Engine()
    assert eng.bf16_stem == "fold"
    with pytest.raises(PtxError, match="bf16") as e:
        eng.dry_plan(_model(arch, mode), SHAPE)
    assert "bf16_stem = 'direct'" in str(e.value) and "PTX_BF16_STEM" in str(e.value)


def test_unaligned_lateral_offset_raises():
    """A user-edited slow stem of 60 channels puts the first lateral slice at a 120-byte offset: refused at plan build."""
    import torch.nn as nn
    model = ptx.slowfast.resnet50(mode="SF", num_classes=51)
    model.slow.conv1 = nn.Conv3d(3, 60, (1, 7, 7), (1, 2, 2), (0, 3, 3), bias=False)
    model.slow.bn1 = nn.BatchNorm3d(60)
    model = model.eval().to(torch.bfloat16)
    with pytest.raises(PtxError, match="8-channel"):
        _direct_engine().dry_plan(model, SHAPE)


def test_other_families_stay_out_of_scope_under_direct():
    m = ptx.i3d(num_classes=51, pretrained=None).eval().to(torch.bfloat16)
    with pytest.raises(PtxError, match="bf16"):
        _direct_engine().dry_plan(m, (1, 3, 16, 224, 224))
    m = ptx.resnext3d50(num_classes=51).eval().to(torch.bfloat16)
    with pytest.raises(PtxError, match="bf16"):
        _direct_engine().dry_plan(m, (1, 3, 8, 64, 64))
