"""bf16 non-local ResNets (nonlocalresnet3d*, nonlocal_r2plus1d50) and the key-split form of the bf16 attention kernel, host side
(no GPU): plans compiled on the 'meta' device under Engine.bf16_stem = "direct", what keeps raising, and the ABI of
include/ptx_amd_nl_ks.h."""
import ctypes as C
import os
import re

import pytest
import torch

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import Engine, PtxError, StemBf16Step

SHAPE = (1, 3, 8, 64, 64)
NAMES = ["ptx_nonlocal_bf16_variant", "ptx_nonlocal_bf16_variant_fwd", "ptx_nonlocal_bf16_variant_supported"]


def _direct_engine():
    eng = Engine()
    eng.bf16_stem = "direct"
    return eng


def _make(name, **kw):
    if name == "nonlocalresnet3d50":
        kw = dict(pretrained=None, **kw)
    elif name == "nonlocal_r2plus1d50":
        kw = dict(num_classes=339, **kw)
    return ptx.__dict__[name](**kw).eval().to(torch.bfloat16)


def _labels(plan):
    return [getattr(st, "tag", None) or getattr(st, "label", None) for st in plan.steps]


# --------------------------------------------------------------------------------------------- plans on the meta device
@pytest.mark.parametrize("name,kw,n_attn", [("nonlocalresnet3d50", {}, 5), ("nonlocal_r2plus1d50", {}, 5),
                                            ("nonlocalresnet3d50", {"shortcut_type": "B"}, 5),
                                            ("nonlocalresnet3d50", {"num_nonlocal_blocks": 10}, 10),
                                            ("nonlocalresnet3d18", {"nonlocal_layers": [0, 1, 1, 0]}, 2)])
def test_dry_plan_under_direct(name, kw, n_attn):
    lib = L.lib()
    plan = _direct_engine().dry_plan(_make(name, **kw), SHAPE)
    assert plan.bf16 and plan.precision == "bf16" and plan.bf16_stem == "direct"
    labels = _labels(plan)
    assert labels.count("nonlocal_attention") == n_attn and plan.attn_steps == n_attn, labels
    assert "nonlocal_unfused" not in labels and "nonlocal_concat_ab" not in labels
    assert isinstance(plan.steps[0], StemBf16Step) and plan.stem_steps == 1
    assert "im2col_hw_bf16" not in labels and "fold_kw" not in labels
    for a in plan.acts:                                   # no fp32 activation anywhere
        assert a.bf16 and a.t.dtype == torch.bfloat16 and a.ld % 8 == 0, (a.C, a.ld, a.t.dtype)
    assert plan.feat.bf16
    assert len(plan.attn_descs) == len(plan.attn_variants) == len(plan.attn_operands) == n_attn
    for d, v, ops in zip(plan.attn_descs, plan.attn_variants, plan.attn_operands):
        assert d.mode & L.PTX_NL_BF16 and lib.ptx_nonlocal_supported(C.byref(d))
        assert v == lib.ptx_nonlocal_bf16_variant(C.byref(d)) and lib.ptx_nonlocal_bf16_variant_supported(C.byref(d), v)
        assert all(a.bf16 and a.ld % 8 == 0 and a.t.storage_offset() % 8 == 0 for a in ops)
    if n_attn == 5:
        # layer2.{0,2}: 512 channels at 2 x 8 x 8 positions, d = dv = 256; layer3.{0,2,4}: 1024 channels at 1 x 4 x 4, d = dv = 512
        assert [(d.d, d.dv) for d in plan.attn_descs] == [(256, 256)] * 2 + [(512, 512)] * 3
        assert [(d.Nq, d.Nk) for d in plan.attn_descs] == [(128, 128)] * 2 + [(16, 16)] * 3
    for st in plan.conv_steps:
        assert st.d.flags & L.PTX_BF16_OPERANDS and st.d.flags & L.PTX_EPI_OUT_F16, st.label
        assert lib.ptx_conv3d_config_name(st.cfg).decode().endswith("/bf16"), st.label


def test_dry_plan_records_the_forced_variant(monkeypatch):
    """attn_variants is the dispatcher's answer at build time: PTX_NL_BF16_KSPLIT=1 turns every d <= 256 launch to the key
    split and leaves the d = 512 launches of layer3 single-group."""
    monkeypatch.setenv("PTX_NL_BF16_KSPLIT", "1")
    plan = _direct_engine().dry_plan(_make("nonlocal_r2plus1d50"), SHAPE)
    assert plan.attn_variants == [1, 1, 0, 0, 0]
    monkeypatch.setenv("PTX_NL_BF16_KSPLIT", "0")
    plan = _direct_engine().dry_plan(_make("nonlocal_r2plus1d50"), SHAPE)
    assert plan.attn_variants == [0] * 5


@pytest.mark.parametrize("name", ["nonlocalresnet3d50", "nonlocal_r2plus1d50"])
def test_default_engine_still_raises_and_names_the_switch(name):
    eng = Engine()
    eng.bf16_stem = "fold"
    with pytest.raises(PtxError, match="bf16") as e:
        eng.dry_plan(_make(name), SHAPE)
    assert "bf16_stem = 'direct'" in str(e.value) and "PTX_BF16_STEM=direct" in str(e.value)


@pytest.mark.parametrize("name,shape", [("resnext3d50", SHAPE), ("wideresnet3d50", SHAPE), ("preact_resnet3d50", SHAPE),
                                        ("resneti3d50", SHAPE), ("i3d", (1, 3, 16, 224, 224))])
def test_others_still_raise_under_direct(name, shape):
    try:
        m = ptx.__dict__[name](num_classes=339, pretrained=None)
    except TypeError:                                     # (factories without a `pretrained` argument, as upstream)
        m = ptx.__dict__[name](num_classes=339)
    with pytest.raises(PtxError, match="bf16"):
        _direct_engine().dry_plan(m.eval().to(torch.bfloat16), shape)


def test_adopted_nonlocal_still_raises_under_direct():
    m = _make("nonlocalresnet3d50")
    m.arch_name = "adopted:NonLocalResNet3D"
    with pytest.raises(PtxError, match="bf16"):
        _direct_engine().dry_plan(m, SHAPE)


# --------------------------------------------------------------------------------------------- the C ABI
def _desc(d, dv=None, ld=None, mode=None, batch=2, Nq=100, Nk=50):
    dv = d if dv is None else dv
    ld = (max(d, dv) + 7) // 8 * 8 if ld is None else ld
    x = L.NonlocalDesc()
    x.batch, x.Nq, x.Nk, x.d, x.dv = batch, Nq, Nk, d, dv
    x.ld_theta = x.ld_phi = x.ld_g = x.ld_y = ld
    x.bs_theta = x.bs_y = Nq * ld
    x.bs_phi = x.bs_g = Nk * ld
    x.mode = (L.PTX_NL_BF16 | L.PTX_NL_SOFTMAX) if mode is None else mode
    return x


def test_header_bindings_and_exports_agree():
    text = open(L.NL_KS_HEADER_PATH).read()
    declared = L.header_symbols(L.NL_KS_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_NL_KS) == NAMES
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.SIGNATURES_YUV16, L.SIGNATURES_COLOR,
                  L.SIGNATURES_RANDAUG, L.SIGNATURES_RESAMPLE, L.SIGNATURES_MIX, L.SIGNATURES_STEM_STRIDED, L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_NL_KS[name][0], list(L.SIGNATURES_NL_KS[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_NL_KS[name][1]), name
    # variant_fwd is ptx_nonlocal_bf16_fwd's signature with the variant after the descriptor
    fwd = L.SIGNATURES["ptx_nonlocal_bf16_fwd"]
    assert list(L.SIGNATURES_NL_KS["ptx_nonlocal_bf16_variant_fwd"][1]) == list(fwd[1][:1]) + [C.c_int32] + list(fwd[1][1:])
    root = os.path.dirname(os.path.dirname(L.HEADER_PATH))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "ptx_amd_nl_ks.h" in integ and all(n in integ for n in declared)
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert len(build.SOURCES) == 10 and any(h.endswith("ptx_amd_nl_ks.h") for h in build.HEADERS)
    assert any(p.endswith("ptx_amd_nl_ks.h") for p in build.tu_files("nonlocal_attn.hip"))
    assert L.binary_source_hash() == L.source_hash()


def test_variant_rule_reads_per_sample_extents_only(monkeypatch):
    lib = L.lib()
    var = lambda d: lib.ptx_nonlocal_bf16_variant(C.byref(d))
    sup = lambda d, v: lib.ptx_nonlocal_bf16_variant_supported(C.byref(d), v)
    for env in (None, "0", "1"):
        if env is None:
            monkeypatch.delenv("PTX_NL_BF16_KSPLIT", raising=False)
        else:
            monkeypatch.setenv("PTX_NL_BF16_KSPLIT", env)
        for d, N in ((256, 1568), (256, 3136), (256, 784), (256, 128), (64, 4096), (512, 196), (1024, 392), (10, 64)):
            answers = {var(_desc(d, batch=b, Nq=N, Nk=N)) for b in (1, 2, 3, 8, 64)}
            assert len(answers) == 1, (env, d, N, answers)
            v = answers.pop()
            assert v in (0, 1) and sup(_desc(d, Nq=N, Nk=N), v)
            if env is not None and d <= 256:
                assert v == int(env), (env, d, N)              # the switch flips the form wherever it is supported
            if d > 256:
                assert v == 0
    # Nq is not an input of the rule either
    monkeypatch.delenv("PTX_NL_BF16_KSPLIT", raising=False)
    assert var(_desc(256, Nq=64, Nk=1568)) == var(_desc(256, Nq=100000, Nk=1568))


def test_variant_supported_table():
    lib = L.lib()
    sup = lambda d, v: lib.ptx_nonlocal_bf16_variant_supported(C.byref(d), v)
    for d in (3, 8, 32, 64, 100, 128, 256):
        for dv in (3, 64, 128, 256, 512):
            for mode in (L.PTX_NL_SOFTMAX, L.PTX_NL_SCALE, L.PTX_NL_SCALE | L.PTX_NL_RELU):
                x = _desc(d, dv, mode=L.PTX_NL_BF16 | mode)
                assert sup(x, 0) == 1 and sup(x, 1) == 1, (d, dv, mode)
    for d in (264, 512, 1024):
        assert sup(_desc(d), 0) == 1 and sup(_desc(d), 1) == 0
    assert sup(_desc(256), 2) == 0 and sup(_desc(256), -1) == 0
    for v in (0, 1):
        assert sup(_desc(64, mode=L.PTX_NL_SOFTMAX), v) == 0           # an fp32 descriptor
        assert sup(_desc(64, mode=L.PTX_NL_SCALE | L.PTX_NL_X3), v) == 0
        assert sup(_desc(1032), v) == 0                                 # what ptx_nonlocal_supported refuses
        assert sup(_desc(64, ld=68), v) == 0
        assert lib.ptx_nonlocal_bf16_variant_supported(None, v) == 0
    assert lib.ptx_nonlocal_bf16_variant(None) == 0
    assert lib.ptx_nonlocal_bf16_variant(C.byref(_desc(64, mode=L.PTX_NL_SOFTMAX))) == 0


def test_variant_fwd_refuses_before_touching_a_pointer():
    """Dummy addresses are never read: every refusal happens on the host."""
    lib = L.lib()
    fake = C.c_void_p(1 << 20)
    fwd = lib.ptx_nonlocal_bf16_variant_fwd
    for d, v in ((512, 1), (1024, 1), (256, 2), (256, -1)):
        rc = fwd(C.byref(_desc(d)), v, fake, fake, fake, fake, None)
        assert rc == 2 and b"variant" in lib.ptx_last_error(), (d, v, rc, lib.ptx_last_error())        # PTX_ERR_UNSUPPORTED
    for v in (0, 1):
        rc = fwd(C.byref(_desc(64, mode=L.PTX_NL_SOFTMAX)), v, fake, fake, fake, fake, None)
        assert rc == 1 and b"PTX_NL_BF16" in lib.ptx_last_error()
        assert fwd(C.byref(_desc(1032)), v, fake, fake, fake, fake, None) == 2
        assert fwd(C.byref(_desc(64)), v, None, fake, fake, fake, None) == 1
        assert fwd(C.byref(_desc(64)), v, C.c_void_p((1 << 20) + 2), fake, fake, fake, None) == 1
