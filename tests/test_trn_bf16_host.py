"""bf16 TRN and 2-D ResNets, host side (no GPU): plans of the 2-D ResNets compiled on the 'meta' device under
Engine.bf16_stem = "direct", what keeps raising, the ABI of include/ptx_amd_linear_bf16.h and the refusals of its `_supported`
twins (made on the host: dummy addresses are never read)."""
import ctypes as C
import hashlib
import os
import re

import pytest
import torch

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import AltStep, ChainStep, ConvStep, Engine, PtxError, StemBf16Step
from pretorched_x_amd.plan import BF16_FAMILIES_2D

NAMES = ["ptx_linear_bf16w_fwd", "ptx_linear_bf16w_supported", "ptx_linear_bf16w_workspace_bytes", "ptx_linear_setsum_bf16w_fwd",
         "ptx_linear_setsum_bf16w_supported", "ptx_relation_linear_bf16w_fwd", "ptx_relation_linear_bf16w_supported"]
SHAPE = (2, 3, 64, 64)
ROOT = os.path.dirname(os.path.dirname(L.HEADER_PATH))


def _direct_engine():
    eng = Engine()
    eng.bf16_stem = "direct"
    return eng


def _model(name, **kw):
    return ptx.__dict__[name](num_classes=51, pretrained=None, **kw).eval()


def _convs(plan):
    out = []
    for s in plan.steps:
        for t in (s.active() if isinstance(s, AltStep) else [s]):
            if isinstance(t, (ConvStep, ChainStep)):
                out.append(t)
    return out


# --------------------------------------------------------------------------------------------- plans
@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_dry_plan_bf16_2d_direct(name):
    assert name in BF16_FAMILIES_2D
    m = _model(name).to(torch.bfloat16)
    plan = _direct_engine().dry_plan(m, SHAPE)
    stems = [s for s in plan.steps if isinstance(s, StemBf16Step)]
    assert len(stems) == 1 and stems[0].d.kT == 1 and stems[0].d.Ti == 1 and stems[0].d.To == 1
    assert (stems[0].d.kH, stems[0].d.kW, stems[0].d.sH, stems[0].d.sW, stems[0].d.Co) == (7, 7, 2, 2, 64)
    assert stems[0].src == L.PTX_STEM_SRC_BF16_NCDHW
    convs = _convs(plan)
    assert len(convs) >= 16
    for c in convs:
        descs = [c.d] if isinstance(c, ConvStep) else [c.d, c.d2]
        for d in descs:
            assert d.flags & L.PTX_BF16_OPERANDS and d.flags & L.PTX_F16_OPERANDS, c.label
    assert plan.bf16 and all(a.bf16 for a in plan.acts)
    assert all(a.t.dtype == torch.bfloat16 for a in plan.acts)
    assert tuple(plan.pooled.shape) == (2, 512 if name == "resnet18" else 2048) and plan.pooled.dtype == torch.float32


@pytest.mark.parametrize("name", ["resnet18", "resnet50"])
def test_dry_plan_bf16_2d_fold_raises_naming_the_switch(name):
    m = _model(name).to(torch.bfloat16)
    with pytest.raises(PtxError) as e:
        Engine().dry_plan(m, SHAPE)
    assert "bf16_stem = 'direct'" in str(e.value) and "PTX_BF16_STEM" in str(e.value)


def test_uint8_frames_plan_under_direct():
    m = _model("resnet18").to(torch.bfloat16)
    norm = L.NormDesc.make([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    from pretorched_x_amd.plan import Plan
    plan = Plan(_direct_engine(), m, SHAPE, torch.device("meta"), norm)
    stems = [s for s in plan.steps if isinstance(s, StemBf16Step)]
    assert len(stems) == 1 and stems[0].src == L.PTX_STEM_SRC_U8_NTHWC and stems[0].d.kT == 1


def test_still_out_of_scope_under_direct():
    for name, shape in (("resnext3d50", (1, 3, 8, 64, 64)), ("i3d", (1, 3, 16, 224, 224))):
        m = (ptx.i3d(num_classes=51, pretrained=None) if name == "i3d" else ptx.__dict__[name](num_classes=51)).eval()
        with pytest.raises(PtxError, match="bf16"):
            _direct_engine().dry_plan(m.to(torch.bfloat16), shape)
    m = _model("resnet18").to(torch.bfloat16)
    m.arch_name = "adopted:ResNet"                       # an adopted 2-D instance is not one of the families
    with pytest.raises(PtxError, match="bf16"):
        _direct_engine().dry_plan(m, SHAPE)
    with pytest.raises(PtxError, match="fp16"):
        _direct_engine().dry_plan(_model("resnet18").half(), SHAPE)


def test_fp32_plan_unchanged():
    for eng in (Engine(), _direct_engine()):
        plan = eng.dry_plan(_model("resnet50"), SHAPE)
        assert not plan.bf16 and not any(isinstance(s, StemBf16Step) for s in plan.steps)
        assert all(not a.bf16 and a.t.dtype == torch.float32 for a in plan.acts)
        for c in _convs(plan):
            for d in ([c.d] if isinstance(c, ConvStep) else []):
                assert not d.flags & L.PTX_BF16_OPERANDS


# --------------------------------------------------------------------------------------------- the C ABI
def test_header_bindings_and_exports_agree():
    text = open(L.LINEAR_BF16_HEADER_PATH).read()
    declared = L.header_symbols(L.LINEAR_BF16_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_LINEAR_BF16) == NAMES
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.SIGNATURES_YUV16, L.SIGNATURES_COLOR,
                  L.SIGNATURES_RANDAUG, L.SIGNATURES_RESAMPLE, L.SIGNATURES_MIX, L.SIGNATURES_STEM_STRIDED, L.SIGNATURES_NL_KS,
                  L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_LINEAR_BF16[name][0], list(L.SIGNATURES_LINEAR_BF16[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_LINEAR_BF16[name][1]), name
    # the gather / set-sum entry points are their fp32 twins' signatures (+ workspace pointer and size for the gather)
    rel, ss = L.SIGNATURES["ptx_relation_linear_fwd"], L.SIGNATURES["ptx_linear_setsum_fwd"]
    assert list(L.SIGNATURES_LINEAR_BF16["ptx_relation_linear_bf16w_fwd"][1]) == list(rel[1][:-1]) + [C.c_void_p, C.c_size_t, C.c_void_p]
    assert list(L.SIGNATURES_LINEAR_BF16["ptx_linear_setsum_bf16w_fwd"][1]) == list(ss[1])
    assert (L.PTX_LIN_X_BF16, L.PTX_LIN_X_F32) == (0, 1)
    assert re.search(r"#define\s+PTX_LIN_X_BF16\s+0\b", plain) and re.search(r"#define\s+PTX_LIN_X_F32\s+1\b", plain)
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ptx_amd_linear_bf16.h" in integ and all(n in integ for n in declared)
    # the build: the header is hashed into the version and is a dependency of the object that holds the kernels
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert any(h.endswith("ptx_amd_linear_bf16.h") for h in build.HEADERS)
    files = build.tu_files("pool_head.hip")
    assert any(p.endswith("linear_bf16.hip") for p in files) and any(p.endswith("ptx_amd_linear_bf16.h") for p in files)
    assert L.binary_source_hash() == L.source_hash()


def test_ptx_amd_h_is_the_parents():
    """include/ptx_amd.h and its symbol census do not move: the file has the bytes of the commit this feature was built on."""
    with open(L.HEADER_PATH, "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == "025c96c09bfd02b38b62b314a4e119d17cc1ed05cd5e6791279bd7cca75de43b"
    assert not set(NAMES) & set(L.header_symbols())


def test_workspace_is_a_function_of_the_extents():
    ws = L.lib().ptx_linear_bf16w_workspace_bytes
    assert ws(1, 8, 1) == 0 and ws(8, 256, 1024) == 0                    # one slab: no split
    big = ws(24, 16384, 1024)
    assert big > 0 and big % (24 * 1024 * 4) == 0 and big // (24 * 1024 * 4) <= 64
    assert ws(8, 16384, 1024) * 3 == big                                 # 8 and 24 rows are one row group: same split
    assert ws(0, 8, 1) == 0 and ws(8, 0, 1) == 0 and ws(8, 8, -1) == 0


FAKE = C.c_void_p(1 << 20)


def _err():
    return L.lib().ptx_last_error().decode()


def test_dense_supported_refusals():
    lib = L.lib()
    sup = lib.ptx_linear_bf16w_supported
    assert sup(FAKE, 0, FAKE, FAKE, FAKE, 8, 2048, 96, 2048, 96, 0) == 1
    assert sup(FAKE, 1, FAKE, None, FAKE, 5, 37, 7, 37, 9, L.PTX_PRO_RELU | L.PTX_EPI_RELU | L.PTX_EPI_ACCUM) == 1
    for args, word in (((None, 0, FAKE, FAKE, FAKE, 8, 64, 8, 64, 8, 0), "null"),
                       ((FAKE, 0, None, FAKE, FAKE, 8, 64, 8, 64, 8, 0), "null"),
                       ((FAKE, 0, FAKE, FAKE, None, 8, 64, 8, 64, 8, 0), "null"),
                       ((FAKE, 2, FAKE, FAKE, FAKE, 8, 64, 8, 64, 8, 0), "x_kind"),
                       ((FAKE, 0, FAKE, FAKE, FAKE, 8, 64, 8, 63, 8, 0), "ldx"),
                       ((FAKE, 0, FAKE, FAKE, FAKE, 8, 64, 8, 64, 7, 0), "ldy"),
                       ((FAKE, 0, FAKE, FAKE, FAKE, 0, 64, 8, 64, 8, 0), "extent"),
                       ((FAKE, 0, FAKE, FAKE, FAKE, 8, 64, 8, 64, 8, L.PTX_EPI_RES_ADD), "flags"),
                       ((C.c_void_p((1 << 20) + 2), 1, FAKE, FAKE, FAKE, 8, 64, 8, 64, 8, 0), "aligned")):
        assert sup(*args) == 0 and word in _err(), (args, _err())
    # the launch makes the same checks first, and asks for its workspace before it touches a pointer
    assert lib.ptx_linear_bf16w_fwd(FAKE, 0, FAKE, FAKE, FAKE, 8, 64, 8, 63, 8, 0, None, 0, None) == 1 and "ldx" in _err()
    assert lib.ptx_linear_bf16w_fwd(FAKE, 0, FAKE, FAKE, FAKE, 24, 4096, 339, 4096, 339, 0, None, 0, None) == 4
    assert "workspace" in _err()


def _rel(B=3, n_sets=2, n_frames=2, frame_len=264):
    d = L.RelationDesc()
    d.B, d.n_sets, d.n_frames, d.frame_len = B, n_sets, n_frames, frame_len
    for r in range(min(n_sets, L.PTX_REL_MAX_SETS)):
        for f in range(min(n_frames, L.PTX_REL_MAX_FRAMES)):
            d.idx[r][f] = (r + f) % 8
    return d


def test_gather_supported_refusals():
    lib = L.lib()
    sup = lib.ptx_relation_linear_bf16w_supported
    ok = _rel()
    assert sup(C.byref(ok), FAKE, 8 * 264, FAKE, FAKE, FAKE, 96, 96, L.PTX_PRO_RELU | L.PTX_EPI_RELU) == 1
    assert sup(C.byref(_rel(frame_len=260)), FAKE, 8 * 260, FAKE, FAKE, FAKE, 96, 96, 0) == 0 and "frame_len" in _err()
    assert sup(C.byref(_rel(frame_len=0)), FAKE, 8 * 264, FAKE, FAKE, FAKE, 96, 96, 0) == 0 and "frame_len" in _err()
    assert sup(None, FAKE, 8 * 264, FAKE, FAKE, FAKE, 96, 96, 0) == 0 and "null" in _err()
    assert sup(C.byref(ok), None, 8 * 264, FAKE, FAKE, FAKE, 96, 96, 0) == 0 and "null" in _err()
    assert sup(C.byref(ok), FAKE, 8 * 264, FAKE, FAKE, None, 96, 96, 0) == 0 and "null" in _err()
    assert sup(C.byref(ok), FAKE, 8 * 264 + 4, FAKE, FAKE, FAKE, 96, 96, 0) == 0 and "ldx" in _err()
    assert sup(C.byref(ok), FAKE, 2 * 264, FAKE, FAKE, FAKE, 96, 96, 0) == 0 and "outside" in _err()         # frame 2 of a 2-frame video
    assert sup(C.byref(ok), FAKE, 8 * 264, FAKE, FAKE, FAKE, 96, 95, 0) == 0 and "ldy" in _err()
    assert sup(C.byref(_rel(n_sets=L.PTX_REL_MAX_SETS + 1)), FAKE, 8 * 264, FAKE, FAKE, FAKE, 96, 96, 0) == 0 and "subsets" in _err()
    assert sup(C.byref(_rel(n_frames=L.PTX_REL_MAX_FRAMES + 1)), FAKE, 32 * 264, FAKE, FAKE, FAKE, 96, 96, 0) == 0
    neg = _rel()
    neg.idx[1][1] = -1
    assert sup(C.byref(neg), FAKE, 8 * 264, FAKE, FAKE, FAKE, 96, 96, 0) == 0 and "negative" in _err()
    assert sup(C.byref(ok), C.c_void_p((1 << 20) + 8), 8 * 264, FAKE, FAKE, FAKE, 96, 96, 0) == 0 and "misaligned" in _err()
    assert lib.ptx_relation_linear_bf16w_fwd(C.byref(_rel(frame_len=260)), FAKE, 8 * 260, FAKE, FAKE, FAKE, 96, 96, 0, None, 0, None) == 1


def test_setsum_supported_refusals():
    lib = L.lib()
    sup = lib.ptx_linear_setsum_bf16w_supported
    assert sup(FAKE, FAKE, FAKE, FAKE, 3, 3, 264, 96, 264, 96, L.PTX_EPI_ACCUM) == 1
    assert sup(None, FAKE, FAKE, FAKE, 3, 3, 264, 96, 264, 96, 0) == 0 and "null" in _err()
    assert sup(FAKE, FAKE, FAKE, None, 3, 3, 264, 96, 264, 96, 0) == 0 and "null" in _err()
    assert sup(FAKE, FAKE, FAKE, FAKE, 3, 0, 264, 96, 264, 96, 0) == 0 and "extent" in _err()
    assert sup(FAKE, FAKE, FAKE, FAKE, 3, 3, 264, 96, 263, 96, 0) == 0 and "ldx" in _err()
    assert sup(FAKE, FAKE, FAKE, FAKE, 3, 3, 264, 96, 264, 95, 0) == 0 and "ldy" in _err()
    assert lib.ptx_linear_setsum_bf16w_fwd(FAKE, FAKE, FAKE, FAKE, 3, 3, 264, 96, 263, 96, 0, None) == 1 and "ldx" in _err()


# --------------------------------------------------------------------------------------------- heads, without a launch
def test_heads_refuse_dtype_mismatch_on_the_host():
    """The dtype rule is checked before anything is launched: CPU tensors are enough to see both refusals."""
    from pretorched_x_amd import heads
    lin16 = torch.nn.Linear(16, 4).to(torch.bfloat16)
    lin32 = torch.nn.Linear(16, 4)
    with pytest.raises(PtxError, match="bfloat16"):
        heads._bf16_head("linear", torch.zeros(2, 16), lin16)
    with pytest.raises(PtxError, match="bfloat16"):
        heads._bf16_head("linear", torch.zeros(2, 16, dtype=torch.bfloat16), lin32)
    assert heads._bf16_head("linear", torch.zeros(2, 16), lin32) is False


def test_trn_forward_views_names_the_switch():
    m = ptx.TRN(51, num_segments=4, arch="resnet18", consensus="TRN", frame_bottleneck_dim=128, video_feature_dim=64,
                pretrained=None).eval().to(torch.bfloat16)
    assert m.base_model.engine().bf16_stem == os.environ.get("PTX_BF16_STEM", "fold")
    if m.base_model.engine().bf16_stem != "direct":
        with pytest.raises(PtxError, match="bf16_stem = 'direct'"):
            m.forward_views(torch.zeros(1, 8, 64, 64, 3, dtype=torch.uint8), views=None)
