"""update_bn, host side (no GPU): the fixture against its generator, batch-statistics plans compiled on the 'meta' device,
what raises, and the ABI of include/ptx_amd_bn.h."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import AltStep, ChainStep, ConvStep, Engine, PackedDual, ProgramStep, PtxError, _WinoExec
from pretorched_x_amd.steps import BnApplyStep, BnStatsStep, BnUpdateStep

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ["ptx_bn_apply_f32", "ptx_bn_batch_stats_f32", "ptx_bn_batch_stats_workspace_bytes", "ptx_bn_batch_update_f32"]


def _golden_module():
    spec = importlib.util.spec_from_file_location("make_update_bn_golden", os.path.join(HERE, "golden", "make_update_bn_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _golden_module()


def _model(name, **kw):
    factory = getattr(ptx, name)
    try:
        return factory(num_classes=51, pretrained=None, **kw).eval()
    except TypeError:
        return factory(num_classes=51, **kw).eval()


# --------------------------------------------------------------------------------------------- the fixture
def test_fixture_matches_its_generator():
    file = G.load()
    assert sorted(file) == sorted(G.CASES)
    for name, rec in file.items():
        assert rec["spec"] == _jsonable(G.CASES[name])
    rec = file["resnet3d18"]
    mean, var, tracked, logits = G.reference(rec["spec"])
    assert np.array_equal(tracked, rec["tracked"]) and set(tracked.tolist()) == {2}
    for got, want in ((mean, rec["mean"]), (var, rec["var"]), (logits, rec["logits"])):
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert os.path.getsize(G.PATH) < 796 * 1024


def _jsonable(spec):
    import json
    return json.loads(json.dumps(spec))


# --------------------------------------------------------------------------------------------- plans
@pytest.mark.parametrize("lanes", ["auto", 2])
@pytest.mark.parametrize("name,shape", [("resnet3d50", (4, 3, 8, 64, 64)), ("r2plus1d18", (4, 3, 8, 64, 64)),
                                        ("preact_resnet3d50", (4, 3, 8, 64, 64)), ("resnet18", (4, 3, 64, 64))])
def test_dry_plan_batch_stats(name, shape, lanes):
    m = _model(name)
    eng = Engine()
    eng.lanes = lanes
    plan = eng.dry_plan(m, shape, batch_stats=True)
    bns = [mod for mod in m.modules() if isinstance(mod, (torch.nn.BatchNorm3d, torch.nn.BatchNorm2d))]
    stats = [s for s in plan.steps if isinstance(s, BnStatsStep)]
    # exactly one statistics step (and one update, one apply) per BatchNorm of the trunk, each on its own module
    assert len(stats) == len(bns) == len(plan.bn_steps) == len(plan.bn_refs)
    plan.bind(m)
    assert {id(plan.get(r)) for r in plan.bn_refs} == {id(b) for b in bns}
    assert sum(isinstance(s, BnUpdateStep) for s in plan.steps) == sum(isinstance(s, BnApplyStep) for s in plan.steps) == len(bns)
    # nothing that jumps over a BN: no chained pairs / tails, no dual-source shortcut GEMM, no conv programs
    assert not any(isinstance(s, (ChainStep, AltStep, ProgramStep)) for s in plan.steps)
    assert not plan.chain_steps and not plan.alt_steps and not plan.program_steps
    assert not any(isinstance(p, PackedDual) for p in plan.packs)
    convs = [t for s in plan.steps for t in (s.direct if isinstance(s, _WinoExec) else [s]) if isinstance(t, ConvStep)]
    assert convs and all(c.x2 is None for c in convs)
    # every conv ahead of a BN is raw: no BN fold, no activation, no residual in its epilogue
    assert all(p.bn is None for p in plan.packs)
    raw = [c for c in convs if not c.d.flags & (L.PTX_EPI_RES_ADD | L.PTX_EPI_RES_PADA)]
    assert all(not c.d.flags & L.PTX_EPI_RELU for c in raw)
    # one lane: the plan is the whole batch, and every statistics step counts all of its positions
    assert plan.shape == shape and plan.batch_stats
    for s in stats:
        assert s.rows % shape[0] == 0 and s.rows >= 2
    assert plan.precision == "fp32" and not plan.x3
    assert plan.bn_ws_bytes >= max(int(L.lib().ptx_bn_batch_stats_workspace_bytes(s.rows, s.C)) for s in stats)
    offs = [o for o, _ in plan.bn_sizes]
    assert offs == sorted(offs) and all(o % 4 == 0 for o in offs)


def test_batch_stats_plan_ignores_x3():
    eng = Engine()
    eng.precision = "x3"
    plan = eng.dry_plan(_model("resnet3d18"), (2, 3, 8, 64, 64), batch_stats=True)
    assert plan.precision == "fp32" and not any(p.x3 for p in plan.packs)


def test_eval_plan_unchanged_by_the_other_flavour():
    m = _model("resnet3d50")
    eng = Engine()
    shape = (2, 3, 8, 64, 64)

    def labels(plan):
        return [(type(s).__name__, getattr(s, "label", None)) for s in plan.steps]
    before = labels(eng.dry_plan(m, shape))
    stats = eng.dry_plan(m, shape, batch_stats=True)
    after = labels(eng.dry_plan(m, shape))
    assert before == after and len(before) < len(stats.steps)
    assert not any(n.startswith("Bn") for n, _ in after)
    assert not eng.dry_plan(m, shape).batch_stats


# --------------------------------------------------------------------------------------------- what raises
def _out_of_scope():
    adopted = _model("resnet3d18")
    adopted.arch_name = "adopted:ResNet3D"
    return [("bf16", _model("resnet3d18").to(torch.bfloat16)), ("fp16", _model("resnet3d18").half()),
            ("non-local", _model("nonlocalresnet3d50")), ("non-local (2+1)D", _model("nonlocal_r2plus1d50")),
            ("MultiViewConv", _model("mvresnet10")), ("SlowFast", ptx.slowfast.resnet18(mode="sf", num_classes=10)),
            ("I3D", ptx.i3d(num_classes=51, pretrained=None)),
            ("TRN", ptx.TRN(51, num_segments=4, arch="resnet18", consensus="TRN", pretrained=None)),
            ("BigGAN", ptx.biggan_deep(128, ch=32)), ("adopted", adopted)]


def test_out_of_scope_models_raise_naming_the_supported_set():
    for what, m in _out_of_scope():
        with pytest.raises(PtxError) as e:
            ptx.update_bn([], m)
        assert "resnet3d10..200" in str(e.value) and "r2plus1d10..50" in str(e.value) and "resnet18..152" in str(e.value), what
        if hasattr(m, "engine") and hasattr(m, "arch") and what != "TRN":
            with pytest.raises(PtxError):
                m.engine().dry_plan(m, (2, 3, 8, 64, 64), batch_stats=True)
            with pytest.raises(PtxError):
                m.update_bn([])


def test_cpu_tensors_raise():
    m = _model("resnet3d18")
    rm = m.bn1.running_mean.clone()
    with pytest.raises(PtxError, match="CUDA"):
        ptx.update_bn([torch.zeros(2, 3, 8, 32, 32)], m, reset=False)
    with pytest.raises(PtxError, match="momentum"):
        ptx.update_bn([], m, momentum=1.5)
    assert torch.equal(m.bn1.running_mean, rm) and not m.training


def test_one_value_per_channel_raises_at_plan_build():
    with pytest.raises(PtxError, match="Expected more than 1 value per channel"):
        Engine().dry_plan(_model("resnet3d18"), (1, 3, 2, 32, 32), batch_stats=True)
    Engine().dry_plan(_model("resnet3d18"), (1, 3, 2, 32, 32))               # the eval plan of that shape compiles
    Engine().dry_plan(_model("resnet3d18"), (2, 3, 2, 32, 32), batch_stats=True)


# --------------------------------------------------------------------------------------------- the C ABI
def test_header_bindings_and_exports_agree():
    text = open(L.BN_HEADER_PATH).read()
    declared = L.header_symbols(L.BN_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_BN) == NAMES
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.SIGNATURES_YUV16, L.SIGNATURES_COLOR,
                  L.SIGNATURES_RANDAUG, L.SIGNATURES_RESAMPLE, L.SIGNATURES_MIX, L.SIGNATURES_STEM_STRIDED, L.SIGNATURES_NL_KS,
                  L.SIGNATURES_LINEAR_BF16, L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_BN[name][0], list(L.SIGNATURES_BN[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_BN[name][1]), name
    # the descriptor: the header's fields in the binding's order, 16 four-byte fields
    body = re.search(r"typedef struct ptx_bn_apply_desc \{(.*?)\} ptx_bn_apply_desc;", plain, flags=re.S).group(1)
    fields = [f.strip() for line in body.split(";") for f in re.sub(r"^\s*(u?int32_t)", "", line.strip()).split(",") if f.strip()]
    assert fields == [n for n, _ in L.BnApplyDesc._fields_] and C.sizeof(L.BnApplyDesc) == 64
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "ptx_amd_bn.h" in integ and all(n in integ for n in declared)
    import importlib.util as iu
    spec = iu.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = iu.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert any(h.endswith("ptx_amd_bn.h") for h in build.HEADERS) and len(build.SOURCES) == 10
    files = build.tu_files("pool_head.hip")
    assert any(p.endswith("bn_batch.hip") for p in files) and any(p.endswith("ptx_amd_bn.h") for p in files)
    assert L.binary_source_hash() == L.source_hash()


def test_refusals_are_made_on_the_host():
    lib = L.lib()
    FAKE = C.c_void_p(0x10000)

    def err():
        return lib.ptx_last_error().decode()
    ws = lib.ptx_bn_batch_stats_workspace_bytes
    assert ws(0, 8) == 0 and ws(100, 0) == 0
    assert ws(200704, 256) == ws(200704, 256) > 0 and ws(200704, 256) % 16 == 0
    assert ws(7, 20) >= 2 * 20 * 4
    # the partial grid is capped: the workspace stops growing with the rows
    assert ws(1 << 30, 256) == ws(1 << 28, 256) <= 1024 * 2 * 256 * 4
    st = lib.ptx_bn_batch_stats_f32
    assert st(FAKE, 100, 8, 6, FAKE, FAKE, FAKE, 1 << 20, None) == 1 and "stride" in err()
    assert st(FAKE, 100, 8, 10, FAKE, FAKE, FAKE, 1 << 20, None) == 1
    assert st(C.c_void_p(0x10004), 100, 8, 8, FAKE, FAKE, FAKE, 1 << 20, None) == 1 and "aligned" in err()
    assert st(FAKE, 100, 8, 8, FAKE, FAKE, FAKE, 16, None) == 4 and "workspace" in err()
    assert st(FAKE, 100, 8, 8, FAKE, FAKE, None, 0, None) == 4
    up = lib.ptx_bn_batch_update_f32
    assert up(FAKE, FAKE, 1, 1.0, 1e-5, None, None, None, None, FAKE, FAKE, 8, None) == 1 and "more than 1 value" in err()
    assert up(FAKE, FAKE, 8, 1.0, 1e-5, None, None, FAKE, None, FAKE, FAKE, 8, None) == 1 and "go together" in err()
    ap = lib.ptx_bn_apply_f32
    d = L.BnApplyDesc()
    d.N, d.T, d.H, d.W, d.C, d.ldx, d.ldy = 2, 3, 5, 7, 22, 24, 24
    d.flags = L.PTX_EPI_RES_ADD | L.PTX_EPI_RES_PADA
    assert ap(C.byref(d), FAKE, FAKE, FAKE, FAKE, FAKE, None) == 1 and "exclusive" in err()
    d.flags = L.PTX_EPI_RES_ADD
    assert ap(C.byref(d), FAKE, FAKE, FAKE, None, FAKE, None) == 1 and "res == NULL" in err()
    d.flags = L.PTX_EPI_RES_PADA
    d.ldr, d.res_C, d.res_T, d.res_H, d.res_W, d.res_sT, d.res_sH, d.res_sW = 12, 10, 5, 10, 12, 2, 2, 2       # (W - 1) * 2 = 12 >= res_W
    assert ap(C.byref(d), FAKE, FAKE, FAKE, FAKE, FAKE, None) == 1 and "shortcut-A" in err()
    d.res_W, d.res_C = 13, 23                                                                                  # wider than the output
    assert ap(C.byref(d), FAKE, FAKE, FAKE, FAKE, FAKE, None) == 1 and "shortcut-A" in err()
    d.flags, d.ldx = 0, 22
    assert ap(C.byref(d), FAKE, FAKE, FAKE, None, FAKE, None) == 1 and "extents" in err()
    d.ldx, d.flags = 24, 0x8000
    assert ap(C.byref(d), FAKE, FAKE, FAKE, None, FAKE, None) == 1 and "flags" in err()
