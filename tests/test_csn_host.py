"""Host tests (no GPU) of the depthwise 3-D convolution's C ABI (include/ptx_amd_dw.h) and of the channel-separated networks
(ir_csn50 .. ip_csn152): the census of the header, the bindings and the exports; the `_supported` answers, clause by clause; the
plans (`Engine.dry_plan`); parameter counts and state-dict keys; everything that raises; the torch.nn path (CPU, train()) against
tests/csn_oracle.py bit for bit."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn as nn

import csn_oracle as O
from pretorched_x_amd._lib import PtxError
from pretorched_x_amd.engine import Engine
from pretorched_x_amd.steps import ConvStep, DwConvStep, PackedDw
from pretorched_x_amd.testing import synth_state_dict

NAMES = ["ir_csn50", "ir_csn101", "ir_csn152", "ip_csn50", "ip_csn101", "ip_csn152"]
LAYERS = {"50": (3, 4, 6, 3), "101": (3, 4, 23, 3), "152": (3, 8, 36, 3)}


# --------------------------------------------------------------------------------------------- 1. header, bindings, exports
def test_dw_header_bindings_and_exports(ptx):
    L = ptx._lib
    lib = L.lib()
    text = open(L.DW_HEADER_PATH).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = L.header_symbols(L.DW_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_DW) == ["ptx_conv3d_dw_f32_force_form", "ptx_conv3d_dw_f32_fwd", "ptx_conv3d_dw_f32_supported",
                                                   "ptx_pack_dw_weight_f32"]
    for name in ("PTX_DW_FORM_STRIP4", "PTX_DW_FORM_STRIP8", "PTX_DW_FORM_LDS"):
        assert int(re.search(r"#define %s\s+(\d+)\b" % name, text).group(1)) == getattr(L, name), name
    for form in (4, 8, 16, 0):                                       # process-wide: back to the library's rule at the end
        assert lib.ptx_conv3d_dw_f32_force_form(form) == 0
    assert lib.ptx_conv3d_dw_f32_force_form(2) == 1 and "PTX_DW_FORM" in lib.ptx_last_error().decode()
    assert not set(declared) & set(L.header_symbols())              # ptx_amd.h stays the census it was
    others = [n for n in dir(L) if n.startswith("SIGNATURES") and n != "SIGNATURES_DW"]
    assert len(others) >= 15
    for n in others:
        assert not set(declared) & set(getattr(L, n)), n
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_DW[name][0], list(L.SIGNATURES_DW[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_DW[name][1]), name
    root = os.path.dirname(os.path.dirname(L.HEADER_PATH))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    section = integ.split("### 1s.", 1)[1].split("\n### ", 1)[0]
    assert "ptx_amd_dw.h" in section and all(n in section for n in declared)
    stub = integ.split("## 2.", 1)[1]
    assert all(n in stub for n in declared)
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "conv_dw_f32.h" in build.HEADERS and any(h.endswith("ptx_amd_dw.h") for h in build.HEADERS)
    files = build.tu_files("pool_head.hip")
    assert any(p.endswith(os.sep + "conv_dw_f32.h") for p in files) and any(p.endswith("ptx_amd_dw.h") for p in files)
    assert L.binary_source_hash() == L.source_hash() == build.source_hash()
    src = open(os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py")).read()       # ptx_version()'s hash names the header
    assert '"ptx_amd_dw.h"' in src.split("def source_hash", 1)[1].split("def obj_path", 1)[0]


# --------------------------------------------------------------------------------------------- 2. _supported, clause by clause
def _desc(L, **kw):
    a = dict(N=2, Ti=8, Hi=14, Wi=14, Ci=64, ldx=64, Co=64, ldy=64, kT=3, kH=3, kW=3, sT=1, sH=1, sW=1, pT=1, pH=1, pW=1, groups=64, flags=0)
    a.update(kw)
    for ax in "THW":
        if ax + "o" not in a:
            a[ax + "o"] = (a[ax + "i"] + 2 * a["p" + ax] - a["k" + ax]) // a["s" + ax] + 1
    d = L.ConvDesc()
    for k, v in a.items():
        setattr(d, k, v)
    return d


def test_dw_supported_answers_from_descriptors(ptx):
    L = ptx._lib
    lib = L.lib()

    def sup(**kw):
        ok = lib.ptx_conv3d_dw_f32_supported(C.byref(_desc(L, **kw)))
        return ok, lib.ptx_last_error().decode()

    assert sup()[0] == 1 and sup(flags=L.PTX_EPI_RELU)[0] == 1
    assert sup(Ci=4, Co=4, groups=4, ldx=4, ldy=4)[0] == 1 and sup(ldx=72, ldy=2048)[0] == 1
    for k in ((1, 3, 3), (3, 1, 1), (1, 1, 1), (3, 3, 1)):
        for s in ((1, 1, 1), (2, 2, 2), (2, 1, 1), (1, 2, 2)):
            kw = dict(zip(("kT", "kH", "kW", "sT", "sH", "sW", "pT", "pH", "pW"), k + s + tuple(v // 2 for v in k)))
            assert sup(**kw)[0] == 1, kw
    assert sup(pT=0, pH=2, pW=0)[0] == 1                            # 0 <= pad < k, per axis
    for kw, why in ((dict(groups=32), "groups == Ci == Co"), (dict(groups=1), "groups == Ci == Co"), (dict(groups=0), "groups == Ci == Co"),
                    (dict(Co=128, ldy=128), "groups == Ci == Co"), (dict(Ci=6, Co=6, groups=6, ldx=8, ldy=8), "multiple of 4"),
                    (dict(kT=5, pT=2), "1 or 3"), (dict(kW=2, pW=0), "1 or 3"), (dict(kH=7, pH=3), "1 or 3"),
                    (dict(sT=3), "1 or 2"), (dict(sW=4), "1 or 2"), (dict(sH=0, Ho=14), "1 or 2"),
                    (dict(pT=3), "pad < k"), (dict(kW=1, pW=1), "pad < k"), (dict(pH=-1), "pad < k"),
                    (dict(ldx=60), "ldx"), (dict(ldx=66), "ldx"), (dict(ldy=60), "ldy"), (dict(ldy=70), "ldy"),
                    (dict(flags=L.PTX_EPI_RES_ADD), "PTX_EPI_RELU"), (dict(flags=L.PTX_EPI_RELU | L.PTX_F16X3_OPERANDS), "PTX_EPI_RELU"),
                    (dict(flags=L.PTX_BF16_OPERANDS | L.PTX_F16_OPERANDS), "PTX_EPI_RELU"),
                    (dict(Wo=13), "output extent"), (dict(To=9), "output extent"), (dict(N=0), "non-positive"),
                    (dict(Hi=1 << 12, Wi=1 << 12, ldx=64), "2^31 bytes"), (dict(Hi=4096, Wi=2048, ldy=1 << 12), "2^31 bytes")):
        ok, msg = sup(**kw)
        assert ok == 0 and why in msg, (kw, msg)
    assert sup(Hi=4096, Wi=2047)[0] == 1                            # 4096 * 2047 * 64 * 4 bytes: just below
    # the forward refuses what _supported refuses, with the library's status for it (2: unsupported), before touching a pointer
    fake = C.c_void_p(1 << 20)
    assert lib.ptx_conv3d_dw_f32_fwd(C.byref(_desc(L, sT=3)), fake, fake, fake, fake, None) == 2
    assert lib.ptx_conv3d_dw_f32_fwd(C.byref(_desc(L)), fake, fake, fake, None, None) == 1
    assert lib.ptx_conv3d_dw_f32_fwd(C.byref(_desc(L)), C.c_void_p((1 << 20) + 4), fake, fake, fake, None) == 1 and "aligned" in \
        lib.ptx_last_error().decode()
    assert lib.ptx_pack_dw_weight_f32(6, 3, 3, 3, fake, None, None, None, None, None, C.c_float(0), fake, fake, None) == 1
    assert lib.ptx_pack_dw_weight_f32(8, 3, 3, 3, fake, None, fake, None, None, None, C.c_float(0), fake, fake, None) == 1
    # ptx_conv3d_fwd keeps refusing depthwise descriptors
    d = _desc(L, Kc=4, Co_pad=128)
    assert lib.ptx_conv3d_fwd(C.byref(d), fake, fake, fake, None, fake, None, 0, -1, 1, None) != 0


# --------------------------------------------------------------------------------------------- 3. the plans
def _model(ptx, name, num_classes=51):
    return ptx.__dict__[name](num_classes=num_classes, pretrained=None)


@pytest.mark.parametrize("name", ["ir_csn50", "ip_csn50"])
@pytest.mark.parametrize("precision", ["fp32", "x3"])
def test_dry_plan(ptx, name, precision):
    m = _model(ptx, name)
    eng = Engine()
    eng.precision = precision
    plan = eng.dry_plan(m, (2, 3, 8, 64, 64))
    blocks = sum(LAYERS["50"])
    dw = [s for s in plan.steps if isinstance(s, DwConvStep)]
    assert len(dw) == blocks                                         # one depthwise launch per block
    assert all(s.d.groups == s.d.Ci == s.d.Co and (s.d.kT, s.d.kH, s.d.kW) == (3, 3, 3) for s in dw)
    assert all(s.d.flags == ptx._lib.PTX_EPI_RELU for s in dw)       # fp32 + ReLU, whatever the plan's precision
    assert all(s.label.endswith(".conv2") and s.macs > 0 and s.hbm_bytes > 0 and s.kernel == "conv_dw_f32" for s in dw)
    assert [s.label for s in dw][:4] == ["layer1.0.conv2", "layer1.1.conv2", "layer1.2.conv2", "layer2.0.conv2"]
    strides = [(s.d.sT, s.d.sH, s.d.sW) for s in dw]
    assert strides[3] == (2, 2, 2) and strides[0] == strides[1] == strides[4] == (1, 1, 1)
    convs = [s for s in plan.steps if isinstance(s, ConvStep)]
    assert not any(s.d.groups > 1 for s in convs) and not any(s.d.groups > 1 for s in plan.conv_steps)
    assert not any(isinstance(s, DwConvStep) for s in plan.conv_steps)
    assert sum(isinstance(p, PackedDw) for p in plan.packs) == blocks
    assert not any(p.x3 for p in plan.packs if isinstance(p, PackedDw))
    # every block: conv1 (+ conv2_pw) and conv3 (with the shortcut conv folded into its K axis) are the pointwise GEMMs
    per_block = 3 if name.startswith("ip") else 2
    assert len(plan.conv_steps) == per_block * blocks
    assert sum(1 for s in plan.conv_steps if s.label.endswith("conv3+downsample")) == 4
    assert (plan.feat.N, plan.feat.C, plan.feat.T, plan.feat.H, plan.feat.W) == (2, 2048, 1, 2, 2)
    assert plan.precision == precision
    # the stem keeps every frame: (3,7,7) conv at stride (1,2,2), then the (1,3,3) pool
    first = dw[0].d
    assert (first.Ti, first.Hi, first.Wi, first.Ci) == (8, 16, 16, 64)


def test_dry_plan_flagship_shape_sums(ptx):
    """ir-CSN-152 at 32 x 224 x 224, counted from the module shapes: 74.05 GMAC per clip -- 61.45 G in 1x1x1 convs (83.0 %), 11.33 G
    in the stem (15.3 %), 1.27 G in the depthwise convs (1.7 %).  The plan's launches carry exactly those."""
    m = _model(ptx, "ir_csn152", 400)
    plan = Engine().dry_plan(m, (1, 3, 32, 224, 224))
    dw = sum(s.macs for s in plan.steps if isinstance(s, DwConvStep))
    total = sum(getattr(s, "macs", 0) or 0 for s in plan.steps)
    assert (dw, total) == (1265338368, 74045425664)
    assert sum(s.macs for s in plan.conv_steps) == 61450747904


# --------------------------------------------------------------------------------------------- 4. parameters and keys
@pytest.mark.parametrize("name,count", [("ir_csn50", 13131152), ("ip_csn50", 14396176), ("ir_csn101", 22213776),
                                        ("ip_csn101", 24601616), ("ir_csn152", 29703568), ("ip_csn152", 33016592)])
def test_parameter_counts(ptx, name, count):
    m = ptx.__dict__[name]()                                        # 400 classes, pretrained=None by default
    assert sum(p.numel() for p in m.parameters()) == count
    assert m.last_linear.out_features == 400 and m.fc is None
    assert name in ptx.model_names and ptx.__dict__[name].__name__ == name
    assert O.layers_of(m.state_dict()) == LAYERS[name.rsplit("csn", 1)[1]]


def test_state_dict_keys_and_modules(ptx):
    for name in ("ir_csn50", "ip_csn50"):
        m = _model(ptx, name)
        keys = list(m.state_dict())
        ip = name.startswith("ip")
        bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
        want = ["conv1.weight"] + ["bn1." + k for k in bn]
        for li, n in enumerate(LAYERS["50"]):
            for bi in range(n):
                p = "layer%d.%d." % (li + 1, bi)
                want += [p + "conv1.weight"] + [p + "bn1." + k for k in bn]
                if ip:
                    want += [p + "conv2_pw.weight"] + [p + "bn2_pw." + k for k in bn]
                want += [p + "conv2.weight"] + [p + "bn2." + k for k in bn] + [p + "conv3.weight"] + [p + "bn3." + k for k in bn]
                if bi == 0:
                    want += [p + "downsample.0.weight"] + [p + "downsample.1." + k for k in bn]
        want += ["last_linear.weight", "last_linear.bias"]
        assert keys == want
        assert tuple(m.conv1.kernel_size) == (3, 7, 7) and tuple(m.conv1.stride) == (1, 2, 2) and tuple(m.conv1.padding) == (1, 3, 3)
        assert tuple(m.maxpool.kernel_size) == (1, 3, 3) and tuple(m.maxpool.stride) == (1, 2, 2) and tuple(m.maxpool.padding) == (0, 1, 1)
        c2 = m.layer3[0].conv2
        assert c2.groups == c2.in_channels == c2.out_channels == 256 and tuple(c2.stride) == (2, 2, 2) and tuple(c2.weight.shape) == (256, 1, 3, 3, 3)
        assert tuple(m.layer3[1].conv2.stride) == (1, 1, 1) and tuple(m.layer1[0].conv2.stride) == (1, 1, 1)
        assert all(b.eps == 1e-3 for b in m.modules() if isinstance(b, nn.BatchNorm3d))
        assert hasattr(m.layer1[0], "conv2_pw") == ip
    assert ptx.resnet3d50(num_classes=7, pretrained=None).bn1.eps == 1e-5          # every other family keeps torch's default


def test_cpu_path_reads_each_modules_own_eps(ptx):
    """The torch.nn path (CPU) calls the modules, so their own eps; the GPU fold is pinned by tests/test_gpu_csn.py."""
    m = _model(ptx, "ir_csn50")
    m.layer1[0].bn2.eps = 0.25
    sd = synth_state_dict(m.state_dict(), 1234)
    m.load_state_dict(sd)
    x = torch.randn(1, 3, 4, 32, 32, generator=torch.Generator().manual_seed(1))
    assert not torch.equal(m(x), O.forward(sd, x))                 # (the CPU path calls the modules: their eps)
    m.layer1[0].bn2.eps = 1e-3
    assert torch.equal(m(x), O.forward(sd, x))


# --------------------------------------------------------------------------------------------- 5. what raises
def test_out_of_scope_raises(ptx):
    with pytest.raises(PtxError, match="pretrained must be None"):
        ptx.ir_csn50(pretrained="kinetics-400")
    for name in ("ir_csn50", "ip_csn50"):
        with pytest.raises(PtxError, match="bf16"):
            Engine().dry_plan(_model(ptx, name).to(torch.bfloat16), (2, 3, 8, 64, 64))
        with pytest.raises(PtxError, match="fp16"):
            Engine().dry_plan(_model(ptx, name).half(), (2, 3, 8, 64, 64))
        m = _model(ptx, name)
        for call in (lambda: ptx.update_bn([], m), lambda: m.engine().dry_plan(m, (2, 3, 8, 64, 64), batch_stats=True)):
            with pytest.raises(PtxError) as e:
                call()
            assert ptx.plan.BATCH_STATS_SCOPE in str(e.value) and "depthwise" in str(e.value)
    m = _model(ptx, "ir_csn50")
    with pytest.raises(PtxError, match="CUDA"):                     # eval mode, CPU input on a CPU model: eager.  A meta one: refused
        m.engine().features(m, torch.zeros(1, 3, 4, 32, 32))


# --------------------------------------------------------------------------------------------- 6. the torch.nn path
@pytest.mark.parametrize("name", ["ir_csn50", "ip_csn50", "ir_csn101"])
def test_cpu_forward_equals_the_oracle(ptx, name):
    m = _model(ptx, name)
    sd = synth_state_dict(m.state_dict(), 1234)
    m.load_state_dict(sd)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 5, 40, 48, generator=g)
    want = O.forward(sd, x)
    assert torch.equal(m(x), want) and torch.equal(m.logits(m.features(x)), want)
    assert torch.equal(m.features(x), O.features(sd, x))
    top = want.topk(2, 1).values
    assert (top[:, 0] - top[:, 1]).min().item() > 2e-3               # the synthetic weights give a decided argmax
    m.train()
    got = m(x)
    assert torch.equal(got, O.forward(sd, x, training=True)) and got.requires_grad
    assert not torch.equal(m.bn1.running_mean, sd["bn1.running_mean"])          # train() moved the running statistics
    m.eval()
    r = m.cam(x, topk=2)                                             # CPU: the definition in plain torch
    assert tuple(r.scores.shape) == (2, 2, 1, 2, 2) and r.maps.dtype == torch.uint8
