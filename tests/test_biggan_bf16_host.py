"""bf16 BigGAN-deep generator, host side (no GPU): plans of `G.to(torch.bfloat16)` compiled on the 'meta' device, the
routing to the bf16 patch kernels and its switches, and the ABI of the new entry points and flag bit."""
import ctypes as C
import re
import subprocess

import pytest
import torch

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd import plans as P
from pretorched_x_amd.engine import ConvStep, Engine, PatchConvStep

RES = (256, 128, 64, 32)
NEW_SYMBOLS = ("ptx_conv3x3_bf16_supported", "ptx_conv3x3_bf16_fwd", "ptx_conv1x1_skip_bf16_supported",
               "ptx_conv1x1_skip_bf16_fwd")


def _kinds(plan):
    """label -> [kernel of each step carrying that label]"""
    out = {}
    for s in plan.steps:
        lab = getattr(s, "label", getattr(s, "__name__", "?"))
        out.setdefault(lab, []).append(s.kernel if isinstance(s, PatchConvStep) else
                                       "tile" if isinstance(s, ConvStep) else "pass")
    return out


def _n_attention(G):
    return sum(1 for stage in G.blocks for b in stage if b.kind == "attention")


@pytest.fixture
def no_guard(monkeypatch):
    """bf16 plans never consult the packed-fp16 affine guard."""
    def boom(*a, **k):
        raise AssertionError("the bf16 generator plan asked plans.half_affine_ok")
    monkeypatch.setattr(P, "half_affine_ok", boom)
    for k in ("PTX_CONV3X3_BF16", "PTX_CONV1X1_BF16"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("res", RES)
def test_dry_plan_bf16_biggan(res, no_guard):
    G = ptx.biggan_deep(res).to(torch.bfloat16)
    plan = Engine().dry_plan(G, (64, G.dim_z))
    assert plan.bf16 and plan.precision == "bf16" and not plan.half_plan
    # every conv (tile or patch kernel) runs on bf16 operands and writes bf16
    convs = [s for s in plan.steps if isinstance(s, (ConvStep, PatchConvStep))]
    assert len(convs) >= 4 * sum(1 for st in G.blocks for b in st if b.kind == "gblock") + 1
    for s in convs:
        assert s.d.flags & L.PTX_BF16_OPERANDS and s.d.flags & L.PTX_F16_OPERANDS and s.d.flags & L.PTX_EPI_OUT_F16, s.label
    # activations: bf16, except the first linear's output (fp32, the first block's skip operand)
    bw = G.bottom_width
    fp32 = [a for a in plan.acts if not a.bf16]
    assert len(fp32) == 1 and (fp32[0].H, fp32[0].W, fp32[0].C) == (bw, bw, G.linear.out_features // bw ** 2)
    for a in plan.acts:
        if a.bf16:
            assert a.t.dtype == torch.bfloat16 and a.ld % 8 == 0
    k = _kinds(plan)
    # no fp16-only consumer kernels (their packed-fp16 input affine is what needs a guard), one cBN pass
    flat = [x for v in k.values() for x in v]
    assert "conv1x1_pro_f16" not in flat and "rgb_conv3x3" not in k and "rgb_conv3x3_f16" not in flat
    assert not any(x.endswith("_f16") for x in flat), k
    assert len(k["affine_act_upsample"]) == 1
    # attention: one bf16 attention launch per block, theta | phi | g one conv on 8-channel boundaries
    n_att = _n_attention(G)
    assert getattr(plan, "attn_steps", 0) == n_att == (0 if res == 32 else 1)
    for d in getattr(plan, "attn_descs", []):
        assert d.mode == L.PTX_NL_BF16 | L.PTX_NL_SOFTMAX and L.lib().ptx_nonlocal_supported(C.byref(d))
    for name in (n for n in k if n.endswith(".theta_phi_g")):
        s, = [s for s in convs if s.label == name]
        c8 = (s.d.Co // 3 + 7) // 8 * 8
        assert s.d.Co % 8 == 0 and s.d.ldy % 8 == 0 and c8 >= 8
    # image conv: tanh, bf16 out, on a bf16 tile
    img, = [s for s in convs if s.label == "output_layer.2"]
    assert img.d.flags & L.PTX_EPI_TANH and plan.feat.bf16 and plan.feat.C == 3


def test_dry_plan_bf16_biggan_flow(no_guard):
    """Config 5 (256, ch 128): the two-output flow everywhere -- each block's conv4 writes the next cBN1 + ReLU and the raw
    sum; the attention's output conv does the same; 3x3 convs and skip-adding 1x1 convs of the >= 32 x 32 stages run on
    the patch-resident bf16 kernels."""
    G = ptx.biggan_deep(256).to(torch.bfloat16)
    plan = Engine().dry_plan(G, (64, G.dim_z))
    k = _kinds(plan)
    byl = {s.label: s for s in plan.steps if isinstance(s, (ConvStep, PatchConvStep))}
    for blk in ("blocks.3.0", "blocks.3.1", "blocks.4.0", "blocks.4.1", "blocks.5.0", "blocks.5.1"):
        assert k[blk + ".conv2"] == k[blk + ".conv3"] == ["conv3x3_bf16"], blk
        assert k[blk + ".conv4"] == ["conv1x1_skip_bf16"], blk
    assert byl["blocks.3.1.conv2"].d.flags & L.PTX_PRO_UP2
    assert k["blocks.3.2.o"] == ["conv1x1_skip_bf16"]
    assert k["blocks.0.0.conv2"] == ["tile"]                            # 4 x 4 maps stay on the implicit-GEMM tiles
    for name, s in byl.items():
        if name.endswith(".conv4") and name not in ("blocks.5.1.conv4", "blocks.3.1.conv4"):
            assert s.d.flags & L.PTX_EPI_DUAL_RAW and s.d.flags & L.PTX_EPI_AFFINE, name
    assert not byl["blocks.3.1.conv4"].d.flags & (L.PTX_EPI_DUAL_RAW | L.PTX_EPI_AFFINE)      # attention next: raw only
    assert byl["blocks.3.2.o"].d.flags & L.PTX_EPI_DUAL_RAW and byl["blocks.3.2.o"].d.flags & L.PTX_RES_F16
    last = byl["blocks.5.1.conv4"].d.flags
    assert last & L.PTX_EPI_AFFINE and last & L.PTX_EPI_RELU and not last & L.PTX_EPI_DUAL_RAW
    # the first block's skip operand is the fp32 linear output; every later skip is bf16
    assert not byl["blocks.0.0.conv4"].d.flags & L.PTX_RES_F16
    assert byl["blocks.0.1.conv4"].d.flags & L.PTX_RES_F16


@pytest.mark.parametrize("ch", [16, 48, 128])
def test_dry_plan_bf16_biggan_pad8_slices(ch, no_guard, monkeypatch):
    """theta | phi | g is ONE pad8 conv: each slice starts on an 8-channel boundary (phi at p8 = round8(c8), g at 2 p8) and
    the attention reads exactly those slices -- exercised where c8 = ch / 4 is not a multiple of 8 (ch = 16: c8 = 4; ch = 48:
    c8 = 12)."""
    from pretorched_x_amd.engine import Plan
    pooled = []
    orig = Plan.maxpool

    def spy(self, x, *a, **k):
        pooled.append(x)
        return orig(self, x, *a, **k)
    monkeypatch.setattr(Plan, "maxpool", spy)
    G = ptx.biggan_deep(128, ch=ch).to(torch.bfloat16)
    plan = Engine().dry_plan(G, (2, G.dim_z))
    att = G.blocks[3][2]
    c8, c2 = att.ch // 8, att.ch // 2
    p8 = (c8 + 7) // 8 * 8
    tpg, = [s for s in plan.steps if getattr(s, "label", "") == "blocks.3.2.theta_phi_g"]
    assert tpg.d.Co == 2 * p8 + (c2 + 7) // 8 * 8 and tpg.d.ldy % 8 == 0
    pk, = [p for p in plan.packs if getattr(p, "pad8", False)]
    assert pk.Co == tpg.d.Co
    (th, ph, g, y), = plan.attn_operands
    phi_in, g_in = pooled                                   # the two 2 x 2 pools read phi and g out of the projection
    assert th.t._base is phi_in.t._base is g_in.t._base
    assert (th.t.storage_offset(), phi_in.t.storage_offset(), g_in.t.storage_offset()) == (0, p8, 2 * p8)
    assert (th.C, phi_in.C, g_in.C) == (c8, c8, c2)
    d, = plan.attn_descs
    assert (d.d, d.dv) == (c8, c2) and L.lib().ptx_nonlocal_supported(C.byref(d))


def test_dry_plan_bf16_biggan_last_attention(no_guard):
    """Resolution 64: the attention block is the network's last; its output conv applies the output layer's BN + ReLU."""
    G = ptx.biggan_deep(64).to(torch.bfloat16)
    plan = Engine().dry_plan(G, (2, G.dim_z))
    byl = {s.label: s for s in plan.steps if isinstance(s, (ConvStep, PatchConvStep))}
    o = byl["blocks.3.2.o"].d.flags
    assert o & L.PTX_EPI_AFFINE and o & L.PTX_EPI_RELU and not o & L.PTX_EPI_DUAL_RAW
    assert len(_kinds(plan)["affine_act_upsample"]) == 1


def test_dry_plan_bf16_patch_switches(monkeypatch, no_guard):
    G = ptx.biggan_deep(256).to(torch.bfloat16)
    monkeypatch.setenv("PTX_CONV3X3_BF16", "0")
    k = _kinds(Engine().dry_plan(G, (8, G.dim_z)))
    assert k["blocks.4.0.conv2"] == ["tile"] and k["blocks.4.0.conv4"] == ["conv1x1_skip_bf16"]
    monkeypatch.setenv("PTX_CONV1X1_BF16", "0")
    k = _kinds(Engine().dry_plan(G, (8, G.dim_z)))
    assert all(v in (["tile"], ["pass"]) or set(v) == {"pass"} for v in k.values()), k


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_fp32_and_fp16_generator_plans_carry_no_bf16_bit(precision, monkeypatch):
    for k in ("PTX_CONV3X3_F16", "PTX_CONV1X1_F16", "PTX_CONV1_PRO", "PTX_RGB_CONV", "PTX_ATTN_F16", "PTX_HALF_AFFINE_GUARD"):
        monkeypatch.delenv(k, raising=False)
    G = ptx.biggan_deep(256, precision=precision)
    plan = Engine().dry_plan(G, (8, G.dim_z))
    assert not plan.bf16 and plan.half_plan == (precision == "fp16")
    flat = [x for v in _kinds(plan).values() for x in v]
    for s in plan.steps:
        if hasattr(s, "d") and hasattr(s.d, "flags"):
            assert not s.d.flags & L.PTX_BF16_OPERANDS, s.label
    assert not any(a.bf16 for a in plan.acts)
    assert not any(x.endswith("_bf16") for x in flat)
    if precision == "fp16":
        assert "conv3x3_f16" in flat and "conv1x1_skip_f16" in flat and "conv1x1_pro_f16" in flat


def test_bf16_generator_precision_follows_the_parameters():
    """`precision=` governs fp32-parameter generators only: a bf16 copy of an fp16-configured generator runs the bf16 flow."""
    G = ptx.biggan_deep(128, ch=32, precision="fp16").to(torch.bfloat16)
    plan = Engine().dry_plan(G, (2, G.dim_z))
    assert plan.bf16 and not plan.half_plan
    assert not any(x.endswith("_f16") for v in _kinds(plan).values() for x in v)


def test_fp16_generator_parameters_raise():
    G = ptx.biggan_deep(128, ch=32).half()
    with pytest.raises(ptx.PtxError, match="fp16"):
        Engine().dry_plan(G, (2, G.dim_z))


def test_generate_refuses_cpu_tensors():
    G = ptx.biggan_deep(128, ch=32).to(torch.bfloat16)
    z = torch.zeros(2, G.dim_z, dtype=torch.bfloat16)
    with pytest.raises(ptx.PtxError, match="bfloat16 CUDA"):
        G(z, torch.zeros(2, G.shared_dim, dtype=torch.bfloat16))


# ---------------------------------------------------------------------------------------------------------------- ABI
def _header_defines():
    text = open(L.HEADER_PATH).read()
    return {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(PTX_\w+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", text)}


def test_abi_new_symbols_agree():
    hdr = L.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in hdr and name in L.SIGNATURES and name not in L.EXPERIMENTAL, name
        assert getattr(L.lib(), name) is not None
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True)
    if nm.returncode == 0:
        exported = set(re.findall(r"\bT\s+(ptx_\w+)", nm.stdout))
        assert set(NEW_SYMBOLS) <= exported


def test_abi_act_out_bf16_bit():
    defs = _header_defines()
    assert defs["PTX_ACT_OUT_BF16"] == L.PTX_ACT_OUT_BF16 == 0x200
    assert not L.PTX_ACT_OUT_BF16 & (L.PTX_ACT_OUT_F16 | 0xff)          # neither the fp16 bit nor an act value


def _desc(bf, Ci=128, Co=128, k=3, H=64, W=64, flags=0):
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = 2, 1, H, W, Ci // 2, Ci // 2
    d.To, d.Ho, d.Wo, d.Co, d.ldy = 1, H, W, Co, Co
    d.kT, d.kH, d.kW = 1, k, k
    d.sT = d.sH = d.sW = 1
    d.pT, d.pH, d.pW = 0, k // 2, k // 2
    d.Kc, d.Co_pad, d.groups = Ci // 2, (Co + 127) // 128 * 128, 1
    d.flags = L.PTX_F16_OPERANDS | L.PTX_EPI_OUT_F16 | (L.PTX_BF16_OPERANDS if bf else 0) | flags
    return d


def test_abi_bf16_entry_points_gate():
    lib = L.lib()
    aff = L.PTX_EPI_AFFINE | L.PTX_EPI_RELU
    for bf in (False, True):
        sup3 = lib.ptx_conv3x3_bf16_supported if bf else lib.ptx_conv3x3_f16_supported
        sup1 = lib.ptx_conv1x1_skip_bf16_supported if bf else lib.ptx_conv1x1_skip_f16_supported
        oth3 = lib.ptx_conv3x3_f16_supported if bf else lib.ptx_conv3x3_bf16_supported
        oth1 = lib.ptx_conv1x1_skip_f16_supported if bf else lib.ptx_conv1x1_skip_bf16_supported
        for C_ in (64, 128, 256):
            d = _desc(bf, C_, C_, flags=aff | L.PTX_PRO_UP2)
            assert sup3(C.byref(d)) and not oth3(C.byref(d))
        d = _desc(bf, 64, 256, k=1, flags=aff | L.PTX_EPI_DUAL_RAW | L.PTX_RES_F16 | L.PTX_EPI_RES_ADD)
        d.ldr = 256
        assert sup1(C.byref(d)) and not oth1(C.byref(d))
        assert not sup3(C.byref(_desc(bf, 96, 96)))                      # 96 channels: not a patch-kernel width
        assert not sup3(C.byref(_desc(bf, 128, 128, W=16)))              # fewer than 32 columns
        assert not sup1(C.byref(_desc(bf, 64, 64, k=1)))                 # Co not a multiple of 128
    fake = C.c_void_p(1 << 20)
    rc = lib.ptx_conv3x3_bf16_fwd(C.byref(_desc(False)), fake, fake, None, fake, None, None)
    assert rc != 0 and b"conv3x3_bf16" in lib.ptx_last_error()
    rc = lib.ptx_conv1x1_skip_bf16_fwd(C.byref(_desc(False, 64, 128, k=1)), fake, fake, None, None, fake, None, None)
    assert rc != 0 and b"conv1x1_skip_bf16" in lib.ptx_last_error()
