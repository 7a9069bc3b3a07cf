"""bf16 non-local blocks, host side (no GPU): plans of bf16 NonLocalBlock1D / 2D / 3D and MNISTNonLocalNet compiled on the
'meta' device, and the ABI gate of the bf16 attention descriptor."""
import ctypes as C
import itertools

import pytest
import torch

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import Engine

MODES = ("embedded_gaussian", "dot_product", "gaussian", "concatenation")
COMBOS = list(itertools.product(MODES, (False, True), (False, True)))        # (mode, sub_sample, bn_layer)


def _shape(dim, C_):
    return {3: (2, C_, 4, 8, 8), 2: (2, C_, 8, 8), 1: (2, C_, 16)}[dim]


def _plan_shape(dim, C_):
    """The plan's (N, C, T, H, W): 1-D / 2-D blocks run as the T = 1 (and H = 1) case of the 3-D plan."""
    s = _shape(dim, C_)
    return s[:2] + (1,) * (5 - len(s)) + s[2:]


def _block(dim, C_, mode, sub, bn, dtype=torch.bfloat16):
    cls = {1: ptx.NonLocalBlock1D, 2: ptx.NonLocalBlock2D, 3: ptx.NonLocalBlock3D}[dim]
    return cls(C_, mode=mode, sub_sample=sub, bn_layer=bn).eval().to(dtype)


def _labels(plan):
    return [getattr(st, "tag", None) or getattr(st, "label", None) for st in plan.steps]


def _check_bf16_block_plan(plan, C_, mode, sub=False):
    assert plan.bf16 and plan.precision == "bf16"
    for a in plan.acts:
        assert a.bf16 and a.t.dtype == torch.bfloat16 and a.ld % 8 == 0, (a.C, a.ld, a.t.dtype)
    labels = _labels(plan)
    assert labels.count("nonlocal_attention") == 1, labels
    assert "nonlocal_unfused" not in labels and "nonlocal_concat_ab" not in labels, labels
    assert len(plan.attn_descs) == 1
    d = plan.attn_descs[0]
    assert d.mode & L.PTX_NL_BF16
    assert L.lib().ptx_nonlocal_supported(C.byref(d))
    ci = max(C_ // 2, 1)
    if mode == "concatenation":
        assert d.d == 8 and d.mode & L.PTX_NL_RELU and d.mode & L.PTX_NL_SCALE
    elif mode == "gaussian":
        assert d.d == C_
    else:
        assert d.d == ci
    assert d.dv == ci
    for st in plan.conv_steps:
        assert st.d.flags & L.PTX_BF16_OPERANDS and st.d.flags & L.PTX_EPI_OUT_F16, st.label
    tpg = [st for st in plan.conv_steps if st.label.endswith(".theta_phi_g")]
    c8 = (ci + 7) // 8 * 8
    if mode in ("gaussian", "concatenation"):        # (concatenation: compact theta / phi / g, read by the row convs)
        assert not tpg
    else:
        # theta | phi | g each start on an 8-channel boundary: the fused projection has 3 x round8(ci) rows
        assert len(tpg) == 1 and tpg[0].d.Co == 3 * c8 and tpg[0].d.ldy == 3 * c8
    (th, ph, g, y), = plan.attn_operands
    offs = [a.t.storage_offset() for a in (th, ph, g, y)]
    assert all(o % 8 == 0 for o in offs), offs
    if mode in ("embedded_gaussian", "dot_product"):       # (sub-sampled phi / g: compact pool outputs)
        assert offs[:3] == ([0, 0, 0] if sub else [0, c8, 2 * c8])
    for a in (th, ph, g, y):
        assert a.bf16 and a.ld % 8 == 0


@pytest.mark.parametrize("C_", [16, 512, 1024])
@pytest.mark.parametrize("mode,sub,bn", COMBOS)
def test_dry_plan_bf16_block3d(mode, sub, bn, C_):
    plan = Engine().dry_plan(_block(3, C_, mode, sub, bn), _plan_shape(3, C_))
    _check_bf16_block_plan(plan, C_, mode, sub)


@pytest.mark.parametrize("dim", [1, 2])
@pytest.mark.parametrize("mode,sub,bn", COMBOS)
def test_dry_plan_bf16_block_1d_2d(dim, mode, sub, bn):
    plan = Engine().dry_plan(_block(dim, 16, mode, sub, bn), _plan_shape(dim, 16))
    _check_bf16_block_plan(plan, 16, mode, sub)


@pytest.mark.parametrize("C_", [6, 20])
@pytest.mark.parametrize("mode,sub,bn", COMBOS)
def test_dry_plan_bf16_odd_widths(mode, sub, bn, C_):
    plan = Engine().dry_plan(_block(3, C_, mode, sub, bn), _plan_shape(3, C_))
    _check_bf16_block_plan(plan, C_, mode, sub)


def test_dry_plan_bf16_theta_phi_g_slices():
    """The attention's theta / phi / g sit 8-channel aligned in the fused projection (C = 20: ci = 10 -> 16 rows each)."""
    plan = Engine().dry_plan(_block(3, 20, "embedded_gaussian", False, True), _plan_shape(3, 20))
    d = plan.attn_descs[0]
    assert d.ld_theta == d.ld_phi == d.ld_g == 48 and d.d == d.dv == 10 and d.ld_y == 16
    (th, ph, g, y), = plan.attn_operands
    assert [a.t.storage_offset() for a in (th, ph, g)] == [0, 16, 32]


def test_dry_plan_bf16_mnist():
    m = ptx.MNISTNonLocalNet().eval().to(torch.bfloat16)
    plan = Engine().dry_plan(m, (2, 1, 28, 28))
    assert plan.bf16
    assert _labels(plan).count("nonlocal_attention") == 2
    assert all(d.mode & L.PTX_NL_BF16 for d in plan.attn_descs)
    for a in plan.acts:
        assert a.bf16 and a.ld % 8 == 0
    assert plan.head is not None and plan.feat.bf16
    first = plan.conv_steps[0]
    assert first.label == "convs.0" and first.d.flags & L.PTX_BF16_OPERANDS


@pytest.mark.parametrize("mode,sub,bn", COMBOS)
def test_dry_plan_fp32_block_has_no_bf16_flag(mode, sub, bn):
    plan = Engine().dry_plan(_block(3, 16, mode, sub, bn, torch.float32), _plan_shape(3, 16))
    assert not plan.bf16
    assert not getattr(plan, "attn_descs", [])
    for st in plan.conv_steps:
        assert not st.d.flags & L.PTX_BF16_OPERANDS
    for a in plan.acts:
        assert a.t.dtype == torch.float32


def _desc(d, dv=None, ld=None, mode=None):
    dv = d if dv is None else dv
    ld = ((max(d, dv) + 7) // 8 * 8) if ld is None else ld
    x = L.NonlocalDesc()
    x.batch, x.Nq, x.Nk, x.d, x.dv = 2, 100, 50, d, dv
    x.ld_theta = x.ld_phi = x.ld_g = x.ld_y = ld
    x.bs_theta = x.bs_y = 100 * ld
    x.bs_phi = x.bs_g = 50 * ld
    x.mode = (L.PTX_NL_BF16 | L.PTX_NL_SOFTMAX) if mode is None else mode
    return x


def test_abi_bf16_descriptor_gate():
    lib = L.lib()
    assert L.PTX_NL_BF16 == 32 and "ptx_nonlocal_bf16_fwd" in L.SIGNATURES
    assert "ptx_nonlocal_bf16_fwd" in L.header_symbols() and "ptx_nonlocal_bf16_fwd" not in L.EXPERIMENTAL
    assert lib.ptx_nonlocal_supported(C.byref(_desc(1024, 512)))
    assert lib.ptx_nonlocal_supported(C.byref(_desc(8, 3, ld=8)))
    for mode in (L.PTX_NL_BF16 | L.PTX_NL_SCALE, L.PTX_NL_BF16 | L.PTX_NL_SCALE | L.PTX_NL_RELU):
        assert lib.ptx_nonlocal_supported(C.byref(_desc(256, mode=mode)))
    assert not lib.ptx_nonlocal_supported(C.byref(_desc(1032)))
    assert not lib.ptx_nonlocal_supported(C.byref(_desc(64, ld=68)))            # ld % 8 != 0
    bad_bs = _desc(64)
    bad_bs.bs_phi += 4
    assert not lib.ptx_nonlocal_supported(C.byref(bad_bs))
    for mode in (L.PTX_NL_BF16 | L.PTX_NL_RELU, L.PTX_NL_BF16 | L.PTX_NL_F16, L.PTX_NL_BF16 | L.PTX_NL_X3):
        assert not lib.ptx_nonlocal_supported(C.byref(_desc(64, mode=mode)))
    # the fp32 answer is unchanged for fp32 descriptors
    f = _desc(64, ld=68, mode=L.PTX_NL_SOFTMAX)
    assert lib.ptx_nonlocal_supported(C.byref(f))


def test_abi_entry_points_refuse_each_other():
    """Each entry point refuses the other's descriptors (before touching any pointer: dummy addresses are never read)."""
    lib = L.lib()
    fake = C.c_void_p(1 << 20)
    rc = lib.ptx_nonlocal_fwd(C.byref(_desc(64)), fake, fake, fake, fake, None)
    assert rc != 0 and b"ptx_nonlocal_bf16_fwd" in lib.ptx_last_error()
    rc = lib.ptx_nonlocal_bf16_fwd(C.byref(_desc(64, mode=L.PTX_NL_SOFTMAX)), fake, fake, fake, fake, None)
    assert rc != 0 and b"PTX_NL_BF16" in lib.ptx_last_error()
    rc = lib.ptx_nonlocal_bf16_fwd(C.byref(_desc(1032)), fake, fake, fake, fake, None)
    assert rc != 0
