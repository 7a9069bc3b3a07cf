"""Footprint tests of the depthwise 3-D convolution (conv_dw_f32.h, include/ptx_amd_dw.h), every form via
ptx_conv3d_dw_f32_force_form, at the two smallest rows of tests/test_gpu_csn.py::KERNEL_CASES with that module's derived
float64 bound (32 * 2^-24 * (conv(|x|, |w|) + |b|)).  x, the packed filter, the bias and y (a channel slice of a wider row) sit
in a guarded arena (tests/arena.py) at 16 bytes -- the entry refuses less ("conv3d_dw: misaligned pointer (16 bytes)") -- once
under each fill; guards and inputs intact, nothing non-finite written, the neighbour channels of the slice still holding the
fill, bit-identical outputs under the two fills and across the forms (no atomics: nothing is excused)."""
import ctypes as C

import pytest
import torch

from arena import FILLS, assert_finite, assert_holds_fill, assert_same_bits
from footprint import P, ST, run
from test_gpu_csn import KERNEL_CASES, _desc, reference

pytestmark = pytest.mark.gpu

F32 = torch.float32
NAN = float("nan")


@pytest.fixture
def force_form(ptx):
    L = ptx._lib

    def force(form):
        L.check(L.lib().ptx_conv3d_dw_f32_force_form(form), "ptx_conv3d_dw_f32_force_form")
    yield force
    force(0)


@pytest.mark.parametrize("case", KERNEL_CASES[:2], ids=["C4_1x2x3", "C20_s2_odd"])
def test_dw_every_form(ptx, case, force_form):
    L = ptx._lib
    lib = L.lib()
    Cc, dims, s, k, _ = case
    p = tuple(kk // 2 for kk in k)
    g = torch.Generator().manual_seed(Cc + 17)
    N, ldx, c0, tail = 2, Cc + 4, 4, 8
    x = torch.full((N,) + dims + (ldx,), NAN)                       # pad channels of x hold NaN: never read
    x[..., :Cc] = torch.randn((N,) + dims + (Cc,), generator=g)
    w = torch.randn(Cc, 1, *k, generator=g) * 0.3
    bn = (torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1,
          torch.rand(Cc, generator=g) + 0.5)
    out = tuple((i + 2 * p_ - k_) // s_ + 1 for i, p_, k_, s_ in zip(dims, p, k, s))
    taps = k[0] * k[1] * k[2]
    ldy = c0 + Cc + tail
    d = _desc(L, N, Cc, dims, out, k, s, p, ldx, ldy, True)
    assert lib.ptx_conv3d_dw_f32_supported(C.byref(d)) == 1, lib.ptx_last_error().decode()

    # the pack runs in the arena as well: w and the BN vectors in, the tap-major filter and the bias out
    def pack(v, ar):
        L.check(lib.ptx_pack_dw_weight_f32(Cc, k[0], k[1], k[2], P(v["w"]), None, P(v["gamma"]), P(v["beta"]), P(v["mean"]), P(v["var"]),
                                           C.c_float(1e-3), P(v["wp"]), P(v["bp"]), ST()), "ptx_pack_dw_weight_f32")

    # (a scalar kernel behind an entry that checks no pointer: everything at 4 bytes)
    packed = run([("w", w, None, 4, "in")] + [(n, t, None, 4, "in") for n, t in zip(("gamma", "beta", "mean", "var"), bn)] +
                 [("wp", (taps, Cc), F32, 4, "out"), ("bp", (Cc,), F32, 4, "out")], pack)
    for name in ("wp", "bp"):
        assert_finite(packed[0][name], name)
        assert_same_bits(packed[0][name], packed[1][name], name)
    wp, bp = packed[0]["wp"], packed[0]["bp"]
    scale = bn[0].double() / (bn[3].double() + 1e-3).sqrt()
    want_w = (w.double().reshape(Cc, -1) * scale[:, None]).t()
    assert ((wp.double() - want_w).abs() <= 4 * 2.0 ** -24 * want_w.abs()).all()          # test_dw_kernel_against_float64's bars
    want_b = bn[1].double() - bn[2].double() * scale
    assert ((bp.double() - want_b).abs() <= 4 * 2.0 ** -24 * (bn[1].abs() + (bn[2] * scale).abs()).double() + 1e-30).all()

    def launch(v, ar):
        L.check(lib.ptx_conv3d_dw_f32_fwd(C.byref(d), P(v["x"]), P(v["wp"]), P(v["bp"]), P(v["y"], c0), ST()), "ptx_conv3d_dw_f32_fwd")

    ref, bound = reference(x, wp, bp, k, s, p, relu=True)
    first = None
    for form in (0, L.PTX_DW_FORM_STRIP4, L.PTX_DW_FORM_STRIP8, L.PTX_DW_FORM_LDS):
        force_form(form)
        res = run([("x", x, None, 16, "in"), ("wp", wp, None, 16, "in"), ("bp", bp, None, 16, "in"),
                   ("y", (N,) + out + (ldy,), F32, 16, "out")], launch)
        for o, fill in zip(res, FILLS):
            y = o["y"]
            got = y[..., c0:c0 + Cc]
            assert_finite(got, "y (form %d)" % form)
            assert ((got.double() - ref).abs() <= bound).all(), (case, form)
            assert_holds_fill(y[..., :c0], fill, "y: channels below the slice (form %d)" % form)
            assert_holds_fill(y[..., c0 + Cc:], fill, "y: channels above the slice (form %d)" % form)
        assert_same_bits(res[0]["y"][..., c0:c0 + Cc], res[1]["y"][..., c0:c0 + Cc], "y (form %d)" % form)
        first = res[0]["y"][..., c0:c0 + Cc] if first is None else first
        assert torch.equal(res[0]["y"][..., c0:c0 + Cc], first), (case, form)
