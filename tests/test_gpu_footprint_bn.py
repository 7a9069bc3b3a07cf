"""Footprint tests of the batch-statistics BatchNorm entry points (bn_batch.hip, include/ptx_amd_bn.h) at the smallest cases of
tests/test_gpu_update_bn.py, whose bars these are: operands and the workspace in a guarded arena (tests/arena.py), once
under each fill; guards and inputs intact, nothing non-finite written, the layout contract, float64 references,
bit-identical outputs under the two fills (no atomics in these kernels: nothing is excused).

Alignment: x / raw / y / res and the workspace 16 bytes (header, and "bn_batch_stats: x must be 16-byte aligned",
"bn_apply: misaligned pointer"); the per-channel vectors (mean, var, gamma, beta, running statistics, scale, shift) are read
and written one float at a time and neither documented nor checked: 4 bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

from arena import FILLS, assert_finite, assert_holds_fill, assert_same_bits
from footprint import P, ST, run
from test_gpu_update_bn import _check_moments, _noise

pytestmark = pytest.mark.gpu

F32 = torch.float32


@pytest.mark.parametrize("rows,C_,ld,pad_nan", [(2, 4, 4, False), (7, 20, 24, True), (300, 22, 28, True)])
def test_batch_stats(ptx, rows, C_, ld, pad_nan):
    """K1's two smallest rows, and one whose last channel quad is half pad (C = 22: channels 22, 23 are read inside the quad and
    must influence nothing, 24..27 are never read) over more than one workgroup row.  The workspace is scratch (not zeroed)."""
    L, lib = ptx._lib, ptx._lib.lib()
    x = _noise(rows, C_, ld, 11 + rows, pad_nan)
    n = int(lib.ptx_bn_batch_stats_workspace_bytes(rows, C_))
    assert n > 0 and n % 16 == 0

    def launch(v, ar):
        L.check(lib.ptx_bn_batch_stats_f32(P(v["x"]), rows, C_, ld, P(v["mean"]), P(v["var"]), P(v["ws"]), n, ST()), "bn_batch_stats")

    res = run([("x", x, None, 16, "in"), ("ws", (n // 4,), F32, 16, "scratch"), ("mean", (C_,), F32, 4, "out"),
               ("var", (C_,), F32, 4, "out")], launch)
    for out in res:
        _check_moments(x, C_, out["mean"].numpy().astype(np.float64), out["var"].numpy().astype(np.float64))
    assert_same_bits(res[0]["mean"], res[1]["mean"], "mean")
    assert_same_bits(res[0]["var"], res[1]["var"], "var")


def test_batch_update(ptx):
    """K4 at n = 2, f = 0.5: the running statistics are `inout`, everything at 4 bytes."""
    L, lib = ptx._lib, ptx._lib.lib()
    C_, n, f, eps = 70, 2, 0.5, 1e-5
    g = torch.Generator().manual_seed(17)
    mean, var = torch.rand(C_, generator=g) * 2 - 1, torch.rand(C_, generator=g) * 1.5 + 0.5
    gamma, beta = torch.rand(C_, generator=g) + 0.5, (torch.rand(C_, generator=g) + 3.0) * torch.sign(torch.randn(C_, generator=g))
    rm0, rv0 = torch.randn(C_, generator=g), torch.rand(C_, generator=g) + 0.5

    def launch(v, ar):
        L.check(lib.ptx_bn_batch_update_f32(P(v["mean"]), P(v["var"]), n, C.c_float(f), C.c_float(eps), P(v["gamma"]), P(v["beta"]),
                                            P(v["rm"]), P(v["rv"]), P(v["scale"]), P(v["shift"]), C_, ST()), "bn_batch_update")

    res = run([("mean", mean, None, 4, "in"), ("var", var, None, 4, "in"), ("gamma", gamma, None, 4, "in"), ("beta", beta, None, 4, "in"),
               ("rm", rm0, None, 4, "inout"), ("rv", rv0, None, 4, "inout"), ("scale", (C_,), F32, 4, "out"),
               ("shift", (C_,), F32, 4, "out")], launch)
    m64, v64, g64, b64, rm64, rv64 = (t.numpy().astype(np.float64) for t in (mean, var, gamma, beta, rm0, rv0))
    f64, eps64 = float(np.float32(f)), float(np.float32(eps))
    want_scale = g64 / np.sqrt(v64 + eps64)
    want_shift = b64 - m64 * want_scale
    want_rm = (1 - f64) * rm64 + f64 * m64
    want_rv = (1 - f64) * rv64 + f64 * v64 * n / (n - 1)
    for out in res:
        got = [out[k].numpy().astype(np.float64) for k in ("scale", "shift", "rm", "rv")]
        assert all(np.isfinite(a).all() for a in got)
        assert (np.abs(got[0] - want_scale) / np.abs(want_scale)).max() <= 2e-6
        assert (np.abs(got[1] - want_shift) / np.abs(want_shift)).max() <= 2e-6
        assert (np.abs(got[2] - want_rm) / (np.abs(want_rm) + np.sqrt(want_rv))).max() <= 1e-6
        assert (np.abs(got[3] - want_rv) / want_rv).max() <= 2e-5
    for k in ("scale", "shift", "rm", "rv"):
        assert_same_bits(res[0][k], res[1][k], k)


@pytest.mark.parametrize("kind", ["none", "add", "padA"])
def test_apply(ptx, kind):
    """K5 with ReLU: ld = 28 > round_up(22, 4), so columns [24, 28) of y keep the fill and [22, 24) are written as zero; the
    shortcut-A residual's pad channels hold NaN.  Bar: 4 * 2^-24 (|raw * scale| + |shift| + |res|) per element."""
    L, lib = ptx._lib, ptx._lib.lib()
    N, T, H, W, C_, ld = 2, 3, 5, 7, 22, 28
    g = torch.Generator().manual_seed(23)
    raw = torch.randn(N, T, H, W, ld, generator=g) * 3
    scale, shift = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
    d = L.BnApplyDesc()
    d.N, d.T, d.H, d.W, d.C, d.ldx, d.ldy = N, T, H, W, C_, ld, ld
    d.flags = L.PTX_EPI_RELU
    want = raw[..., :C_].double() * scale.double() + shift.double()
    bound = (raw[..., :C_].double() * scale.double()).abs() + shift.double().abs()
    specs = [("raw", raw, None, 16, "in"), ("scale", scale, None, 4, "in"), ("shift", shift, None, 4, "in")]
    if kind == "add":
        r = torch.randn(N, T, H, W, ld, generator=g)
        d.flags |= L.PTX_EPI_RES_ADD
        d.ldr = ld
        want, bound = want + r[..., :C_].double(), bound + r[..., :C_].double().abs()
        specs.append(("res", r, None, 16, "in"))
    elif kind == "padA":
        rT, rH, rW, rC, ldr = 2 * T - 1, 2 * H, 2 * W - 1, 10, 12
        r = torch.full((N, rT, rH, rW, ldr), float("nan"))
        r[..., :rC] = torch.randn(N, rT, rH, rW, rC, generator=g)
        d.flags |= L.PTX_EPI_RES_PADA
        d.ldr, d.res_C, d.res_T, d.res_H, d.res_W = ldr, rC, rT, rH, rW
        d.res_sT = d.res_sH = d.res_sW = 2
        sub = r[:, ::2, ::2, ::2, :rC].double()
        want[..., :rC] += sub
        bound[..., :rC] += sub.abs()
        specs.append(("res", r, None, 16, "in"))
    want = want.clamp_min(0)
    specs.append(("y", (N, T, H, W, ld), F32, 16, "out"))

    def launch(v, ar):
        L.check(lib.ptx_bn_apply_f32(C.byref(d), P(v["raw"]), P(v["scale"]), P(v["shift"]), P(v["res"]) if "res" in v else None,
                                     P(v["y"]), ST()), "bn_apply")

    res = run(specs, launch)
    for out, fill in zip(res, FILLS):
        y = out["y"]
        assert_finite(y[..., :24], "y")
        assert bool(((y[..., :C_].double() - want).abs() <= 4 * 2.0 ** -24 * bound).all())
        assert bool((y[..., C_:24] == 0).all())
        assert_holds_fill(y[..., 24:], fill, "y: columns past the last channel quad")
    assert_same_bits(res[0]["y"][..., :24], res[1]["y"][..., :24], "y")
