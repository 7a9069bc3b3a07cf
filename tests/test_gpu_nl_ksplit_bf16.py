"""The key-split form of the bf16 attention kernel (variant 1 of include/ptx_amd_nl_ks.h: 8 waves, two key groups on 64-key
tiles, one merge through LDS) through ptx_nonlocal_bf16_variant_fwd: parity against an fp64 CPU computation from the same
bf16 inputs.  The harness is test_gpu_nl_bf16.py's: operands are channel slices of wider rows, y is NaN-filled before the
launch, pad columns up to round8(dv) must be zero and everything outside the slice untouched.  The bar is that file's,
2^-7 max|g| + 2^-7 |ref| (one rounding of P to bf16 against |g|, plus one bf16 ulp of y)."""
import ctypes as C
import os

import pytest
import torch

from pretorched_x_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KMODES = {"softmax": L.PTX_NL_SOFTMAX, "scale": L.PTX_NL_SCALE, "relu": L.PTX_NL_SCALE | L.PTX_NL_RELU}


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _r8(v):
    return (v + 7) // 8 * 8


def _p16(t, offset_elems=0):
    return C.c_void_p(t.data_ptr() + 2 * offset_elems)


def _ref_attention(th, ph, g, kind):
    s = th.double() @ ph.double().transpose(1, 2)
    if kind == "softmax":
        p = torch.softmax(s, -1)
    elif kind == "scale":
        p = s / s.shape[-1]
    else:
        p = s.clamp_min(0) / s.shape[-1]
    return p @ g.double()


def _inputs(d, dv, Nq, Nk, B=3, seed=0):
    gen = torch.Generator().manual_seed(seed + 7 * d + dv)
    amp = (2.0 / d ** 0.5) ** 0.5                    # |s| = |theta . phi| of order 2, rarely above 8
    th = (torch.randn(B, Nq, d, generator=gen) * amp).to(torch.bfloat16)
    ph = (torch.randn(B, Nk, d, generator=gen) * amp).to(torch.bfloat16)
    g = torch.randn(B, Nk, dv, generator=gen).to(torch.bfloat16)
    return th, ph, g


def _launch(data, kind, variant):
    """theta a channel slice at column 8 of a wider row; phi and g slices of one [Nk][phi | g | spare] buffer; y at column 8
    of a NaN-filled row with 16 spare columns.  variant None: ptx_nonlocal_bf16_fwd (the dispatcher's choice)."""
    th, ph, g = data
    (B, Nq, d), Nk, dv = th.shape, ph.shape[1], g.shape[2]
    d8, dv8 = _r8(d), _r8(dv)
    ldt, ldk, ldy = 8 + d8 + 8, d8 + dv8 + 8, 8 + dv8 + 16
    T = torch.zeros(B, Nq, ldt, dtype=torch.bfloat16)
    T[:, :, 8:8 + d] = th
    K = torch.zeros(B, Nk, ldk, dtype=torch.bfloat16)
    K[:, :, :d] = ph
    K[:, :, d8:d8 + dv] = g
    K[:, :, d8 + dv8:] = float("nan")                 # beyond round8: never read
    Td, Kd = T.to(DEV), K.to(DEV)
    Y = torch.full((B, Nq, ldy), float("nan"), dtype=torch.bfloat16, device=DEV)
    desc = L.NonlocalDesc()
    desc.batch, desc.Nq, desc.Nk, desc.d, desc.dv = B, Nq, Nk, d, dv
    desc.ld_theta, desc.ld_phi, desc.ld_g, desc.ld_y = ldt, ldk, ldk, ldy
    desc.bs_theta, desc.bs_phi, desc.bs_g, desc.bs_y = Nq * ldt, Nk * ldk, Nk * ldk, Nq * ldy
    desc.mode = L.PTX_NL_BF16 | KMODES[kind]
    lib = L.lib()
    if variant is None:
        rc = lib.ptx_nonlocal_bf16_fwd(C.byref(desc), _p16(Td, 8), _p16(Kd), _p16(Kd, d8), _p16(Y, 8), _st())
    else:
        assert lib.ptx_nonlocal_bf16_variant_supported(C.byref(desc), variant)
        rc = lib.ptx_nonlocal_bf16_variant_fwd(C.byref(desc), variant, _p16(Td, 8), _p16(Kd), _p16(Kd, d8), _p16(Y, 8), _st())
    assert rc == 0, lib.ptx_last_error()
    torch.cuda.synchronize()
    return Y.cpu()


def _check_kernel(Y, ref, g, dv):
    y = Y[:, :, 8:8 + dv].double()
    assert not torch.isnan(y).any()
    bar = 2.0 ** -7 * float(g.abs().max()) + ref.abs() * 2.0 ** -7
    err = (y - ref).abs()
    assert bool((err <= bar).all()), float((err - bar).max())
    assert bool((Y[:, :, 8 + dv:8 + _r8(dv)].float() == 0).all())         # pad columns up to round8(dv): zeros
    assert bool(torch.isnan(Y[:, :, :8].float()).all())                    # below the slice: untouched
    assert bool(torch.isnan(Y[:, :, 8 + _r8(dv):].float()).all())          # above round8(dv): untouched


# (d, dv, Nq, Nk).  A tile is 64 keys: group 0 takes keys [64 t, 64 t + 32), group 1 keys [64 t + 32, 64 t + 64)
KERNEL_CASES = [
    (256, 256, 70, 33),       # group 0 full, group 1 one key; two query tiles
    (256, 256, 130, 144),     # Nk = 64 k + 16: group 1 sees nothing in the last tile
    (256, 256, 64, 9),        # group 1 sees no key at all: the merge's exp(-inf) path
    (32, 256, 37, 65),        # Nk = 64 k + 1; the widest merge buffer against the smallest key tiles
    (64, 100, 1, 300),        # one query
    (128, 64, 70, 128),       # D = 128, DV = 64; whole tiles only
    (256, 512, 17, 65),       # dv split over blockIdx.y
    (10, 10, 64, 64),         # odd widths
    (256, 256, 70, 96),       # Nk = 64 k + 32: group 1 idle in the last tile, group 0's half exactly full
    (256, 256, 70, 97),       # Nk = 64 k + 33: group 1 owns one key of the last tile
    (256, 128, 64, 32),       # a single half tile, DV = 128
]


@pytest.mark.parametrize("kind", list(KMODES))
@pytest.mark.parametrize("d,dv,Nq,Nk", KERNEL_CASES)
def test_ksplit_kernel_parity(kind, d, dv, Nq, Nk):
    data = _inputs(d, dv, Nq, Nk)
    Y = _launch(data, kind, 1)
    _check_kernel(Y, _ref_attention(*data, kind), data[2], dv)


def test_ksplit_kernel_parity_config3():
    """config 3's layer2 attention shape (2 clips here: the fp64 reference runs on the CPU)."""
    data = _inputs(256, 256, 1568, 1568, B=2)
    Y = _launch(data, "softmax", 1)
    _check_kernel(Y, _ref_attention(*data, "softmax"), data[2], 256)


def test_ksplit_batch_independent():
    """Clip 1 of 3 equals that clip alone, bitwise, under variant 1."""
    th, ph, g = _inputs(256, 256, 200, 200, B=3, seed=5)
    Y3 = _launch((th, ph, g), "softmax", 1)
    Y1 = _launch((th[1:2], ph[1:2], g[1:2]), "softmax", 1)
    assert torch.equal(Y3[1, :, 8:264], Y1[0, :, 8:264])


def test_variant0_is_the_single_group_kernel(monkeypatch):
    """variant_fwd(0) and ptx_nonlocal_bf16_fwd under PTX_NL_BF16_KSPLIT=0 are the same launch; =1 routes the plain call to
    variant 1."""
    data = _inputs(256, 256, 130, 197, seed=2)
    monkeypatch.setenv("PTX_NL_BF16_KSPLIT", "0")
    Y0 = _launch(data, "softmax", None)
    monkeypatch.delenv("PTX_NL_BF16_KSPLIT")
    V0 = _launch(data, "softmax", 0)
    assert torch.equal(Y0[:, :, 8:264], V0[:, :, 8:264])
    monkeypatch.setenv("PTX_NL_BF16_KSPLIT", "1")
    Y1 = _launch(data, "softmax", None)
    monkeypatch.delenv("PTX_NL_BF16_KSPLIT")
    V1 = _launch(data, "softmax", 1)
    assert torch.equal(Y1[:, :, 8:264], V1[:, :, 8:264])
    assert "PTX_NL_BF16_KSPLIT" not in os.environ
