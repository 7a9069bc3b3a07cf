"""bf16 non-local blocks on the GPU: parity of the bf16 attention kernel (ptx_nonlocal_bf16_fwd) against an fp64 CPU
computation from the same bf16 inputs, block and MNISTNonLocalNet parity calibrated against PyTorch's own bf16 arithmetic,
and the public API of a bf16 block.  Output buffers are NaN-filled before a launch, so a kernel that leaves a column it
owns unwritten fails, and one that writes past round8(dv) fails too."""
import ctypes as C
import itertools

import pytest
import torch

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import PtxError
from pretorched_x_amd.testing import synth_state_dict
from oracle import functional as OF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("embedded_gaussian", "dot_product", "gaussian", "concatenation")
COMBOS = list(itertools.product(MODES, (False, True), (False, True)))        # (mode, sub_sample, bn_layer)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _r8(v):
    return (v + 7) // 8 * 8


def _p16(t, offset_elems=0):
    """Device address of element `offset_elems` of a bf16 tensor."""
    return C.c_void_p(t.data_ptr() + 2 * offset_elems)


# ------------------------------------------------------------------------------------------------ kernel parity
KMODES = {"softmax": L.PTX_NL_SOFTMAX, "scale": L.PTX_NL_SCALE, "relu": L.PTX_NL_SCALE | L.PTX_NL_RELU}


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


def _run_kernel(kind, d, dv, Nq, Nk, B=3, seed=0, data=None):
    """theta a channel slice at column 8 of a wider row; phi and g slices of one [Nk][phi | g | spare] buffer; y at
    column 8 of a NaN-filled row with 16 spare columns.  Pad columns up to round8 are zero, as the contract asks."""
    th, ph, g = _inputs(d, dv, Nq, Nk, B, seed) if data is None else data
    B = th.shape[0]
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
    assert lib.ptx_nonlocal_supported(C.byref(desc))
    rc = lib.ptx_nonlocal_bf16_fwd(C.byref(desc), _p16(Td, 8), _p16(Kd), _p16(Kd, d8), _p16(Y, 8), _st())
    assert rc == 0, lib.ptx_last_error()
    torch.cuda.synchronize()
    return Y.cpu(), _ref_attention(th, ph, g, kind), g


def _check_kernel(Y, ref, g, dv):
    y = Y[:, :, 8:8 + dv].double()
    assert not torch.isnan(y).any()
    bar = 2.0 ** -7 * float(g.abs().max()) + ref.abs() * 2.0 ** -7        # + one bf16 ulp of y
    err = (y - ref).abs()
    assert bool((err <= bar).all()), float((err - bar).max())
    assert bool((Y[:, :, 8 + dv:8 + _r8(dv)].float() == 0).all())         # pad columns up to round8(dv): zeros
    assert bool(torch.isnan(Y[:, :, :8].float()).all())                    # below the slice: untouched
    assert bool(torch.isnan(Y[:, :, 8 + _r8(dv):].float()).all())          # above round8(dv): untouched


KERNEL_CASES = [(d, dv, Nq, Nk) for d, dv in itertools.product((8, 64, 256, 512, 1024), (8, 256, 512))
                for Nq, Nk in ((70, 33),)] + [(256, 256, 130, 197), (3, 3, 37, 9), (10, 10, 64, 64), (64, 100, 1, 300),
                                              (1024, 512, 17, 65)]


@pytest.mark.parametrize("kind", list(KMODES))
@pytest.mark.parametrize("d,dv,Nq,Nk", KERNEL_CASES)
def test_bf16_attention_kernel_parity(kind, d, dv, Nq, Nk):
    Y, ref, g = _run_kernel(kind, d, dv, Nq, Nk)
    _check_kernel(Y, ref, g, dv)


@pytest.mark.parametrize("d,N", [(256, 1568), (512, 196)])
def test_bf16_attention_kernel_parity_config3(d, N):
    """config 3's layer2 / layer3 attention shapes (2 clips here: the fp64 reference runs on the CPU)."""
    Y, ref, g = _run_kernel("softmax", d, d, N, N, B=2)
    _check_kernel(Y, ref, g, d)


def test_bf16_attention_batch_independent():
    """A clip's bits do not depend on the batch it arrives in: the variant is chosen from per-sample extents."""
    th, ph, g = _inputs(256, 256, 200, 200, B=3, seed=5)
    Y3, _, _ = _run_kernel("softmax", 256, 256, 200, 200, data=(th, ph, g))
    Y1, _, _ = _run_kernel("softmax", 256, 256, 200, 200, data=(th[1:2], ph[1:2], g[1:2]))
    assert torch.equal(Y3[1, :, 8:264], Y1[0, :, 8:264])


# ------------------------------------------------------------------------------------------------ block parity
def _shape(dim, C_):
    return {3: (2, C_, 4, 6, 6), 2: (2, C_, 8, 8), 1: (2, C_, 20)}[dim]


def _setup_block(dim, C_, mode, sub, bn, seed=3):
    cls = {1: ptx.NonLocalBlock1D, 2: ptx.NonLocalBlock2D, 3: ptx.NonLocalBlock3D}[dim]
    m = cls(C_, mode=mode, sub_sample=sub, bn_layer=bn)
    sd = synth_state_dict(m.state_dict(), 1234 + C_)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    m.load_state_dict(sd)
    m = m.eval().to(torch.bfloat16).to(DEV)
    gen = torch.Generator().manual_seed(seed)
    amp = 0.1 if mode == "gaussian" else 1.0          # theta = phi = x: keep the logits x . x moderate
    x = (torch.randn(*_shape(dim, C_), generator=gen) * amp).to(torch.bfloat16)
    return m, sd, x


def _block_bars(sd, x, mode, sub, bn):
    sdp = {("." + k): v for k, v in sd.items()}                    # the oracle addresses keys as prefix + ".name"
    ref = OF.nonlocal_block(sdp, x.float(), "", mode=mode, sub_sample=sub, bn_layer=bn)
    sd16 = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in sdp.items()}
    torch_bf16 = OF.nonlocal_block(sd16, x, "", mode=mode, sub_sample=sub, bn_layer=bn).float()
    err_torch = float((torch_bf16 - ref).abs().max())
    return ref, 2 * err_torch + 1e-3 * float(ref.abs().max())


def _check_block(m, sd, x, mode, sub, bn):
    ref, bar = _block_bars(sd, x, mode, sub, bn)
    with torch.no_grad():
        out = m(x.to(DEV))
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and out.shape == x.shape
    err = float((out.float().cpu() - ref).abs().max())
    assert err <= bar, (err, bar)
    assert not torch.equal(out.cpu(), x)                          # W is not at its zero init: the block changes x


@pytest.mark.parametrize("C_", [16, 512, 1024])
@pytest.mark.parametrize("mode,sub,bn", COMBOS)
def test_bf16_block3d_parity(mode, sub, bn, C_):
    m, sd, x = _setup_block(3, C_, mode, sub, bn)
    _check_block(m, sd, x, mode, sub, bn)


@pytest.mark.parametrize("dim", [1, 2])
@pytest.mark.parametrize("C_", [16, 512])
@pytest.mark.parametrize("mode,sub,bn", COMBOS)
def test_bf16_block_1d_2d_parity(dim, C_, mode, sub, bn):
    m, sd, x = _setup_block(dim, C_, mode, sub, bn)
    _check_block(m, sd, x, mode, sub, bn)


@pytest.mark.parametrize("C_", [6, 20])
@pytest.mark.parametrize("mode,sub,bn", COMBOS)
def test_bf16_block_odd_width_parity(mode, sub, bn, C_):
    m, sd, x = _setup_block(3, C_, mode, sub, bn)
    _check_block(m, sd, x, mode, sub, bn)


# ------------------------------------------------------------------------------------------------ MNIST
def test_bf16_mnist_parity():
    m = ptx.MNISTNonLocalNet()
    sd = synth_state_dict(m.state_dict(), 77)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    m.load_state_dict(sd)
    m = m.eval().to(torch.bfloat16).to(DEV)
    x = torch.randn(8, 1, 28, 28, generator=torch.Generator().manual_seed(11)).to(torch.bfloat16)
    ref = OF.mnist_nonlocal_forward(sd, x.float())
    sd16 = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in sd.items()}
    torch_bf16 = OF.mnist_nonlocal_forward(sd16, x).float()
    bar = 2 * float((torch_bf16 - ref).abs().max()) + 1e-3 * float(ref.abs().max())
    with torch.no_grad():
        out = m(x.to(DEV))
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and out.shape == (8, 10)
    o = out.float().cpu()
    assert float((o - ref).abs().max()) <= bar, (float((o - ref).abs().max()), bar)
    top2 = ref.topk(2, 1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * bar
    assert torch.equal(o.argmax(1)[sure], ref.argmax(1)[sure])


# ------------------------------------------------------------------------------------------------ API
def test_bf16_block_api():
    m, sd, x = _setup_block(3, 64, "embedded_gaussian", True, True)
    xd = x.to(DEV)
    eng = m.engine()
    with torch.no_grad():
        out = m(xd)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and out.shape == xd.shape
    # dtype mismatches raise both ways
    with pytest.raises(PtxError):
        m(xd.float())
    m32 = ptx.NonLocalBlock3D(64, sub_sample=True).eval().to(DEV)
    with pytest.raises(PtxError):
        m32(xd)
    # graph replay equals eager bitwise
    eng.use_graph = True
    with torch.no_grad():
        g1 = m(xd)
        g2 = m(xd)
    eng.use_graph = False
    torch.cuda.synchronize()
    assert torch.equal(g1, out) and torch.equal(g2, out)
    # batch independence: sample 1 of a batch of 3 equals that sample alone, bitwise
    x3 = torch.cat([xd, xd[:1] * 0.5], 0)
    with torch.no_grad():
        o3 = m(x3)
        o1 = m(x3[1:2].contiguous())
    assert torch.equal(o3[1:2], o1)
    # an in-place update of W[1].weight changes the output
    with torch.no_grad():
        m.W[1].weight.mul_(1.5)
        out2 = m(xd)
    assert not torch.equal(out2, out)
    # a .data edit is seen under check_weights = "checksum"
    eng.check_weights = "checksum"
    with torch.no_grad():
        base = m(xd)
        m.W[1].bias.data.add_(0.25)
        out3 = m(xd)
    assert not torch.equal(out3, base)
