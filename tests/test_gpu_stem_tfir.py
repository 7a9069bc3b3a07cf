"""GPU tests of the fp32 stem as a fast FIR along time (csrc/conv_stem_tfir_f32.hip, include/ptx_amd_tfir.h): every scheme,
driven through ctypes into NaN-filled buffers, against float64 conv3d + batch_norm + relu on the CPU, against the direct stem
kernel on the same buffers, and bit-for-bit across two launches."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCHEMES = (1, 2, 3)
# error bar against the float64 reference, x max|ref|: about 10x the fp32 emulation of the schemes (8.9e-7 for 1 and 2, 4.4e-6
# for 3); the direct kernel's is set the same way from its emulated 2.1e-7
BAR = {1: 1e-5, 2: 1e-5, 3: 5e-5}
BAR_DIRECT = 2e-6
GUARD = 4096       # floats past the end of y that must stay untouched

# name: (N, Ti, H, W, Co, spatial stride, frame step of the source tensor)
CASES = {
    "short_clip": (1, 4, 16, 16, 64, 2, 1),          # Ti < kT: every group mixes padding
    "ragged_groups": (2, 9, 20, 24, 64, 2, 1),       # To % m == 1 for both m, one partial tile
    "two_tiles": (1, 6, 36, 40, 96, 2, 1),           # two row tiles, the second partial; a ragged second channel tile
    "pitch_stride1": (1, 5, 18, 22, 40, 1, 1),       # W % 4 != 0 (pitch 24), stride 1, ragged channels inside the first tile
    "one_frame": (1, 1, 16, 16, 64, 2, 1),           # To == 1
    "frame_stride": (1, 4, 16, 16, 64, 2, 2),        # short_clip read as x[:, :, ::2] of an 8-frame tensor
    "wide_patch": (1, 2, 8, 248, 64, 2, 1),          # 11 x 256 patch = 2112 pieces: the 12-pieces-per-thread kernels
}


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _r4(v):
    return (v + 3) // 4 * 4


def _rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Inputs and the float64 reference of a case, computed once: (x as stored [N,3,Ti*step,H,pitch], w, bn, ref NCDHW)."""
    N, Ti, H, W, Co, s, step = CASES[name]
    full = _rnd(N, 3, Ti * step, H, W, seed=310)
    w = _rnd(Co, 3, 7, 7, 7, seed=311, scale=(3 * 343) ** -0.5)
    g = torch.Generator().manual_seed(312)
    bn = (torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.1, torch.randn(Co, generator=g) * 0.1,
          torch.rand(Co, generator=g) + 0.5, 1e-5)
    x = full[:, :, ::step].double()
    y = F.conv3d(x, w.double(), None, (1, s, s), (3, 3, 3))
    y = F.batch_norm(y, bn[2].double(), bn[3].double(), bn[0].double(), bn[1].double(), False, 0.1, bn[4])
    ref = F.relu(y)
    stored = F.pad(full, (0, _r4(W) - W)).contiguous()         # rows at a 16-byte pitch, zero pad columns
    return stored, w, bn, ref


@functools.lru_cache(maxsize=None)
def _device_side(name):
    """The case on the device, once: descriptor, strides, x, packed direct filter, bias, and the direct kernel's y (with its
    guard tail)."""
    import pretorched_x_amd as ptx
    L = ptx._lib
    lib = L.lib()
    N, Ti, H, W, Co, s, step = CASES[name]
    stored, w, bn, ref = _problem(name)
    To, Ho, Wo = ref.shape[2:]
    pitch = _r4(W)
    Co_pad, Kc = (Co + 127) // 128 * 128, 24
    pd = L.PackDesc(Co, 3, 7, 7, 7, Kc, Co_pad, 1)
    wf = torch.empty(lib.ptx_packed_weight_elems(C.byref(pd)), device=DEV)
    bp = torch.empty(Co_pad, device=DEV)
    ts = [t.to(DEV) for t in bn[:4]]
    wd = w.contiguous().to(DEV)
    L.check(lib.ptx_pack_conv_weight(C.byref(pd), _p(wd), None, _p(ts[0]), _p(ts[1]), _p(ts[2]), _p(ts[3]), C.c_float(bn[4]),
                                     _p(wf), _p(bp), _st()), "pack folded")
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, Ti, H, W, 3, (pitch if pitch != W else 0)
    d.To, d.Ho, d.Wo, d.Co, d.ldy = To, Ho, Wo, Co, _r4(Co)
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = 7, 7, 7, 1, s, s, 3, 3, 3
    d.Kc, d.Co_pad, d.flags = Kc, Co_pad, L.PTX_EPI_RELU
    plane = H * pitch
    strides = (3 * Ti * step * plane, Ti * step * plane, step * plane)
    assert lib.ptx_conv_stem_f32_supported(C.byref(d), *strides), name
    xd = stored.to(DEV)
    ws = torch.full((lib.ptx_stem_f32_weight_elems(C.byref(d)),), float("nan"), device=DEV)
    L.check(lib.ptx_pack_stem_f32_weight(C.byref(d), _p(wf), Kc, _p(ws), _st()), "pack stem f32")
    yd = torch.full((N * To * Ho * Wo * d.ldy + GUARD,), float("nan"), device=DEV)
    L.check(lib.ptx_conv_stem_f32_fwd(C.byref(d), _p(xd), *strides, _p(ws), _p(bp), _p(yd), _st()), "stem f32")
    torch.cuda.synchronize()
    return d, strides, xd, ws, bp, yd.cpu()


def _ncdhw(flat, d):
    n = d.N * d.To * d.Ho * d.Wo * d.ldy
    return flat[:n].reshape(d.N, d.To, d.Ho, d.Wo, d.ldy)[..., :d.Co].permute(0, 4, 1, 2, 3).double()


def test_scheme_tables_on_device_library(ptx):
    """The loaded library reports the three schemes with the documented sizes."""
    lib = ptx._lib.lib()
    for sid, (m, P) in zip(SCHEMES, ((2, 8), (4, 13), (4, 10))):
        mm, pp = C.c_int32(), C.c_int32()
        assert lib.ptx_stem_tfir_scheme(sid, C.byref(mm), C.byref(pp), None, None, None) == 0
        assert (mm.value, pp.value) == (m, P)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_stem_tfir_against_reference_direct_and_itself(ptx, case, scheme):
    """ptx_stem_tfir_in_f32 + ptx_conv_stem_tfir_f32_fwd into NaN-filled V and y: within BAR[scheme] x max|ref| of the float64
    reference, within that plus the direct kernel's own bar of ptx_conv_stem_f32_fwd, bit-identical across two launches, and
    every float the direct kernel leaves untouched (pad columns, the guard tail) left untouched here too.
    Measured on MI355X (max over the cases, x max|ref|): see DESIGN.md 3.30."""
    L = ptx._lib
    lib = L.lib()
    d, strides, xd, ws, bp, y_direct = _device_side(case)
    ref = _problem(case)[3]
    scale = ref.abs().max().item()
    assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(d), *strides, scheme) == 1
    wt = torch.full((lib.ptx_stem_tfir_f32_weight_elems(C.byref(d), scheme),), float("nan"), device=DEV)
    L.check(lib.ptx_pack_stem_tfir_f32_weight(C.byref(d), scheme, _p(ws), _p(wt), _st()), "pack tfir")
    v_elems = lib.ptx_stem_tfir_f32_workspace_bytes(C.byref(d), scheme) // 4
    outs = []
    for _ in range(2):
        V = torch.full((v_elems + GUARD,), float("nan"), device=DEV)
        y = torch.full_like(y_direct, float("nan"), device=DEV)
        L.check(lib.ptx_stem_tfir_in_f32(C.byref(d), scheme, _p(xd), *strides, _p(V), _st()), "tfir in")
        L.check(lib.ptx_conv_stem_tfir_f32_fwd(C.byref(d), scheme, _p(V), _p(wt), _p(bp), _p(y), _st()), "tfir fwd")
        torch.cuda.synchronize()
        outs.append((V.cpu(), y.cpu()))
    (V0, y0), (V1, y1) = outs
    assert not torch.isnan(V0[:v_elems]).any() and bool(torch.isnan(V0[v_elems:]).all())       # V: all of it, nothing past it
    assert torch.equal(torch.isnan(y0), torch.isnan(y_direct))      # the floats the direct kernel writes, no others
    assert torch.equal(V0[:v_elems], V1[:v_elems]) and torch.equal(torch.nan_to_num(y0), torch.nan_to_num(y1))
    got, direct = _ncdhw(y0, d), _ncdhw(y_direct, d)
    err_ref = (got - ref).abs().max().item() / scale
    err_direct = (got - direct).abs().max().item() / scale
    err_direct_ref = (direct - ref).abs().max().item() / scale
    print("tfir %-14s scheme %d: vs float64 %.3e  vs direct %.3e  (direct vs float64 %.3e)" % (case, scheme, err_ref, err_direct, err_direct_ref))
    assert err_direct_ref <= BAR_DIRECT
    assert err_ref <= BAR[scheme], (case, scheme, err_ref)
    assert err_direct <= BAR[scheme] + BAR_DIRECT, (case, scheme, err_direct)
    pad = y0[:d.N * d.To * d.Ho * d.Wo * d.ldy].reshape(-1, d.ldy)[:, d.Co:]
    pad_direct = y_direct[:d.N * d.To * d.Ho * d.Wo * d.ldy].reshape(-1, d.ldy)[:, d.Co:]
    assert torch.equal(torch.nan_to_num(pad, nan=-1.0), torch.nan_to_num(pad_direct, nan=-1.0))


def test_stem_tfir_refusals(ptx):
    """Refused with PTX_ERR_UNSUPPORTED, not mis-computed: a temporal stride, a (1,7,7) stem, an unknown scheme."""
    L = ptx._lib
    lib = L.lib()
    d0, strides, xd, ws, bp, y_direct = _device_side("short_clip")
    d = L.ConvDesc.from_buffer_copy(d0)
    V = torch.full((lib.ptx_stem_tfir_f32_workspace_bytes(C.byref(d), 2) // 4,), float("nan"), device=DEV)
    y = torch.full_like(y_direct, float("nan"), device=DEV)
    wt = torch.zeros(lib.ptx_stem_tfir_f32_weight_elems(C.byref(d), 2), device=DEV)
    for edit in (dict(sT=2, To=2), dict(kT=1, pT=0), dict(flags=L.PTX_EPI_RELU | L.PTX_EPI_RES_ADD)):
        d = L.ConvDesc.from_buffer_copy(d0)
        for k, v in edit.items():
            setattr(d, k, v)
        assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(d), *strides, 2) == 0, edit
        assert lib.ptx_stem_tfir_in_f32(C.byref(d), 2, _p(xd), *strides, _p(V), _st()) == 2
        assert lib.ptx_conv_stem_tfir_f32_fwd(C.byref(d), 2, _p(V), _p(wt), _p(bp), _p(y), _st()) == 2
    for bad in (0, 4):
        assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(d0), *strides, bad) == 0
        assert lib.ptx_conv_stem_tfir_f32_fwd(C.byref(d0), bad, _p(V), _p(wt), _p(bp), _p(y), _st()) == 2
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(V).all())
