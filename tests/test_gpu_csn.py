"""GPU tests of the depthwise 3-D convolution (include/ptx_amd_dw.h) and of the channel-separated networks built on it (ir_csn50 ..
ip_csn152).  The kernel is held to float64 on the PACKED fp32 operands within a bound that is derived, not measured; every buffer of
a direct launch is NaN-filled first and the output is a channel slice of a wider tensor whose neighbours must stay NaN.  The models
are held to tests/csn_oracle.py (torch.nn.functional on the CPU, fp32) at the bar of the other fp32 families."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import csn_oracle as O
from pretorched_x_amd.testing import synth_frames, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3          # max |logits_gpu - logits_cpu| of the fp32 families (BASELINE.json north_star), with equal argmax
MARGIN = 2e-3       # ... and the oracle's own top-2 margin must exceed twice that: a flipped argmax cannot hide behind a near-tie
NAN = float("nan")
OPTS = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], input_size=[3, 64, 64])


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr())


# --------------------------------------------------------------------------------------------- 1. the kernel, direct launches
# (C, (T, H, W), stride, taps): every window touches every padding | odd extents, stride 2, C no multiple of a wave's 64 quads |
# an 8-column strip boundary (70 = 8 * 8 + 6) and a ragged channel group (68 = 17 quads) | mixed strides, 4-column strips |
# (1,3,3) and (3,1,1) taps | 8-column strips at stride 2 along W (3 taps, then 1) | no padding at all
KERNEL_CASES = [
    (4, (1, 2, 3), (1, 1, 1), (3, 3, 3), None),
    (20, (5, 9, 11), (2, 2, 2), (3, 3, 3), None),
    (68, (3, 8, 70), (1, 1, 1), (3, 3, 3), None),
    (128, (4, 14, 14), (2, 1, 1), (3, 3, 3), None),
    (8, (3, 6, 10), (1, 2, 2), (1, 3, 3), None),
    (8, (4, 5, 6), (2, 1, 1), (3, 1, 1), None),
    (12, (2, 4, 37), (1, 1, 2), (3, 3, 3), None),
    (12, (3, 3, 40), (1, 2, 2), (3, 1, 1), None),
    (20, (5, 9, 11), (1, 1, 1), (3, 3, 3), (0, 0, 0)),
]


def _desc(L, N, Cc, dims, out, k, s, p, ldx, ldy, relu):
    d = L.ConvDesc()
    d.N, (d.Ti, d.Hi, d.Wi), d.Ci, d.ldx = N, dims, Cc, ldx
    (d.To, d.Ho, d.Wo), d.Co, d.ldy = out, Cc, ldy
    (d.kT, d.kH, d.kW), (d.sT, d.sH, d.sW), (d.pT, d.pH, d.pW) = k, s, p
    d.groups, d.flags = Cc, (L.PTX_EPI_RELU if relu else 0)
    return d


def run_dw(ptx, x, w, bn, eps, s, p, relu, c0=4, tail=8):
    """Pack and launch through ctypes.  x [N, T, H, W, ldx] (channels-last, pad channels NaN), w [C, 1, kT, kH, kW], bn = (gamma,
    beta, mean, var) or None.  Returns (y [N, To, Ho, Wo, c0 + C + tail] with the launch's slice at [c0, c0 + C), packed w, bias)."""
    L = ptx._lib
    lib = L.lib()
    N, T, H, W, ldx = x.shape
    Cc, k = w.shape[0], tuple(w.shape[2:])
    out = tuple((i + 2 * p_ - k_) // s_ + 1 for i, p_, k_, s_ in zip((T, H, W), p, k, s))
    taps = k[0] * k[1] * k[2]
    wp = torch.full((taps, Cc), NAN, device=DEV)
    bp = torch.full((Cc,), NAN, device=DEV)
    d_w = w.to(DEV)
    d_bn = [t.to(DEV) for t in bn] if bn is not None else [None] * 4
    L.check(lib.ptx_pack_dw_weight_f32(Cc, k[0], k[1], k[2], ptr(d_w), None, *[ptr(t) if t is not None else None for t in d_bn],
                                       C.c_float(eps), ptr(wp), ptr(bp), stream()), "ptx_pack_dw_weight_f32")
    ldy = c0 + Cc + tail
    y = torch.full((N,) + out + (ldy,), NAN, device=DEV)
    d = _desc(L, N, Cc, (T, H, W), out, k, s, p, ldx, ldy, relu)
    assert lib.ptx_conv3d_dw_f32_supported(C.byref(d)) == 1, lib.ptx_last_error().decode()
    x_dev = x.to(DEV)
    L.check(lib.ptx_conv3d_dw_f32_fwd(C.byref(d), ptr(x_dev), ptr(wp), ptr(bp), C.c_void_p(y.data_ptr() + 4 * c0), stream()),
            "ptx_conv3d_dw_f32_fwd")
    torch.cuda.synchronize()
    return y.cpu(), wp.cpu(), bp.cpu()


def reference(x, wp, bp, k, s, p, relu):
    """float64 F.conv3d on the packed fp32 operands, and the bound: 32 * 2^-24 * (conv(|x|, |w|) + |b|) -- at most 27 fused
    multiply-adds and one add, each rounded once to fp32, in any order: (1 + 2^-24)^28 - 1 < 32 * 2^-24."""
    Cc = wp.shape[1]
    x64 = x[..., :Cc].permute(0, 4, 1, 2, 3).double()
    w64 = wp.double().t().reshape(Cc, 1, *k)
    ref = F.conv3d(x64, w64, bp.double(), s, p, 1, Cc)
    mag = F.conv3d(x64.abs(), w64.abs(), bp.double().abs(), s, p, 1, Cc)
    if relu:
        ref = ref.clamp_min(0)       # |max(a, 0) - max(b, 0)| <= |a - b|
    return ref.permute(0, 2, 3, 4, 1), 32 * 2.0 ** -24 * mag.permute(0, 2, 3, 4, 1)


@pytest.mark.parametrize("case", KERNEL_CASES, ids=["C%d_%dx%dx%d_s%d%d%d_k%d%d%d%s" % ((c[0],) + c[1] + c[2] + c[3] + ("_nopad" if c[4] else "",))
                                                    for c in KERNEL_CASES])
def test_dw_kernel_against_float64(ptx, case):
    Cc, dims, s, k, pad = case
    p = tuple(kk // 2 for kk in k) if pad is None else pad
    g = torch.Generator().manual_seed(Cc * 1000 + dims[2])
    N = 2
    w = torch.randn(Cc, 1, *k, generator=g) * 0.3
    bn = (torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1,
          torch.rand(Cc, generator=g) + 0.5)
    for with_bn in (False, True):
        for ldx in (Cc, Cc + 8):
            x = torch.full((N,) + dims + (ldx,), NAN)
            x[..., :Cc] = torch.randn((N,) + dims + (Cc,), generator=g)
            y, wp, bp = run_dw(ptx, x, w, bn if with_bn else None, 1e-3, s, p, relu=with_bn)
            # the pack: w * gamma / sqrt(var + eps) and beta - mean * scale in fp32 (a few roundings each), tap-major
            scale = (bn[0].double() / (bn[3].double() + 1e-3).sqrt()) if with_bn else torch.ones(Cc, dtype=torch.float64)
            want_w = (w.double().reshape(Cc, -1) * scale[:, None]).t()
            want_b = (bn[1].double() - bn[2].double() * scale) if with_bn else torch.zeros(Cc, dtype=torch.float64)
            assert ((wp.double() - want_w).abs() <= 4 * 2.0 ** -24 * want_w.abs()).all(), case
            assert ((bp.double() - want_b).abs() <= 4 * 2.0 ** -24 * (bn[1].abs() + (bn[2] * scale).abs()).double() + 1e-30).all(), case
            ref, bound = reference(x, wp, bp, k, s, p, relu=with_bn)
            got = y[..., 4:4 + Cc]
            assert got.shape == ref.shape, (case, got.shape, ref.shape)
            assert not torch.isnan(got).any(), (case, "an output was not written")
            err = (got.double() - ref).abs()
            worst = (err / bound.clamp_min(1e-300)).max().item()
            print("dw %s bn=%d ldx=%d: max err / bound = %.3f" % (case, with_bn, ldx, worst))
            assert (err <= bound).all(), (case, with_bn, ldx, worst)
            assert torch.isnan(y[..., :4]).all() and torch.isnan(y[..., 4 + Cc:]).all(), (case, "a neighbour channel was written")


@pytest.mark.parametrize("case", [KERNEL_CASES[1], KERNEL_CASES[2]], ids=["C20_s2", "C68_strips8"])
def test_dw_kernel_batch_independence(ptx, case):
    """The N = 3 launch equals the three N = 1 launches bit for bit."""
    Cc, dims, s, k, _ = case
    p = tuple(kk // 2 for kk in k)
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3,) + dims + (Cc,), generator=g)
    w = torch.randn(Cc, 1, *k, generator=g) * 0.3
    bn = (torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1,
          torch.rand(Cc, generator=g) + 0.5)
    whole = run_dw(ptx, x, w, bn, 1e-3, s, p, relu=True)[0][..., 4:4 + Cc]
    for n in range(3):
        one = run_dw(ptx, x[n:n + 1].contiguous(), w, bn, 1e-3, s, p, relu=True)[0][..., 4:4 + Cc]
        assert torch.equal(whole[n:n + 1], one), (case, n)


FORM_CASES = [KERNEL_CASES[0], KERNEL_CASES[1], KERNEL_CASES[2], KERNEL_CASES[3], KERNEL_CASES[4], KERNEL_CASES[5], KERNEL_CASES[8]]


@pytest.fixture
def force_form(ptx):
    """ptx_conv3d_dw_f32_force_form for the length of a test; the library's own rule afterwards."""
    L = ptx._lib

    def force(form):
        L.check(L.lib().ptx_conv3d_dw_f32_force_form(form), "ptx_conv3d_dw_f32_force_form")
    yield force
    force(0)


@pytest.mark.parametrize("case", FORM_CASES, ids=["C4_1x2x3", "C20_s2_odd", "C68_W70", "C128_s211", "C8_k133", "C8_k311", "C20_nopad"])
def test_dw_kernel_forms_agree_bit_for_bit(ptx, case, force_form):
    """Every form a launch can take -- strips of 4 and of 8 output columns, the LDS-staged halo tile -- within the float64 bound, and
    with the bits of the library's own choice: frames smaller than a tile | odd extents at stride 2, 5 channel quads in a 16-quad
    group | 70 columns (ragged 8-column strips and tiles), 17 quads (a second, ragged quad group) | mixed strides | (1,3,3) and
    (3,1,1) taps | no padding."""
    L = ptx._lib
    Cc, dims, s, k, pad = case
    p = tuple(kk // 2 for kk in k) if pad is None else pad
    g = torch.Generator().manual_seed(Cc + 17)
    x = torch.full((2,) + dims + (Cc + 4,), NAN)
    x[..., :Cc] = torch.randn((2,) + dims + (Cc,), generator=g)
    w = torch.randn(Cc, 1, *k, generator=g) * 0.3
    bn = (torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1, torch.randn(Cc, generator=g) * 0.1,
          torch.rand(Cc, generator=g) + 0.5)
    got = {}
    for form in (0, L.PTX_DW_FORM_STRIP4, L.PTX_DW_FORM_STRIP8, L.PTX_DW_FORM_LDS):
        force_form(form)
        y, wp, bp = run_dw(ptx, x, w, bn, 1e-3, s, p, relu=True)
        assert torch.isnan(y[..., :4]).all() and torch.isnan(y[..., 4 + Cc:]).all(), (case, form)
        got[form] = y[..., 4:4 + Cc]
        assert not torch.isnan(got[form]).any(), (case, form)
    ref, bound = reference(x, wp, bp, k, s, p, relu=True)
    for form, y in got.items():
        assert ((y.double() - ref).abs() <= bound).all(), (case, form)
        assert torch.equal(y, got[0]), (case, form)


def test_dw_kernel_lds_form_batch_independence(ptx, force_form):
    Cc, dims, s, k, _ = KERNEL_CASES[2]
    g = torch.Generator().manual_seed(6)
    x = torch.randn((3,) + dims + (Cc,), generator=g)
    w = torch.randn(Cc, 1, *k, generator=g) * 0.3
    force_form(ptx._lib.PTX_DW_FORM_LDS)
    whole = run_dw(ptx, x, w, None, 0.0, s, (1, 1, 1), relu=False)[0][..., 4:4 + Cc]
    assert not torch.isnan(whole).any()
    for n in range(3):
        one = run_dw(ptx, x[n:n + 1].contiguous(), w, None, 0.0, s, (1, 1, 1), relu=False)[0][..., 4:4 + Cc]
        assert torch.equal(whole[n:n + 1], one), n


# --------------------------------------------------------------------------------------------- 2. the models
_REF = {}


def _case(ptx, name, shape):
    """(model on the GPU, state dict, clips, the oracle's logits) -- the oracle runs once per (name, shape)."""
    key = (name, shape)
    if key not in _REF:
        model = ptx.__dict__[name](num_classes=51, pretrained=None)
        sd = synth_state_dict(model.state_dict(), 1234)
        g = torch.Generator().manual_seed(shape[0] * 100 + shape[2])
        x = torch.randn(shape, generator=g)
        _REF[key] = (sd, x, O.forward(sd, x))
    sd, x, want = _REF[key]
    model = ptx.__dict__[name](num_classes=51, pretrained=None)
    model.load_state_dict(sd)
    model = model.to(DEV).eval()
    model.engine().lanes = 1
    return model, sd, x, want


def _check(got, want, what):
    got = got.detach().float().cpu()
    top = want.topk(2, 1).values
    margin = (top[:, 0] - top[:, 1]).min().item()
    err = (got - want).abs().max().item()
    print("%s: max|dlogits| %.3e, oracle top-2 margin %.3e, max|logit| %.3f" % (what, err, margin, want.abs().max().item()))
    assert margin > MARGIN, "%s: the oracle's own top-2 margin %.3e is a near-tie" % (what, margin)
    assert got.shape == want.shape and err <= TOL, "%s: max abs err %.3e > %.1e" % (what, err, TOL)
    assert torch.equal(got.argmax(1), want.argmax(1)), what


SMALL, RAGGED = (2, 3, 8, 64, 64), (3, 3, 9, 48, 80)


@pytest.mark.parametrize("name", ["ir_csn50", "ip_csn50", "ir_csn101"])
@pytest.mark.parametrize("shape", [SMALL, RAGGED], ids=["2x8x64x64", "3x9x48x80"])
def test_csn_against_oracle(ptx, name, shape):
    model, sd, x, want = _case(ptx, name, shape)
    xd = x.to(DEV)
    got = model(xd)
    _check(got, want, "%s %s" % (name, shape))
    feats = model.features(xd)
    _check(model.logits(feats), want, "%s %s logits(features)" % (name, shape))
    assert tuple(feats.shape) == (shape[0], 2048, -(-shape[2] // 8), -(-shape[3] // 32), -(-shape[4] // 32))
    assert torch.equal(model(xd), got), "the forward is not repeatable"


def test_csn_split_operands(ptx):
    model, sd, x, want = _case(ptx, "ir_csn50", SMALL)
    model.engine().precision = "x3"
    _check(model(x.to(DEV)), want, "ir_csn50 x3")


def test_csn_forward_frames_equals_tensor_path(ptx):
    model, sd, x, want = _case(ptx, "ir_csn50", SMALL)
    TF = ptx.transforms
    frames = torch.from_numpy(synth_frames(2 * 8, 64, 64, 3)).reshape(2, 8, 64, 64, 3).to(DEV)
    a = model.forward_frames(frames, OPTS)
    b = model(TF.FramesToTensor(OPTS)(frames))
    assert torch.equal(a, b)


def test_csn_cam(ptx):
    model, sd, x, want = _case(ptx, "ir_csn50", SMALL)
    xd = x.to(DEV)
    r = model.cam(xd, topk=2)
    assert torch.equal(r.logits, model(xd))
    assert tuple(r.scores.shape) == (2, 2, 1, 2, 2) and tuple(r.maps.shape) == (2, 2, 1, 2, 2) and r.maps.dtype == torch.uint8
    assert torch.equal(r.classes.cpu(), r.logits.topk(2, 1).indices.cpu())
    # the mean of a class's scores over the positions is its logit (fp32 summation order aside)
    mean = r.scores.float().mean((2, 3, 4)).cpu()
    assert (mean - r.logits.cpu().gather(1, r.classes.cpu().long())).abs().max().item() <= 1e-4


def test_csn_weight_edit_changes_the_output(ptx):
    model, sd, x, want = _case(ptx, "ir_csn50", SMALL)
    xd = x.to(DEV)
    before = model(xd).clone()
    with torch.no_grad():
        model.layer2[1].conv2.weight.mul_(-3.0)          # one depthwise filter bank, in place
    after = model(xd)
    assert not torch.equal(before, after)
    sd2 = dict(sd)
    sd2["layer2.1.conv2.weight"] = sd["layer2.1.conv2.weight"] * -3.0
    _check(after, O.forward(sd2, x), "ir_csn50 after an in-place edit of layer2.1.conv2.weight")


def test_csn_fold_reads_each_modules_own_eps(ptx):
    """Every depthwise conv's BatchNorm at eps = 0.25, the rest at 1e-3: the packs must fold each module's own eps.  The oracle
    moves by 15 times the bar between the two settings (asserted), so a fold with a fixed eps cannot pass."""
    model, sd, x, want = _case(ptx, "ir_csn50", SMALL)
    names = [n for n, m in model.named_modules() if n.endswith(".bn2")]
    assert len(names) == 16
    for n in names:
        model.get_submodule(n).eps = 0.25
    moved = O.forward(sd, x, eps={n: 0.25 for n in names})
    assert (moved - want).abs().max().item() > 10 * TOL
    _check(model(x.to(DEV)), moved, "ir_csn50 with eps = 0.25 on every bn2")
