"""update_bn on the GPU: the batch-statistics BatchNorm kernels (include/ptx_amd_bn.h) against float64 numpy, and
pretorched_x_amd.update_bn against tests/golden/update_bn.npz -- torch.optim.swa_utils.update_bn run in float64 on the CPU
(tests/golden/make_update_bn_golden.py).  No torch.nn forward runs here (conftest's autouse fixture): the oracle is the file.

Bars.  Moments (K1 / K3): |dmean| <= 1e-6 (|mean| + std), |dvar| <= 2e-5 var -- torch's own fp32 BatchNorm1d lands at 7.7e-7 of
the variance on the K3 input, raw E[x^2] - E[x]^2 in fp32 at 1.4e-3.  Update (K4): the same bars for the running statistics,
2e-6 of their own magnitude for scale / shift; the inputs keep |beta| above |mean * scale|, because a difference that cancels
has no bounded relative error in any arithmetic.  Apply (K5): 4 * 2^-24 (|raw * scale| + |shift| + |res|) per element -- one
rounding of the fused multiply-add, one of the residual add, with room for the fp32 roundings of scale and shift themselves
being absent (they are inputs).  Models (M1 / M3): 1e-3 of the golden tensor's max-abs, the project's model bar."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


def _golden_module():
    spec = importlib.util.spec_from_file_location("make_update_bn_golden", os.path.join(HERE, "golden", "make_update_bn_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _golden_module()
_FILE = {}


def _case(name):
    if not _FILE:
        _FILE.update(G.load())
    return _FILE[name]


def _p(t):
    return C.c_void_p(t.data_ptr())


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _stats(ptx, x, C_):
    """One ptx_bn_batch_stats_f32 call on x [rows][ld] (a CUDA tensor): (mean, var) as float64 numpy."""
    L, lib = ptx._lib, ptx._lib.lib()
    rows, ld = x.shape
    n = int(lib.ptx_bn_batch_stats_workspace_bytes(rows, C_))
    assert n > 0 and n % 16 == 0
    ws, mean, var = _nan(n // 4), _nan(C_), _nan(C_)
    L.check(lib.ptx_bn_batch_stats_f32(_p(x), rows, C_, ld, _p(mean), _p(var), _p(ws), n, _st()), "ptx_bn_batch_stats_f32")
    torch.cuda.synchronize()
    return mean.cpu().numpy().astype(np.float64), var.cpu().numpy().astype(np.float64)


def _noise(rows, C_, ld, seed, pad_nan=False):
    """Unit-variance noise with per-channel means in [-3, 3] as [rows][ld] fp32 (pad channels zero, or NaN)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.full((rows, ld), float("nan") if pad_nan else 0.0)
    x[:, :C_] = torch.randn(rows, C_, generator=g) + (torch.rand(C_, generator=g) * 6 - 3)
    return x


def _check_moments(x, C_, mean, var):
    ref = x[:, :C_].numpy().astype(np.float64)
    m, v = ref.mean(0), ref.var(0)
    em, ev = np.abs(mean - m) / (np.abs(m) + np.sqrt(v)), np.abs(var - v) / v
    print("moments %s: max |dmean| / (|mean| + std) = %.3g, max |dvar| / var = %.3g" % (tuple(x.shape), em.max(), ev.max()))
    assert np.isfinite(mean).all() and np.isfinite(var).all()
    assert em.max() <= 1e-6 and ev.max() <= 2e-5


# ------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("rows,C_,ld,pad_nan", [(2, 4, 4, False), (7, 20, 24, True), (5000, 64, 64, False), (3137, 256, 256, False),
                                                 (100003, 8, 8, False)])
def test_k1_batch_stats_against_float64(ptx, rows, C_, ld, pad_nan):
    x = _noise(rows, C_, ld, 11 + rows, pad_nan)
    mean, var = _stats(ptx, x.to(DEV), C_)
    _check_moments(x, C_, mean, var)


def test_k2_batch_stats_same_bits_twice(ptx):
    x = _noise(3137, 256, 256, 5).to(DEV)
    a, b = _stats(ptx, x, 256), _stats(ptx, x, 256)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_k3_batch_stats_cancellation(ptx):
    g = torch.Generator().manual_seed(3)
    x = 100.0 + torch.randn(65536, 8, generator=g)
    mean, var = _stats(ptx, x.to(DEV), 8)
    _check_moments(x, 8, mean, var)
    # the condition the bar separates: raw E[x^2] - E[x]^2 in fp32 misses it by two orders of magnitude on this input
    raw = ((x * x).mean(0) - x.mean(0) ** 2).numpy().astype(np.float64)
    assert (np.abs(raw - x.numpy().astype(np.float64).var(0)) / x.numpy().astype(np.float64).var(0)).max() > 2e-5


@pytest.mark.parametrize("n", [2, 5000])
@pytest.mark.parametrize("f", [1.0, 0.5, 0.1])
def test_k4_update(ptx, f, n):
    L, lib = ptx._lib, ptx._lib.lib()
    C_ = 70
    g = torch.Generator().manual_seed(17)
    mean, var = torch.rand(C_, generator=g) * 2 - 1, torch.rand(C_, generator=g) * 1.5 + 0.5
    gamma, beta = torch.rand(C_, generator=g) + 0.5, (torch.rand(C_, generator=g) + 3.0) * torch.sign(torch.randn(C_, generator=g))
    rm0, rv0 = torch.randn(C_, generator=g), torch.rand(C_, generator=g) + 0.5
    eps = 1e-5
    d = [t.to(DEV) for t in (mean, var, gamma, beta, rm0, rv0)]
    scale, shift = _nan(C_), _nan(C_)
    L.check(lib.ptx_bn_batch_update_f32(_p(d[0]), _p(d[1]), n, C.c_float(f), C.c_float(eps), _p(d[2]), _p(d[3]), _p(d[4]), _p(d[5]),
                                        _p(scale), _p(shift), C_, _st()), "ptx_bn_batch_update_f32")
    torch.cuda.synchronize()
    m64, v64, g64, b64, rm64, rv64 = (t.numpy().astype(np.float64) for t in (mean, var, gamma, beta, rm0, rv0))
    f64, eps64 = float(np.float32(f)), float(np.float32(eps))
    want_scale = g64 / np.sqrt(v64 + eps64)
    want_shift = b64 - m64 * want_scale
    want_rm = (1 - f64) * rm64 + f64 * m64
    want_rv = (1 - f64) * rv64 + f64 * v64 * n / (n - 1)
    got = [t.cpu().numpy().astype(np.float64) for t in (scale, shift, d[4], d[5])]
    e_scale, e_shift = np.abs(got[0] - want_scale) / np.abs(want_scale), np.abs(got[1] - want_shift) / np.abs(want_shift)
    e_rm, e_rv = np.abs(got[2] - want_rm) / (np.abs(want_rm) + np.sqrt(want_rv)), np.abs(got[3] - want_rv) / want_rv
    print("update f=%g n=%d: scale %.3g shift %.3g running_mean %.3g running_var %.3g" % (f, n, e_scale.max(), e_shift.max(), e_rm.max(), e_rv.max()))
    assert e_scale.max() <= 2e-6 and e_shift.max() <= 2e-6 and e_rm.max() <= 1e-6 and e_rv.max() <= 2e-5
    # without affine parameters and tracked statistics: scale 1 / sqrt(var + eps), nothing else written
    L.check(lib.ptx_bn_batch_update_f32(_p(d[0]), _p(d[1]), n, C.c_float(f), C.c_float(eps), None, None, None, None,
                                        _p(scale), _p(shift), C_, _st()), "ptx_bn_batch_update_f32")
    torch.cuda.synchronize()
    assert (np.abs(scale.cpu().numpy() - 1 / np.sqrt(v64 + eps64)) <= 2e-6 / np.sqrt(v64 + eps64)).all()


def test_k4_update_refuses_one_value_per_channel(ptx):
    lib = ptx._lib.lib()
    t = torch.ones(4, device=DEV)
    assert lib.ptx_bn_batch_update_f32(_p(t), _p(t), 1, C.c_float(1), C.c_float(1e-5), None, None, None, None, _p(t), _p(t), 4, _st()) == 1
    assert b"more than 1 value" in lib.ptx_last_error()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("kind", ["none", "add", "padA"])
def test_k5_apply(ptx, kind, relu):
    L, lib = ptx._lib, ptx._lib.lib()
    N, T, H, W, C_, ld = 2, 3, 5, 7, 22, 28          # ld > round_up(C, 4): 24 live-quad channels, 4 never touched
    g = torch.Generator().manual_seed(23)
    raw = torch.randn(N, T, H, W, ld, generator=g) * 3
    scale, shift = torch.rand(C_, generator=g) + 0.5, torch.randn(C_, generator=g)
    d = L.BnApplyDesc()
    d.N, d.T, d.H, d.W, d.C, d.ldx, d.ldy = N, T, H, W, C_, ld, ld
    d.flags = L.PTX_EPI_RELU if relu else 0
    want = raw[..., :C_].double() * scale.double() + shift.double()
    bound = (raw[..., :C_].double() * scale.double()).abs() + shift.double().abs()
    res = None
    if kind == "add":
        res = torch.randn(N, T, H, W, ld, generator=g)
        d.flags |= L.PTX_EPI_RES_ADD
        d.ldr = ld
        want, bound = want + res[..., :C_].double(), bound + res[..., :C_].double().abs()
    elif kind == "padA":      # the block input: stride 2, 10 of the 22 channels (2 of its last quad are pad: NaN must not leak)
        rT, rH, rW, rC, ldr = 2 * T - 1, 2 * H, 2 * W - 1, 10, 12
        res = torch.full((N, rT, rH, rW, ldr), float("nan"))
        res[..., :rC] = torch.randn(N, rT, rH, rW, rC, generator=g)
        d.flags |= L.PTX_EPI_RES_PADA
        d.ldr, d.res_C, d.res_T, d.res_H, d.res_W = ldr, rC, rT, rH, rW
        d.res_sT = d.res_sH = d.res_sW = 2
        sub = res[:, ::2, ::2, ::2, :rC].double()
        assert sub.shape[1:4] == (T, H, W)
        want[..., :rC] += sub
        bound[..., :rC] += sub.abs()
    if relu:
        want = want.clamp_min(0)
    x, y = raw.to(DEV), _nan(N, T, H, W, ld)
    keep = [scale.to(DEV), shift.to(DEV), res.to(DEV) if res is not None else None]
    ptrs = (_p(x), _p(keep[0]), _p(keep[1]), _p(keep[2]) if res is not None else None)
    L.check(lib.ptx_bn_apply_f32(C.byref(d), *ptrs, _p(y), _st()), "ptx_bn_apply_f32")
    torch.cuda.synchronize()
    got = y.cpu()
    err = (got[..., :C_].double() - want).abs()
    tol = 4 * 2.0 ** -24 * bound
    print("apply %s relu=%d: max err / tol = %.3g" % (kind, relu, (err / tol).max()))
    assert torch.isfinite(got[..., :C_]).all() and (err <= tol).all()
    assert torch.isnan(got[..., 24:]).all()          # columns past the last channel quad are not written
    # in place on raw: the same bits
    L.check(lib.ptx_bn_apply_f32(C.byref(d), *ptrs, _p(x), _st()), "ptx_bn_apply_f32 in place")
    torch.cuda.synchronize()
    assert torch.equal(x.cpu()[..., :C_], got[..., :C_])


# ------------------------------------------------------------------------------------------------------ models
def _run_case(ptx, name, lanes=None):
    """update_bn of fixture case `name` on the GPU: (model, batches on the GPU, file record, BN layers)."""
    rec = _case(name)
    model = G.build_model(rec["spec"]).to(DEV)
    if lanes is not None:
        model.engine().lanes = lanes
    xs = [x.to(DEV) for x in G.batches(rec["spec"])]
    momenta = [bn.momentum for bn in G.bn_layers(model)]
    ptx.update_bn([(x, None) for x in xs], model, **rec["spec"]["call"])
    assert model.training is False and [bn.momentum for bn in G.bn_layers(model)] == momenta
    return model, xs, rec, G.bn_layers(model)


def _check_case(model, xs, rec, layers, name):
    mean = torch.cat([bn.running_mean for bn in layers]).cpu().numpy().astype(np.float64)
    var = torch.cat([bn.running_var for bn in layers]).cpu().numpy().astype(np.float64)
    tracked = np.array([int(bn.num_batches_tracked) for bn in layers])
    e_mean = np.abs(mean - rec["mean"]).max() / np.abs(rec["mean"]).max()
    e_var = np.abs(var - rec["var"]).max() / np.abs(rec["var"]).max()
    logits = model(xs[0]).cpu().numpy().astype(np.float64)           # eval mode, no refresh(): the new statistics
    e_log = np.abs(logits - rec["logits"]).max() / np.abs(rec["logits"]).max()
    print("update_bn %s: running_mean %.3g running_var %.3g logits %.3g (of the golden max-abs)" % (name, e_mean, e_var, e_log))
    assert np.array_equal(tracked, rec["tracked"])
    assert e_mean <= 1e-3 and e_var <= 1e-3
    assert e_log <= 1e-3 and np.array_equal(logits.argmax(1), rec["logits"].argmax(1))


@pytest.mark.parametrize("name", list(G.CASES))
def test_m1_update_bn_matches_float64_torch(ptx, name):
    model, xs, rec, layers = _run_case(ptx, name)
    _check_case(model, xs, rec, layers, name)


def test_m2_update_bn_twice_same_bits(ptx):
    model, xs, rec, layers = _run_case(ptx, "resnet3d18")
    first = [(bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()) for bn in layers]
    model.update_bn(xs)
    for bn, (m, v, t) in zip(layers, first):
        assert torch.equal(bn.running_mean, m) and torch.equal(bn.running_var, v) and torch.equal(bn.num_batches_tracked, t)


def test_m3_update_bn_ignores_clip_lanes(ptx):
    model, xs, rec, layers = _run_case(ptx, "resnet3d18", lanes=2)
    _check_case(model, xs, rec, layers, "resnet3d18 / lanes=2")
