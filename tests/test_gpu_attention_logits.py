"""The attention kernels at the logit magnitudes trained non-local blocks produce (no 1 / sqrt(d) in the reference: |s| of a
hundred and more), on the exact-integer inputs of tests/attention_cases.py.  Every other attention test of the suite keeps
|s| at a few units, where a kernel that never subtracts the running max, shares it between queries or merges two key groups
wrongly is numerically invisible (tests/test_attention_logits_host.py shows that on the CPU).

Because the logits are the same integers in every precision, the bars are the ones of the files that own the kernels,
unchanged: 2e-5 max(1, max|want|) for fp32 and split operands and 5e-3 for PTX_NL_F16 (test_gpu_kernels.py),
2^-7 max|g| + 2^-7 |ref| for bf16 (test_gpu_nl_bf16.py), 1e-6 for ptx_softmax_rows and ptx_views_mean.  On top of parity:
  * no NaN / Inf in the written columns, guard columns untouched (y is NaN-filled before a launch);
  * the run with the per-query shift r_i is BIT-IDENTICAL to the run with r_i = 0 (s - m is the same integer in both; every
    kernel here forms its exponent as exp(s - m), none folds log2(e) into a multiply-add, so none is exempt);
  * one-hot profiles: y[i] == g[j*] bit for bit on the fp32 and bf16 kernels (l rounds to 1, every other weight is below
    e^-72); PTX_NL_F16 / PTX_NL_X3 round or split g on the way, so there the bar decides;
  * `high`, `low` and b = 0 give bit-identical outputs.
Harnesses: the bf16 launch and checks are test_gpu_nl_ksplit_bf16.py's, the fp32 one follows
test_gpu_kernels.py::test_fused_nonlocal_attention (operands as channel slices of one fused projection tensor)."""
import ctypes as C

import pytest
import torch

import attention_cases as AC
import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.testing import synth_state_dict
from oracle import functional as OF
from test_gpu_kernels import DEV, _p, _r4, _st, close
from test_gpu_nl_bf16 import _check_block, _shape
from test_gpu_nl_ksplit_bf16 import _check_kernel, _launch as _launch_bf16

pytestmark = pytest.mark.gpu
NAN = float("nan")


# ------------------------------------------------------------------------------------------- fp32 / f16 / x3 kernels
def _launch32(data, flavour, kind, streamk=False):
    """theta = columns [0, d) of the query rows of one fused [rows][theta | phi | g | 4 spare] tensor, phi and g columns
    [d, 2d) and [2d, 2d + dv) of the key rows; everything the kernel has no business reading is NaN, and so is y."""
    th, ph, g = data
    (B, Nq, d), Nk, dv = th.shape, ph.shape[1], g.shape[2]
    ld = _r4(2 * d + dv) + 4
    tq = torch.full((B, Nq, ld), NAN)
    tk = torch.full((B, Nk, ld), NAN)
    tq[..., :d], tk[..., d:2 * d], tk[..., 2 * d:2 * d + dv] = th, ph, g
    tq, tk = tq.to(DEV), tk.to(DEV)
    ldy = _r4(dv) + 8
    y = torch.full((B, Nq, ldy), NAN, device=DEV)
    desc = L.NonlocalDesc()
    desc.batch, desc.Nq, desc.Nk, desc.d, desc.dv = B, Nq, Nk, d, dv
    desc.ld_theta = desc.ld_phi = desc.ld_g = ld
    desc.ld_y = ldy
    desc.bs_theta, desc.bs_phi, desc.bs_g, desc.bs_y = Nq * ld, Nk * ld, Nk * ld, Nq * ldy
    desc.mode = ((L.PTX_NL_SOFTMAX if kind == "softmax" else L.PTX_NL_SCALE) | (L.PTX_NL_RELU if kind == "relu" else 0) |
                 (L.PTX_NL_F16 if flavour == "f16" else 0) | (L.PTX_NL_X3 if flavour == "x3" else 0))
    lib = L.lib()
    assert lib.ptx_nonlocal_supported(C.byref(desc))
    need = lib.ptx_nonlocal_workspace_bytes(C.byref(desc))
    if streamk:
        assert need > 0                                   # the stream-K form covers this descriptor
        ws = torch.full((need // 4 + 4,), NAN, device=DEV)
        L.check(lib.ptx_nonlocal_ws_fwd(C.byref(desc), _p(tq), _p(tk, d), _p(tk, 2 * d), _p(y), _p(ws), need, _st()), "nonlocal ws")
        torch.cuda.synchronize()
        assert torch.isnan(ws[need // 4:]).all()          # nothing written past the workspace asked for
    else:
        assert need == 0                                  # ... and no other row is routed to it
        L.check(lib.ptx_nonlocal_fwd(C.byref(desc), _p(tq), _p(tk, d), _p(tk, 2 * d), _p(y), _st()), "nonlocal")
        torch.cuda.synchronize()
    return y.cpu()


def _check32(y, want, flavour, what):
    dv = want.shape[-1]
    got = y[..., :dv]
    assert torch.isnan(y[..., dv:]).all(), what           # columns beyond dv are left untouched
    assert torch.isfinite(got).all(), what
    err = float((got.double() - want).abs().max())
    bar = (5e-3 if flavour == "f16" else 2e-5) * max(1.0, float(want.abs().max()))
    assert err <= bar, (what, err, bar)


def _profile_case(row, profile, launch):
    """Assertions 1-4 of the module docstring for one fp32-family row and one profile."""
    name, flavour, kind, B, Nq, Nk, d, dv, gk = row
    data = AC.make_inputs(profile, B, Nq, Nk, d, dv, gk)
    want = AC.reference(*data, kind)
    y = launch(data)
    _check32(y, want, flavour, (name, profile))
    if kind == "relu":
        dead = (AC.logits(*data[:2]) < 0).all(-1)         # queries with every a_i + b_j < 0: exactly zero
        assert bool((y[..., :dv][dead] == 0).all())
        if profile == "late_peak":
            assert bool(dead.any())
    if kind != "softmax":                                 # S / Nk is not shift invariant: parity (exact integers / Nk) only
        return
    plain = AC.make_inputs(profile, B, Nq, Nk, d, dv, gk, shift=False)
    assert torch.equal(launch(plain)[..., :dv], y[..., :dv]), (name, profile, "row shift")
    if profile in AC.ONE_HOT and flavour == "":
        j = AC.peak_key(profile, Nk, gk)
        assert torch.equal(y[..., :dv], data[2][:, j:j + 1].expand(B, Nq, dv)), (name, profile, "one-hot")


def _equivalence_case(row, launch):
    """Assertion 5: high, low and b = 0 differ by a constant per row; the outputs are the same bits."""
    name, flavour, kind, B, Nq, Nk, d, dv, gk = row
    ys = [launch(AC.make_inputs(p, B, Nq, Nk, d, dv, gk))[..., :dv] for p in ("high", "low", "zero")]
    assert torch.isfinite(ys[0]).all()
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2]), name


def _params(rows):
    return [pytest.param(r, p, id="%s-%s" % (r[0], p)) for r in rows for p in AC.profiles_for(r[5], r[8])]


SOFTMAX_ROWS32 = [r for r in AC.FP32_ROWS if r[2] == "softmax"]


@pytest.mark.parametrize("row,profile", _params(AC.FP32_ROWS))
def test_nonlocal_fwd_integer_logits(row, profile):
    """ptx_nonlocal_fwd, one row per kernel of its dispatcher (AC.FP32_ROWS names the dispatch condition of each)."""
    _profile_case(row, profile, lambda data: _launch32(data, row[1], row[2]))


@pytest.mark.parametrize("row", SOFTMAX_ROWS32, ids=lambda r: r[0])
def test_nonlocal_fwd_high_low_zero_identical(row):
    _equivalence_case(row, lambda data: _launch32(data, row[1], row[2]))


@pytest.mark.parametrize("profile", AC.profiles_for(AC.STREAMK_ROW[5], AC.STREAMK_ROW[8]))
def test_stream_k_integer_logits(profile, monkeypatch):
    """ptx_nonlocal_ws_fwd under PTX_NL_STREAMK=1 (the branch is asserted: a non-zero workspace is asked for and used)."""
    monkeypatch.setenv("PTX_NL_STREAMK", "1")
    _profile_case(AC.STREAMK_ROW, profile, lambda data: _launch32(data, "", "softmax", streamk=True))


def test_stream_k_high_low_zero_identical(monkeypatch):
    monkeypatch.setenv("PTX_NL_STREAMK", "1")
    _equivalence_case(AC.STREAMK_ROW, lambda data: _launch32(data, "", "softmax", streamk=True))


# ------------------------------------------------------------------------------------------------------ bf16 kernels
def _bf16_data(profile, d, dv, Nq, Nk, shift=True):
    th, ph, g = AC.make_inputs(profile, AC.BF16_BATCH, Nq, Nk, d, dv, 32, shift)
    return th.to(torch.bfloat16), ph.to(torch.bfloat16), g.to(torch.bfloat16)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("d,dv,Nq,Nk", AC.BF16_ROWS)
def test_bf16_integer_logits(d, dv, Nq, Nk, variant):
    """ptx_nonlocal_bf16_variant_fwd, variant 0 (single group, 32-key tiles) and 1 (key split, 32 | 32 of 64 keys): the
    variant is the argument, so the branch is reached by construction."""
    for profile in AC.profiles_for(Nk, 32):
        data = _bf16_data(profile, d, dv, Nq, Nk)
        Y = _launch_bf16(data, "softmax", variant)
        _check_kernel(Y, AC.reference(*data), data[2], dv)
        y = Y[:, :, 8:8 + dv]
        assert torch.isfinite(y.float()).all(), profile
        Y0 = _launch_bf16(_bf16_data(profile, d, dv, Nq, Nk, shift=False), "softmax", variant)
        assert torch.equal(Y0[:, :, 8:8 + dv], y), (profile, "row shift")
        if profile in AC.ONE_HOT:
            j = AC.peak_key(profile, Nk, 32)
            assert torch.equal(y, data[2][:, j:j + 1].expand_as(y)), (profile, "one-hot")
    ys = [_launch_bf16(_bf16_data(p, d, dv, Nq, Nk), "softmax", variant)[:, :, 8:8 + dv] for p in ("high", "low", "zero")]
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])


# ------------------------------------------------------------------------------------ softmax_rows and views_mean
@pytest.mark.parametrize("cols", AC.SOFTMAX_COLS)
def test_softmax_rows_integer_logits(cols):
    x, n = AC.softmax_rows_logits(cols)
    rows, ld = x.shape[0], _r4(cols) + 4
    xp = torch.full((rows, ld), NAN)                       # pad columns: not read, zeroed
    xp[:, :cols] = x
    xd = xp.to(DEV)
    L.check(L.lib().ptx_softmax_rows(_p(xd), rows, cols, ld, 0, _st()), "softmax")
    torch.cuda.synchronize()
    got = xd.cpu()
    assert torch.isfinite(got).all() and bool((got[:, cols:] == 0).all())
    close(got[:, :cols], torch.softmax(x.double(), -1).float(), 1e-6)
    for k in range(1, 8):                                  # every row shift: the same bits
        assert torch.equal(got[k * n:(k + 1) * n], got[:n]), k
    hi, lo, zero = (AC.SOFTMAX_ROWS.index(p) for p in ("high", "low", "zero"))
    assert torch.equal(got[hi], got[lo]) and torch.equal(got[hi], got[zero])
    for p in AC.ONE_HOT:                                   # a gap of 72 and more: exactly one-hot
        i, j = AC.SOFTMAX_ROWS.index(p), AC.peak_key(p, cols, 16)
        assert float(got[i, j]) == 1.0 and float(got[i].sum()) == 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_views_mean_integer_logits(dtype):
    """ptx_views_mean, softmax mode, K = 339, V = 3: a video is three consecutive rows (three profiles), and a shift block
    is three videos, so video v of every shifted block must equal video v of block 0 bit for bit."""
    K, V = 339, 3
    x, n = AC.softmax_rows_logits(K)
    N = x.shape[0] // V
    xp = torch.full((N * V, K + 5), NAN)                   # a padded row stride
    xp[:, :K] = x
    xd = xp.to(dtype).to(DEV)[:, :K]
    got = ptx.engine.views_mean(xd, N, V, "softmax")
    torch.cuda.synchronize()
    got = got.cpu()
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    want = torch.softmax(x.double(), -1).view(N, V, K).mean(1)
    close(got.double(), want, 1e-6)
    assert float((got.double().sum(1) - 1).abs().max()) <= 1e-6
    per = n // V
    for k in range(1, 8):
        assert torch.equal(got[k * per:(k + 1) * per], got[:per]), k


# ------------------------------------------------------------------------------------------------------ block level
BLOCK_CASES = [(mode, sub) for mode in ("gaussian", "embedded_gaussian") for sub in (False, True)]


def _integer_block(mode, sub, bf16):
    """NonLocalBlock3D(64) with integer x (unit amplitude: {-2 .. 2}) and sparse integer theta / phi weights, zero bias: the
    block's own logits are exact integers.  The other weights are the synthetic ones, bf16-representable."""
    m = ptx.NonLocalBlock3D(64, mode=mode, sub_sample=sub, bn_layer=True)
    sd = synth_state_dict(m.state_dict(), 1234 + 64)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    gen = torch.Generator().manual_seed(31)
    for k in sd:
        if k.startswith(("theta.", "phi.")):
            w = torch.randint(-1, 2, sd[k].shape, generator=gen).float() * (torch.rand(sd[k].shape, generator=gen) < 0.06)
            sd[k] = w if k.endswith("weight") else torch.zeros_like(sd[k])
    m.load_state_dict(sd)
    m = m.eval()
    m = (m.to(torch.bfloat16) if bf16 else m).to(DEV)
    x = torch.randint(-2, 3, _shape(3, 64), generator=gen).float()
    return m, sd, x


def _block_logits(sd, x, mode, sub):
    """theta . phi of the block from the oracle's projections (oracle/functional.py: nonlocal_block), fp64."""
    import torch.nn.functional as F
    b, c = x.shape[:2]
    xd = x.double()
    pool = (lambda t: F.max_pool3d(t, 2)) if sub else (lambda t: t)
    if mode == "gaussian":
        theta, phi = xd, pool(xd)
    else:
        pk = "phi.0" if sub else "phi"
        theta = F.conv3d(xd, sd["theta.weight"].double(), sd["theta.bias"].double())
        phi = pool(F.conv3d(xd, sd[pk + ".weight"].double(), sd[pk + ".bias"].double()))
    s = theta.reshape(b, theta.shape[1], -1).permute(0, 2, 1) @ phi.reshape(b, phi.shape[1], -1)
    assert torch.equal(s, s.round()) and float(theta.abs().max()) <= 128 and float(phi.abs().max()) <= 128
    return s


@pytest.mark.parametrize("mode,sub", BLOCK_CASES)
def test_block_integer_logits_fp32(mode, sub):
    """fp32 NonLocalBlock3D against oracle.functional.nonlocal_block in fp64.  There is no project bar for an fp32 block: it
    is measured here as 4 x max|oracle fp32 - oracle fp64| (another summation order over the same arithmetic) plus the
    attention kernel's 2e-5 max(1, max|ref|)."""
    m, sd, x = _integer_block(mode, sub, False)
    assert float(_block_logits(sd, x, mode, sub).abs().max()) >= 40          # what keeps this test meaningful
    sdp = {("." + k): v for k, v in sd.items()}
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sdp.items()}
    ref = OF.nonlocal_block(sd64, x.double(), "", mode=mode, sub_sample=sub, bn_layer=True)
    ref32 = OF.nonlocal_block(sdp, x, "", mode=mode, sub_sample=sub, bn_layer=True).double()
    bar = 4 * float((ref32 - ref).abs().max()) + 2e-5 * max(1.0, float(ref.abs().max()))
    with torch.no_grad():
        out = m(x.to(DEV))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == x.shape and torch.isfinite(out).all()
    err = float((out.cpu().double() - ref).abs().max())
    print("fp32 block %s sub_sample=%s: max|out - fp64| = %.3e, bar %.3e" % (mode, sub, err, bar))
    assert err <= bar, "max|out - fp64| = %.3e above the bar %.3e" % (err, bar)
    assert not torch.equal(out.cpu(), x)


@pytest.mark.parametrize("mode,sub", BLOCK_CASES)
def test_block_integer_logits_bf16(mode, sub):
    """The bf16 block under test_gpu_nl_bf16.py's own check and bar (_block_bars: twice PyTorch's bf16 error + 1e-3 max|ref|)."""
    m, sd, x = _integer_block(mode, sub, True)
    # at most 256: PyTorch's bf16 arithmetic, which sets the bar, rounds the logits to bf16 and must see the same integers
    assert 40 <= float(_block_logits(sd, x, mode, sub).abs().max()) <= 256
    x = x.to(torch.bfloat16)
    _check_block(m, sd, x, mode, sub, True)
    with torch.no_grad():
        assert torch.isfinite(m(x.to(DEV)).float()).all()
