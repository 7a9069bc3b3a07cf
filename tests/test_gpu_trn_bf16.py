"""bf16 TRN and 2-D ResNets on the GPU: the bf16-weight Linear kernels (include/ptx_amd_linear_bf16.h) against fp64 under the
project's accumulation bound, exact tap mapping, bit equality of runs and of gather against dense; then the relation modules,
the 2-D ResNets and TRN calibrated against PyTorch's own bf16 arithmetic, uint8 frames / views, and the public API.
Every output buffer is NaN-filled (or holds a known value) before a launch, so an element the kernel leaves unwritten fails."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import pretorched_x_amd as ptx
from pretorched_x_amd import _lib as L
from pretorched_x_amd.engine import PtxError, _ptr
from pretorched_x_amd.testing import synth_state_dict
from oracle import functional as OF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
XB, XF = L.PTX_LIN_X_BF16, L.PTX_LIN_X_F32
RELU_IN, RELU_OUT, ACCUM = L.PTX_PRO_RELU, L.PTX_EPI_RELU, L.PTX_EPI_ACCUM
IMAGENET_BGR255 = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], input_space="BGR", input_range=[0, 255])


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bf(t):
    """bf16-exact fp32 values."""
    return t.to(torch.bfloat16).float()


def _ws(M, K, Nout):
    n = int(L.lib().ptx_linear_bf16w_workspace_bytes(M, K, Nout))
    t = torch.full(((n + 3) // 4 + 4,), float("nan"), device=DEV, dtype=torch.float32)
    return t, _ptr(t), n


def _null():
    return C.c_void_p(0)


def _dense(x, kind, w, b, M, K, Nout, flags, ldy=None, y0=None, ldx=None):
    """One ptx_linear_bf16w_fwd launch -> y [M][ldy] fp32 on the CPU (NaN-filled, or y0, before the launch)."""
    ldy = Nout if ldy is None else ldy
    y = torch.full((M, ldy), float("nan"), device=DEV, dtype=torch.float32) if y0 is None else y0.clone().to(DEV)
    keep, wsp, wsn = _ws(M, K, Nout)
    L.check(L.lib().ptx_linear_bf16w_fwd(_ptr(x), kind, _ptr(w), _ptr(b) if b is not None else _null(), _ptr(y), M, K, Nout,
                                         K if ldx is None else ldx, ldy, flags, wsp, wsn, _st()), "ptx_linear_bf16w_fwd")
    torch.cuda.synchronize()
    return y.cpu()


def _rel_desc(B, subsets, F_):
    d = L.RelationDesc()
    d.B, d.n_sets, d.n_frames, d.frame_len = B, len(subsets), len(subsets[0]), F_
    for r, sub in enumerate(subsets):
        for f, i in enumerate(sub):
            d.idx[r][f] = int(i)
    return d


def _gather(x, subsets, w, b, Nout, flags, ldy=None):
    """One ptx_relation_linear_bf16w_fwd launch on x [B][T][F] bf16 -> y [n_sets*B][ldy]."""
    B, T, F_ = x.shape
    M, K = len(subsets) * B, len(subsets[0]) * F_
    ldy = Nout if ldy is None else ldy
    y = torch.full((M, ldy), float("nan"), device=DEV, dtype=torch.float32)
    d = _rel_desc(B, subsets, F_)
    keep, wsp, wsn = _ws(M, K, Nout)
    L.check(L.lib().ptx_relation_linear_bf16w_fwd(C.byref(d), _ptr(x), T * F_, _ptr(w), _ptr(b) if b is not None else _null(), _ptr(y),
                                                  Nout, ldy, flags, wsp, wsn, _st()), "ptx_relation_linear_bf16w_fwd")
    torch.cuda.synchronize()
    return y.cpu()


def _bound(got, x, w, b, relu_in, what, bias_scale=1.0, base=None, relu_out=False):
    """|got - ref| <= 2^-20 (|x| |W|^T + |b|): the accumulation term of the project's bf16 bound -- y is fp32, so there is no
    output-rounding term.  x, w, b: the operands' values (fp64 on the CPU); base: what PTX_EPI_ACCUM adds to."""
    x = x.double().clamp_min(0) if relu_in else x.double()
    ref = x @ w.double().t()
    mag = x.abs() @ w.double().abs().t()
    if b is not None:
        ref = ref + bias_scale * b.double()
        mag = mag + bias_scale * b.double().abs()
    if base is not None:
        ref = ref + base.double()
        mag = mag + base.double().abs()
    if relu_out:
        ref = ref.clamp_min(0)
    err = (got.double() - ref).abs()
    bar = 2.0 ** -20 * mag + 1e-30
    print("%s: max err %.3e, max err / bar %.3f" % (what, float(err.max()), float((err / bar).max())))
    assert not torch.isnan(got).any(), what
    assert torch.all(err <= bar), (what, float((err - bar).max()))


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
DENSE = [(1, 8, 1), (8, 2048, 96), (9, 2056, 100), (24, 4096, 339), (5, 37, 7)]


@pytest.mark.parametrize("M,K,Nout", DENSE)
@pytest.mark.parametrize("kind", [XB, XF])
def test_dense_against_fp64(M, K, Nout, kind):
    g = torch.Generator().manual_seed(100 + M)
    x = _bf(torch.randn(M, K, generator=g))
    w = _bf(torch.randn(Nout, K, generator=g) * K ** -0.5)
    b = _bf(torch.randn(Nout, generator=g))
    xd = (x.to(torch.bfloat16) if kind == XB else x).to(DEV).contiguous()
    wd, bd = w.to(torch.bfloat16).to(DEV), b.to(torch.bfloat16).to(DEV)
    ldy = Nout + 5
    for flags in (0, RELU_IN | RELU_OUT):
        got = _dense(xd, kind, wd, bd, M, K, Nout, flags, ldy=ldy)
        assert torch.isnan(got[:, Nout:]).all(), "padding columns were written"
        _bound(got[:, :Nout], x, w, b, bool(flags & RELU_IN), "dense %s kind %d flags %d" % ((M, K, Nout), kind, flags),
               relu_out=bool(flags & RELU_OUT))
        assert torch.equal(got[:, :Nout], _dense(xd, kind, wd, bd, M, K, Nout, flags, ldy=ldy)[:, :Nout])       # run to run
    # no bias, accumulating into a known y
    y0 = _bf(torch.randn(M, ldy, generator=g))
    got = _dense(xd, kind, wd, None, M, K, Nout, ACCUM, ldy=ldy, y0=y0)
    assert torch.equal(got[:, Nout:], y0[:, Nout:])
    _bound(got[:, :Nout], x, w, None, False, "dense accum %s kind %d" % ((M, K, Nout), kind), base=y0[:, :Nout])


SUBSETS = {2: [(6, 1), (0, 7), (3, 2)], 5: [(7, 0, 3, 1, 4), (1, 2, 4, 5, 6), (6, 5, 0, 2, 3)],
           8: [(0, 1, 2, 3, 4, 5, 6, 7), (7, 6, 5, 4, 3, 2, 1, 0), (3, 0, 7, 1, 6, 2, 5, 4)]}


@pytest.mark.parametrize("n_frames", [2, 5, 8])
@pytest.mark.parametrize("n_sets", [1, 3])
def test_gather_against_fp64_and_dense(n_frames, n_sets):
    B, T, F_, Nout = 3, 8, 264, 96
    g = torch.Generator().manual_seed(200 + n_frames)
    x = _bf(torch.randn(B, T, F_, generator=g))
    subsets = SUBSETS[n_frames][:n_sets]
    K = n_frames * F_
    w = _bf(torch.randn(Nout, K, generator=g) * K ** -0.5)
    b = _bf(torch.randn(Nout, generator=g))
    xd, wd, bd = x.to(torch.bfloat16).to(DEV), w.to(torch.bfloat16).to(DEV), b.to(torch.bfloat16).to(DEV)
    flags = RELU_IN | RELU_OUT
    got = _gather(xd, subsets, wd, bd, Nout, flags, ldy=Nout + 8)
    assert torch.isnan(got[:, Nout:]).all()
    rows = torch.cat([x[:, list(s), :].reshape(B, K) for s in subsets], 0)            # row r*B + v
    _bound(got[:, :Nout], rows, w, b, True, "gather %d frames x %d sets" % (n_frames, n_sets), relu_out=True)
    assert torch.equal(got[:, :Nout], _gather(xd, subsets, wd, bd, Nout, flags, ldy=Nout + 8)[:, :Nout])          # run to run
    dense = _dense(rows.to(torch.bfloat16).to(DEV).contiguous(), XB, wd, bd, n_sets * B, K, Nout, flags)
    assert torch.equal(got[:, :Nout], dense), "a gather launch has the bits of the dense launch on the gathered rows"


@pytest.mark.parametrize("accum", [False, True])
def test_setsum_against_fp64(accum):
    B, n_sets, K, Nout = 3, 3, 264, 96
    g = torch.Generator().manual_seed(300)
    x = _bf(torch.randn(n_sets * B, K, generator=g))
    w = _bf(torch.randn(Nout, K, generator=g) * K ** -0.5)
    b = _bf(torch.randn(Nout, generator=g))
    y0 = _bf(torch.randn(B, Nout + 3, generator=g))
    y = y0.clone().to(DEV) if accum else torch.full((B, Nout + 3), float("nan"), device=DEV)
    xd, wd, bd = x.to(DEV), w.to(torch.bfloat16).to(DEV), b.to(torch.bfloat16).to(DEV)
    outs = []
    for _ in range(2):
        yy = y.clone()
        L.check(L.lib().ptx_linear_setsum_bf16w_fwd(_ptr(xd), _ptr(wd), _ptr(bd), _ptr(yy), B, n_sets, K, Nout, K, Nout + 3,
                                                    ACCUM if accum else 0, _st()), "ptx_linear_setsum_bf16w_fwd")
        torch.cuda.synchronize()
        outs.append(yy.cpu())
    got = outs[0]
    assert torch.equal(outs[0][:, :Nout], outs[1][:, :Nout])
    assert torch.equal(got[:, Nout:], y0[:, Nout:]) if accum else torch.isnan(got[:, Nout:]).all()
    # the set sum of bf16-exact values is taken in fp32: its rounding is inside the bound's |x| term (sum of |x_r|)
    xs = x.view(n_sets, B, K).double()
    ref_x, abs_x = xs.sum(0), xs.abs().sum(0)
    ref = ref_x @ w.double().t() + n_sets * b.double() + (y0[:, :Nout].double() if accum else 0)
    mag = abs_x @ w.double().abs().t() + n_sets * b.double().abs() + (y0[:, :Nout].double().abs() if accum else 0)
    err = (got[:, :Nout].double() - ref).abs()
    print("setsum accum=%s: max err %.3e, max err / bar %.3f" % (accum, float(err.max()), float((err / (2.0 ** -20 * mag)).max())))
    assert torch.all(err <= 2.0 ** -20 * mag)


# ------------------------------------------------------------------------------------------------ 2. exact tap mapping
@pytest.mark.parametrize("M,K,Nout", [(8, 2048, 96), (9, 2056, 100), (24, 4096, 339), (5, 37, 7)])
def test_exact_tap_dense(M, K, Nout):
    """One 1.0 per weight row at a seeded k, a seeded permutation of the integers -125 .. 125 in x (bf16-exact, neighbours
    differ): y[m][n] is x[m][k(n)] exactly -- a wrong LDS or fragment index selects another integer."""
    g = torch.Generator().manual_seed(400 + M)
    x = (torch.randperm(M * K, generator=g) % 251 - 125).float().view(M, K)
    taps = torch.randint(0, K, (Nout,), generator=g)
    taps[0], taps[-1] = 0, K - 1
    w = torch.zeros(Nout, K)
    w[torch.arange(Nout), taps] = 1.0
    want = x[:, taps]
    for kind in (XB, XF):
        xd = (x.to(torch.bfloat16) if kind == XB else x).to(DEV).contiguous()
        got = _dense(xd, kind, w.to(torch.bfloat16).to(DEV), None, M, K, Nout, 0)
        assert torch.equal(got, want), (kind, float((got - want).abs().max()))


def test_exact_tap_gather():
    B, T, F_, Nout = 3, 8, 264, 96
    g = torch.Generator().manual_seed(500)
    x = (torch.randperm(B * T * F_, generator=g) % 251 - 125).float().view(B, T, F_)
    for n_frames in (2, 5, 8):
        subsets = SUBSETS[n_frames]
        K = n_frames * F_
        taps = torch.randint(0, K, (Nout,), generator=g)
        taps[0], taps[-1] = 0, K - 1
        w = torch.zeros(Nout, K)
        w[torch.arange(Nout), taps] = 1.0
        rows = torch.cat([x[:, list(s), :].reshape(B, K) for s in subsets], 0)
        got = _gather(x.to(torch.bfloat16).to(DEV), subsets, w.to(torch.bfloat16).to(DEV), None, Nout, 0)
        assert torch.equal(got, rows[:, taps]), n_frames


# ------------------------------------------------------------------------------------------------ 3. relation modules
def _bf_sd(sd):
    return {k: (_bf(v) if v.is_floating_point() else v) for k, v in sd.items()}


def _sd16(sd):
    return {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in sd.items()}


NP_SEED = 7


@functools.lru_cache(maxsize=None)
def _relation_case(kind):
    """(module in bf16 on the CPU, x bf16 [4,1,8,256], fp32 reference, bar) -- reference and bar are computed once."""
    mod = ptx.Relation(8, 256, 96, 128) if kind == "relation" else ptx.MultiScaleRelation(8, 256, 96, 128, 3)
    sd = _bf_sd(synth_state_dict(mod.state_dict(), 77))
    mod.load_state_dict(sd)
    x = torch.randn(4, 1, 8, 256, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)

    def oracle(s, xx):
        if kind == "relation":
            return OF.relation(s, xx, "", 8)
        return OF.multiscale_relation(s, xx, 8, 3, np.random.RandomState(NP_SEED))
    with torch.no_grad():
        ref = oracle(sd, x.float())
        err_torch = float((oracle(_sd16(sd), x).float() - ref).abs().max())
    bar = 2 * err_torch + 1e-3 * float(ref.abs().max())
    return mod.to(torch.bfloat16), x, ref, bar


@pytest.mark.parametrize("kind", ["relation", "multiscale"])
def test_relation_modules(kind):
    mod, x, ref, bar = _relation_case(kind)
    mod = mod.to(DEV)
    np.random.seed(NP_SEED)
    with torch.no_grad():
        out = mod(x.to(DEV))
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (4, 1, 96)
    err = float((out.float().cpu() - ref).abs().max())
    print("%s: max|ref| %.3f  bar %.4f  err %.4f" % (kind, float(ref.abs().max()), bar, err))
    assert err <= bar, (err, bar)
    np.random.seed(NP_SEED)
    with torch.no_grad():
        assert torch.equal(mod(x.to(DEV)), out)


# ------------------------------------------------------------------------------------------------ 4. 2-D model parity
MODEL_CASES = {"resnet18_64": ("resnet18", (3, 3, 64, 64)), "resnet18_75x90": ("resnet18", (2, 3, 75, 90)),
               "resnet50_64": ("resnet50", (2, 3, 64, 64))}
# seeds whose REFERENCE alone satisfies margin > 2 bar for every sample (checked on the CPU before they were committed)
MODEL_SEED = {"resnet18_64": 1234, "resnet18_75x90": 1234, "resnet50_64": 7}


def _margin(ref):
    top2 = ref.topk(2, -1).values
    return top2[..., 0] - top2[..., 1]


@functools.lru_cache(maxsize=None)
def _model_case(case):
    """(fp32 model on the CPU holding the bf16-exact state dict, x bf16, fp32 reference, bar)."""
    arch, shape = MODEL_CASES[case]
    m = ptx.__dict__[arch](num_classes=51, pretrained=None)
    sd = _bf_sd(synth_state_dict(m.state_dict(), MODEL_SEED[case]))
    m.load_state_dict(sd)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    ref = OF.forward(OF.ARCHS[arch], sd, x.float())
    err_torch = float((OF.forward(OF.ARCHS[arch], _sd16(sd), x).float() - ref).abs().max())
    bar = 2 * err_torch + 1e-3 * float(ref.abs().max())
    return m, x, ref, bar


def _to_device_bf16(m, stem="direct"):
    m = m.eval().to(torch.bfloat16).to(DEV)
    eng = m.engine() if hasattr(m, "engine") else m.base_model.engine()
    eng.lanes = 1
    eng.bf16_stem = stem
    return m


@pytest.mark.parametrize("case", list(MODEL_CASES))
def test_model_parity_2d(case):
    import copy
    m, x, ref, bar = _model_case(case)
    m = _to_device_bf16(copy.deepcopy(m))
    with torch.no_grad():
        out = m(x.to(DEV))
        assert torch.equal(m.logits(m.features(x.to(DEV))), out)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (x.shape[0], 51)
    o = out.float().cpu()
    err = float((o - ref).abs().max())
    margin = _margin(ref)
    print("%s: max|ref| %.3f  bar %.4f  err %.4f  smallest margin %.3f" % (case, float(ref.abs().max()), bar, err, float(margin.min())))
    assert torch.all(margin > 2 * bar), (margin, bar)
    assert err <= bar, (err, bar)
    assert torch.equal(o.argmax(1), ref.argmax(1))


# ------------------------------------------------------------------------------------------------ 5. TRN
TRN_SEED = {"TRN": 1234, "MSTRN": 1234, "HTRN": 7}            # chosen like MODEL_SEED


def _trn(consensus):
    return ptx.TRN(51, num_segments=4, arch="resnet18", consensus=consensus, frame_bottleneck_dim=128, video_feature_dim=64,
                   pretrained=None)


@functools.lru_cache(maxsize=None)
def _trn_case(consensus):
    m = _trn(consensus)
    sd = _bf_sd(synth_state_dict(m.state_dict(), TRN_SEED[consensus]))
    m.load_state_dict(sd)
    x = torch.randn(2, 4, 3, 64, 64, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16)
    cfg = OF.ARCHS["resnet18"]
    ref = OF.trn_forward(cfg, sd, x.float(), 4, consensus, np.random.RandomState(NP_SEED))
    err_torch = float((OF.trn_forward(cfg, _sd16(sd), x, 4, consensus, np.random.RandomState(NP_SEED)).float() - ref).abs().max())
    bar = 2 * err_torch + 1e-3 * float(ref.abs().max())
    return m, x, ref, bar


@pytest.mark.parametrize("consensus", ["TRN", "MSTRN", "HTRN"])
def test_trn_parity(consensus):
    import copy
    m, x, ref, bar = _trn_case(consensus)
    m = _to_device_bf16(copy.deepcopy(m))
    xd = x.to(DEV)
    with torch.no_grad():
        np.random.seed(NP_SEED)
        out = m(xd)
        np.random.seed(NP_SEED)
        feats = m.features(xd)
        assert feats.dtype == torch.bfloat16 and tuple(feats.shape) == (2, 64)
        assert torch.equal(m.logits(feats), out)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and tuple(out.shape) == (2, 51)
    o = out.float().cpu()
    err = float((o - ref).abs().max())
    margin = _margin(ref)
    print("%s: max|ref| %.3f  bar %.4f  err %.4f  smallest margin %.3f" % (consensus, float(ref.abs().max()), bar, err, float(margin.min())))
    assert torch.all(margin > 2 * bar), (margin, bar)
    assert err <= bar, (err, bar)
    assert torch.equal(o.argmax(1), ref.argmax(1))


# ------------------------------------------------------------------------------------------------ 6. frames and views
def _video(n, t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, t, h, w, 3), dtype=torch.uint8, generator=g).to(DEV)


def test_frames_resnet18():
    import copy
    TF = ptx.transforms
    opts = dict(IMAGENET_BGR255, input_size=[3, 64, 64])
    m = _to_device_bf16(copy.deepcopy(_model_case("resnet18_64")[0]))
    frames = _video(1, 3, 64, 64, 61)[0]                                              # [3,64,64,3]: three images
    with torch.no_grad():
        got = m.forward_frames(frames, opts)
        clip = TF.FramesToTensor(opts)(frames[None])                                  # [1,3,T,H,W]
        want = m(clip[0].permute(1, 0, 2, 3).contiguous().to(torch.bfloat16))
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == (3, 51)
    assert torch.equal(got, want), float((got.float() - want.float()).abs().max())


def test_frames_and_views_trn():
    import copy
    TF = ptx.transforms
    opts = dict(IMAGENET_BGR255, input_size=[3, 64, 64])
    m = _to_device_bf16(copy.deepcopy(_trn_case("TRN")[0]))
    with torch.no_grad():
        frames = _video(2, 4, 64, 64, 62)
        got = m.forward_frames(frames, opts)
        clip = TF.FramesToTensor(opts)(frames)                                        # [2,3,4,64,64]
        want = m(clip.permute(0, 2, 1, 3, 4).contiguous().to(torch.bfloat16))
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (2, 51)
        assert torch.equal(got, want), float((got.float() - want.float()).abs().max())
        video = _video(2, 40, 90, 120, 63)
        vs = TF.SampleViews(opts, num_frames=4, clips=2, crops=1, sampling="segments")
        views = vs(video)                                                             # [2,2,4,64,64,3]
        assert tuple(views.shape) == (2, 2, 4, 64, 64, 3)
        per_view = m.forward_frames(views.reshape((4,) + tuple(views.shape[2:])), opts).reshape(2, 2, 51)
        probs = m.forward_views(video, opts, views=vs)
        assert probs.dtype == torch.float32 and tuple(probs.shape) == (2, 51)
        assert torch.allclose(probs, torch.softmax(per_view.float(), -1).mean(1), rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------ 7. API
def test_api_dtype_mismatch_and_fold():
    import copy
    mod, x, _, _ = _relation_case("relation")
    mod = copy.deepcopy(mod).to(DEV)
    with torch.no_grad():
        with pytest.raises(PtxError, match="bfloat16"):
            mod(x.float().to(DEV))
        with pytest.raises(PtxError, match="bfloat16"):
            copy.deepcopy(mod).float()(x.to(DEV))
        ms = copy.deepcopy(_relation_case("multiscale")[0]).to(DEV)
        with pytest.raises(PtxError, match="bfloat16"):
            ms(x.float().to(DEV))
        with pytest.raises(PtxError, match="bfloat16"):
            ms.float()(x.to(DEV))
        trn = _to_device_bf16(copy.deepcopy(_trn_case("TRN")[0]), stem="fold")
        with pytest.raises(PtxError, match="bf16_stem = 'direct'"):
            trn(_trn_case("TRN")[1].to(DEV))


def test_graph_capture_resnet18():
    """The engine's captured forward (Engine.use_graph: torch.cuda.graph around the plan's launches) replays to the eager bits,
    also after the static input buffer is refilled."""
    import copy
    m, x, _, _ = _model_case("resnet18_64")
    m = _to_device_bf16(copy.deepcopy(m))
    xd = x.to(DEV)
    with torch.no_grad():
        eager = m(xd).clone()
        eager2 = m(xd.flip(0).contiguous()).clone()
        torch.cuda.synchronize()
        m.engine().use_graph = True
        assert torch.equal(m(xd), eager)                 # captures
        assert torch.equal(m(xd.flip(0).contiguous()), eager2)         # replays on new input
        assert torch.equal(m(xd), eager)
        torch.cuda.synchronize()
