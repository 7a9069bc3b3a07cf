"""GPU tests of the class activation maps (include/ptx_amd_cam.h; `model.cam`, `model.cam_frames`, `model.logits_map`,
`pretorched.transforms.CamOverlay`).  `ptx_cam_scores` is held to a float64 reference within a bound that is derived, not tuned, and
holds for any summation order; `ptx_cam_quantize` and `ptx_cam_overlay` to their numpy statements bit for bit.  Output buffers of the
direct launches are pre-filled (NaN / 0xAA bytes) so an element the kernel does not write fails.  References are built with plain
torch / numpy on CPU copies, never through a CPU model."""
import ctypes as C

import numpy as np
import pytest
import torch

from pretorched_x_amd.testing import synth_frames, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPTS = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], input_size=[3, 96, 96])
CLASSES = 11


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def score_bound(x64, w64, b64, cls):
    """1.01 (C + 2) 2^-24 (|b| + sum_c |w_c x_c|) per element: C products and C adds (the bias is one of them), each rounded once to
    fp32 in whatever order, (1 + 2^-24)^(C + 1) - 1 <= 1.01 (C + 2) 2^-24 for every C the models have.  x64 [N, S, C] (positions
    first), w64 [classes, C], cls [N, k] -> [N, k, S]."""
    mag = torch.einsum("nkc,nsc->nks", w64[cls].abs(), x64.abs())
    if b64 is not None:
        mag = mag + b64.abs()[cls][:, :, None]
    return 1.01 * (x64.shape[2] + 2) * 2.0 ** -24 * mag


def scores_f64(x64, w64, b64, cls):
    out = torch.einsum("nkc,nsc->nks", w64[cls], x64)
    return out + b64[cls][:, :, None] if b64 is not None else out


def run_scores(ptx, x_dev, bf16, w, b, cls, S, Cc, ld):
    """ptx_cam_scores and ptx_cam_quantize through ctypes into pre-filled buffers."""
    L = ptx._lib
    lib = L.lib()
    N, k = cls.shape
    assert lib.ptx_cam_scores_supported(N, S, Cc, ld, k, w.shape[0], int(bf16)) == 1, lib.ptx_last_error().decode()
    d_w, d_cls = w.to(DEV), cls.to(torch.int32).to(DEV)
    d_b = b.to(DEV) if b is not None else None
    y = torch.full((N, k, S), float("nan"), device=DEV)
    L.check(lib.ptx_cam_scores(ptr(x_dev), int(bf16), ptr(d_w), ptr(d_b) if d_b is not None else None, ptr(d_cls), ptr(y), N, S, Cc, ld, k,
                               w.shape[0], stream()), "ptx_cam_scores")
    q = torch.full((N, k, S), 0xAA, dtype=torch.uint8, device=DEV)
    L.check(lib.ptx_cam_quantize(ptr(y), ptr(q), N * k, S, stream()), "ptx_cam_quantize")
    torch.cuda.synchronize()
    return y.cpu(), q.cpu()


# --------------------------------------------------------------------------------------------- 1. scores and maps, direct launches
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("Cc", [36, 510, 512, 2048])
def test_cam_scores_against_float64_and_maps_against_numpy(ptx, Cc, bf16):
    """C: below one 16-byte step of a wave | a tail behind the last full group (510 = 127 * 4 + 2 = 63 * 8 + 6) | exact | the widest
    head (8 rows fill the LDS).  S: one position | one workgroup's 16 and a ragged last one | more than one wave round.  fp32 rows
    with pad channels behind C (16-byte rows, and an odd pitch: the one-channel loop), bf16 rows with ld % 8 == 0; the pad holds NaN."""
    g = torch.Generator().manual_seed(Cc + int(bf16))
    w = torch.randn(CLASSES, Cc, generator=g) * 0.05
    b = torch.randn(CLASSES, generator=g)
    N = 2
    lds = [(Cc + 7) // 8 * 8 + 8] if bf16 else [(Cc + 3) // 4 * 4 + 4, Cc + 1]
    for ld in lds:
        for S in (1, 49, 98, 130):
            x = torch.full((N, S, ld), float("nan"))
            x[:, :, :Cc] = torch.randn(N, S, Cc, generator=g)
            if bf16:
                x = x.to(torch.bfloat16)
            x_dev = x.to(DEV)
            x64 = x[:, :, :Cc].double()
            for k in (1, 3, 8):
                cls = torch.randint(0, CLASSES, (N, k), generator=g)
                if k > 1:
                    cls[:, -1] = cls[:, 0]                          # a repeated class
                for bias in ((b, None) if (S == 49 and k == 3) else (b,)):
                    y, q = run_scores(ptx, x_dev, bf16, w, bias, cls, S, Cc, ld)
                    b64 = bias.double() if bias is not None else None
                    want, bound = scores_f64(x64, w.double(), b64, cls), score_bound(x64, w.double(), b64, cls)
                    err = (y.double() - want).abs()
                    assert bool(torch.isfinite(y).all()) and bool((err <= bound).all()), (Cc, bf16, ld, S, k, float((err / bound).max()))
                    if k > 1:
                        assert torch.equal(y[:, -1], y[:, 0])
                    assert np.array_equal(q.numpy(), ptx.transforms.cam_quantize_numpy(y.numpy())), (Cc, bf16, ld, S, k)


def test_cam_scores_clamps_a_wrong_class_and_quantize_handles_flat_and_nan_maps(ptx):
    L = ptx._lib
    lib = L.lib()
    g = torch.Generator().manual_seed(4)
    w, b = torch.randn(CLASSES, 40, generator=g), torch.randn(CLASSES, generator=g)
    x = torch.randn(1, 20, 40, generator=g)
    y, _ = run_scores(ptx, x.to(DEV), False, w, b, torch.tensor([[-5, CLASSES + 3]]), 20, 40, 40)
    ref, _ = run_scores(ptx, x.to(DEV), False, w, b, torch.tensor([[0, CLASSES - 1]]), 20, 40, 40)
    assert torch.equal(y, ref)
    s = torch.randn(6, 300, generator=g) * 3
    s[1] = 2.5                                                       # flat
    s[2, 7] = float("nan")
    s[3] = float("nan")                                              # no score at all
    s[4, 0], s[4, 1] = float("inf"), float("-inf")
    s[5, :] = 0.0
    s[5, 3] = -0.0
    q = torch.full((6, 300), 0xAA, dtype=torch.uint8, device=DEV)
    d = s.to(DEV)
    L.check(lib.ptx_cam_quantize(ptr(d), ptr(q), 6, 300, stream()), "ptx_cam_quantize")
    torch.cuda.synchronize()
    want = ptx.transforms.cam_quantize_numpy(s.numpy()[None])[0]
    assert np.array_equal(q.cpu().numpy(), want)
    assert not want[1].any() and not want[3].any() and not want[5].any() and want[2, 7] == 0 and want[0].max() == 255


# --------------------------------------------------------------------------------------------- 2. the overlay, direct launches
# (h, w) -> (H, W), (T, Tm), k: the host test's geometries; W = 53 gives rows of 159 bytes and frames of an odd byte count, so clips
# start at every alignment (the byte path), 224 x 224 is the dword path over seven chunks with a ragged last one
OVERLAYS = [((1, 1), (16, 16), (5, 2), 1), ((2, 3), (5, 7), (4, 1), 3), ((7, 7), (37, 53), (5, 2), 3), ((7, 7), (224, 224), (3, 3), 3),
            ((3, 7), (3, 50), (4, 1), 2), ((14, 14), (10, 10), (3, 3), 1)]


def run_overlay(ptx, maps, frames, lut, alpha, steps, mode):
    L, TF = ptx._lib, ptx.transforms
    lib = L.lib()
    N, k, Tm, h, w = maps.shape
    T, H, W = frames.shape[1:4]
    rows, cols = TF.resize_axis_table(h, H), TF.resize_axis_table(w, W)
    desc = L.CamOverlayDesc(N, k, Tm, h, w, T, H, W, rows[2].shape[1], cols[2].shape[1], mode, alpha)
    rk, ck = np.ascontiguousarray(rows[2]), np.ascontiguousarray(cols[2])
    assert lib.ptx_cam_overlay_supported(C.byref(desc), C.c_void_p(rk.ctypes.data), C.c_void_p(ck.ctypes.data)) == 1, lib.ptx_last_error().decode()
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in rows + cols]
    d_step = torch.from_numpy(np.asarray(steps, np.int32)).to(DEV)
    d_maps, d_frames, d_lut = (torch.from_numpy(a).to(DEV) for a in (maps, frames, lut))
    y = torch.full((N, k, T, H, W) + (() if mode == L.PTX_CAM_OUT_MAP else (3,)), 0xAA, dtype=torch.uint8, device=DEV)
    L.check(lib.ptx_cam_overlay(C.byref(desc), ptr(d_maps), ptr(d_frames) if mode == L.PTX_CAM_OUT_OVERLAY else None, ptr(d_lut),
                                *[ptr(t) for t in dev], ptr(d_step), ptr(y), stream()), "ptx_cam_overlay")
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("case", OVERLAYS, ids=["%dx%d_to_%dx%d_T%dof%d_k%d" % (c[0] + c[1] + c[2] + (c[3],)) for c in OVERLAYS])
def test_cam_overlay_equals_the_numpy_statement(ptx, case):
    TF = ptx.transforms
    (h, w), (H, W), (T, Tm), k = case
    rng = np.random.default_rng(H * 7 + W)
    N = 2
    maps = rng.integers(0, 256, (N, k, Tm, h, w), dtype=np.uint8)
    maps[0, 0] = 255 * rng.integers(0, 2, (Tm, h, w), dtype=np.uint8)
    frames = rng.integers(0, 256, (N, T, H, W, 3), dtype=np.uint8)
    frames[1, 0, : H // 2] = 255
    frames[1, 0, H // 2:] = 0
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    steps = TF.cam_default_steps(T, Tm)
    for alpha in (0.4, 0.0, 1.0):
        got = run_overlay(ptx, maps, frames, lut, alpha, steps, 0)
        want = TF.cam_overlay_numpy(maps, frames, lut, alpha)
        assert np.array_equal(got, want), (case, alpha, int((got != want).sum()))
    back = steps[::-1].copy()                                        # any step row, not only the default
    assert np.array_equal(run_overlay(ptx, maps, frames, lut, 0.4, back, 0), TF.cam_overlay_numpy(maps, frames, lut, 0.4, steps=back))
    assert np.array_equal(run_overlay(ptx, maps, frames, lut, 0.4, steps, 1), TF.cam_overlay_numpy(maps, (T, H, W), lut, out="heat"))
    assert np.array_equal(run_overlay(ptx, maps, frames, lut, 0.4, steps, 2), TF.cam_overlay_numpy(maps, (T, H, W), out="map"))


def test_cam_overlay_public_call(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    rng = np.random.default_rng(11)
    maps = rng.integers(0, 256, (2, 3, 2, 3, 3), dtype=np.uint8)
    frames = rng.integers(0, 256, (2, 5, 37, 53, 3), dtype=np.uint8)
    d_maps, d_frames = torch.from_numpy(maps).to(DEV), torch.from_numpy(frames).to(DEV)
    ov = TF.CamOverlay()
    got = ov(d_frames, d_maps)
    assert got.shape == (2, 3, 5, 37, 53, 3) and np.array_equal(got.cpu().numpy(), TF.cam_overlay_numpy(maps, frames))
    assert torch.equal(ov(d_frames, d_maps), got) and len(ov._cache) == 1          # the tables are built once per geometry
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    heat = TF.CamOverlay(colormap=lut, out="heat")(d_frames, d_maps, steps=[1, 0, 1, 0, 1])
    assert np.array_equal(heat.cpu().numpy(), TF.cam_overlay_numpy(maps, (5, 37, 53), lut, steps=[1, 0, 1, 0, 1], out="heat"))
    big = TF.CamOverlay(out="map")(d_frames, d_maps)
    assert big.shape == (2, 3, 5, 37, 53) and np.array_equal(big.cpu().numpy(), TF.cam_overlay_numpy(maps, (5, 37, 53), out="map"))
    # the 2-D form: one frame, one map
    flat = TF.CamOverlay(alpha=0.7)(d_frames[:, 0], d_maps[:, :, 0])
    assert flat.shape == (2, 3, 37, 53, 3)
    assert np.array_equal(flat.cpu().numpy(), TF.cam_overlay_numpy(maps[:, :, :1], frames[:, :1], alpha=0.7)[:, :, 0])
    # launches of ranges of (n, j) when the output passes the per-launch limit: whole clips, then runs of one clip's classes
    for limit in (2 * 3 * 5 * 37 * 53 * 3 - 1, 2 * 5 * 37 * 53 * 3):
        small = TF.CamOverlay()
        small.LIMIT_BYTES = limit
        assert torch.equal(small(d_frames, d_maps), got)
    small.LIMIT_BYTES = 100
    with pytest.raises(E, match="2 GiB"):
        small(d_frames, d_maps)
    with pytest.raises(E, match="steps"):
        ov(d_frames, d_maps, steps=[0, 0, 0, 0, 2])
    with pytest.raises(E, match="expected frames"):
        ov(d_frames, d_maps[:, :, 0])


# --------------------------------------------------------------------------------------------- 3. the models
def _model(ptx, name, bf16=False):
    m = ptx.__dict__[name](num_classes=CLASSES, pretrained=None)
    sd = synth_state_dict(m.state_dict(), 1234)
    if bf16:
        sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    m.load_state_dict(sd)
    m = m.eval()
    return (m.to(torch.bfloat16) if bf16 else m).to(DEV)


def _check_result(ptx, m, x, r, k):
    """One CamResult against model(x), model.features(x) and the classifier, recomputed in float64 on CPU copies."""
    head = m.head_module
    logits = m(x)
    assert torch.equal(r.logits, logits) and r.logits.dtype == logits.dtype
    feats = m.features(x).float().cpu()                              # NCDHW; bf16 features widen exactly
    N, Cf = feats.shape[:2]
    pos = tuple(feats.shape[2:])
    assert r.classes.shape == (N, k) and r.classes.dtype == torch.int64
    assert r.scores.shape == (N, k) + pos and r.scores.dtype == torch.float32 and r.maps.shape == r.scores.shape and r.maps.dtype == torch.uint8
    x64 = feats.double().flatten(2).transpose(1, 2)                  # [N, S, C]
    w64, b64 = head.weight.detach().float().cpu().double(), head.bias.detach().float().cpu().double()
    cls = r.classes.cpu()
    want, bound = scores_f64(x64, w64, b64, cls), score_bound(x64, w64, b64, cls)
    err = (r.scores.cpu().double().flatten(2) - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert np.array_equal(r.maps.cpu().numpy(), ptx.transforms.cam_quantize_numpy(r.scores.cpu().numpy()))
    return logits, pos


@pytest.mark.parametrize("name,bf16,shape", [("resnet3d18", False, (2, 3, 32, 96, 96)), ("resnet3d18", True, (2, 3, 32, 96, 96)),
                                              ("resnet18", False, (2, 3, 96, 96))], ids=["resnet3d18", "resnet3d18_bf16", "resnet18_2d"])
def test_model_cam(ptx, name, bf16, shape):
    m = _model(ptx, name, bf16)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    if bf16:
        x = x.to(torch.bfloat16)
    with torch.no_grad():
        r = m.cam(x, topk=3)
        logits, pos = _check_result(ptx, m, x, r, 3)
        assert pos == ((2, 3, 3) if len(shape) == 5 else (3, 3)) and r.frames is None
        assert torch.equal(r.classes, logits.float().topk(3, dim=1).indices)
        # named classes: a list per clip with a repeat, more classes than one launch takes, one class for every clip
        lst = m.cam(x, classes=[[4, 0, 4], [7, 7, 1]])
        _check_result(ptx, m, x, lst, 3)
        assert lst.classes.tolist() == [[4, 0, 4], [7, 7, 1]]
        assert torch.equal(lst.scores[0, 0], lst.scores[0, 2]) and torch.equal(lst.scores[1, 0], lst.scores[1, 1])
        every = m.cam(x, topk=CLASSES)                               # 11 classes: two launches of 8 and 3
        _check_result(ptx, m, x, every, CLASSES)
        one = m.cam(x, classes=2)
        assert one.classes.tolist() == [[2], [2]]
        _check_result(ptx, m, x, one, 1)
        if not bf16:
            # every class at every position: the chosen rows agree with the scores (two summation orders: twice the bound)
            feats = m.features(x)
            lm = m.logits_map(feats)
            assert lm.shape == (shape[0], CLASSES) + pos
            x64 = feats.cpu().double().flatten(2).transpose(1, 2)
            head = m.head_module
            w64, b64 = head.weight.detach().cpu().double(), head.bias.detach().cpu().double()
            allc = torch.arange(CLASSES)[None].expand(shape[0], CLASSES)
            err = (lm.cpu().double().flatten(2) - scores_f64(x64, w64, b64, allc)).abs()
            assert bool((err <= score_bound(x64, w64, b64, allc)).all())
        else:
            with pytest.raises(ptx._lib.PtxError, match="float32 features"):
                m.logits_map(m.features(x))
        # another head: raises, naming the supported set
        import torch.nn as nn
        keep = m.head_module
        setattr(m, m.arch.head, nn.Identity())
        with pytest.raises(ptx._lib.PtxError, match="nn.Linear head"):
            m.cam(x)
        setattr(m, m.arch.head, keep)
        assert torch.equal(m.cam(x, topk=3).scores, r.scores)


@pytest.mark.parametrize("name", ["resnet3d18", "resnet18"])
def test_model_cam_frames_and_overlay(ptx, name):
    TF = ptx.transforms
    m = _model(ptx, name)
    dims = m.arch.dims
    raw = synth_frames(2 * (8 if dims == 3 else 1), 120, 150, 21).reshape((2, 8, 120, 150, 3) if dims == 3 else (2, 120, 150, 3))
    raw = torch.from_numpy(raw).to(DEV)
    tf = TF.TransformFrames(OPTS, out="frames")
    with torch.no_grad():
        r = m.cam_frames(raw, OPTS, transform=tf, topk=2)
        seen = tf(raw)
        assert r.frames.dtype == torch.uint8 and torch.equal(r.frames, seen) and tuple(seen.shape[-3:]) == (96, 96, 3)
        assert torch.equal(r.logits, m.forward_frames(raw, OPTS, transform=tf))
        assert torch.equal(r.classes, r.logits.topk(2, dim=1).indices)
        # the same clip through the tensor entry point: FramesToTensor's bits feed the same trunk
        clip = TF.FramesToTensor(OPTS)(seen if dims == 3 else seen[:, None])
        clip = clip if dims == 3 else clip[:, :, 0].contiguous()
        _check_result(ptx, m, clip, m.cam(clip, classes=r.classes), 2)
        same = m.cam_frames(seen, OPTS, classes=r.classes)
        assert torch.equal(same.scores, r.scores) and torch.equal(same.maps, r.maps) and torch.equal(same.frames, seen)
        assert np.array_equal(r.maps.cpu().numpy(), TF.cam_quantize_numpy(r.scores.cpu().numpy()))
        for out in TF.CAM_OUT:
            got = TF.CamOverlay(out=out)(r.frames, r.maps)
            f5 = seen.cpu().numpy() if dims == 3 else seen.cpu().numpy()[:, None]
            m5 = r.maps.cpu().numpy() if dims == 3 else r.maps.cpu().numpy()[:, :, None]
            want = TF.cam_overlay_numpy(m5, f5, out=out)
            assert np.array_equal(got.cpu().numpy(), want if dims == 3 else want[:, :, 0]), out
