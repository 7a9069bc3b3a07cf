"""Host tests (no GPU) of the class activation maps (include/ptx_amd_cam.h; `pretorched.transforms.cam_quantize_numpy`,
`cam_overlay_numpy`, `CamOverlay`; `model.cam`, `model.logits_map`): the numpy statement of the overlay against Pillow itself, bit
for bit; the quantiser on flat, NaN-holding and ordinary maps; the census of the header, the bindings and the exports; the
`_supported` answers from descriptors alone; the CPU (eager.py) answers of a 3-D and a 2-D ResNet against the definition written
out in torch; everything that raises."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
from PIL import Image

from pretorched_x_amd.testing import synth_state_dict

# (h, w) -> (H, W): one cell | odd both ways | a map of 7x7 to odd sizes | the flagship geometry | an axis that is not resampled |
# down-sampling
GEOMETRIES = [((1, 1), (16, 16)), ((2, 3), (5, 7)), ((7, 7), (37, 53)), ((7, 7), (224, 224)), ((3, 7), (3, 50)), ((14, 14), (10, 10))]
ALPHAS = (0.0, 0.4, 1.0)


def pillow_overlay(q, frame, lut, alpha, H, W):
    heat = Image.fromarray(lut[np.asarray(Image.fromarray(q, "L").resize((W, H), Image.BILINEAR))])
    return np.asarray(Image.blend(Image.fromarray(frame), heat, alpha))


# --------------------------------------------------------------------------------------------- 1. the overlay is Pillow's
@pytest.mark.parametrize("geom", GEOMETRIES, ids=["%dx%d_to_%dx%d" % (g[0] + g[1]) for g in GEOMETRIES])
def test_cam_overlay_numpy_equals_pillow(ptx, geom):
    TF = ptx.transforms
    (h, w), (H, W) = geom
    rng = np.random.default_rng(h * 1000 + W)
    lut = TF.jet_colormap()
    other = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    reps = 2 if H * W > 10000 else 6
    for rep in range(reps):
        maps = rng.integers(0, 256, (1, 2, 1, h, w), dtype=np.uint8)
        if rep == 1:
            maps[0, 0] = 255 * (rng.integers(0, 2, (1, h, w), dtype=np.uint8))      # hard edges: both ends of the clip
        frames = rng.integers(0, 256, (1, 1, H, W, 3), dtype=np.uint8)
        for alpha in ALPHAS:
            for table in ((lut, other) if rep == 0 else (lut,)):
                got = TF.cam_overlay_numpy(maps, frames, table, alpha)
                assert got.shape == (1, 2, 1, H, W, 3) and got.dtype == np.uint8
                for j in range(2):
                    want = pillow_overlay(maps[0, j, 0], frames[0, 0], table, alpha, H, W)
                    assert np.array_equal(got[0, j, 0], want), (geom, alpha, j, int((got[0, j, 0] != want).sum()))
        big = TF.cam_overlay_numpy(maps, (1, H, W), out="map")
        assert big.shape == (1, 2, 1, H, W)
        for j in range(2):
            assert np.array_equal(big[0, j, 0], np.asarray(Image.fromarray(maps[0, j, 0], "L").resize((W, H), Image.BILINEAR)))
        assert np.array_equal(TF.cam_overlay_numpy(maps, (1, H, W), lut, out="heat"), lut[big])


def test_cam_overlay_numpy_steps_and_arguments(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    rng = np.random.default_rng(3)
    maps = rng.integers(0, 256, (2, 3, 2, 3, 4), dtype=np.uint8)
    frames = rng.integers(0, 256, (2, 5, 9, 11, 3), dtype=np.uint8)
    assert TF.cam_default_steps(5, 2).tolist() == [0, 0, 0, 1, 1] and TF.cam_default_steps(4, 1).tolist() == [0] * 4
    assert TF.cam_default_steps(3, 3).tolist() == [0, 1, 2] and TF.cam_default_steps(16, 2).tolist() == [0] * 8 + [1] * 8
    got = TF.cam_overlay_numpy(maps, frames)
    assert got.shape == (2, 3, 5, 9, 11, 3)
    lut = TF.jet_colormap()
    for n, j, t in ((0, 0, 0), (1, 2, 2), (1, 1, 3), (0, 2, 4)):
        assert np.array_equal(got[n, j, t], pillow_overlay(maps[n, j, [0, 0, 0, 1, 1][t]], frames[n, t], lut, 0.4, 9, 11))
    swapped = TF.cam_overlay_numpy(maps, frames, steps=[1, 1, 0, 0, 1])
    assert np.array_equal(swapped[0, 1, 0], pillow_overlay(maps[0, 1, 1], frames[0, 0], lut, 0.4, 9, 11))
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert lut[0].tolist() == [0, 0, 128] and lut[255].tolist() == [128, 0, 0] and lut[128, 1] == 255       # blue ... green ... red
    for bad in dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(out="blend"), dict(steps=[0, 0, 0, 2, 1]), \
            dict(steps=[0, 1]), dict(lut=np.zeros((255, 3), np.uint8)), dict(lut="viridis"):
        with pytest.raises(E):
            TF.cam_overlay_numpy(maps, frames, **bad)
    with pytest.raises(E, match="needs the frames"):
        TF.cam_overlay_numpy(maps, (5, 9, 11))
    with pytest.raises(E, match="uint8 CUDA"):                      # host tensors: refused, no fallback
        TF.CamOverlay()(torch.from_numpy(frames), torch.from_numpy(maps))
    for bad in dict(alpha=2), dict(colormap="hot"), dict(out="both"):
        with pytest.raises(E):
            TF.CamOverlay(**bad)


# --------------------------------------------------------------------------------------------- 2. the quantiser
def test_cam_quantize_numpy(ptx):
    q = ptx.transforms.cam_quantize_numpy
    rng = np.random.default_rng(5)
    s = rng.standard_normal((2, 3, 2, 3, 5)).astype(np.float32) * 7
    got = q(s)
    assert got.shape == s.shape and got.dtype == np.uint8
    for n in range(2):
        for j in range(3):
            m = s[n, j]
            want = (np.float32(255) * ((m - m.min()) / (m.max() - m.min()))).astype(np.uint8)       # fp32 throughout; trunc
            assert np.array_equal(got[n, j], want)
            assert got[n, j].min() == 0 and got[n, j].max() == 255
    flat = np.full((1, 2, 4, 4), 3.25, np.float32)
    flat[0, 1] = -0.0
    flat[0, 1, 0, 0] = 0.0
    assert not q(flat).any()
    nan = s.copy()
    nan[0, 0, 0, 0, 0] = np.nan
    nan[1, 2] = np.nan                                               # no score at all: zeros
    got = q(nan)
    rest = np.delete(s[0, 0].reshape(-1), 0)
    want = (np.float32(255) * ((rest - rest.min()) / (rest.max() - rest.min()))).astype(np.uint8)
    assert got[0, 0].reshape(-1)[0] == 0 and np.array_equal(np.delete(got[0, 0].reshape(-1), 0), want)
    assert not got[1, 2].any() and np.array_equal(got[1, 0], q(s)[1, 0])
    inf = np.array([[[0.0, 1.0, np.inf, -1.0]]], np.float32)
    assert q(inf).tolist() == [[[0, 0, 0, 0]]]                       # (s - mn) / inf = 0, inf / inf = NaN -> 0
    two = np.array([[[1.0, 2.0]]], np.float32)
    assert q(two).tolist() == [[[0, 255]]]
    with pytest.raises(ptx._lib.PtxError):
        q(np.zeros(4, np.float32))


# --------------------------------------------------------------------------------------------- 3. header, bindings, exports
def test_cam_header_bindings_and_exports(ptx):
    L = ptx._lib
    lib = L.lib()
    text = open(L.CAM_HEADER_PATH).read()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = L.header_symbols(L.CAM_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_CAM) == ["ptx_cam_overlay", "ptx_cam_overlay_supported", "ptx_cam_quantize", "ptx_cam_scores",
                                                    "ptx_cam_scores_supported"]
    assert not set(declared) & set(L.header_symbols())              # ptx_amd.h stays the census it was
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_CAM[name][0], list(L.SIGNATURES_CAM[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_CAM[name][1]), name
    body = re.search(r"typedef struct ptx_cam_overlay_desc \{(.*?)\}", plain, flags=re.S).group(1)
    fields = [n.strip() for line in body.split(";") for n in line.replace("int32_t", "").replace("float", "").split(",") if n.strip()]
    assert fields == [n for n, _ in L.CamOverlayDesc._fields_]
    assert C.sizeof(L.CamOverlayDesc) == 48 and L.CamOverlayDesc._fields_[-1] == ("alpha", C.c_float)
    for name in ("PTX_CAM_MAX_CLASSES", "PTX_CAM_MAX_LDS_BYTES", "PTX_CAM_MAX_MAP_BYTES", "PTX_CAM_OUT_OVERLAY", "PTX_CAM_OUT_HEAT",
                 "PTX_CAM_OUT_MAP"):
        assert int(re.search(r"#define %s\s+(\d+)\b" % name, text).group(1)) == getattr(L, name), name
    assert L.PTX_CAM_MAX_CLASSES == 8 and ptx.transforms.CAM_OUT == ("overlay", "heat", "map")
    root = os.path.dirname(os.path.dirname(L.HEADER_PATH))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    section = integ.split("### 1r.", 1)[1].split("\n### ", 1)[0]
    assert "ptx_amd_cam.h" in section and all(n in section for n in declared)
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "cam.h" in build.HEADERS and any(h.endswith("ptx_amd_cam.h") for h in build.HEADERS)
    files = build.tu_files("pack_layout.hip")
    assert any(p.endswith(os.sep + "cam.h") for p in files) and any(p.endswith("ptx_amd_cam.h") for p in files)
    assert L.binary_source_hash() == L.source_hash() == build.source_hash()
    src = open(os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py")).read()       # ptx_version()'s hash names the header
    assert '"ptx_amd_cam.h"' in src.split("def source_hash", 1)[1].split("def obj_path", 1)[0]


# --------------------------------------------------------------------------------------------- 4. _supported, no device
def test_cam_supported_answers_from_descriptors(ptx):
    L, TF = ptx._lib, ptx.transforms
    lib = L.lib()

    def scores(N=8, S=98, Cc=2048, ld=2048, k=5, classes=400, bf16=0):
        ok = lib.ptx_cam_scores_supported(N, S, Cc, ld, k, classes, bf16)
        return ok, lib.ptx_last_error().decode()

    assert scores()[0] == 1 and scores(k=8)[0] == 1 and scores(Cc=510, ld=512)[0] == 1 and scores(Cc=1, ld=1, S=1, N=1, k=1)[0] == 1
    assert scores(Cc=36, ld=40, bf16=1)[0] == 1
    for kw, why in ((dict(k=0), "PTX_CAM_MAX_CLASSES"), (dict(k=9), "PTX_CAM_MAX_CLASSES"), (dict(ld=2047), "below C"),
                    (dict(Cc=36, ld=36, bf16=1), "ld % 8"), (dict(Cc=4096, ld=4096, k=8), "LDS"), (dict(S=0), "non-positive"),
                    (dict(S=1 << 21), "32-bit"), (dict(N=70000), "grid"), (dict(classes=0), "non-positive")):
        ok, msg = scores(**kw)
        assert ok == 0 and why in msg, (kw, msg)
    assert scores(Cc=4096, ld=4096, k=4)[0] == 1

    def overlay(rows=None, cols=None, **kw):
        args = dict(N=8, k=5, Tm=2, h=7, w=7, T=16, H=224, W=224, taps_h=2, taps_w=2, mode=0, alpha=0.4)
        args.update(kw)
        d = L.CamOverlayDesc(*[args[n] for n, _ in L.CamOverlayDesc._fields_])
        ok = lib.ptx_cam_overlay_supported(C.byref(d), None if rows is None else C.c_void_p(rows.ctypes.data),
                                           None if cols is None else C.c_void_p(cols.ctypes.data))
        return ok, lib.ptx_last_error().decode()

    assert overlay()[0] == 1 and overlay(mode=1)[0] == 1 and overlay(mode=2)[0] == 1
    # the tap cap: a 1100-row map down to 8 rows needs 2 * ceil(137.5) + 1 taps
    big = TF.resize_axis_table(1100, 8)[2].shape[1]
    assert big > L.PTX_RESIZE_MAX_TAPS
    ok, msg = overlay(h=1100, w=4, H=8, W=8, taps_h=big)
    assert ok == 0 and "PTX_RESIZE_MAX_TAPS" in msg
    assert overlay(taps_w=L.PTX_RESIZE_MAX_TAPS)[0] == 1 and overlay(taps_w=L.PTX_RESIZE_MAX_TAPS + 1)[0] == 0
    # the 2 GiB limit: 8 x 5 maps over 16 frames of 224 x 224 x 3 are 96 MB; 180 clips are past it, the map mode a third of it
    assert overlay(N=178)[0] == 1
    ok, msg = overlay(N=179)
    assert ok == 0 and "2 GiB" in msg
    assert overlay(N=179, mode=2)[0] == 1 and overlay(N=3 * 179, mode=2)[0] == 0
    for kw, why in ((dict(alpha=1.5), "alpha"), (dict(alpha=float("nan")), "alpha"), (dict(mode=3), "mode"), (dict(h=0), "non-positive"),
                    (dict(taps_h=0), "positive"), (dict(h=200, w=200), "PTX_CAM_MAX_MAP_BYTES"), (dict(T=70000, N=1, k=1, H=8, W=8), "grid")):
        ok, msg = overlay(**kw)
        assert ok == 0 and why in msg, (kw, msg)
    assert overlay(alpha=1.5, mode=1)[0] == 1                        # alpha is the overlay mode's
    # coefficient tables: Pillow's pass, a coefficient of 2**23 and an overflowing entry do not
    rows, cols = TF.resize_axis_table(7, 224), TF.resize_axis_table(7, 224)
    assert overlay(rows[2], cols[2])[0] == 1
    bad = rows[2].copy()
    bad[5, 0] = 1 << 23
    ok, msg = overlay(bad, cols[2])
    assert ok == 0 and "2^23" in msg
    wide = np.full((224, 4), (1 << 23) - 1, np.int32)
    ok, msg = overlay(rows[2], wide, taps_w=4)
    assert ok == 0 and "accumulator" in msg
    with pytest.raises(L.PtxError, match="2\\^23"):
        TF._cam_overlay_supported(TF._cam_overlay_desc(1, 1, 1, 7, 7, 1, 224, 224, 2, 2, 0, 0.4), (rows[0], rows[1], bad), cols)


# --------------------------------------------------------------------------------------------- 5. CPU models: the definition
def _cpu_model(ptx, name, classes):
    m = ptx.__dict__[name](num_classes=classes, pretrained=None)
    m.load_state_dict(synth_state_dict(m.state_dict(), 1234))
    return m.eval()


def logit_bound(feats, w, b, cls):
    """|mean over positions of the scores - logit| and |scores - float64| stay inside 1.01 (C + 2) 2^-24 (|b| + sum |w x|) for any
    order of fp32 summation of C products and a bias (each add rounds once: (1 + 2^-24)^(C + 1) - 1 <= 1.01 (C + 2) 2^-24)."""
    f64, w64 = feats.double(), w.double()[cls]                       # [N, C, *pos], [N, k, C]
    mag = torch.einsum("nkc,nc...->nk...", w64.abs(), f64.abs())
    if b is not None:
        mag = mag + b.double().abs()[cls].reshape(cls.shape + (1,) * (feats.dim() - 2))
    return 1.01 * (feats.shape[1] + 2) * 2.0 ** -24 * mag


@pytest.mark.parametrize("name,shape", [("resnet3d18", (1, 3, 32, 96, 96)), ("resnet18", (1, 3, 96, 96))])
def test_cpu_cam_is_the_definition(ptx, name, shape):
    m = _cpu_model(ptx, name, 13)
    head = m.head_module
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        feats = m.features(x)
        logits = m(x)
        r = m.cam(x, topk=3)
        assert isinstance(r, ptx.CamResult) and r.frames is None
        assert torch.equal(r.logits, logits)
        assert r.classes.dtype == torch.int64 and torch.equal(r.classes, logits.topk(3, dim=1).indices)
        pos = tuple(feats.shape[2:])
        assert r.scores.shape == (1, 3) + pos and r.maps.shape == r.scores.shape and r.maps.dtype == torch.uint8
        assert pos == ((2, 3, 3) if len(shape) == 5 else (3, 3))
        want = torch.einsum("nkc,nc...->nk...", head.weight[r.classes], feats) + head.bias[r.classes].reshape((1, 3) + (1,) * len(pos))
        assert torch.equal(r.scores, want)
        assert np.array_equal(r.maps.numpy(), ptx.transforms.cam_quantize_numpy(r.scores.numpy()))
        # the mean over the positions is the logit.  Every score lies within the bound of its exact value, so their mean within the
        # mean bound; the logit is the pool (S adds and a division per channel) and the classifier (C adds and the bias) on the
        # same products: C + S + 2 roundings where a score has C + 1, so (C + S + 3) / (C + 2) of the mean bound
        Cf, S = feats.shape[1], int(np.prod(pos))
        bound = logit_bound(feats, head.weight, head.bias, r.classes).flatten(2).mean(2) * (1.0 + (Cf + S + 3) / (Cf + 2))
        err = (r.scores.double().flatten(2).mean(2) - logits.gather(1, r.classes).double()).abs()
        assert bool((err <= bound).all()), (err, bound)
        # named classes: an int, a list with a repeat
        one = m.cam(x, classes=5)
        assert one.classes.tolist() == [[5]] and torch.equal(one.logits, logits)
        lst = m.cam(x, classes=[[2, 9, 2]])
        assert lst.classes.tolist() == [[2, 9, 2]] and torch.equal(lst.scores[:, 0], lst.scores[:, 2])
        alone = m.cam(x, classes=torch.tensor([[9]]))               # torch sums a [1, C] product in another order than a [3, C] one
        assert bool(((lst.scores[:, 1:2].double() - alone.scores.double()).abs() <= 2 * logit_bound(feats, head.weight, head.bias, alone.classes)).all())
        # every class at every position agrees with the scores on the chosen classes
        lm = m.logits_map(feats)
        assert lm.shape == (1, 13) + pos
        picked = lm[0, r.classes[0]].unsqueeze(0)
        assert bool(((picked.double() - r.scores.double()).abs() <= 2 * logit_bound(feats, head.weight, head.bias, r.classes)).all())


# --------------------------------------------------------------------------------------------- 6. what raises
def test_cam_raises_outside_the_supported_set(ptx):
    E = ptx._lib.PtxError
    x = torch.zeros(1, 3, 8, 32, 32)
    m = _cpu_model(ptx, "resnet3d18", 7)
    m.last_linear = nn.Identity()
    for call in (lambda: m.cam(x), lambda: m.logits_map(torch.zeros(1, 512, 1, 1, 1)), lambda: m.cam_frames(torch.zeros(1, 8, 32, 32, 3, dtype=torch.uint8))):
        with pytest.raises(E, match="nn.Linear head"):
            call()
    m.last_linear = nn.Sequential(nn.Dropout(0.5), nn.Linear(512, 7))
    with pytest.raises(E, match="Sequential"):
        m.cam(x)
    models = [ptx.slowfast.resnet18(mode="sf", num_classes=5), ptx.i3d(num_classes=5, pretrained=None),
              ptx.TRN(5, num_segments=4, arch="resnet18", pretrained=None)]
    for other in models:
        for name in ("cam", "cam_frames", "logits_map"):
            with pytest.raises(E, match="VideoResNet families"):
                getattr(other, name)(x)
    gen = ptx.biggan_deep(128, ch=32)
    with pytest.raises(E, match="VideoResNet families"):
        gen.cam(x)
    # an adopted instance's bound methods
    from pretorched_x_amd import adopt
    foreign = nn.Linear(3, 3)
    adopt._bind(foreign)
    for name in ("cam", "cam_frames", "logits_map"):
        with pytest.raises(E, match="VideoResNet families"):
            getattr(foreign, name)(x)
    # bf16 features, wrong class lists, wrong topk
    good = _cpu_model(ptx, "resnet3d18", 7)
    with pytest.raises(E, match="float32 features"):
        good.logits_map(torch.zeros(1, 512, 1, 2, 2, dtype=torch.bfloat16))
    for bad in (7, -1, [[0, 7]], [[0.5]], [0, 1], [[0], [1]]):
        with pytest.raises(E):
            good.cam(x, classes=bad)
    for bad in (0, 8, 1.0, True):
        with pytest.raises(E, match="topk"):
            good.cam(x, topk=bad)
    with pytest.raises(E):                                           # frames on the host: no CPU route for decoded frames
        good.cam_frames(torch.zeros(1, 8, 32, 32, 3, dtype=torch.uint8), dict(input_space="RGB", input_range=[0, 1], mean=[0.5] * 3, std=[0.5] * 3))
