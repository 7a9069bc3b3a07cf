"""No-GPU tests of the resize + crop edge (`pretorched.transforms.TransformFrames`): the host-built coefficient tables and
a numpy apply of them against PIL's stored outputs (tests/golden/transform_frames.npz, written by
tests/golden/make_transform_golden.py with PIL only), the size / crop rules, the table invariants, the C ABI's argument
checks (every call returns before a launch) and the Python-side errors.  Every comparison is exact equality."""
import ctypes as C
import json
import math
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

from pretorched_x_amd.testing import synth_frames


def golden_cases():
    blob = load_golden("transform_frames")
    return blob, json.loads(str(blob["cases"]))


def case_tables(TF, c):
    crop = c["crop"] if isinstance(c["crop"], str) else tuple(c["crop"])
    return TF.build_tables(c["H"], c["W"], c["input_size"], c["scale"], c["preserve_aspect_ratio"], crop, c["hflip"])


def test_golden_covers_the_required_cases():
    _, cases = golden_cases()
    by = {c["name"]: c for c in cases}
    assert len(by) == len(cases) >= 13
    sizes = {(c["H"], c["W"], max(c["input_size"])) for c in cases}
    assert {(240, 320, 224), (320, 240, 224), (256, 340, 224), (270, 480, 112), (1080, 1920, 224), (50, 70, 112),
            (360, 360, 112)} <= sizes
    assert any(not c["preserve_aspect_ratio"] for c in cases) and any(c["hflip"] for c in cases)
    assert any(c["crop"] == [0, 0] for c in cases) and any(c["content"] == "gradient" for c in cases)
    br = by["corner_bottom_right"]
    assert br["crop"] == [br["resized"][0] - 64, br["resized"][1] - 64]
    assert by["crop_only_256x340"]["resized"] == [256, 340] and by["hd_1080x1920"]["resized"] == [256, 455]
    assert by["landscape_240x320"]["resized"] == [256, 341] and by["portrait_320x240"]["resized"] == [341, 256]


def test_tables_and_numpy_apply_equal_pil_goldens(ptx):
    """The table builder + the integer arithmetic the kernel runs == PIL, bit for bit, on every stored case."""
    TF = ptx.transforms
    blob, cases = golden_cases()
    for c in cases:
        want = blob["out_" + c["name"]]
        frames = synth_frames(c["count"], c["H"], c["W"], c["seed"], c["content"])
        tables = case_tables(TF, c)
        assert list(tables["resized"]) == c["resized"] and list(tables["window"]) == c["window"], c["name"]
        assert want.shape == (c["count"], tables["S"], tables["S"], 3) and want.dtype == np.uint8
        for f, w in zip(frames, want):
            got = TF.apply_tables_numpy(f, tables)
            assert got.dtype == np.uint8 and np.array_equal(got, w), c["name"]
    # the crop-only case is the input window itself; at ratio 4.22 PIL's kernel is 2 * ceil(4.22) + 1 = 11 entries wide, of
    # which the 2 * 4.22 = 8.4 wide support reaches at most 9 pixels: the tables keep the widest row's count
    by = {c["name"]: c for c in cases}
    c = by["crop_only_256x340"]
    f = synth_frames(1, 256, 340, c["seed"])[0]
    assert np.array_equal(blob["out_crop_only_256x340"][0], f[16:240, 58:282])
    t = case_tables(TF, by["hd_1080x1920"])
    assert t["rows"][2].shape[1] == 9 and t["cols"][2].shape[1] == 9
    t = case_tables(TF, c)
    assert t["rows"][2].shape[1] == 1 and t["cols"][2].shape[1] == 1


def test_random_draws_equal_live_pil(ptx):
    """50 seeded draws of (H, W, R, S), up-scales and ratios above 4 included, against PIL itself."""
    Image = pytest.importorskip("PIL.Image")
    TF = ptx.transforms
    rs = np.random.RandomState(2024)
    ups = big = 0
    for i in range(50):
        S = int(rs.randint(8, 65))
        scale = float(rs.uniform(0.5, 1.0))
        R = int(math.floor(S / scale))
        kind = i % 3                                      # 0: ratio above 4, 1: up-scale, 2: anything between
        short = int(R * rs.uniform(4.1, 9.5)) if kind == 0 else int(max(4, R * rs.uniform(0.3, 0.95))) if kind == 1 else \
            int(rs.randint(R, 4 * R))
        long = int(short * rs.uniform(1.0, 1.8))
        H, W = (short, long) if rs.randint(2) else (long, short)
        ups += short < R
        big += short > 4 * R
        frame = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        tables = TF.build_tables(H, W, [3, S, S], scale)
        h, w = tables["resized"]
        top, left = tables["window"]
        img = Image.fromarray(frame)
        if (h, w) != (H, W):
            img = img.resize((w, h), Image.BILINEAR)
        want = np.asarray(img.crop((left, top, left + S, top + S)))
        assert np.array_equal(TF.apply_tables_numpy(frame, tables), want), (i, H, W, scale, S)
    assert ups >= 15 and big >= 15


def test_size_and_crop_rules(ptx):
    """Hand-derived from torchvision's documented semantics: Resize(int R) puts the short side at R and the long side at
    int(R * long / short), and leaves a frame whose short side is R alone; CenterCrop(S) starts at
    int(round((extent - S) / 2.0)) with Python's round (half to even)."""
    TF = ptx.transforms
    table = [
        # H, W, input_size, scale, preserve -> h, w, top, left
        (240, 320, [3, 224, 224], 0.875, True, 256, 341, 16, 58),     # 341 - 224 = 117 -> 58.5 -> 58 (half to even)
        (320, 240, [3, 224, 224], 0.875, True, 341, 256, 58, 16),
        (256, 340, [3, 224, 224], 0.875, True, 256, 340, 16, 58),     # short side already R
        (340, 256, [3, 224, 224], 0.875, True, 340, 256, 58, 16),
        (1080, 1920, [3, 224, 224], 0.875, True, 256, 455, 16, 116),  # 231 / 2 = 115.5 -> 116 (half to even)
        (270, 480, [3, 112, 112], 0.875, True, 128, 227, 8, 58),      # 115 / 2 = 57.5 -> 58
        (360, 360, [3, 112, 112], 0.875, True, 128, 128, 8, 8),
        (50, 70, [3, 112, 112], 0.875, True, 128, 179, 8, 34),        # int(128 * 70 / 50) = 179; 67 / 2 = 33.5 -> 34
        (200, 300, [3, 64, 64], 0.875, False, 73, 73, 4, 4),          # int(64 / 0.875) = 73; 9 / 2 = 4.5 -> 4
        (300, 200, [3, 112, 96], 0.875, False, 128, 109, 8, -1),      # S = 112 does not fit the 109 columns
        (100, 100, [3, 224, 224], 1.0, True, 224, 224, 0, 0),
        (480, 640, [3, 299, 299], 0.875, True, 341, 454, 21, 78),     # int(341 * 640 / 480) = 454; 155 / 2 = 77.5 -> 78
    ]
    for H, W, isz, scale, keep, h, w, top, left in table:
        assert TF.resized_size(H, W, isz, scale, keep) == (h, w), (H, W)
        if left < 0:
            with pytest.raises(ptx._lib.PtxError):
                TF.crop_window(h, w, max(isz), "center")
            continue
        assert TF.crop_window(h, w, max(isz), "center") == (top, left), (H, W)
        t = TF.build_tables(H, W, isz, scale, keep)
        assert t["resized"] == (h, w) and t["window"] == (top, left) and t["S"] == max(isz)
    assert TF.crop_window(73, 97, 64, (9, 33)) == (9, 33)
    for bad in [(10, 0), (0, 34), (-1, 0), "corner", (1,)]:
        with pytest.raises(ptx._lib.PtxError):
            TF.crop_window(73, 97, 64, bad)


def test_table_invariants_and_tap_cap(ptx):
    TF, L = ptx.transforms, ptx._lib
    one = 1 << TF.PRECISION_BITS
    for n_in, n_out in [(90, 64), (64, 90), (1080, 256), (1920, 455), (37, 224), (97, 33), (500, 17), (3100, 100),
                        (31 * 64, 64), (7, 7), (1, 5), (5, 1)]:
        lo, n, k = TF.resize_axis_table(n_in, n_out)
        assert lo.dtype == n.dtype == k.dtype == np.int32 and k.shape == (n_out, int(n.max()))
        assert (lo >= 0).all() and (n >= 1).all() and (lo + n <= n_in).all()
        assert (k >= 0).all() and (k <= one).all()
        for i in range(n_out):
            assert abs(int(k[i, :n[i]].sum()) - one) <= n[i] and not k[i, n[i]:].any()
        assert k.shape[1] <= 2 * math.ceil(max(n_in / n_out, 1.0)) + 1
        if n_in <= 31 * n_out:
            assert k.shape[1] <= L.PTX_RESIZE_MAX_TAPS
    lo, n, k = TF.resize_axis_table(7, 7)                 # not resampled: one tap of 2**22
    assert lo.tolist() == list(range(7)) and k.tolist() == [[one]] * 7
    # a window's tables are the window's slice of the axis tables, columns reversed under hflip
    t = TF.build_tables(120, 90, [3, 64, 64], hflip=True)
    full = TF.resize_axis_table(90, 73)
    left = t["window"][1]
    assert t["cols"][0].tolist() == full[0][left:left + 64][::-1].tolist()
    assert t["rows"][0].tolist() == TF.resize_axis_table(120, 97)[0][t["window"][0]:t["window"][0] + 64].tolist()
    # ratio 31 fits the cap, a ratio beyond it raises
    assert TF.build_tables(31 * 73, 31 * 73, [3, 64, 64])["rows"][2].shape[1] <= L.PTX_RESIZE_MAX_TAPS
    with pytest.raises(L.PtxError, match="PTX_RESIZE_MAX_TAPS"):
        TF.build_tables(40 * 73, 40 * 73, [3, 64, 64])


def test_resize_abi(ptx):
    L = ptx._lib
    lib = L.lib()
    text = open(L.HEADER_PATH).read()
    for name in ("ptx_resize_frames_u8", "ptx_resize_frames_u8_supported"):
        assert name in L.header_symbols() and name in L.SIGNATURES and name not in L.EXPERIMENTAL
        assert name not in L.experimental_symbols() and hasattr(lib, name)
    body = re.sub(r"/\*.*?\*/", "", text.split("typedef struct ptx_resize_desc {")[1].split("}")[0], flags=re.S)
    fields = [n.strip() for decl in body.split(";") for n in decl.replace("int32_t", "").split(",") if n.strip()]
    assert fields == [f for f, _ in L.ResizeDesc._fields_] and C.sizeof(L.ResizeDesc) == 4 * len(fields) == 40
    for name in ("PTX_RESIZE_OUT_U8", "PTX_RESIZE_OUT_F32", "PTX_RESIZE_OUT_BF16", "PTX_RESIZE_MAX_TAPS"):
        assert re.search(r"#define %s %d\b" % (name, getattr(L, name)), text), name

    P = C.c_void_p(64)                                    # never dereferenced: every call below returns before a launch
    norm = L.NormDesc.make([0.4, 0.4, 0.4], [0.2, 0.2, 0.2])

    def call(desc, frames=P, tables=(P,) * 6, y=P, nd=norm):
        return lib.ptx_resize_frames_u8(C.byref(desc) if desc is not None else None, frames, *tables, y,
                                        C.byref(nd) if nd is not None else None, None)

    def err():
        msg = lib.ptx_last_error().decode()
        assert "ptx_resize_frames_u8" in msg
        return msg

    good = (2, 4, 270, 480, 3, 112, 112, 5, 5, L.PTX_RESIZE_OUT_F32)
    assert lib.ptx_resize_frames_u8_supported(C.byref(L.ResizeDesc(*good))) == 1
    assert lib.ptx_resize_frames_u8_supported(C.byref(L.ResizeDesc(1, 16, 1080, 1920, 3, 224, 224, 11, 11, 0))) == 1
    assert call(None) == 1 and "null" in err()
    assert lib.ptx_resize_frames_u8_supported(None) == 0 and "null" in err()
    assert call(L.ResizeDesc(*good), frames=None) == 1 and "null pointer" in err()
    assert call(L.ResizeDesc(*good), y=None) == 1 and "null pointer" in err()
    for i in range(6):
        assert call(L.ResizeDesc(*good), tables=tuple(None if j == i else P for j in range(6))) == 1 and "null pointer" in err()
    assert call(L.ResizeDesc(*good), nd=None) == 1 and "norm" in err()
    for field in ("N", "T", "H", "W", "Ho", "Wo"):
        d = L.ResizeDesc(*good)
        setattr(d, field, 0)
        assert call(d) == 1 and "extent" in err(), field
        assert lib.ptx_resize_frames_u8_supported(C.byref(d)) == 0
    for ch in (0, 5):
        d = L.ResizeDesc(*good)
        d.C = ch
        assert call(d) == 1 and "C=" in err()
    for field in ("taps_h", "taps_w"):
        d = L.ResizeDesc(*good)
        setattr(d, field, L.PTX_RESIZE_MAX_TAPS + 1)
        assert call(d) == 2 and "PTX_RESIZE_MAX_TAPS" in err(), field           # PTX_ERR_UNSUPPORTED
        assert lib.ptx_resize_frames_u8_supported(C.byref(d)) == 0
        setattr(d, field, 0)
        assert call(d) == 1 and "taps" in err()
    d = L.ResizeDesc(*good)
    d.out_mode = 3
    assert call(d) == 1 and "out_mode" in err()
    zero = L.NormDesc.make([0.4, 0.4, 0.4], [0.2, 0.0, 0.2])
    assert call(L.ResizeDesc(*good), nd=zero) == 1 and "std[1]" in err()
    bgr = L.NormDesc.make([0.4], [0.2], "BGR")
    d = L.ResizeDesc(*good)
    d.C = 2
    assert call(d, nd=bgr) == 1 and "BGR" in err()
    d = L.ResizeDesc(1, 1, 4000, 4000, 3, 1200, 1200, 9, 9, 0)                   # rows too wide for the on-chip staging
    assert call(d) == 2 and "LDS" in err()
    assert lib.ptx_resize_frames_u8_supported(C.byref(d)) == 0


def test_transform_frames_errors(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    opts = dict(input_size=[3, 64, 64], input_space="RGB", input_range=[0, 1], mean=[0.4, 0.4, 0.4], std=[0.2, 0.2, 0.2])
    assert ptx.transforms.TransformFrames is TF.TransformFrames
    tf = TF.TransformFrames(opts)
    assert (tf.size, tf.out, tf.dtype, tf.hflip) == (64, "tensor", torch.float32, False)
    with pytest.raises(E, match="uint8 CUDA"):
        tf(torch.zeros(90, 120, 3, dtype=torch.uint8))                            # CPU tensor: no fallback
    with pytest.raises(E, match="uint8 CUDA"):
        tf(torch.zeros(90, 120, 3))                                               # float tensor
    with pytest.raises(E, match="uint8 CUDA"):
        tf(np.zeros((90, 120, 3), np.uint8))
    with pytest.raises(E, match="bfloat16|dtype"):
        TF.TransformFrames(opts, out="frames", dtype=torch.bfloat16)
    with pytest.raises(E, match="dtype"):
        TF.TransformFrames(opts, dtype=torch.float16)
    with pytest.raises(E, match="out"):
        TF.TransformFrames(opts, out="clip")
    with pytest.raises(E, match="crop"):
        TF.TransformFrames(opts, crop="random")
    with pytest.raises(E, match="does not fit"):
        TF.TransformFrames(opts, crop=(-1, 0))
    with pytest.raises(E, match="does not fit"):
        TF.TransformFrames(opts, crop=(10, 0)).tables(90, 120)                    # 73 rows: 10 + 64 > 73
    with pytest.raises(E, match="does not fit"):
        TF.TransformFrames(dict(opts, input_size=[3, 112, 96]), preserve_aspect_ratio=False).tables(300, 200)
    with pytest.raises(E, match="PTX_RESIZE_MAX_TAPS"):
        tf.tables(40 * 73, 40 * 73)
    with pytest.raises((AttributeError, KeyError)):
        TF.TransformFrames(dict(mean=[0.0], std=[1.0]))                           # no input_size / space / range
    with pytest.raises(E, match="3 interleaved channels"):
        tf(torch.zeros(90, 120, 4, dtype=torch.uint8))                            # RGBA
    with pytest.raises(E, match="expected"):
        tf(torch.zeros(120, 3, dtype=torch.uint8))
    with pytest.raises(E, match="expected"):
        tf(torch.zeros(1, 1, 1, 90, 120, 3, dtype=torch.uint8))
    model = ptx.__dict__["resnet3d18"](num_classes=10, pretrained=None).eval()
    frames = torch.zeros(1, 4, 90, 120, 3, dtype=torch.uint8)
    for bad in (tf, TF.FramesToTensor(opts), "center", lambda f: f):              # tf is out="tensor": not a frames transform
        with pytest.raises(E, match="transform must be"):
            model.forward_frames(frames, opts, transform=bad)
        with pytest.raises(E, match="transform must be"):
            model.engine().forward_frames(model, frames, opts, transform=bad)
    sf = ptx.slowfast.resnet18(mode="sf", num_classes=10).eval()
    with pytest.raises(E, match="transform must be"):
        sf.forward_frames(frames, opts, transform=tf)
    with pytest.raises(E, match="transform must be"):
        ptx.i3d(10).eval().forward_frames(frames, opts, transform=tf)
    ok = TF.TransformFrames(opts, out="frames")
    with pytest.raises(E, match="uint8 CUDA"):
        model.forward_frames(frames, opts, transform=ok)                          # the transform itself refuses CPU frames
