"""No-GPU tests of YUV 4:2:0 sources (`pretorched.transforms.YUV420`): the colour contract (integer coefficients, the numpy
statement of the conversion against float64 and against PIL), the stored cases (tests/golden/yuv_frames.npz, written by
tests/golden/make_yuv_golden.py with PIL only), the container's views and errors, and the C ABI's host-side checks."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

from pretorched_x_amd.testing import synth_yuv420

TABLE = {                                                 # (matrix, range) -> y_off, ky, krv, kgu, kgv, kbu
    ("bt601", "full"): (0, 65536, 91881, 22553, 46802, 116130),
    ("bt601", "limited"): (16, 76309, 104597, 25675, 53279, 132201),
    ("bt709", "full"): (0, 65536, 103206, 12276, 30679, 121609),
    ("bt709", "limited"): (16, 76309, 117489, 13975, 34925, 138438),
}
OPTS = dict(input_size=[3, 64, 64], input_space="RGB", input_range=[0, 1], mean=[0.4, 0.4, 0.4], std=[0.2, 0.2, 0.2])


def golden_cases():
    blob = load_golden("yuv_frames")
    return blob, json.loads(str(blob["cases"]))


def all_triples():
    """Every (Y, Cb, Cr) once: three uint8 arrays of 2^24 entries."""
    g = np.arange(1 << 24, dtype=np.int64)
    return (g >> 16).astype(np.uint8), ((g >> 8) & 255).astype(np.uint8), (g & 255).astype(np.uint8)


def convert_triples(TF, y, u, v, matrix, color_range):
    # [n] triples as n frames of 1 x 1 pixels: the chroma plane of a 1 x 1 frame is 1 x 1
    return TF.yuv420_to_rgb_numpy(y.reshape(-1, 1, 1), u.reshape(-1, 1, 1), v.reshape(-1, 1, 1), matrix, color_range).reshape(-1, 3)


def test_coefficient_table(ptx):
    TF = ptx.transforms
    for (matrix, rng), want in TABLE.items():
        assert TF.yuv_coefficients(matrix, rng) == want, (matrix, rng)
    assert TF.yuv_coefficients() == TABLE[("bt709", "limited")]
    for bad in (("bt2020", "full"), ("bt709", "tv"), (None, "full")):
        with pytest.raises(ptx._lib.PtxError):
            TF.yuv_coefficients(*bad)


@pytest.mark.parametrize("matrix,rng", sorted(TABLE))
def test_model_against_float64_on_all_triples(ptx, matrix, rng):
    """|integer model - clip(floor(exact + 0.5))| <= 1 on all 2^24 triples, and at most 0.1 % of them differ: the
    coefficients are rounded to 2^-16, which moves a sum by less than 0.006 of a level, so only near-ties move."""
    TF = ptx.transforms
    y, u, v = all_triples()
    got = convert_triples(TF, y, u, v, matrix, rng).astype(np.int16)
    kr, kb = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}[matrix]
    kg = 1.0 - kr - kb
    sy, sc, y_off = (255.0 / 219.0, 255.0 / 224.0, 16) if rng == "limited" else (1.0, 1.0, 0)
    yy = sy * (y.astype(np.float64) - y_off)
    cb, cr = sc * (u.astype(np.float64) - 128.0), sc * (v.astype(np.float64) - 128.0)
    exact = np.stack([yy + 2.0 * (1.0 - kr) * cr,
                      yy - 2.0 * kb * (1.0 - kb) / kg * cb - 2.0 * kr * (1.0 - kr) / kg * cr,
                      yy + 2.0 * (1.0 - kb) * cb], -1)
    want = np.clip(np.floor(exact + 0.5), 0, 255).astype(np.int16)
    diff = np.abs(got - want)
    share = float((diff.max(-1) > 0).mean())
    print("%s/%s: max diff %d, differing triples %.4f %%" % (matrix, rng, diff.max(), 100 * share))
    assert diff.max() <= 1
    assert share <= 0.001
    # every sum stays far inside 32 bits (the kernel multiplies with 24-bit operands)
    y_off, ky, krv, kgu, kgv, kbu = TF.yuv_coefficients(matrix, rng)
    assert max(ky, krv, kgu, kgv, kbu) < 1 << 23
    assert ky * 255 + max(krv, kbu, kgu + kgv) * 128 + 32768 < 1 << 26


def test_model_against_pil_bt601_full(ptx):
    """Sanity bound against PIL's own YCbCr -> RGB (JFIF: bt601, full range; 6-bit tables): at most 1 level apart."""
    Image = pytest.importorskip("PIL.Image")
    TF = ptx.transforms
    y, u, v = all_triples()
    got = convert_triples(TF, y, u, v, "bt601", "full").astype(np.int16)
    ycc = np.stack([y, u, v], -1).reshape(4096, 4096, 3)
    want = np.asarray(Image.fromarray(ycc, "YCbCr").convert("RGB")).reshape(-1, 3).astype(np.int16)
    diff = np.abs(got - want)
    print("PIL: max diff %d, differing triples %.2f %%" % (diff.max(), 100 * float((diff.max(-1) > 0).mean())))
    assert diff.max() <= 1


def test_numpy_model_equals_stored_cases(ptx):
    TF = ptx.transforms
    blob, cases = golden_cases()
    by = {c["name"]: c for c in cases}
    assert list(by) == ["nv12_up_50x70", "nv12_down_270x480", "i420_hflip_120x90", "planes_odd_73x99_crop_only",
                        "planes_odd_window_73x99", "nv12_pitched_90x120", "i420_stretch_200x300", "nv12_hd_1080x1920",
                        "nv12_clip_8x90x120", "nv12_extremes_36x50"]
    assert {(c["matrix"], c["color_range"]) for c in cases} == set(TABLE)
    for c in cases:
        y, u, v = synth_yuv420(c["count"], c["H"], c["W"], c["seed"], c["content"])
        rgb = TF.yuv420_to_rgb_numpy(y, u, v, c["matrix"], c["color_range"])
        crop = c["crop"] if isinstance(c["crop"], str) else tuple(c["crop"])
        tables = TF.build_tables(c["H"], c["W"], c["input_size"], c["scale"], c["preserve_aspect_ratio"], crop, c["hflip"])
        want = blob["out_" + c["name"]]
        assert want.shape == (c["count"], tables["S"], tables["S"], 3)
        for i in range(c["count"]):
            assert np.array_equal(TF.apply_tables_numpy(rgb[i], tables), want[i]), (c["name"], i)
        if c["content"] == "noise":
            assert min(c["clamped"]) > 0.05 * rgb.size, c["name"]              # both clamps are exercised
    c = by["planes_odd_73x99_crop_only"]
    assert c["resized"] == [73, 99] and by["planes_odd_window_73x99"]["window"] == [5, 17]
    y, u, v = synth_yuv420(3, 36, 50, 0, "extremes")
    assert [int(p[i, 0, 0]) for i in range(3) for p in (y, u, v)] == [255, 255, 255, 0, 0, 0, 16, 240, 16]
    # nearest chroma replication, odd sizes: pixel (r, c) takes sample (r >> 1, c >> 1)
    y, u, v = synth_yuv420(1, 5, 7, 3)
    rgb = TF.yuv420_to_rgb_numpy(y[0], u[0], v[0], "bt601", "full")
    for r, col in ((0, 0), (4, 6), (3, 5), (4, 1)):
        one = TF.yuv420_to_rgb_numpy(y[0, r:r + 1, col:col + 1], u[0, r >> 1:(r >> 1) + 1, col >> 1:(col >> 1) + 1],
                                     v[0, r >> 1:(r >> 1) + 1, col >> 1:(col >> 1) + 1], "bt601", "full")
        assert np.array_equal(rgb[r, col], one[0, 0])


def test_yuv420_views_and_shapes(ptx):
    TF = ptx.transforms
    H, W = 6, 8
    packed = torch.arange(2 * 3 * (H * 3 // 2) * W, dtype=torch.int64).remainder(251).to(torch.uint8).view(2, 3, H * 3 // 2, W)
    s = TF.YUV420.from_nv12(packed)
    assert (s.N, s.T, s.H, s.W, s.lead, s.device.type) == (2, 3, H, W, 3, "cpu")
    assert (s.matrix, s.color_range, s.coefficients) == ("bt709", "limited", TABLE[("bt709", "limited")])
    assert s.v is None and s.y.shape == (2, 3, H, W) and s.u.shape == (2, 3, H // 2, W // 2, 2)
    assert s.y.data_ptr() == packed.data_ptr() and s.u.data_ptr() == packed.data_ptr() + H * W
    assert s.u.stride()[-3:] == (W, 2, 1) and s.y.stride() == packed.stride()
    assert torch.equal(s.u[1, 2, 1, 3], packed[1, 2, H + 1, 6:8])
    # a pitched surface (rows of a wider buffer) stays a view
    wide = torch.zeros(3, H * 3 // 2, W + 10, dtype=torch.uint8)
    s = TF.YUV420.from_nv12(wide[..., 2:2 + W], color_range="full")
    assert (s.N, s.T, s.lead) == (1, 3, 2) and s.y.data_ptr() == wide.data_ptr() + 2 and s.y.stride(-2) == W + 10
    s = TF.YUV420.from_nv12(packed[0, 0], matrix="bt601")
    assert (s.N, s.T, s.lead, s.lead_shape) == (1, 1, 1, ())
    i = TF.YUV420.from_i420(packed)
    q = (H // 2) * (W // 2)
    assert i.y.data_ptr() == packed.data_ptr() and i.u.data_ptr() == packed.data_ptr() + H * W
    assert i.v.data_ptr() == packed.data_ptr() + H * W + q and i.u.shape == i.v.shape == (2, 3, H // 2, W // 2)
    flat = packed.reshape(2, 3, -1)
    assert torch.equal(i.u[1, 1].reshape(-1), flat[1, 1, H * W:H * W + q]) and torch.equal(i.v[0, 2].reshape(-1), flat[0, 2, H * W + q:])
    # planes, odd sizes
    y, u, v = (torch.from_numpy(a) for a in synth_yuv420(4, 5, 7, 1))
    p = TF.YUV420(y, u, v, "bt601", "full")
    assert (p.N, p.T, p.H, p.W, p.lead) == (1, 4, 5, 7, 2) and p.u.shape == (4, 3, 4)
    p = TF.YUV420(y.view(2, 2, 5, 7), torch.stack([u, v], -1).view(2, 2, 3, 4, 2))
    assert (p.N, p.T, p.lead) == (2, 2, 3) and p.v is None
    assert np.array_equal(p.to_rgb_numpy().reshape(4, 5, 7, 3), TF.yuv420_to_rgb_numpy(y.numpy(), u.numpy(), v.numpy()))
    # in-place rules of the descriptor (strides only; no device is touched)
    R = TF.YUV420._rows_in_place
    assert R(wide[..., 2:2 + W], (W,)) and R(packed[:, ::2], (W,)) and not R(packed[..., ::2], (W // 2,))
    assert R(s.u, (W // 2, 2)) and not R(s.u[..., ::2, :], (W // 4, 2)) and not R(packed.transpose(-1, -2), (H * 3 // 2,))


def test_yuv420_errors(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    y, u, v = (torch.from_numpy(a) for a in synth_yuv420(2, 6, 8, 1))
    with pytest.raises(E, match="uint8"):
        TF.YUV420(y.float(), u, v)
    with pytest.raises(E, match="uint8"):
        TF.YUV420(y.numpy(), u, v)
    with pytest.raises(E, match="different devices"):
        TF.YUV420(y, u.to("meta"), v)
    for bad_u, bad_v in ((u[:, :2], v), (u, v[..., :3]), (u[0], v[0]), (torch.stack([u, v], -1), v)):
        with pytest.raises(E, match="ceil"):
            TF.YUV420(y, bad_u, bad_v)
    with pytest.raises(E, match="ceil"):
        TF.YUV420(y, u)                                                        # a uv plane needs a trailing pair
    assert TF.YUV420(y[..., :7], u, v).W == 7                                  # 7 columns: ceil(7 / 2) = 4 chroma columns
    with pytest.raises(E, match="ceil"):
        TF.YUV420(y[..., :6], u, v)                                            # 6 columns need 3
    with pytest.raises(E, match="luma plane"):
        TF.YUV420(y[0, 0], u[0, 0], v[0, 0])
    with pytest.raises(E, match="matrix"):
        TF.YUV420(y, u, v, matrix="bt2020")
    with pytest.raises(E, match="color_range"):
        TF.YUV420(y, u, v, color_range="pc")
    for shape in ((10, 8), (8, 8), (9, 7), (2, 3, 12, 7)):                      # rows that are not H*3/2 of an even H, odd W
        with pytest.raises(E, match="even H and W"):
            TF.YUV420.from_nv12(torch.zeros(shape, dtype=torch.uint8))
        with pytest.raises(E, match="even H and W"):
            TF.YUV420.from_i420(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(E, match="uint8"):
        TF.YUV420.from_nv12(torch.zeros(9, 8))
    src = TF.YUV420(y, u, v)                                                   # CPU planes: refused at the call, no fallback
    tf = TF.TransformFrames(OPTS, out="frames")
    with pytest.raises(E, match="CUDA"):
        tf(src)
    with pytest.raises(E, match="CUDA"):
        TF.SampleViews(OPTS, num_frames=2, clips=1, crops=1)(src)
    with pytest.raises(E, match="one frame"):
        TF.SampleViews(OPTS, num_frames=2, clips=1, crops=1)(TF.YUV420(y[0], u[0], v[0]))
    empty = TF.YUV420(y[:0].to("meta"), u[:0].to("meta"), v[:0].to("meta"))
    with pytest.raises(E):
        empty.source()
    model = ptx.__dict__["resnet3d18"](num_classes=10, pretrained=None).eval()
    for call in (lambda: model.forward_frames(src, OPTS), lambda: model.engine().forward_frames(model, src, OPTS),
                 lambda: ptx.i3d(10).eval().forward_frames(src, OPTS),
                 lambda: ptx.slowfast.resnet18(mode="sf", num_classes=10).eval().forward_frames(src, OPTS)):
        with pytest.raises(E, match="needs transform"):
            call()
    with pytest.raises(E, match="transform must be"):
        model.forward_frames(src, OPTS, transform=TF.TransformFrames(OPTS))    # out="tensor" is not a frames transform
    with pytest.raises(E, match="CUDA"):
        model.forward_frames(src, OPTS, transform=tf)
    vs = TF.SampleViews(OPTS, num_frames=2, clips=1, crops=1)
    with pytest.raises(E, match="CUDA"):
        model.forward_views(src, OPTS, views=vs)
    with pytest.raises(E, match="YUV420 video"):
        model.forward_views(TF.YUV420(y[0], u[0], v[0]), OPTS, views=vs)


def test_yuv_abi(ptx):
    L = ptx._lib
    lib = L.lib()
    text = open(L.HEADER_PATH).read()
    names = ("ptx_resize_frames_yuv420", "ptx_resize_frames_yuv420_supported", "ptx_resize_views_yuv420",
             "ptx_resize_views_yuv420_supported")
    for name in names:
        assert name in L.header_symbols() and name in L.SIGNATURES and name not in L.EXPERIMENTAL
        assert name not in L.experimental_symbols() and hasattr(lib, name)
    # the ctypes mirror, field for field
    body = re.sub(r"/\*.*?\*/", "", text.split("typedef struct ptx_yuv420_src {")[1].split("}")[0], flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = "p" if "*" in decl else ("q" if "int64_t" in decl else "i")
        rest = re.sub(r"const|uint8_t|int64_t|int32_t|\*", " ", decl)
        fields += [(n.strip(), kind) for n in rest.split(",") if n.strip()]
    ctype = {"p": C.c_void_p, "q": C.c_int64, "i": C.c_int32}
    assert [(n, ctype[k]) for n, k in fields] == list(L.Yuv420Src._fields_)
    assert C.sizeof(L.Yuv420Src) == 3 * 8 + 4 * 8 + 9 * 4 + 4                  # 92 bytes of fields, padded to 8
    assert "92 stable" in open(L.HEADER_PATH.replace("include/ptx_amd.h", "INTEGRATION.md")).read()

    P = 64                                                 # never dereferenced: every call below returns before a launch
    good = (2, 4, 270, 480, 3, 112, 112, 5, 5, L.PTX_RESIZE_OUT_U8)

    def src(**kw):
        s = L.Yuv420Src()
        s.y, s.u, s.v = P, 2 * P, 2 * P + 1
        s.stride_n_y, s.stride_t_y, s.stride_n_c, s.stride_t_c = 4 * 270 * 480, 270 * 480, 4 * 135 * 480, 135 * 480
        s.pitch_y, s.pitch_c, s.step_c = 480, 480, 2
        s.y_off, s.ky, s.krv, s.kgu, s.kgv, s.kbu = TABLE[("bt709", "limited")]
        for k, val in kw.items():
            setattr(s, k, val)
        return s

    def frames_ok(d, s):
        return lib.ptx_resize_frames_yuv420_supported(C.byref(d) if d is not None else None, C.byref(s) if s is not None else None)

    def err(who="yuv420"):
        msg = lib.ptx_last_error().decode()
        assert who in msg
        return msg

    assert frames_ok(L.ResizeDesc(*good), src()) == 1
    assert frames_ok(L.ResizeDesc(1, 1, 73, 99, 3, 64, 64, 1, 1, 0), src(pitch_y=99, pitch_c=50, step_c=1, v=3 * P)) == 1   # odd sizes
    assert frames_ok(L.ResizeDesc(*good), src(u=2 * P + 1, v=2 * P)) == 1                     # V first
    assert frames_ok(None, src()) == 0 and "null" in err()
    assert frames_ok(L.ResizeDesc(*good), None) == 0 and "null" in err()
    for plane in ("y", "u", "v"):
        assert frames_ok(L.ResizeDesc(*good), src(**{plane: None})) == 0 and "null plane" in err()
    for k in ("pitch_y", "pitch_c"):
        assert frames_ok(L.ResizeDesc(*good), src(**{k: 0})) == 0 and "positive" in err()
        assert frames_ok(L.ResizeDesc(*good), src(**{k: -480})) == 0 and "positive" in err()
    assert frames_ok(L.ResizeDesc(*good), src(pitch_y=479)) == 0 and "shorter than a row" in err()
    assert frames_ok(L.ResizeDesc(*good), src(pitch_c=479)) == 0 and "shorter than a row" in err()
    assert frames_ok(L.ResizeDesc(*good), src(pitch_c=240, step_c=1, v=3 * P)) == 1
    assert frames_ok(L.ResizeDesc(*good), src(pitch_c=239, step_c=1, v=3 * P)) == 0 and "shorter than a row" in err()
    for step in (0, 3, -1):
        assert frames_ok(L.ResizeDesc(*good), src(step_c=step)) == 0 and "step_c" in err()
    assert frames_ok(L.ResizeDesc(*good), src(v=3 * P)) == 0 and "interleaved" in err()
    assert frames_ok(L.ResizeDesc(*good), src(pitch_y=1 << 24)) == 0 and "32-bit" in err()      # 270 rows of 16 MiB
    assert frames_ok(L.ResizeDesc(*good), src(pitch_c=1 << 25)) == 0 and "32-bit" in err()
    for ch in (1, 2, 4):
        d = L.ResizeDesc(*good)
        d.C = ch
        assert frames_ok(d, src()) == 0 and "3 channels" in err()
    d = L.ResizeDesc(*good)
    d.taps_h = L.PTX_RESIZE_MAX_TAPS + 1
    assert frames_ok(d, src()) == 0 and "PTX_RESIZE_MAX_TAPS" in err()                          # what the RGB path refuses
    assert frames_ok(L.ResizeDesc(1, 1, 4000, 4000, 3, 1200, 1200, 9, 9, 0), src(pitch_y=4000, pitch_c=4000)) == 0 and "LDS" in err()
    # the launching calls run the same checks first and return a status
    tables = (C.c_void_p(P),) * 6
    call = lambda d, s, y=C.c_void_p(P): lib.ptx_resize_frames_yuv420(C.byref(d), C.byref(s) if s is not None else None,
                                                                       *tables, y, None, None)
    assert call(L.ResizeDesc(*good), None) == 1 and "null" in err()
    assert call(L.ResizeDesc(*good), src(pitch_y=10)) == 1 and "shorter" in err()
    assert call(L.ResizeDesc(*good), src(), None) == 1 and "null pointer" in err()
    d = L.ResizeDesc(*good)
    d.out_mode = L.PTX_RESIZE_OUT_F32
    assert call(d, src()) == 1 and "norm" in err()

    # views: 0 / 1 / 2 as the RGB entry point, the descriptor's own strides ignored
    vs = ptx.transforms.SampleViews(OPTS, num_frames=4, clips=3, crops=3)
    for (H, W) in ((90, 160), (160, 90), (90, 400)):
        t = vs.tables(H, W)
        s = src(pitch_y=W, pitch_c=2 * ((W + 1) // 2))
        for share, want in (("always", 2), ("never", 1)):
            vs.share = share
            rgb = vs._desc(2, 12, H, W, 3, H * W * 3, H * W * 3, t, 0, 9)
            yuv = vs._desc(2, 12, H, W, 3, 0, 0, t, 0, 9)                                       # strides of 0: not read
            assert lib.ptx_resize_views_u8_supported(C.byref(rgb)) == want
            assert lib.ptx_resize_views_yuv420_supported(C.byref(yuv), C.byref(s)) == want
        vs.share = "auto"
        yuv = vs._desc(2, 12, H, W, 3, 0, 0, t, 0, 9)
        rgb = vs._desc(2, 12, H, W, 3, H * W * 3, H * W * 3, t, 0, 9)
        assert lib.ptx_resize_views_yuv420_supported(C.byref(yuv), C.byref(s)) == lib.ptx_resize_views_u8_supported(C.byref(rgb))
        assert lib.ptx_resize_views_yuv420_supported(C.byref(yuv), C.byref(src(pitch_y=W - 1))) == 0 and "shorter" in err()
        assert lib.ptx_resize_views_yuv420_supported(C.byref(yuv), None) == 0 and "null" in err()
        yuv.C = 4
        assert lib.ptx_resize_views_yuv420_supported(C.byref(yuv), C.byref(s)) == 0 and "3 channels" in err()
    yuv = vs._desc(2, 12, 90, 160, 3, 0, 0, vs.tables(90, 160), 0, 9)
    assert lib.ptx_resize_views_yuv420(C.byref(yuv), None, *((C.c_void_p(P),) * 7), C.c_void_p(P), None, None) == 1 and "null" in err()
    assert lib.ptx_resize_views_yuv420(C.byref(yuv), C.byref(src(pitch_y=160, pitch_c=160, step_c=5)), *((C.c_void_p(P),) * 7),
                                       C.c_void_p(P), None, None) == 1 and "step_c" in err()
