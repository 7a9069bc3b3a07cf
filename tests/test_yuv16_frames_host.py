"""No-GPU tests of 10- / 12-bit YUV 4:2:0 sources (`pretorched.transforms.YUV420P16`: P010 / P012 / P016 surfaces and
yuv420p10le / yuv420p12le planes): the colour contract (the coefficient table, the numpy statement of the conversion against
float64, against the 8-bit model on shifted samples and across the two containers), the stored cases
(tests/golden/yuv16_frames.npz, written by tests/golden/make_yuv16_golden.py with PIL only), the container's views and
errors, and the C ABI of include/ptx_amd_yuv16.h with its host-side checks."""
import ctypes as C
import functools
import json
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

from pretorched_x_amd.testing import synth_yuv420, synth_yuv420p16

# (matrix, range, bits) -> y_off, ky, krv, kgu, kgv, kbu; limited range: the 8-bit coefficients, y_off = 16 << (bits - 8)
LIMITED = {"bt601": (76309, 104597, 25675, 53279, 132201), "bt709": (76309, 117489, 13975, 34925, 138438),
           "bt2020": (76309, 110014, 12277, 42626, 140363)}
FULL = {("bt601", 10): (65344, 91612, 22487, 46664, 115789), ("bt601", 12): (65296, 91545, 22471, 46630, 115704),
        ("bt709", 10): (65344, 102903, 12240, 30589, 121252), ("bt709", 12): (65296, 102828, 12232, 30567, 121163),
        ("bt2020", 10): (65344, 96356, 10753, 37334, 122938), ("bt2020", 12): (65296, 96285, 10745, 37307, 122848)}
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
OPTS = dict(input_size=[3, 64, 64], input_space="RGB", input_range=[0, 1], mean=[0.4, 0.4, 0.4], std=[0.2, 0.2, 0.2])
NAMES = ("ptx_resize_frames_yuv420p16", "ptx_resize_frames_yuv420p16_supported", "ptx_resize_frames_yuv420p16_windows",
         "ptx_resize_frames_yuv420p16_windows_supported", "ptx_resize_frames_yuv420p16_tables",
         "ptx_resize_frames_yuv420p16_tables_supported", "ptx_resize_clips_yuv420p16", "ptx_resize_clips_yuv420p16_supported",
         "ptx_resize_views_yuv420p16", "ptx_resize_views_yuv420p16_supported")


def table(matrix, rng, bits):
    return ((16 << (bits - 8),) + LIMITED[matrix]) if rng == "limited" else ((0,) + FULL[(matrix, bits)])


@functools.lru_cache(None)
def sample_triples(bits):
    """The seeded sample of the contract: 2^22 random (Y, Cb, Cr) from RandomState(0) plus the 11^3 lattice of the range end
    points (both ends of the full and of the limited ranges and their neighbours, and mid-scale).  Three int64 arrays."""
    d, top = bits - 8, (1 << bits) - 1
    rs = np.random.RandomState(0)
    rnd = rs.randint(0, top + 1, (3, 1 << 22)).astype(np.int64)
    ends = np.array([0, 1, (16 << d) - 1, 16 << d, (16 << d) + 1, 128 << d, 235 << d, 240 << d, (240 << d) + 1, top - 1, top], np.int64)
    assert len(set(ends.tolist())) == 11
    lattice = np.stack(np.meshgrid(ends, ends, ends, indexing="ij")).reshape(3, -1)
    return tuple(np.concatenate([rnd[k], lattice[k]]) for k in range(3))


def convert_triples(TF, y, u, v, bits, align, matrix, rng):
    # [n] triples as n frames of 1 x 1 pixels: the chroma plane of a 1 x 1 frame is 1 x 1
    w = [(a << (16 - bits) if align == "msb" else a).astype(np.uint16).reshape(-1, 1, 1) for a in (y, u, v)]
    return TF.yuv420p16_to_rgb_numpy(*w, bits, align, matrix, rng).reshape(-1, 3)


def test_coefficient_table(ptx):
    TF = ptx.transforms
    for matrix in MATRICES:
        for rng in ("limited", "full"):
            for bits in (10, 12):
                assert TF.yuv_coefficients_p16(matrix, rng, bits) == table(matrix, rng, bits), (matrix, rng, bits)
        # limited range: the 8-bit coefficients (bt2020 is new: the 8-bit function keeps refusing it)
        if matrix != "bt2020":
            assert TF.yuv_coefficients(matrix, "limited")[1:] == LIMITED[matrix]
    assert TF.yuv_coefficients_p16() == table("bt709", "limited", 10)
    for bad in (("bt2100", "full", 10), ("bt709", "tv", 10), (None, "full", 10), ("bt709", "full", 8), ("bt709", "full", 16),
                ("bt709", "limited", "10")):
        with pytest.raises(ptx._lib.PtxError):
            TF.yuv_coefficients_p16(*bad)
    with pytest.raises(ptx._lib.PtxError, match="matrix"):
        TF.yuv_coefficients("bt2020", "limited")


@pytest.mark.parametrize("matrix,rng", [(m, r) for m in sorted(MATRICES) for r in ("full", "limited")])
def test_model_against_float64_on_the_seeded_sample(ptx, matrix, rng):
    """|integer model - clip(floor(exact + 0.5))| <= 1 on the seeded sample and at most 0.2 % of the triples differ (the cap;
    0.054-0.107 % measured): the coefficients are rounded to 2^-16, so only near-ties move.  Every sum stays below 2^31 and
    every coefficient below 2^23 (the kernel multiplies with 24-bit operands)."""
    TF = ptx.transforms
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    for bits in (10, 12):
        d, top = bits - 8, (1 << bits) - 1
        y, u, v = sample_triples(bits)
        got = convert_triples(TF, y, u, v, bits, "lsb", matrix, rng).astype(np.int16)
        if rng == "limited":
            sy, sc, y_off = 255.0 / 219.0 / (1 << d), 255.0 / 224.0 / (1 << d), 16 << d
        else:
            sy = sc = 255.0 / top
            y_off = 0
        yy = sy * (y.astype(np.float64) - y_off)
        cb, cr = sc * (u.astype(np.float64) - (128 << d)), sc * (v.astype(np.float64) - (128 << d))
        exact = np.stack([yy + 2.0 * (1.0 - kr) * cr,
                          yy - 2.0 * kb * (1.0 - kb) / kg * cb - 2.0 * kr * (1.0 - kr) / kg * cr,
                          yy + 2.0 * (1.0 - kb) * cb], -1)
        want = np.clip(np.floor(exact + 0.5), 0, 255).astype(np.int16)
        diff = np.abs(got - want)
        share = float((diff.max(-1) > 0).mean())
        print("%s/%s/%d: max diff %d, differing triples %.4f %%" % (matrix, rng, bits, diff.max(), 100 * share))
        assert diff.max() <= 1
        assert share <= 0.002
        y_off, ky, krv, kgu, kgv, kbu = TF.yuv_coefficients_p16(matrix, rng, bits)
        assert max(ky, krv, kgu, kgv, kbu) < 1 << 23
        half = 1 << (15 + d)
        sums = [ky * (y - y_off) + krv * (v - (128 << d)) + half, ky * (y - y_off) - kgu * (u - (128 << d)) - kgv * (v - (128 << d)) + half,
                ky * (y - y_off) + kbu * (u - (128 << d)) + half]
        assert max(int(np.abs(s).max()) for s in sums) < 1 << 31
        assert ky * top + max(krv, kbu, kgu + kgv) * (128 << d) + half < 1 << 31      # the bound over every triple


def test_shifted_8bit_samples_reproduce_the_8bit_model(ptx):
    """Limited range has the 8-bit coefficients, so samples v8 << d convert exactly as `yuv420_to_rgb_numpy` converts v8."""
    TF = ptx.transforms
    y, u, v = synth_yuv420(3, 37, 53, 11)
    for matrix in ("bt601", "bt709"):
        want = TF.yuv420_to_rgb_numpy(y, u, v, matrix, "limited")
        for bits in (10, 12):
            for align in ("msb", "lsb"):
                up = (bits - 8) + (16 - bits if align == "msb" else 0)
                planes = [(a.astype(np.uint16) << up) for a in (y, u, v)]
                assert np.array_equal(TF.yuv420p16_to_rgb_numpy(*planes, bits, align, matrix, "limited"), want), (matrix, bits, align)


def test_msb_and_lsb_containers_ignore_the_other_bits(ptx):
    TF = ptx.transforms
    for bits in (10, 12):
        msb = synth_yuv420p16(2, 9, 13, 21, bits, "msb")
        low = (1 << (16 - bits)) - 1
        assert all(int((p & low).max()) > 0 for p in msb)                      # the helper fills the ignored bits
        clean = [p >> (16 - bits) for p in msb]                                # the samples, LSB-aligned, high bits zero
        dirty = [c | (np.random.RandomState(5).randint(0, 1 << (16 - bits), c.shape).astype(np.uint16) << bits) for c in clean]
        for matrix, rng in (("bt2020", "limited"), ("bt709", "full")):
            want = TF.yuv420p16_to_rgb_numpy(*clean, bits, "lsb", matrix, rng)
            assert np.array_equal(TF.yuv420p16_to_rgb_numpy(*msb, bits, "msb", matrix, rng), want)
            assert np.array_equal(TF.yuv420p16_to_rgb_numpy(*dirty, bits, "lsb", matrix, rng), want)
            assert np.array_equal(TF.yuv420p16_to_rgb_numpy(*[(c << (16 - bits)).astype(np.uint16) for c in clean], bits, "msb", matrix, rng), want)
            # int16 arrays are the same bits, read unsigned
            assert np.array_equal(TF.yuv420p16_to_rgb_numpy(*[p.view(np.int16) for p in msb], bits, "msb", matrix, rng), want)
        lsb = synth_yuv420p16(2, 9, 13, 21, bits, "lsb")
        assert all(int((p >> bits).max()) > 0 for p in lsb)
    with pytest.raises(ptx._lib.PtxError, match="uint16"):
        TF.yuv420p16_to_rgb_numpy(*[p.astype(np.uint8) for p in msb], 10, "msb")
    with pytest.raises(ptx._lib.PtxError, match="align"):
        TF.yuv420p16_to_rgb_numpy(*msb, 10, "high")
    with pytest.raises(ptx._lib.PtxError, match="do not match"):
        TF.yuv420p16_to_rgb_numpy(msb[0], msb[1][:, :2], msb[2], 10, "msb")


def golden_cases():
    blob = load_golden("yuv16_frames")
    return blob, json.loads(str(blob["cases"]))


def test_numpy_model_equals_stored_cases_and_pil(ptx):
    TF = ptx.transforms
    blob, cases = golden_cases()
    by = {c["name"]: c for c in cases}
    assert list(by) == ["p010_up_50x70", "p010_down_270x480", "i420p12_hflip_120x90", "planes_odd_73x99_crop_only",
                        "planes_uv_odd_window_73x99", "p010_pitched_90x120", "p016_pitched_2x90x120", "p010_extremes_36x50",
                        "i420p12_extremes_36x50", "planes_stretch_80x81", "planes_uv_stretch_80x95", "p010_wide_6x2300",
                        "p010_clip_8x40x56"]
    assert {c["matrix"] for c in cases} == set(MATRICES) and {(c["bits"], c["align"]) for c in cases} == {(10, "msb"), (10, "lsb"), (12, "msb"), (12, "lsb")}
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for c in cases:
        y, u, v = synth_yuv420p16(c["count"], c["H"], c["W"], c["seed"], c["bits"], c["align"], c["content"])
        rgb = TF.yuv420p16_to_rgb_numpy(y, u, v, c["bits"], c["align"], c["matrix"], c["color_range"])
        crop = c["crop"] if isinstance(c["crop"], str) else tuple(c["crop"])
        tables = TF.build_tables(c["H"], c["W"], c["input_size"], c["scale"], c["preserve_aspect_ratio"], crop, c["hflip"])
        want = blob["out_" + c["name"]]
        assert want.shape == (c["count"], tables["S"], tables["S"], 3)
        lo, n = tables["cols"][0], tables["cols"][1]
        assert [int(lo.min()), int((lo + n).max())] == c["span"]
        for i in range(c["count"]):
            assert np.array_equal(TF.apply_tables_numpy(rgb[i], tables), want[i]), (c["name"], i)
        if c["content"] == "noise":
            assert min(c["clamped"]) > 0.02 * rgb.size, c["name"]              # both clamps are exercised
        if Image is not None:                                                  # PIL on the converted frame, restated here
            img = Image.fromarray(rgb[0])
            h, w = c["resized"]
            if (h, w) != (c["H"], c["W"]):
                img = img.resize((w, h), Image.BILINEAR)
            top, left = c["window"]
            out = np.asarray(img.crop((left, top, left + tables["S"], top + tables["S"])))
            assert np.array_equal(out[:, ::-1] if c["hflip"] else out, want[0]), c["name"]
    # the spans the GPU cases rely on: an odd first column, last groups of 1 and 15 pixels, a row beyond 2048 pixels
    assert by["planes_uv_odd_window_73x99"]["span"] == [17, 81] and by["planes_odd_73x99_crop_only"]["resized"] == [73, 99]
    assert by["planes_stretch_80x81"]["span"] == [0, 81] and by["planes_uv_stretch_80x95"]["span"] == [0, 95]
    assert by["p010_wide_6x2300"]["span"] == [0, 2300]
    for bits in (10, 12):
        d, top = bits - 8, (1 << bits) - 1
        y, u, v = (p >> (16 - bits) for p in synth_yuv420p16(3, 36, 50, 0, bits, "msb", "extremes"))
        assert [int(p[i, 0, 0]) for i in range(3) for p in (y, u, v)] == [top, top, top, 0, 0, 0, 16 << d, 240 << d, 16 << d]
    # nearest chroma replication, odd sizes: pixel (r, c) takes sample (r >> 1, c >> 1)
    y, u, v = synth_yuv420p16(1, 5, 7, 3, 12, "lsb")
    rgb = TF.yuv420p16_to_rgb_numpy(y[0], u[0], v[0], 12, "lsb", "bt2020", "full")
    for r, col in ((0, 0), (4, 6), (3, 5), (4, 1)):
        one = TF.yuv420p16_to_rgb_numpy(y[0, r:r + 1, col:col + 1], u[0, r >> 1:(r >> 1) + 1, col >> 1:(col >> 1) + 1],
                                        v[0, r >> 1:(r >> 1) + 1, col >> 1:(col >> 1) + 1], 12, "lsb", "bt2020", "full")
        assert np.array_equal(rgb[r, col], one[0, 0])


def test_yuv420p16_views_and_shapes(ptx):
    TF = ptx.transforms
    H, W = 6, 8
    packed = torch.arange(2 * 3 * (H * 3 // 2) * W, dtype=torch.int64).mul(97).remainder(65521).to(torch.int32).to(torch.int16).view(2, 3, H * 3 // 2, W)
    s = TF.YUV420P16.from_p010(packed)
    assert (s.N, s.T, s.H, s.W, s.lead, s.device.type) == (2, 3, H, W, 3, "cpu")
    assert (s.bits, s.align, s.shift, s.matrix, s.color_range) == (10, "msb", 6, "bt709", "limited")
    assert s.coefficients == table("bt709", "limited", 10)
    assert s.v is None and s.y.shape == (2, 3, H, W) and s.u.shape == (2, 3, H // 2, W // 2, 2)
    assert s.y.data_ptr() == packed.data_ptr() and s.u.data_ptr() == packed.data_ptr() + 2 * H * W      # views, bytes
    assert s.u.stride()[-3:] == (W, 2, 1) and s.y.stride() == packed.stride()
    assert torch.equal(s.u[1, 2, 1, 3], packed[1, 2, H + 1, 6:8])
    p12 = TF.YUV420P16.from_p010(packed, 12, "bt2020", "full")
    assert (p12.bits, p12.shift, p12.coefficients) == (12, 4, table("bt2020", "full", 12))
    # uint16 tensors are the same bits: the same views, the same conversion
    u16 = TF.YUV420P16.from_p010(packed.view(torch.uint16))
    assert u16.y.data_ptr() == packed.data_ptr() and np.array_equal(u16.to_rgb_numpy(), s.to_rgb_numpy())
    # a pitched surface (rows of a wider buffer) stays a view
    wide = torch.zeros(3, H * 3 // 2, W + 10, dtype=torch.int16)
    w = TF.YUV420P16.from_p010(wide[..., 2:2 + W], color_range="full")
    assert (w.N, w.T, w.lead) == (1, 3, 2) and w.y.data_ptr() == wide.data_ptr() + 4 and w.y.stride(-2) == W + 10
    one = TF.YUV420P16.from_p010(packed[0, 0], matrix="bt601")
    assert (one.N, one.T, one.lead, one.lead_shape) == (1, 1, 1, ())
    i = TF.YUV420P16.from_i420p16(packed, 12)
    q = (H // 2) * (W // 2)
    assert (i.bits, i.align, i.shift) == (12, "lsb", 0)
    assert i.y.data_ptr() == packed.data_ptr() and i.u.data_ptr() == packed.data_ptr() + 2 * H * W
    assert i.v.data_ptr() == packed.data_ptr() + 2 * (H * W + q) and i.u.shape == i.v.shape == (2, 3, H // 2, W // 2)
    # planes, odd sizes, and the numpy model through the class
    y, u, v = (torch.from_numpy(a.view(np.int16)) for a in synth_yuv420p16(4, 5, 7, 1, 10, "lsb"))
    p = TF.YUV420P16(y, u, v, 10, "lsb", "bt601", "full")
    assert (p.N, p.T, p.H, p.W, p.lead) == (1, 4, 5, 7, 2) and p.u.shape == (4, 3, 4)
    p = TF.YUV420P16(y.view(2, 2, 5, 7), torch.stack([u, v], -1).view(2, 2, 3, 4, 2), bits=10, align="lsb")
    assert (p.N, p.T, p.lead) == (2, 2, 3) and p.v is None
    assert np.array_equal(p.to_rgb_numpy().reshape(4, 5, 7, 3), TF.yuv420p16_to_rgb_numpy(y.numpy(), u.numpy(), v.numpy(), 10, "lsb"))
    assert isinstance(p, TF.YUV420) and TF.YUV420P16._ABI == "yuv420p16" and TF.YUV420._ABI == "yuv420"


def test_yuv420p16_errors(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    y, u, v = (torch.from_numpy(a.view(np.int16)) for a in synth_yuv420p16(2, 6, 8, 1))
    with pytest.raises(E, match="YUV420 source"):
        TF.YUV420P16(y.to(torch.uint8), u.to(torch.uint8), v.to(torch.uint8))  # 8-bit planes: the message names YUV420
    with pytest.raises(E, match="int16 / uint16"):
        TF.YUV420P16(y.float(), u, v)
    with pytest.raises(E, match="int16 / uint16"):
        TF.YUV420P16(y.numpy(), u, v)
    with pytest.raises(E, match="uint8"):
        TF.YUV420(y, u, v)                                                     # and YUV420 keeps refusing words
    with pytest.raises(E, match="different devices"):
        TF.YUV420P16(y, u.to("meta"), v)
    for bad_u, bad_v in ((u[:, :2], v), (u, v[..., :3]), (u[0], v[0]), (torch.stack([u, v], -1), v)):
        with pytest.raises(E, match="YUV420P16: the . plane .*ceil"):
            TF.YUV420P16(y, bad_u, bad_v)
    with pytest.raises(E, match="ceil"):
        TF.YUV420P16(y, u)                                                     # a uv plane needs a trailing pair
    with pytest.raises(E, match="YUV420P16: expected a luma plane"):
        TF.YUV420P16(y[0, 0], u[0, 0], v[0, 0])
    with pytest.raises(E, match="matrix"):
        TF.YUV420P16(y, u, v, matrix="bt2100")
    with pytest.raises(E, match="color_range"):
        TF.YUV420P16(y, u, v, color_range="pc")
    for bits in (8, 14, 16, None):
        with pytest.raises(E, match="bits must be 10 or 12"):
            TF.YUV420P16(y, u, v, bits=bits)
    with pytest.raises(E, match="align"):
        TF.YUV420P16(y, u, v, align="left")
    for shape in ((10, 8), (8, 8), (9, 7), (2, 3, 12, 7)):                      # rows that are not H*3/2 of an even H, odd W
        with pytest.raises(E, match="YUV420P16.from_p010: .*even H and W"):
            TF.YUV420P16.from_p010(torch.zeros(shape, dtype=torch.int16))
        with pytest.raises(E, match="even H and W"):
            TF.YUV420P16.from_i420p16(torch.zeros(shape, dtype=torch.int16), 10)
    with pytest.raises(E, match="int16 / uint16"):
        TF.YUV420P16.from_p010(torch.zeros(9, 8, dtype=torch.uint8))
    src = TF.YUV420P16(y, u, v)                                                # CPU planes: refused at the call, no fallback
    tf = TF.TransformFrames(OPTS, out="frames")
    with pytest.raises(E, match="YUV420P16 source must be int16 / uint16 CUDA"):
        tf(src)
    with pytest.raises(E, match="CUDA"):
        TF.SampleViews(OPTS, num_frames=2, clips=1, crops=1)(src)
    with pytest.raises(E, match="YUV420P16 video .* one frame"):
        TF.SampleViews(OPTS, num_frames=2, clips=1, crops=1)(TF.YUV420P16(y[0], u[0], v[0]))
    # SampleClips: a list is all of one source kind; depth, alignment, matrix and range may differ inside it
    y8, u8, v8 = (torch.from_numpy(a) for a in synth_yuv420(2, 6, 8, 1))
    sc = TF.SampleClips(dict(OPTS, input_size=[3, 4, 4]), num_frames=2, out="frames")
    with pytest.raises(E, match="one source kind"):
        sc([src, TF.YUV420(y8, u8, v8)])
    with pytest.raises(E, match="one source kind"):
        sc([TF.YUV420(y8, u8, v8), src])
    with pytest.raises(E, match="all tensors or all YUV420"):
        sc([src, torch.zeros(2, 6, 8, 3, dtype=torch.uint8)])
    mixed = [src, TF.YUV420P16(y, u, v, 12, "lsb", "bt2020", "full")]
    assert [type(s) for s in TF.SampleClips._videos(mixed)] == [TF.YUV420P16] * 2
    split = TF.SampleClips._videos(TF.YUV420P16(y.view(2, 1, 6, 8), u.view(2, 1, 3, 4), v.view(2, 1, 3, 4), 12, "lsb", "bt2020"))
    assert [(s.bits, s.align, s.matrix, s.lead) for s in split] == [(12, "lsb", "bt2020", 2)] * 2
    with pytest.raises(E, match="CUDA"):
        sc(mixed)
    model = ptx.__dict__["resnet3d18"](num_classes=10, pretrained=None).eval()
    for call in (lambda: model.forward_frames(src, OPTS), lambda: model.engine().forward_frames(model, src, OPTS)):
        with pytest.raises(E, match="a YUV420P16 source needs transform"):
            call()
    with pytest.raises(E, match="CUDA"):
        model.forward_frames(src, OPTS, transform=tf)
    with pytest.raises(E, match="CUDA"):
        model.forward_views(src, OPTS, views=TF.SampleViews(OPTS, num_frames=2, clips=1, crops=1))


def struct_fields(text, name):
    """[(field, kind)] of `typedef struct name { ... }` in a header: p pointer, q int64, i int32, or a nested struct's name."""
    body = re.sub(r"/\*.*?\*/", "", text.split("typedef struct %s {" % name)[1].split("}")[0], flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        nested = re.match(r"(ptx_\w+)\s+(\w+)$", decl)
        if nested:
            fields.append((nested.group(2), nested.group(1)))
            continue
        kind = "p" if "*" in decl else ("q" if "int64_t" in decl else "i")
        rest = re.sub(r"const|uint16_t|uint8_t|int64_t|int32_t|\*", " ", decl)
        fields += [(n.strip(), kind) for n in rest.split(",") if n.strip()]
    return fields


def test_yuv16_header_bindings_and_exports_agree(ptx):
    """The ten calls live in include/ptx_amd_yuv16.h: that header, _lib.SIGNATURES_YUV16 and the library's exports name the
    same functions, disjoint from every other table, listed in INTEGRATION.md; the ctypes mirrors match field for field."""
    L = ptx._lib
    text = open(L.YUV16_HEADER_PATH).read()
    declared = L.header_symbols(L.YUV16_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_YUV16) == sorted(NAMES) and len(declared) == 10
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_YUV16[name][0], list(L.SIGNATURES_YUV16[name][1]))
        twin = L.SIGNATURES[name.replace("_yuv420p16", "_yuv420")]
        assert len(twin[1]) == len(fn.argtypes) and twin[0] == fn.restype          # arguments otherwise those of the twin
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_YUV16[name][1]), name
    integ = open(L.HEADER_PATH.replace("include/ptx_amd.h", "INTEGRATION.md")).read()
    assert "ptx_amd_yuv16.h" in integ and all(n in integ for n in declared)
    assert "92 stable" in integ                                                    # ptx_amd.h's census does not move
    # the ctypes mirrors, field for field
    ctype = {"p": C.c_void_p, "q": C.c_int64, "i": C.c_int32, "ptx_yuv420p16_src": L.Yuv420P16Src}
    assert [(n, ctype[k]) for n, k in struct_fields(text, "ptx_yuv420p16_src")] == list(L.Yuv420P16Src._fields_)
    assert [(n, ctype[k]) for n, k in struct_fields(text, "ptx_clip_src_yuv420p16")] == list(L.ClipSrcYuv420P16._fields_)
    assert [n for n, _ in L.Yuv420P16Src._fields_] == [n for n, _ in L.Yuv420Src._fields_] + ["bits", "shift"]
    assert C.sizeof(L.Yuv420P16Src) == 3 * 8 + 4 * 8 + 11 * 4 + 4 and C.sizeof(L.ClipSrcYuv420P16) == 104 + 16
    # the build: the header is hashed into the version and is a dependency of the objects
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert len(build.SOURCES) == 10 and any(h.endswith("ptx_amd_yuv16.h") for h in build.HEADERS)
    assert any(p.endswith("ptx_amd_yuv16.h") for p in build.tu_files("pack_layout.hip"))


def test_yuv16_descriptor_checks_without_a_device(ptx):
    L = ptx._lib
    lib = L.lib()
    P = 64                                                 # never dereferenced: every call below returns before a launch
    good = (2, 4, 270, 480, 3, 112, 112, 5, 5, L.PTX_RESIZE_OUT_U8)

    def src(**kw):
        s = L.Yuv420P16Src()
        s.y, s.u, s.v = P, 2 * P, 2 * P + 2
        s.stride_n_y, s.stride_t_y, s.stride_n_c, s.stride_t_c = 8 * 270 * 480, 2 * 270 * 480, 8 * 135 * 480, 2 * 135 * 480
        s.pitch_y, s.pitch_c, s.step_c = 960, 960, 4
        s.y_off, s.ky, s.krv, s.kgu, s.kgv, s.kbu = table("bt709", "limited", 10)
        s.bits, s.shift = 10, 6
        for k, val in kw.items():
            setattr(s, k, val)
        return s

    def frames_ok(d, s):
        return lib.ptx_resize_frames_yuv420p16_supported(C.byref(d) if d is not None else None, C.byref(s) if s is not None else None)

    def err(who="yuv420p16"):
        msg = lib.ptx_last_error().decode()
        assert who in msg
        return msg

    D = lambda: L.ResizeDesc(*good)
    assert frames_ok(D(), src()) == 1
    assert frames_ok(D(), src(shift=0)) == 1 and frames_ok(D(), src(bits=12, shift=4)) == 1 and frames_ok(D(), src(bits=12, shift=0)) == 1
    assert frames_ok(L.ResizeDesc(1, 1, 73, 99, 3, 64, 64, 1, 1, 0), src(pitch_y=198, pitch_c=100, step_c=2, v=3 * P)) == 1   # odd sizes
    assert frames_ok(D(), src(u=2 * P + 2, v=2 * P)) == 1                                       # V first
    assert frames_ok(None, src()) == 0 and "null" in err()
    assert frames_ok(D(), None) == 0 and "null" in err()
    for plane in ("y", "u", "v"):
        assert frames_ok(D(), src(**{plane: None})) == 0 and "null plane" in err()
    for bits, shift in ((8, 0), (16, 0), (11, 5), (0, 0)):
        assert frames_ok(D(), src(bits=bits, shift=shift)) == 0 and "bits" in err()
    for bits, shift in ((10, 4), (10, 2), (12, 6), (10, -6), (12, 16)):
        assert frames_ok(D(), src(bits=bits, shift=shift)) == 0 and "shift" in err()
    for k in ("pitch_y", "pitch_c"):
        assert frames_ok(D(), src(**{k: 0})) == 0 and "positive" in err()
        assert frames_ok(D(), src(**{k: -960})) == 0 and "positive" in err()
        assert frames_ok(D(), src(**{k: 961})) == 0 and "even" in err()
    for k in ("y", "u"):
        assert frames_ok(D(), src(**{k: 2 * P + 1})) == 0 and ("even" in err() or "interleaved" in err())
    assert frames_ok(D(), src(y=P + 1)) == 0 and "even" in err()
    assert frames_ok(D(), src(stride_t_y=2 * 270 * 480 + 1)) == 0 and "even" in err()
    assert frames_ok(D(), src(pitch_y=958)) == 0 and "shorter than a row" in err()            # a row is 480 samples of 2 bytes
    assert frames_ok(D(), src(pitch_y=480)) == 0 and "shorter than a row" in err()            # the 8-bit pitch
    assert frames_ok(D(), src(pitch_c=958)) == 0 and "shorter than a row" in err()
    assert frames_ok(D(), src(pitch_c=480, step_c=2, v=3 * P)) == 1
    assert frames_ok(D(), src(pitch_c=478, step_c=2, v=3 * P)) == 0 and "shorter than a row" in err()
    for step in (0, 1, 3, 8, -2):
        assert frames_ok(D(), src(step_c=step)) == 0 and "step_c" in err()
    assert frames_ok(D(), src(v=3 * P)) == 0 and "interleaved" in err()
    assert frames_ok(D(), src(v=2 * P + 1)) == 0                                               # one BYTE on is not one sample on
    assert frames_ok(D(), src(pitch_y=1 << 24)) == 0 and "32-bit" in err()                    # 270 rows of 16 MiB
    assert frames_ok(D(), src(pitch_c=1 << 25)) == 0 and "32-bit" in err()
    for ch in (1, 2, 4):
        d = D()
        d.C = ch
        assert frames_ok(d, src()) == 0 and "3 channels" in err()
    d = D()
    d.taps_h = L.PTX_RESIZE_MAX_TAPS + 1
    assert frames_ok(d, src()) == 0 and "PTX_RESIZE_MAX_TAPS" in err()                          # what the RGB path refuses
    # the other entry points run the same checks
    assert lib.ptx_resize_frames_yuv420p16_tables_supported(C.byref(D()), C.byref(src())) == 1
    assert lib.ptx_resize_frames_yuv420p16_tables_supported(C.byref(D()), C.byref(src(bits=9))) == 0 and "bits" in err()
    assert lib.ptx_resize_frames_yuv420p16_windows_supported(C.byref(D()), C.byref(src()), 128, 227) == 1
    assert lib.ptx_resize_frames_yuv420p16_windows_supported(C.byref(D()), C.byref(src()), 100, 227) == 0 and "window" in err()
    assert lib.ptx_resize_frames_yuv420p16_windows_supported(C.byref(D()), C.byref(src(shift=3)), 128, 227) == 0 and "shift" in err()
    assert lib.ptx_resize_clips_yuv420p16_supported(C.byref(D())) == 1
    d = D()
    d.C = 4
    assert lib.ptx_resize_clips_yuv420p16_supported(C.byref(d)) == 0 and "3 channels" in err()
    vd = L.ViewsDesc()
    vd.N, vd.Tv, vd.H, vd.W, vd.C, vd.S, vd.clips, vd.crops, vd.T = 1, 8, 270, 480, 3, 112, 2, 1, 4
    vd.Ur = vd.Uc = 112
    vd.taps_h = vd.taps_w = 5
    vd.nv = 2
    assert lib.ptx_resize_views_yuv420p16_supported(C.byref(vd), C.byref(src())) == 1
    assert lib.ptx_resize_views_yuv420p16_supported(C.byref(vd), C.byref(src(pitch_y=900))) == 0 and "shorter" in err()
    assert lib.ptx_resize_views_yuv420p16_supported(C.byref(vd), None) == 0 and "null" in err()
    # the launching calls run the same checks first and return a status
    tables = (C.c_void_p(P),) * 6
    call = lambda d, s, y=C.c_void_p(P): lib.ptx_resize_frames_yuv420p16(C.byref(d), C.byref(s) if s is not None else None,
                                                                          *tables, y, None, None)
    assert call(D(), None) == 1 and "null" in err()
    assert call(D(), src(pitch_y=10)) == 1 and "shorter" in err()
    assert call(D(), src(bits=11)) == 1 and "bits" in err()
    assert call(D(), src(), None) == 1 and "null pointer" in err()
    d = D()
    d.out_mode = L.PTX_RESIZE_OUT_F32
    assert call(d, src()) == 1 and "norm" in err()
    assert lib.ptx_resize_clips_yuv420p16(C.byref(D()), None, C.c_void_p(P), *tables, C.c_void_p(P), None, None) == 1 and "null" in err()
    assert lib.ptx_resize_views_yuv420p16(C.byref(vd), None, C.c_void_p(P), *tables, C.c_void_p(P), None, None) == 1 and "null" in err()
