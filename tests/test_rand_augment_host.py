"""Host tests (no GPU) of per-clip RandAugment (`pretorched.transforms.RandAugment`, include/ptx_amd_randaug.h): the numpy
statement of the arithmetic contract against Pillow, bit for bit -- every op at every bin and both signs on three frame sizes,
the pointwise LUT ops over all 256 values, the smoothing filter on degenerate sizes, the histogram ops on degenerate frames,
chains of two and four ops --, the stored golden, the draw and its order, argument errors, and the C ABI with its host checks."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image, ImageFilter, ImageOps

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import make_rand_augment_golden as MG                    # noqa: E402   (PIL's ops, the fixed lists)

from pretorched_x_amd.testing import synth_color_frames  # noqa: E402

OPTS = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], input_size=[3, 32, 32])
NAMES = ["ptx_rand_augment_apply", "ptx_rand_augment_stats", "ptx_rand_augment_supported"]
FILL = MG.FILL


def gen(seed):
    return torch.Generator().manual_seed(seed)


def one(TF, frame, code, mag, fill=FILL):
    return TF.rand_augment_numpy(frame[None, None], (np.array([[code]], np.int32), np.array([[mag]], np.float64)), fill)[0, 0]


# --------------------------------------------------------------------------------------------- the contract against PIL
@pytest.mark.parametrize("H,W", [(9, 11), (32, 20), (224, 224)])
def test_every_op_at_every_bin_and_sign_equals_pil(ptx, H, W):
    """Non-square sizes: translate_x takes its table from W, translate_y from H."""
    TF = ptx.transforms
    frame = synth_color_frames(1, 1, H, W, 6000 + H)[0, 0]
    for code in range(14):
        signs = (False, True) if TF.RANDAUG_SIGNED[code] else (False,)
        bins = range(MG.BINS) if TF.rand_augment_space(MG.BINS, H, W)[code] is not None else (0,)
        for b in bins:
            for neg in signs:
                mag = MG.magnitude(code, b, H, W, neg)
                assert np.array_equal(one(TF, frame, code, mag), MG.pil_op(frame, code, mag)), (TF.RANDAUG_OPS[code], b, neg)
    space = TF.rand_augment_space(MG.BINS, H, W)
    assert float(space[3][30]) == float(torch.tensor(150.0 / 331.0 * W)) and float(space[4][30]) == float(torch.tensor(150.0 / 331.0 * H))
    assert space[10].tolist()[:5] == [8, 8, 8, 8, 7] and space[10].tolist()[-1] == 4 and float(space[11][0]) == 255.0


def test_pointwise_lut_ops_over_all_256_values(ptx):
    TF = ptx.transforms
    v = np.arange(256, dtype=np.uint8)
    frame = np.stack([v, v[::-1], np.roll(v, 77)], -1).reshape(16, 16, 3)
    for b in range(MG.BINS):
        for code in (10, 11):
            mag = MG.magnitude(code, b, 16, 16)
            assert np.array_equal(one(TF, frame, code, mag), MG.pil_op(frame, code, mag)), (code, b)
    for thr in (-3.0, 0.0, 0.5, 127.5, 128.0, 254.999, 255.0, 300.0):   # any threshold: c < thr is c < ceil(thr)
        assert np.array_equal(one(TF, frame, 11, thr), np.asarray(ImageOps.solarize(Image.fromarray(frame, "RGB"), thr))), thr
    for bits in range(1, 9):
        assert np.array_equal(one(TF, frame, 10, float(bits)), np.asarray(ImageOps.posterize(Image.fromarray(frame, "RGB"), bits))), bits


@pytest.mark.parametrize("H,W", [(1, 9), (2, 2), (3, 3), (9, 1), (3, 7), (13, 17)])
def test_sharpness_and_the_smoothing_filter_on_small_frames(ptx, H, W):
    TF = ptx.transforms
    frame = synth_color_frames(1, 1, H, W, 6100 + 31 * H + W)[0, 0]
    want = np.asarray(Image.fromarray(frame, "RGB").filter(ImageFilter.SMOOTH))
    assert np.array_equal(TF.randaug_smooth_numpy(frame).astype(np.uint8), want)
    for mag in (0.9, -0.9, 0.27):
        assert np.array_equal(one(TF, frame, 9, mag), MG.pil_op(frame, 9, mag))


def test_histogram_ops_on_degenerate_frames(ptx):
    TF = ptx.transforms
    const = np.empty((12, 10, 3), np.uint8)
    const[...] = (0, 130, 255)
    two = const.copy()
    two[::2, 1::3] = (200, 3, 9)                                     # two levels per channel
    part = synth_color_frames(1, 1, 40, 30, 6200)[0, 0].copy()
    part[..., 1] = 77                                                # only one channel is constant
    near = np.full((16, 16, 3), 10, np.uint8)                        # 255 pixels off the last bin: step == 1; 254: step == 0
    near.reshape(-1, 3)[:255] = np.arange(255)[:, None] % 7
    zero = near.copy()
    zero.reshape(-1, 3)[254] = 10
    over = np.full((23, 23, 3), 200, np.uint8)                       # a quotient above 255 at the last bin is stored as 255
    over.reshape(-1, 3)[:509] = 5
    for name, frame in (("const", const), ("two", two), ("part", part), ("near", near), ("zero", zero), ("over", over)):
        for code in (12, 13, 8):
            mag = 0.45 if code == 8 else 0.0
            assert np.array_equal(one(TF, frame, code, mag), MG.pil_op(frame, code, mag)), (name, code)
    assert np.array_equal(one(TF, const, 13, 0.0), const) and np.array_equal(one(TF, const, 12, 0.0), const)
    assert np.array_equal(one(TF, part, 12, 0.0)[..., 1], part[..., 1]) and not np.array_equal(one(TF, part, 13, 0.0)[..., 0], part[..., 0])
    h = np.bincount(over[..., 0].ravel(), minlength=256)
    step = (h.sum() - h[200]) // 255
    assert (step // 2 + h[:200].sum()) // step > 255 and TF.randaug_equalize_lut(h)[200] == 255
    assert TF.randaug_equalize_lut(np.bincount(zero[..., 0].ravel(), minlength=256)) == list(range(256))


def test_chains_equal_the_same_pil_calls_in_sequence(ptx):
    TF = ptx.transforms
    frames = synth_color_frames(2, 2, 32, 20, 6300)
    for names in (MG.CHAIN2, MG.CHAIN4, [MG.CHAIN4[1][::-1], MG.CHAIN4[0][::-1]]):
        codes, mags = MG.chain_params(names, 32, 20, bin_=17)
        assert np.array_equal(TF.rand_augment_numpy(frames, (codes, mags), FILL), MG.pil_clips(frames, codes, mags))
    # an integer fill is the grey of that level; fill 0 is the default
    codes, mags = MG.chain_params([[("shear_x", False), ("rotate", True)]] * 2, 32, 20)
    assert np.array_equal(TF.rand_augment_numpy(frames, (codes, mags), 99), MG.pil_clips(frames, codes, mags, (99, 99, 99)))
    assert np.array_equal(TF.rand_augment_numpy(frames, (codes, mags)), MG.pil_clips(frames, codes, mags, (0, 0, 0)))


def test_stored_golden(ptx):
    TF = ptx.transforms
    blob = load_golden("rand_augment")
    fill = tuple(int(v) for v in blob["fill"])
    assert fill == FILL
    codes, mags = MG.every_cases(9, 11)
    assert np.array_equal(blob["every_codes"], codes) and np.array_equal(blob["every_mags"], mags)
    assert blob["every_in"].shape == (3, 2, 9, 11, 3) and blob["chain2_in"].shape == (2, 2, 32, 20, 3) and blob["big_in"].shape == (1, 2, 224, 224, 3)
    for j in range(len(codes)):
        got = TF.rand_augment_numpy(blob["every_in"][j % 3:j % 3 + 1], (codes[j:j + 1], mags[j:j + 1]), fill)
        assert np.array_equal(got[0], blob["every_out"][j]), j
    for group in ("chain2", "chain4"):
        got = TF.rand_augment_numpy(blob[group + "_in"], (blob[group + "_codes"], blob[group + "_mags"]), fill)
        assert np.array_equal(got, blob[group + "_out"])
    for j in range(3):
        got = TF.rand_augment_numpy(blob["big_in"], (blob["big_codes"][j:j + 1], blob["big_mags"][j:j + 1]), fill)
        assert np.array_equal(got[0], blob["big_out"][j])
    assert os.path.getsize(os.path.join(GOLDEN, "rand_augment.npz")) < 512 * 1024


# --------------------------------------------------------------------------------------------- draws
def test_draw_is_reproducible_and_follows_the_stated_order(ptx):
    TF = ptx.transforms
    a, b = TF.RandAugment(3, 11, generator=gen(5)).draw(8, 20, 32), TF.RandAugment(3, 11, generator=gen(5)).draw(8, 20, 32)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].dtype == torch.int32 and a[1].dtype == torch.float64 and a[0].shape == a[1].shape == (8, 3)
    g = gen(5)                                                      # the same stream, consumed as torchvision consumes it
    space = TF.rand_augment_space(31, 20, 32)
    signed = 0
    for n in range(8):
        for k in range(3):
            op = int(torch.randint(14, (1,), generator=g))
            mag = float(space[op][11].item()) if space[op] is not None else 0.0
            if TF.RANDAUG_SIGNED[op]:
                signed += 1
                if torch.randint(2, (1,), generator=g):
                    mag *= -1.0
            assert int(a[0][n, k]) == op and float(a[1][n, k]) == mag
    assert signed and (a[1] < 0).any() and len(set(a[0].reshape(-1).tolist())) > 4
    torch.manual_seed(3)                                             # torch's global generator is the default
    c = TF.RandAugment(1).draw(4, 8, 8)
    torch.manual_seed(3)
    assert int(c[0][0, 0]) == int(torch.randint(14, (1,)))
    # a drawn list passes the checks and replays; translate magnitudes follow the frame size
    ra = TF.RandAugment(3, 11, generator=gen(6))
    codes, mags = ra.check_params(a, 8, 20, 32)
    assert torch.equal(codes, a[0]) and torch.equal(mags, a[1])
    assert float(TF.rand_augment_space(31, 20, 32)[3][30]) > float(TF.rand_augment_space(31, 20, 32)[4][30])


def test_geometry_and_colour_are_the_same_with_and_without_augment(ptx):
    TF = ptx.transforms
    kw = dict(random_resized_crop=True, random_hflip=True)
    g1, g2 = gen(10), gen(10)
    both = TF.TransformFrames(OPTS, generator=g1, color=TF.ColorJitter(0.4, generator=g1), augment=TF.RandAugment(generator=g1), **kw)
    geo, col = both.draw_geometry(3, 90, 120), both.color.draw(3)
    aug = both.augment.draw(3, 32, 32)
    plain = TF.TransformFrames(OPTS, generator=g2, color=TF.ColorJitter(0.4, generator=g2), **kw)
    assert torch.equal(plain.draw_geometry(3, 90, 120), geo) and torch.equal(plain.color.draw(3)[1], col[1])
    assert torch.equal(TF.RandAugment(generator=g2).draw(3, 32, 32)[0], aug[0])
    assert both._resize.out == "frames" and both._resize.color is None and both._resize.augment is None
    assert both._resize.generator is both.generator and plain.augment is None
    only = TF.TransformFrames(OPTS, generator=gen(8), augment=TF.RandAugment(generator=gen(9)), **kw)
    assert torch.equal(only.draw_geometry(4, 90, 120), TF.TransformFrames(OPTS, generator=gen(8), **kw).draw_geometry(4, 90, 120))
    assert only._resize is not None and only._resize.out == "frames" and TF.TransformFrames(OPTS, **kw)._resize is None
    ra = TF.RandAugment(generator=gen(12))
    sc = TF.SampleClips(OPTS, 4, 2, 2, generator=gen(11), augment=ra, **kw)
    ref = TF.SampleClips(OPTS, 4, 2, 2, generator=gen(11), **kw)
    a, b = sc.draw([(12, 60, 80), (9, 50, 44)]), ref.draw([(12, 60, 80), (9, 50, 44)])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and sc._resize.out == "frames" and sc._resize.augment is None and ref._resize is None


# --------------------------------------------------------------------------------------------- errors
def test_argument_errors(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    for kw, what in ((dict(num_ops=0), "num_ops must be 1..4"), (dict(num_ops=5), "num_ops must be 1..4"), (dict(num_ops=2.0), "num_ops must be an integer"),
                     (dict(magnitude=31), "magnitude must be a bin 0..30"), (dict(magnitude=-1), "magnitude must be a bin"),
                     (dict(num_magnitude_bins=1, magnitude=0), "num_magnitude_bins must be at least 2"), (dict(magnitude=True), "magnitude must be an integer"),
                     (dict(fill=256), "fill must be"), (dict(fill=-1), "fill must be"), (dict(fill=(1, 2)), "fill must be"),
                     (dict(fill=1.5), "fill must be"), (dict(fill=(1, 2, 3.0)), "fill must be"), (dict(generator=7), "generator must be")):
        with pytest.raises(E, match="RandAugment: " + re.escape(what)):
            TF.RandAugment(**kw)
    assert TF.RandAugment(fill=7).fill == (7, 7, 7) and TF.RandAugment(fill=[1, 2, 3]).fill == (1, 2, 3) and TF.RandAugment(4).num_ops == 4
    ra = TF.RandAugment()
    ok = (np.array([[1, 8]], np.int32), np.array([[0.1, -0.5]]))
    ra.check_params(ok, 1, 8, 8)

    def bad(codes=None, mags=None, match="", N=None, H=8, W=8):
        with pytest.raises(E, match=match):
            ra.check_params((ok[0] if codes is None else codes, ok[1] if mags is None else mags), N, H, W)

    bad(codes=np.array([[1, 14]], np.int32), match="op code 14 out of range 0..13")
    bad(codes=np.array([[-1, 8]], np.int32), match="out of range")
    bad(mags=np.array([[0.1, -1.5]]), match="negative factor")
    bad(mags=np.array([[float("nan"), 0.0]]), match="not finite")
    bad(codes=np.array([[10, 0]], np.int32), mags=np.array([[9.0, 0.0]]), match="posterize keeps")
    bad(codes=np.zeros((1, 5), np.int32), mags=np.zeros((1, 5)), match=r"num_ops 1\.\.4")
    bad(codes=np.zeros((2, 2), np.int32), match="differ in shape")
    bad(codes=np.zeros((1, 2), np.float32), match="integers")
    bad(N=3, match="N = 3")
    bad(codes=np.array([[3, 0]], np.int32), mags=np.array([[40000.0, 0.0]]), match="fixed-point range", H=4, W=4)
    bad(codes=np.array([[5, 0]], np.int32), mags=np.array([[20.0, 0.0]]), match="fixed-point range", H=2, W=40000)
    with pytest.raises(E, match="pair"):
        ra.check_params(5)
    with pytest.raises(E, match="empty"):
        ra.check_params((np.zeros((0, 2), np.int32), np.zeros((0, 2))))
    with pytest.raises(E, match="uint8 CUDA"):
        ra(torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(E, match="expected"):
        ra(torch.zeros(2, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(E, match="N = 1"):                            # params are validated before a device is touched
        ra(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), params=(np.zeros((2, 2), np.int32), np.zeros((2, 2))))
    with pytest.raises(E, match="augment must be"):
        TF.TransformFrames(OPTS, augment="rand")
    with pytest.raises(E, match="augment must be"):
        TF.SampleClips(OPTS, augment=TF.ColorJitter(0.4))
    with pytest.raises(E, match="augment_params"):
        TF.TransformFrames(OPTS)(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), augment_params=ok)
    with pytest.raises(E, match="augment_params"):
        TF.TransformFrames(OPTS, color=TF.ColorJitter(0.4))(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), augment_params=ok)
    with pytest.raises(E, match="augment_params"):
        TF.SampleClips(OPTS)([torch.zeros(9, 8, 8, 3, dtype=torch.uint8)], augment_params=ok)
    with pytest.raises(E, match="out of range"):                     # a replay is validated before the resize touches a device
        TF.TransformFrames(OPTS, augment=ra)(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), augment_params=(np.array([[14, 0]]), np.zeros((1, 2))))
    with pytest.raises(E, match="uint8"):
        TF.rand_augment_numpy(np.zeros((1, 1, 4, 4, 3), np.float32), ok)
    with pytest.raises(E, match="not geometric"):
        TF.rand_augment_matrix(6, 0.1, 8, 8)
    assert "augment" not in TF.SampleViews.__init__.__code__.co_varnames        # test-time sampling has no augment option


# --------------------------------------------------------------------------------------------- the C ABI
def test_randaug_header_bindings_and_exports_agree(ptx):
    """The three calls live in include/ptx_amd_randaug.h: that header, _lib.SIGNATURES_RANDAUG and the library's exports name the
    same functions, disjoint from every other table, listed in INTEGRATION.md; the ctypes mirror matches field for field."""
    L = ptx._lib
    text = open(L.RANDAUG_HEADER_PATH).read()
    declared = L.header_symbols(L.RANDAUG_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_RANDAUG) == NAMES
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.SIGNATURES_YUV16, L.SIGNATURES_COLOR, L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd_color.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_RANDAUG[name][0], list(L.SIGNATURES_RANDAUG[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_RANDAUG[name][1]), name
    root = os.path.dirname(os.path.dirname(L.HEADER_PATH))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "ptx_amd_randaug.h" in integ and all(n in integ for n in declared) and "### 1l." in integ
    assert "92 stable" in integ                                                    # ptx_amd.h's census does not move
    body = re.search(r"typedef struct ptx_randaug_desc \{(.*?)\}", plain, flags=re.S).group(1)
    fields = [n.strip() for line in body.split(";") for n in line.replace("int32_t", "").split(",") if n.strip()]
    assert fields == [n for n, _ in L.RandAugDesc._fields_] and all(t is C.c_int32 for _, t in L.RandAugDesc._fields_)
    assert C.sizeof(L.RandAugDesc) == 48
    for code, name in enumerate(ptx.transforms.RANDAUG_OPS):
        assert re.search(r"#define PTX_RANDAUG_%s\s+%d\b" % (name.upper(), code), text) and getattr(L, "PTX_RANDAUG_" + name.upper()) == code
    for name, val in (("NUM_CODES", 14), ("MAX_OPS", 4), ("ROW", 8), ("STATS_WORDS", 770)):
        assert re.search(r"#define PTX_RANDAUG_%s\s+%d\b" % (name, val), text) and getattr(L, "PTX_RANDAUG_" + name) == val
    assert ptx.transforms.RANDAUG_MAX_OPS == 4 and len(ptx.transforms.RANDAUG_OPS) == len(ptx.transforms.RANDAUG_SIGNED) == 14
    # the build: both headers are hashed into the version and are dependencies of the object that holds the kernels
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert len(build.SOURCES) == 10
    assert "rand_augment.h" in build.HEADERS and any(h.endswith("ptx_amd_randaug.h") for h in build.HEADERS)
    files = build.tu_files("pack_layout.hip")
    assert any(p.endswith("rand_augment.h") for p in files) and any(p.endswith("ptx_amd_randaug.h") for p in files)
    assert L.binary_source_hash() == L.source_hash()


def test_randaug_descriptor_checks_without_a_device(ptx):
    L, TF = ptx._lib, ptx.transforms
    lib = L.lib()
    P = C.c_void_p(64)                                     # never dereferenced: every call below returns before a launch
    params = (np.array([[8, 1], [0, 10]], np.int32), np.array([[0.27, -0.09], [0.0, 6.0]]))
    rows = TF.rand_augment_rows(params, 19, 23)
    assert rows.shape == (2, 2, 8) and rows.dtype == np.int32 and rows[1, 1, 1] == 0xFC
    assert rows[0, 0, 1:2].view(np.float32)[0] == np.float32(1.27) and rows[0, 1, 1] == 65536 and rows[0, 1, 5] == 65536

    def ok(desc, r=rows):
        r = None if r is None else np.ascontiguousarray(r)
        return lib.ptx_rand_augment_supported(C.byref(desc) if desc is not None else None, C.c_void_p(r.ctypes.data) if r is not None else None)

    def err():
        return lib.ptx_last_error().decode()

    base = dict(N=2, T=3, H=19, W=23, out_mode=L.PTX_RESIZE_OUT_U8, num_ops=2, position=0, stats=1, fill_r=0, fill_g=128, fill_b=255, reserved=0)
    D = lambda **kw: L.RandAugDesc(**dict(base, **kw))
    assert ok(D()) == 1 and ok(D(out_mode=L.PTX_RESIZE_OUT_F32)) == 1 and ok(D(out_mode=L.PTX_RESIZE_OUT_BF16)) == 1
    assert ok(D(position=1, stats=0)) == 1
    assert ok(None) == 0 and "null" in err()
    assert ok(D(), r=None) == 0 and "null" in err()
    for k in ("N", "T", "H", "W"):
        assert ok(D(**{k: 0})) == 0 and "non-positive" in err()
    assert ok(D(out_mode=3)) == 0 and "out_mode" in err()
    assert ok(D(num_ops=0)) == 0 and "num_ops" in err() and ok(D(num_ops=5)) == 0 and "PTX_RANDAUG_MAX_OPS" in err()
    assert ok(D(position=2)) == 0 and "position" in err() and ok(D(position=-1)) == 0 and "position" in err()
    assert ok(D(fill_g=256)) == 0 and "fill" in err() and ok(D(fill_r=-1)) == 0 and "fill" in err()
    assert ok(D(H=40000, W=40000)) == 0 and "32-bit" in err()
    assert ok(D(T=70000)) == 0 and "grid" in err()
    assert ok(D(stats=0)) == 0 and "statistics" in err() and ok(D(position=1, stats=1)) == 0 and "statistics" in err()
    for (n, k, word, val, what) in ((0, 0, 0, 14, "out of range"), (1, 1, 0, -1, "out of range"), (1, 1, 1, 256, "posterize mask"),
                                    (0, 0, 1, int(np.float32(-0.5).view(np.int32)), "finite and >= 0"),
                                    (0, 0, 1, int(np.float32("nan").view(np.int32)), "finite and >= 0"),
                                    (0, 1, 3, 2 ** 31 - 1, "fixed-point range"), (0, 1, 6, -2 ** 31, "fixed-point range"),
                                    (0, 1, 1, 2 ** 30, "fixed-point range")):
        r = rows.copy()
        r[n, k, word] = val
        d = D(stats=int(r[0, 0, 0] in (8, 12, 13)))
        assert ok(d, r=r) == 0 and what in err() and ("clip %d position %d" % (n, k)) in err(), (what, err())
    sol = rows.copy()
    sol[1, 1, 0], sol[1, 1, 1] = 11, int(np.float32("inf").view(np.int32))
    assert ok(D(), r=sol) == 0 and "solarize threshold" in err()
    # the launches' own checks (status PTX_ERR_INVALID = 1), before anything reaches a device
    stream = None
    assert lib.ptx_rand_augment_stats(None, P, P, P, stream) == 1 and "null" in err()
    assert lib.ptx_rand_augment_stats(C.byref(D()), None, P, P, stream) == 1 and "null" in err()
    assert lib.ptx_rand_augment_stats(C.byref(D()), P, P, None, stream) == 1 and "null" in err()
    assert lib.ptx_rand_augment_stats(C.byref(D()), P, P, C.c_void_p(68), stream) == 1 and "misaligned" in err()
    assert lib.ptx_rand_augment_stats(C.byref(D(T=0)), P, P, P, stream) == 1 and "non-positive" in err()
    norm = L.NormDesc.make(OPTS["mean"], OPTS["std"])
    assert lib.ptx_rand_augment_apply(C.byref(D()), P, P, None, P, None, stream) == 1 and "null" in err()        # stats=1 needs them
    assert lib.ptx_rand_augment_apply(C.byref(D()), P, P, P, None, None, stream) == 1 and "null" in err()
    assert lib.ptx_rand_augment_apply(C.byref(D(out_mode=1)), P, P, P, P, None, stream) == 1 and "norm" in err()
    assert lib.ptx_rand_augment_apply(C.byref(D(out_mode=1)), P, P, P, C.c_void_p(66), C.byref(norm), stream) == 1 and "misaligned" in err()
    assert lib.ptx_rand_augment_apply(C.byref(D(out_mode=2)), P, P, P, C.c_void_p(65), C.byref(norm), stream) == 1 and "misaligned" in err()
    assert lib.ptx_rand_augment_apply(C.byref(D(out_mode=7)), P, P, P, P, C.byref(norm), stream) == 1 and "out_mode" in err()
    assert lib.ptx_rand_augment_apply(C.byref(D(num_ops=9)), P, P, P, P, None, stream) == 1 and "num_ops" in err()
