"""Host tests (no GPU) of per-clip ColorJitter / RandomGrayscale (`pretorched.transforms.ColorJitter`,
include/ptx_amd_color.h): the numpy statement of the arithmetic contract against Pillow -- the chain on random frames for all
24 op orders, the luma and both HSV conversions on the full 256^3 cubes, the blend on all 256 x 256 pairs -- the stored
golden, the draw and its order, argument errors, and the C ABI with its host-side checks."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import make_color_jitter_golden as MG                    # noqa: E402   (PIL's chain, the fixed op lists)

from pretorched_x_amd.testing import synth_color_frames  # noqa: E402

OPTS = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], input_size=[3, 32, 32])
BLEND_FACTORS = (0.0, 0.2, 0.6, 0.999, 1.0, 1.0001, 1.4, 1.8, 2.5)
NAMES = ["ptx_color_jitter_apply", "ptx_color_jitter_stats", "ptx_color_jitter_supported"]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def cube(r0, r1):
    """uint8 [(r1 - r0) * 256, 256, 3]: every (r, g, b) with r in [r0, r1)."""
    r, g, b = np.meshgrid(np.arange(r0, r1), np.arange(256), np.arange(256), indexing="ij")
    return np.stack([r, g, b], -1).astype(np.uint8).reshape(-1, 256, 3)


# --------------------------------------------------------------------------------------------- the contract against PIL
def test_numpy_chain_equals_pil_for_all_24_orders(ptx):
    TF = ptx.transforms
    rng = np.random.RandomState(7)
    ops = [MG.B, MG.C, MG.S, MG.H]
    for i, order in enumerate(itertools.permutations(range(4))):
        H_, W_ = 9 + 2 * (i % 5), 7 + 2 * (i % 7)                    # odd sizes
        frames = synth_color_frames(1, 2, H_, W_, 900 + i)
        fac = {MG.B: rng.uniform(0.3, 1.9), MG.C: rng.uniform(0.0, 2.2), MG.S: rng.uniform(0.0, 2.5), MG.H: rng.uniform(-0.5, 0.5)}
        lst = [(ops[k], fac[ops[k]]) for k in order] + ([(MG.G, 1.0)] if i % 6 == 5 else [])
        want = np.stack([MG.pil_chain(f, lst) for f in frames[0]])[None]
        assert np.array_equal(TF.color_jitter_numpy(frames, MG.op_rows([lst])), want), lst


def test_stored_golden(ptx):
    TF = ptx.transforms
    blob = load_golden("color_jitter")
    for group, (lists, T, H_, W_, seed) in MG.GROUPS.items():
        assert [int(v) for v in blob[group + "_shape"]] == [len(lists), T, H_, W_, seed]
        codes, factors = MG.op_rows(lists)
        assert np.array_equal(blob[group + "_codes"], codes) and np.array_equal(blob[group + "_factors"], factors)
        frames = synth_color_frames(len(lists), T, H_, W_, seed)
        assert np.array_equal(TF.color_jitter_numpy(frames, (codes, factors)), blob[group + "_out"])
    small = os.path.getsize(os.path.join(GOLDEN, "color_jitter.npz"))
    assert 4 * small < os.path.getsize(os.path.join(GOLDEN, "transform_frames.npz"))


def test_luma_equals_pil_on_the_full_cube(ptx):
    TF = ptx.transforms
    for r0 in range(0, 256, 64):
        rgb = cube(r0, r0 + 64)
        want = np.asarray(Image.fromarray(rgb, "RGB").convert("L"))
        assert np.array_equal(TF.color_luma_numpy(rgb), want)


def test_hsv_conversions_equal_pil_on_the_full_cubes(ptx):
    TF = ptx.transforms
    for r0 in range(0, 256, 32):
        block = cube(r0, r0 + 32)
        assert np.array_equal(TF.color_rgb_to_hsv_numpy(block), np.asarray(Image.fromarray(block, "RGB").convert("HSV")))
        want = np.asarray(Image.frombytes("HSV", (256, block.shape[0]), block.tobytes()).convert("RGB"))     # block read as (h, s, v)
        assert np.array_equal(TF.color_hsv_to_rgb_numpy(block), want)


def test_blend_equals_pil_on_all_pairs(ptx):
    TF = ptx.transforms
    d, x = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    deg, img = Image.fromarray(d.astype(np.uint8), "L"), Image.fromarray(x.astype(np.uint8), "L")
    for f in BLEND_FACTORS:
        f32 = float(np.float32(f))
        assert np.array_equal(TF.color_blend_numpy(d, x, f32), np.asarray(Image.blend(deg, img, f32))), f


# --------------------------------------------------------------------------------------------- draws
def test_draw_is_reproducible_and_follows_the_stated_order(ptx):
    TF, L = ptx.transforms, ptx._lib
    kw = dict(brightness=0.4, contrast=(0.5, 1.5), saturation=0.3, hue=0.1, grayscale=0.5)
    a, b = TF.ColorJitter(generator=gen(5), **kw).draw(6), TF.ColorJitter(generator=gen(5), **kw).draw(6)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].dtype == torch.int32 and a[1].dtype == torch.float32 and a[0].shape == a[1].shape == (6, 5)
    g = gen(5)                                                      # the same stream, consumed as torchvision consumes it
    ranges = [(1.0 - 0.4, 1.0 + 0.4), (0.5, 1.5), (1.0 - 0.3, 1.0 + 0.3), (-0.1, 0.1)]
    for n in range(6):
        order = torch.randperm(4, generator=g).tolist()
        drawn = [torch.empty(1).uniform_(lo, hi, generator=g)[0] for lo, hi in ranges]
        gray = bool(torch.rand(1, generator=g) < 0.5)
        codes = [fn + 1 for fn in order] + [L.PTX_COLOR_GRAYSCALE if gray else 0]
        assert a[0][n].tolist() == codes
        for k, fn in enumerate(order):
            want = float(TF.hue_shift(float(drawn[fn]))) if fn == 3 else float(drawn[fn])       # fp32 factors, integer hue shifts
            assert float(a[1][n, k]) == want
    assert len({tuple(r) for r in a[0].tolist()}) > 1
    # torch's global generator is the default; an op that is off draws nothing and does not run
    torch.manual_seed(3)
    c = TF.ColorJitter(brightness=0.2).draw(2)
    torch.manual_seed(3)
    assert float(c[1][0, 0]) == float((torch.randperm(4), torch.empty(1).uniform_(0.8, 1.2))[1])
    assert c[0].tolist() == [[1, 0, 0, 0, 0]] * 2
    assert not TF.ColorJitter().draw(3)[0].any() and not TF.ColorJitter(hue=(0, 0), contrast=(1, 1)).draw(1)[0].any()
    assert TF.ColorJitter(brightness=2).brightness == (0.0, 3.0) and TF.ColorJitter(hue=0.5).hue == (-0.5, 0.5)
    assert TF.hue_shift(-0.5) == 129 and TF.hue_shift(0.5) == 127 and TF.hue_shift(0.0) == 0 and TF.hue_shift(-0.001) == 0
    # a drawn list passes the library's check and replays
    codes, factors = TF.ColorJitter(generator=gen(6), **kw).check_params(a, 6)
    assert torch.equal(codes, a[0]) and torch.equal(factors, a[1])


def test_geometry_is_the_same_with_and_without_colour(ptx):
    TF = ptx.transforms
    kw = dict(random_resized_crop=True, random_hflip=True)
    cj = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, generator=gen(9))
    with_c, without = TF.TransformFrames(OPTS, generator=gen(8), color=cj, **kw), TF.TransformFrames(OPTS, generator=gen(8), **kw)
    assert torch.equal(with_c.draw_geometry(4, 90, 120), without.draw_geometry(4, 90, 120))
    assert with_c.color is cj and without.color is None and with_c._resize.out == "frames" and with_c._resize.color is None
    assert with_c._resize.generator is with_c.generator
    # one shared generator: the colour draws come after every geometry draw of the call
    g1, g2 = gen(10), gen(10)
    both = TF.TransformFrames(OPTS, generator=g1, color=TF.ColorJitter(0.4, generator=g1), **kw)
    geo = both.draw_geometry(3, 90, 120)
    col = both.color.draw(3)
    assert torch.equal(TF.TransformFrames(OPTS, generator=g2, **kw).draw_geometry(3, 90, 120), geo)
    assert torch.equal(TF.ColorJitter(0.4, generator=g2).draw(3)[1], col[1])
    sc = TF.SampleClips(OPTS, 4, 2, 2, generator=gen(11), color=cj, **kw)
    plain = TF.SampleClips(OPTS, 4, 2, 2, generator=gen(11), **kw)
    a, b = sc.draw([(12, 60, 80), (9, 50, 44)]), plain.draw([(12, 60, 80), (9, 50, 44)])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and sc._resize.out == "frames"


# --------------------------------------------------------------------------------------------- errors
def test_argument_errors(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    for kw in (dict(brightness=-0.1), dict(hue=0.6), dict(hue=(-0.6, 0.1)), dict(contrast=(1.5, 0.5)), dict(saturation=(-1, 1)),
               dict(brightness="a"), dict(brightness=True), dict(contrast=(1, 2, 3)), dict(saturation=float("inf")),
               dict(grayscale=1.5), dict(grayscale=-0.1), dict(grayscale="x"), dict(generator=7)):
        with pytest.raises(E, match="ColorJitter"):
            TF.ColorJitter(**kw)
    ok = (np.array([[1, 2, 3, 4, 5]], np.int32), np.array([[1.0, 1.0, 1.0, 7.0, 0.0]], np.float32))
    TF.check_color_params(ok, 1)

    def bad(codes=None, factors=None, match="", N=None):
        with pytest.raises(E, match=match):
            TF.check_color_params((ok[0] if codes is None else codes, ok[1] if factors is None else factors), N)

    bad(codes=np.array([[1, 2, 3, 4, 6]], np.int32), match="out of range")
    bad(codes=np.array([[-1, 2, 3, 4, 5]], np.int32), match="out of range")
    bad(codes=np.array([[1, 2, 2, 4, 5]], np.int32), match="repeated")
    bad(factors=np.array([[1.0, 1.0, 1.0, 256.0, 0.0]], np.float32), match="hue shift")
    bad(factors=np.array([[1.0, 1.0, 1.0, -1.0, 0.0]], np.float32), match="hue shift")
    bad(factors=np.array([[1.0, 1.0, 1.0, 7.5, 0.0]], np.float32), match="hue shift")
    bad(factors=np.array([[-0.5, 1.0, 1.0, 7.0, 0.0]], np.float32), match="finite and >= 0")
    bad(factors=np.array([[1.0, float("nan"), 1.0, 7.0, 0.0]], np.float32), match="finite and >= 0")
    bad(factors=np.array([[1.0, 1.0, float("inf"), 7.0, 0.0]], np.float32), match="finite and >= 0")
    bad(codes=np.zeros((1, 4), np.int32), match=r"\[N, 5\]")
    bad(codes=np.zeros((2, 5), np.int32), match="differ in shape")
    bad(codes=np.zeros((1, 5), np.float32), match="integers")
    bad(N=3, match="N = 3")
    with pytest.raises(E, match="pair"):
        TF.check_color_params(5)
    with pytest.raises(E, match="empty"):
        TF.check_color_params((np.zeros((0, 5), np.int32), np.zeros((0, 5), np.float32)))
    cj = TF.ColorJitter(0.4)
    with pytest.raises(E, match="uint8 CUDA"):
        cj(torch.zeros(1, 2, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(E, match="expected"):
        cj(torch.zeros(2, 8, 8, 4, dtype=torch.uint8))
    with pytest.raises(E, match="N = 1"):                            # params are validated before a device is touched
        cj(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), params=(np.zeros((2, 5), np.int32), np.zeros((2, 5), np.float32)))
    with pytest.raises(E, match="color must be"):
        TF.TransformFrames(OPTS, color="jitter")
    with pytest.raises(E, match="color must be"):
        TF.SampleClips(OPTS, color=0.4)
    with pytest.raises(E, match="color_params"):
        TF.TransformFrames(OPTS)(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), color_params=ok)
    with pytest.raises(E, match="uint8"):
        TF.color_jitter_numpy(np.zeros((1, 1, 4, 4, 3), np.float32), ok)
    assert "color" not in TF.SampleViews.__init__.__code__.co_varnames          # test-time sampling has no colour option


# --------------------------------------------------------------------------------------------- the C ABI
def test_color_header_bindings_and_exports_agree(ptx):
    """The three calls live in include/ptx_amd_color.h: that header, _lib.SIGNATURES_COLOR and the library's exports name the
    same functions, disjoint from every other table, listed in INTEGRATION.md; the ctypes mirror matches field for field."""
    L = ptx._lib
    text = open(L.COLOR_HEADER_PATH).read()
    declared = L.header_symbols(L.COLOR_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_COLOR) == NAMES
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.SIGNATURES_YUV16, L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_COLOR[name][0], list(L.SIGNATURES_COLOR[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_COLOR[name][1]), name
    root = os.path.dirname(os.path.dirname(L.HEADER_PATH))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "ptx_amd_color.h" in integ and all(n in integ for n in declared) and "### 1k." in integ
    assert "92 stable" in integ                                                    # ptx_amd.h's census does not move
    body = re.search(r"typedef struct ptx_color_desc \{(.*?)\}", plain, flags=re.S).group(1)
    fields = [n.strip() for line in body.split(";") for n in line.replace("int32_t", "").split(",") if n.strip()]
    assert fields == [n for n, _ in L.ColorDesc._fields_] and all(t is C.c_int32 for _, t in L.ColorDesc._fields_)
    assert C.sizeof(L.ColorDesc) == 24
    for code, name in enumerate(ptx.transforms.COLOR_OPS):
        assert re.search(r"#define PTX_COLOR_%s\s+%d\b" % (name.upper(), code), text) and getattr(L, "PTX_COLOR_" + name.upper()) == code
    assert re.search(r"#define PTX_COLOR_MAX_OPS\s+5\b", text) and L.PTX_COLOR_MAX_OPS == ptx.transforms.COLOR_MAX_OPS == 5
    # the build: both headers are hashed into the version and are dependencies of the object that holds the kernels
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert len(build.SOURCES) == 10
    assert "color_jitter.h" in build.HEADERS and any(h.endswith("ptx_amd_color.h") for h in build.HEADERS)
    files = build.tu_files("pack_layout.hip")
    assert any(p.endswith("color_jitter.h") for p in files) and any(p.endswith("ptx_amd_color.h") for p in files)
    assert L.binary_source_hash() == L.source_hash()


def test_color_descriptor_checks_without_a_device(ptx):
    L = ptx._lib
    lib = L.lib()
    P = C.c_void_p(64)                                     # never dereferenced: every call below returns before a launch
    codes = np.array([[1, 2, 3, 4, 5], [0, 0, 0, 0, 0]], np.int32)
    factors = np.array([[1.0, 0.5, 2.0, 129.0, 0.0], [0.0] * 5], np.float32)

    def ok(desc, c=codes, f=factors):
        return lib.ptx_color_jitter_supported(C.byref(desc) if desc is not None else None,
                                              C.c_void_p(c.ctypes.data) if c is not None else None,
                                              C.c_void_p(f.ctypes.data) if f is not None else None)

    def err():
        return lib.ptx_last_error().decode()

    D = lambda **kw: L.ColorDesc(**dict(dict(N=2, T=3, H=19, W=23, out_mode=L.PTX_RESIZE_OUT_U8, contrast=1), **kw))
    assert ok(D()) == 1 and ok(D(out_mode=L.PTX_RESIZE_OUT_F32)) == 1 and ok(D(out_mode=L.PTX_RESIZE_OUT_BF16)) == 1
    assert ok(D(N=1, H=1, W=1, T=1)) == 1
    assert ok(None) == 0 and "null" in err()
    assert ok(D(), c=None) == 0 and "null" in err()
    assert ok(D(), f=None) == 0 and "null" in err()
    for k in ("N", "T", "H", "W"):
        assert ok(D(**{k: 0})) == 0 and "non-positive" in err()
    assert ok(D(out_mode=3)) == 0 and "out_mode" in err()
    assert ok(D(H=40000, W=40000)) == 0 and "32-bit" in err()
    assert ok(D(contrast=0)) == 0 and "contrast" in err()
    assert ok(D(N=1, contrast=0), c=codes[1:], f=factors[1:]) == 1 and ok(D(N=1), c=codes[1:], f=factors[1:]) == 0
    for row, col, val, what in ((0, 0, 6, "out of range"), (1, 4, -1, "out of range"), (0, 4, 1, "repeated")):
        c = codes.copy()
        c[row, col] = val
        assert ok(D(contrast=int((c == 2).any())), c=c) == 0 and what in err() and "clip %d entry %d" % (row, col) in err()
    for col, val, what in ((3, 256.0, "hue shift"), (3, 0.5, "hue shift"), (3, -1.0, "hue shift"), (0, -1.0, "finite"), (1, float("nan"), "finite"),
                           (2, float("inf"), "finite")):
        f = factors.copy()
        f[0, col] = val
        assert ok(D(), f=f) == 0 and what in err()
    # the launches' own checks (status PTX_ERR_INVALID = 1), before anything reaches a device
    stream = None
    assert lib.ptx_color_jitter_stats(None, P, P, P, P, stream) == 1 and "null" in err()
    assert lib.ptx_color_jitter_stats(C.byref(D()), None, P, P, P, stream) == 1 and "null" in err()
    assert lib.ptx_color_jitter_stats(C.byref(D()), P, P, P, None, stream) == 1 and "null" in err()
    assert lib.ptx_color_jitter_stats(C.byref(D()), P, P, P, C.c_void_p(68), stream) == 1 and "misaligned" in err()
    assert lib.ptx_color_jitter_stats(C.byref(D(T=0)), P, P, P, P, stream) == 1 and "non-positive" in err()
    norm = L.NormDesc.make(OPTS["mean"], OPTS["std"])
    assert lib.ptx_color_jitter_apply(C.byref(D()), P, P, P, None, P, None, stream) == 1 and "null" in err()      # contrast needs sums
    assert lib.ptx_color_jitter_apply(C.byref(D()), P, P, P, P, None, None, stream) == 1 and "null" in err()
    assert lib.ptx_color_jitter_apply(C.byref(D(out_mode=1)), P, P, P, P, P, None, stream) == 1 and "norm" in err()
    assert lib.ptx_color_jitter_apply(C.byref(D(out_mode=1)), P, P, P, P, C.c_void_p(66), C.byref(norm), stream) == 1 and "misaligned" in err()
    assert lib.ptx_color_jitter_apply(C.byref(D(out_mode=2)), P, P, P, P, C.c_void_p(65), C.byref(norm), stream) == 1 and "misaligned" in err()
    bad = L.NormDesc.make(OPTS["mean"], [0.2, 0.0, 0.2])
    assert lib.ptx_color_jitter_apply(C.byref(D(out_mode=1)), P, P, P, P, P, C.byref(bad), stream) == 1 and "std" in err()
    assert lib.ptx_color_jitter_apply(C.byref(D(out_mode=7)), P, P, P, P, P, C.byref(norm), stream) == 1 and "out_mode" in err()
