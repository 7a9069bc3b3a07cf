"""Host tests (no GPU) of the resize filters other than bilinear (`interpolation=` of `pretorched.transforms.TransformFrames`,
`SampleViews`, `SampleClips`; include/ptx_amd_resample.h): the table builder + the numpy statement of the kernel's arithmetic
against Pillow's stored outputs (tests/golden/resample_frames.npz) and, where Pillow imports, against Pillow itself on a sweep
of extents; the default's bits; the tap counts of the per-clip path; the coefficient guards; the accepted spellings; what a
per-clip geometry supports; the draws; the C ABI.  Every comparison is exact equality."""
import ctypes as C
import enum
import functools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import make_resample_golden as MG                        # noqa: E402   (the cases, the inputs)

OPTS = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225], input_size=[3, 32, 32])
FILTERS = MG.FILTERS
NAMES = ["ptx_resize_build_tables_clips_filter", "ptx_resize_build_tables_filter"]
PIL_CODES = {"nearest": 0, "lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}


@functools.lru_cache(None)
def golden():
    blob = load_golden("resample_frames")
    return blob, json.loads(str(blob["cases"]))


def gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------------------------- the tables against Pillow
@pytest.mark.parametrize("f", FILTERS)
def test_tables_and_numpy_model_equal_the_pil_fixtures(ptx, f):
    TF = ptx.transforms
    blob, cases = golden()
    assert [c["name"] for c in cases] == [c["name"] for c in MG.CASES] and json.loads(json.dumps(MG.CASES)) == cases
    for c in cases:
        frames = MG.case_frames(c)
        want = blob["out_%s_%s" % (c["name"], f)]
        assert want.shape == (2, MG.T, 32, 32, 3) and want.dtype == np.uint8
        geo = TF.geometry_tables(MG.geometry_row(c), 32, f)
        fixed = TF.build_tables(c["H"], c["W"], c["input_size"], c["scale"], False, (c["top"], c["left"]), bool(c["hflip"]),
                                bool(c["vflip"]), interpolation=f)
        assert fixed["resized"] == (c["h"], c["w"])
        for a, b in zip(geo["rows"] + geo["cols"], fixed["rows"] + fixed["cols"]):
            assert np.array_equal(a, b), (c["name"], f)
        for n in range(2):
            for t in range(MG.T):
                assert np.array_equal(TF.apply_tables_numpy(frames[n, t], geo), want[n, t]), (c["name"], f, n, t)
    if f in ("bicubic", "lanczos"):                       # the saturated clip is what a clamp that mistreats negative sums fails on
        c = cases[0]
        shares = MG.clip_shares(MG.case_frames(c)[1, 0], TF.geometry_tables(MG.geometry_row(c), 32, f))
        assert len(shares) == 2 and all(lo >= MG.CLIP_SHARE and hi >= MG.CLIP_SHARE for lo, hi in shares), shares
    # the deep case is what reaches more than half the tap cap: Lanczos needs 38 row taps there
    if f == "lanczos":
        assert TF.geometry_tables(MG.geometry_row(cases[2]), 32, f)["rows"][2].shape[1] == 38


@pytest.mark.parametrize("f", FILTERS)
def test_axis_tables_equal_live_pil_on_a_sweep_of_extents(ptx, f):
    """n_in 1..70 x n_out in {1, 2, 7, 16, 33, 64}: one axis resized by Pillow itself against the table of that axis."""
    Image = pytest.importorskip("PIL.Image")
    TF = ptx.transforms
    code = getattr(Image.Resampling, f.upper())
    assert int(code) == PIL_CODES[f] == TF.INTERPOLATIONS.index(f)
    rng = np.random.RandomState(11)
    checker = (np.arange(70)[:, None, None] // 3 + np.arange(4)[None, :, None]) % 2 * 255 + np.zeros((1, 1, 3), np.int64)
    for n_in in range(1, 71):
        noise = rng.randint(0, 256, (n_in, 4, 3)).astype(np.uint8)
        for frame in (noise, checker[:n_in].astype(np.uint8)):
            for n_out in (1, 2, 7, 16, 33, 64):
                want = np.asarray(Image.fromarray(frame).resize((4, n_out), code))
                tables = {"rows": TF.resize_axis_table(n_in, n_out, f), "cols": TF.resize_axis_table(4, 4, f)}
                assert np.array_equal(TF.apply_tables_numpy(frame, tables), want), (f, n_in, n_out)


def test_default_is_todays_bilinear_table_and_the_scalar_restatement_agrees(ptx):
    TF = ptx.transforms
    for a, b in [(1, 1), (1, 9), (9, 1), (37, 53), (53, 37), (90, 32), (360, 256), (29, 40), (64, 64), (70, 7), (200, 32)]:
        default, named = TF.resize_axis_table(a, b), TF.resize_axis_table(a, b, "bilinear")
        assert len(default) == len(named) == 3
        for x, y in zip(default, named):
            assert x.dtype == y.dtype == np.int32 and np.array_equal(x, y)
        for spelled in (2, "bilinear"):
            for x, y in zip(default, TF.resize_axis_table(a, b, spelled)):
                assert np.array_equal(x, y)
        if a != b:                                         # PIL's C restated scalar by scalar gives the vectorised builder's bits
            for x, y in zip(default, TF._filter_axis_table(a, b, "bilinear")):
                assert np.array_equal(x, y), (a, b)
    # an axis whose extent does not change is one tap of 2**22 for every filter, and cached tables cannot be written
    for f in FILTERS:
        lo, n, k = TF.resize_axis_table(17, 17, f)
        assert np.array_equal(lo, np.arange(17)) and (n == 1).all() and k.shape == (17, 1) and (k == 1 << 22).all()
        if f != "bilinear":
            t = TF.resize_axis_table(40, 17, f)
            assert t[0] is TF.resize_axis_table(40, 17, f)[0] and not t[2].flags.writeable
    # signatures: the filter is a trailing keyword everywhere, so positional callers keep working
    import inspect
    for fn in (TF.resize_axis_table, TF.build_tables, TF.build_frame_tables, TF.geometry_tables, TF._axis_taps, TF._check_taps):
        p = list(inspect.signature(fn).parameters.values())
        assert "interpolation" in [q.name for q in p] and p[[q.name for q in p].index("interpolation")].default == "bilinear", fn
    assert TF.build_tables(90, 160, [3, 32, 32])["rows"][2].shape == TF.build_tables(90, 160, [3, 32, 32], interpolation="bilinear")["rows"][2].shape


@pytest.mark.parametrize("f", FILTERS)
def test_axis_taps_equal_the_tables_widest_entry(ptx, f):
    TF = ptx.transforms
    S = 8
    cases = [(n_in, n_out, start) for n_in in (8, 9, 17, 31, 64, 100, 203) for n_out in (8, 9, 13, 32, 77)
             for start in (0, (n_out - S) // 2, n_out - S)]
    n_in, n_out, start = (np.array(v, np.int64) for v in zip(*cases))
    got = TF._axis_taps(n_in, n_out, start, S, f)
    for i, (a, b, s) in enumerate(cases):
        lo, n, k = TF.resize_axis_table(a, b, f)
        assert got[i] == n[s:s + S].max() == TF._select((lo, n, k), s, S)[2].shape[1], (f, a, b, s)
    if f == "bilinear":
        assert np.array_equal(got, TF._axis_taps(n_in, n_out, start, S))


def test_the_deep_case_reaches_the_chunked_bands(ptx):
    """With BOX and NEAREST a band of the 6.25x row down-scale references more input rows than the launch plan's bound for
    overlapping taps (rows_of in resize_plan: b * taps / 2 + taps + 1, or b for one tap), so on the GPU the kernel's chunk loop
    runs for that fixture case: this pins the shapes that make it so.  The filters of support >= 1 stay inside the bound."""
    TF = ptx.transforms
    c = {c["name"]: c for c in golden()[1]}["deep_200x120"]
    band = 16
    for f in FILTERS:
        lo, n, k = TF.geometry_tables(MG.geometry_row(c), 32, f)["rows"]
        taps = k.shape[1]
        bound = (band * taps + 1) // 2 + taps + 1 if taps > 1 else band
        spans = [int((lo[b:b + band] + n[b:b + band]).max() - lo[b:b + band].min()) for b in (0, band)]
        assert (max(spans) > bound) == (f in ("box", "nearest")), (f, taps, spans, bound)
    assert TF.geometry_tables(MG.geometry_row(c), 32, "nearest")["rows"][2].shape[1] == 1


def test_coefficient_guards(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    TF.check_coefficients(np.array([[(1 << 23) - 1], [-((1 << 23) - 1)]]))               # the largest magnitudes that pass
    with pytest.raises(E, match=r"2\*\*23"):
        TF.check_coefficients(np.array([[1 << 23, 0]]))
    with pytest.raises(E, match=r"2\*\*23"):
        TF.check_coefficients(np.array([[0, -(1 << 23)]]))
    over = ((1 << 31) - (1 << 21)) // 255 + 1                                            # smallest sum|k| that overflows
    TF.check_coefficients(np.array([[over - 1 - (1 << 22), 1 << 22]]))
    with pytest.raises(E, match="accumulator"):
        TF.check_coefficients(np.array([[over - (1 << 22), -(1 << 22)]]))
    # wherever tables are built or accepted: _check_taps (build_tables, build_frame_tables, SampleViews.tables)
    good = TF.resize_axis_table(40, 17, "bicubic")
    bad = (good[0], good[1], np.where(np.arange(good[2].shape[1])[None, :] == 0, 1 << 23, good[2]).astype(np.int32))
    with pytest.raises(E, match=r"2\*\*23"):
        TF._check_taps(bad, good, 40, 40, 17, 17, "bicubic")
    wide = (good[0], good[1], np.full_like(good[2], (1 << 23) - 1))
    assert 255 * int(np.abs(wide[2]).sum(axis=1).max()) + (1 << 21) >= 1 << 31
    with pytest.raises(E, match="accumulator"):
        TF._check_taps(good, wide, 40, 40, 17, 17, "bicubic")
    # Pillow's own tables keep far inside both bounds, and the bound the per-clip path takes of tables it does not build holds
    worst = 0
    for f in FILTERS:
        for a, b in [(70, 7), (7, 70), (200, 32), (31, 64), (53, 37), (600, 40)]:
            k = TF.resize_axis_table(a, b, f)[2].astype(np.int64)
            TF.check_coefficients(k)
            worst = max(worst, int(np.abs(k).sum(axis=1).max()))
    assert (1 << 22) < worst < 1.6 * (1 << 22)
    cases = [(70, 7, 0), (7, 70, 31), (200, 40, 4), (31, 64, 16), (53, 37, 2), (64, 64, 3)]
    n_in, n_out, start = (np.array(v, np.int64) for v in zip(*cases))
    kmax, ksum = TF._axis_bicubic_bound(n_in, n_out, start, 5)
    for i, (a, b, s) in enumerate(cases):
        k = np.abs(TF._select(TF.resize_axis_table(a, b, "bicubic"), s, 5)[2].astype(np.int64))
        assert k.max() <= kmax[i] <= k.max() + 1 and k.sum(axis=1).max() <= ksum[i] <= k.sum(axis=1).max() + k.shape[1], (a, b, s)


def test_tap_cap_message_names_the_filter(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    with pytest.raises(E, match=r"lanczos filter needs 113 taps.*PTX_RESIZE_MAX_TAPS = 64"):
        TF.build_tables(600, 800, [3, 32, 32], scale=1.0, interpolation="lanczos")
    with pytest.raises(E, match=r"lanczos filter needs 113 taps"):
        TF.TransformFrames(OPTS, scale=1.0, interpolation="lanczos").frame_tables(600, 800)
    with pytest.raises(E, match=r"SampleViews.*bicubic filter needs"):
        TF.SampleViews(OPTS, clips=1, crops=1, scale=1.0, interpolation="bicubic").tables(600, 800)
    TF.build_tables(600, 800, [3, 32, 32], scale=1.0)                                    # bilinear: 39 taps
    with pytest.raises(E, match=r"geometry\[1\].*bicubic filter needs"):
        TF.TransformFrames(OPTS, interpolation="bicubic").check_geometry(
            [[0, 0, 64, 64, 32, 32, 0, 0, 0, 0], [0, 0, 600, 64, 32, 32, 0, 0, 0, 0]], 2, 600, 64)
    for call in (lambda: TF.build_tables(2100, 64, [3, 32, 32], scale=1.0, preserve_aspect_ratio=False),
                 lambda: TF.TransformFrames(OPTS).check_geometry([[0, 0, 2100, 64, 32, 32, 0, 0, 0, 0]], 1, 2100, 64)):
        with pytest.raises(E, match=r"needs 1\d\d taps") as e:                            # the default's message is today's
            call()
        assert "filter" not in str(e.value)


class _Mode(enum.Enum):
    BICUBIC = "bicubic"
    LANCZOS = 1


def test_accepted_spellings(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    assert TF.TransformFrames(OPTS).interpolation == "bilinear" == TF.SampleViews(OPTS).interpolation == TF.SampleClips(OPTS).interpolation
    for name, code in PIL_CODES.items():
        for spelled in (name, code):
            assert TF.TransformFrames(OPTS, interpolation=spelled).interpolation == name
            assert TF.SampleViews(OPTS, interpolation=spelled).interpolation == name
    assert TF.TransformFrames(OPTS, interpolation=_Mode.BICUBIC).interpolation == "bicubic"
    assert TF.TransformFrames(OPTS, interpolation=_Mode.LANCZOS).interpolation == "lanczos"
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        for name in FILTERS:
            assert TF.TransformFrames(OPTS, interpolation=getattr(Image.Resampling, name.upper())).interpolation == name
    sc = TF.SampleClips(OPTS, interpolation=3, random_resized_crop=True)
    assert sc.interpolation == sc.spatial.interpolation == "bicubic"
    for bad in ("cubic", "BICUBIC", 6, -1, 2.0, True, None, ("bicubic",)):
        for make in (TF.TransformFrames, TF.SampleViews, TF.SampleClips):
            with pytest.raises(E, match="interpolation"):
                make(OPTS, interpolation=bad)
    with pytest.raises(E, match="interpolation"):
        TF.resize_axis_table(9, 5, "cubic")


def test_trigonometric_filters_refuse_a_per_clip_geometry(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    rows = [[0, 0, 40, 40, 32, 32, 0, 0, 0, 0]]
    for f in ("hamming", "lanczos"):
        for kw in (dict(random_short_side=(32, 40)), dict(random_resized_crop=True)):
            with pytest.raises(E, match=r"per-clip geometry.*nearest, box, bilinear, bicubic"):
                TF.TransformFrames(OPTS, interpolation=f, **kw)
        with pytest.raises(E, match=r"per-clip geometry.*nearest, box, bilinear, bicubic"):
            TF.SampleClips(OPTS, interpolation=f)
        tf = TF.TransformFrames(OPTS, interpolation=f, random_crop=True, random_hflip=True)      # a fixed geometry: fine
        assert tf.frame_tables(48, 64)["rows"][2].shape[1] > 1
        with pytest.raises(E, match=r"geometry=.*nearest, box, bilinear, bicubic"):
            tf.check_geometry(rows, 1, 40, 40)
        with pytest.raises(E, match=r"geometry=.*nearest, box, bilinear, bicubic"):         # before a device is asked for
            tf(torch.zeros((1, 1, 40, 40, 3), dtype=torch.uint8), geometry=rows)
    for f in TF.DEVICE_INTERPOLATIONS:
        tf = TF.TransformFrames(OPTS, interpolation=f, random_resized_crop=True)
        assert torch.equal(tf.check_geometry(rows, 1, 40, 40), torch.tensor(rows, dtype=torch.int32))
        TF.SampleClips(OPTS, interpolation=f, random_short_side=(32, 48))
    assert TF.DEVICE_INTERPOLATIONS == ("nearest", "box", "bilinear", "bicubic")


def test_draws_do_not_depend_on_the_filter(ptx):
    TF = ptx.transforms
    kw = dict(random_crop=True, random_hflip=True, random_vflip=True)
    want = TF.TransformFrames(OPTS, generator=gen(7), **kw).draw(6, 90, 120)
    for f in FILTERS:
        assert torch.equal(TF.TransformFrames(OPTS, generator=gen(7), interpolation=f, **kw).draw(6, 90, 120), want), f
    for extra in (dict(random_short_side=(32, 48)), dict(random_resized_crop=True)):
        want = TF.TransformFrames(OPTS, generator=gen(8), **kw, **extra).draw_geometry(6, 90, 120) if "random_short_side" in extra else \
            TF.TransformFrames(OPTS, generator=gen(8), random_hflip=True, random_vflip=True, **extra).draw_geometry(6, 90, 120)
        for f in TF.DEVICE_INTERPOLATIONS:
            sw = dict(kw) if "random_short_side" in extra else dict(random_hflip=True, random_vflip=True)
            got = TF.TransformFrames(OPTS, generator=gen(8), interpolation=f, **sw, **extra).draw_geometry(6, 90, 120)
            assert torch.equal(got, want), (f, extra)
        shapes = [(20, 90, 120), (9, 64, 48)]
        sw = dict(random_hflip=True, **extra)
        idx, geo = TF.SampleClips(OPTS, num_frames=4, frame_stride=2, clips=2, generator=gen(9), **sw).draw(shapes)
        for f in TF.DEVICE_INTERPOLATIONS:
            i2, g2 = TF.SampleClips(OPTS, num_frames=4, frame_stride=2, clips=2, generator=gen(9), interpolation=f, **sw).draw(shapes)
            assert torch.equal(i2, idx) and torch.equal(g2, geo), (f, extra)


# --------------------------------------------------------------------------------------------- the C ABI
def test_resample_header_bindings_and_exports_agree(ptx):
    """The two builders live in include/ptx_amd_resample.h: that header, _lib.SIGNATURES_RESAMPLE and the library's exports
    name the same functions, disjoint from every other table, listed in INTEGRATION.md; the filter codes are Pillow's."""
    L = ptx._lib
    text = open(L.RESAMPLE_HEADER_PATH).read()
    declared = L.header_symbols(L.RESAMPLE_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_RESAMPLE) == NAMES
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.SIGNATURES_YUV16, L.SIGNATURES_COLOR,
                  L.SIGNATURES_RANDAUG, L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_RESAMPLE[name][0], list(L.SIGNATURES_RESAMPLE[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_RESAMPLE[name][1]), name
        twin = L.SIGNATURES[name[:-len("_filter")]]                                       # the bilinear twin + the filter code
        assert len(L.SIGNATURES_RESAMPLE[name][1]) == len(twin[1]) + 1 and L.SIGNATURES_RESAMPLE[name][1].count(C.c_int32) == 1
    for name, code in PIL_CODES.items():
        assert re.search(r"#define PTX_RESAMPLE_%s\s+%d\b" % (name.upper(), code), text) and getattr(L, "PTX_RESAMPLE_" + name.upper()) == code
        assert ptx.transforms.INTERPOLATIONS[code] == name
    assert re.search(r"#define PTX_RESAMPLE_NEAREST_MAX_EXTENT\s+65536\b", text) and L.PTX_RESAMPLE_NEAREST_MAX_EXTENT == 65536
    assert "MAY BE NEGATIVE" in text and "2^23" in text and "2^31" in text                  # the headers state the two bounds
    root = os.path.dirname(os.path.dirname(L.HEADER_PATH))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "ptx_amd_resample.h" in integ and all(n in integ for n in declared) and "### 1m." in integ
    assert "92 stable" in integ                                                             # ptx_amd.h's census does not move
    # the build: the header is hashed into the version and is a dependency of the object that holds the kernels
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert any(h.endswith("ptx_amd_resample.h") for h in build.HEADERS)
    assert any(p.endswith("ptx_amd_resample.h") for p in build.tu_files("pack_layout.hip"))
    assert L.binary_source_hash() == L.source_hash()


def test_builder_argument_checks_without_a_device(ptx):
    """Filter codes and null pointers are refused on the host, before any launch."""
    L = ptx._lib
    lib = L.lib()
    desc = L.ResizeDesc(1, 1, 40, 40, 3, 32, 32, 5, 5, L.PTX_RESIZE_OUT_U8)
    one = C.c_void_p(16)                                                                    # never dereferenced: the checks come first
    for name, lead in (("ptx_resize_build_tables_filter", [one]), ("ptx_resize_build_tables_clips_filter", [one, one])):
        fn = getattr(lib, name)
        for code, status, word in ((L.PTX_RESAMPLE_HAMMING, 2, "hamming"), (L.PTX_RESAMPLE_LANCZOS, 2, "lanczos"), (6, 1, "PTX_RESAMPLE"),
                                   (-1, 1, "PTX_RESAMPLE")):
            assert fn(C.byref(desc), *lead, code, one, one, one, one, one, one, None) == status
            msg = lib.ptx_last_error().decode()
            assert word in msg and name in msg
            if status == 2:
                assert "nearest, box, bilinear and bicubic" in msg
        for code in (L.PTX_RESAMPLE_NEAREST, L.PTX_RESAMPLE_BOX, L.PTX_RESAMPLE_BILINEAR, L.PTX_RESAMPLE_BICUBIC):
            assert fn(C.byref(desc), *lead, code, None, one, one, one, one, one, None) == 1
            assert "null pointer" in lib.ptx_last_error().decode()
