"""Host tests (no GPU) of the interpolated per-clip warps (include/ptx_amd_warp.h; `pretorched.transforms.warp_numpy`,
`RandAugment(interpolation=..)`, `RandomAffine`, `RandomRotation`, `RandomPerspective`): the numpy statement of the arithmetic
contract against Pillow's Image.transform / Image.rotate, bit for bit, on random and fixed coefficient sets; RandAugment's
numpy model with an interpolation against the Pillow chain; the draws of the three classes; the host-side check of the C ABI,
one case per refusal; the census of the header, the bindings and the exports; the unchanged default."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import warp_oracle as WO

from pretorched_x_amd.testing import synth_color_frames

NAMES = ["ptx_warp_frames", "ptx_warp_frames_supported"]
FILL = WO.FILL
COMBOS = [("bilinear", WO.AFFINE), ("bilinear", WO.PERSPECTIVE), ("bicubic", WO.AFFINE), ("bicubic", WO.PERSPECTIVE),
          ("nearest", WO.PERSPECTIVE)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------------------------- the contract against Pillow
@pytest.mark.parametrize("interpolation,kind", COMBOS)
def test_random_coefficients_equal_pillow(ptx, interpolation, kind):
    """52 coefficient sets on each of 1x1, 2x3, 9x11, 33x65: 208 per (filter, kind)."""
    TF = ptx.transforms
    total = 0
    for H, W in WO.SIZES:
        rng = np.random.default_rng(100 * H + W + kind)
        frame = synth_color_frames(1, 1, H, W, 7000 + H)[0, 0]
        for i in range(52):
            a = WO.random_coeffs(rng, kind, H, W)
            got = TF.warp_numpy(frame[None, None], [kind], [a], interpolation, FILL)[0, 0]
            assert np.array_equal(got, WO.pil_warp(frame, kind, a, interpolation)), (H, W, i, a)
            total += 1
    assert total >= 200


@pytest.mark.parametrize("H,W", WO.SIZES)
@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic", "nearest"])
def test_fixed_cases_equal_pillow(ptx, interpolation, H, W):
    TF = ptx.transforms
    frame = synth_color_frames(1, 1, H, W, 7100 + W)[0, 0]
    one = lambda kind, a: TF.warp_numpy(frame[None, None], [kind], [a], interpolation, FILL)[0, 0]
    for name, a in WO.fixed_affine(H, W):
        a = a + [0.0, 0.0]
        for kind in ((WO.PERSPECTIVE,) if interpolation == "nearest" else (WO.AFFINE, WO.PERSPECTIVE)):
            got = one(kind, a)
            assert np.array_equal(got, WO.pil_warp(frame, kind, a, interpolation)), (name, kind)
            if name == "identity":
                assert np.array_equal(got, frame)
            if name == "beyond":
                assert (got == np.array(FILL, np.uint8)).all()
    assert np.array_equal(one(WO.IDENTITY, [float("nan")] * 8), frame)
    a = WO.strong_perspective(H, W)
    assert np.array_equal(one(WO.PERSPECTIVE, a), WO.pil_warp(frame, WO.PERSPECTIVE, a, interpolation))
    if interpolation != "nearest":
        for r in WO.ROTATIONS + (360.0,):                          # Image.rotate itself, against its restated matrix
            assert np.array_equal(one(WO.AFFINE, TF.rotation_matrix(r, H, W) + [0.0, 0.0]), WO.pil_rotate(frame, r, interpolation)), r
        assert np.array_equal(one(WO.AFFINE, TF.rotation_matrix(33.0, H, W, (1.5, 0.25)) + [0.0, 0.0]),
                              WO.pil_rotate(frame, 33.0, interpolation, center=(1.5, 0.25)))
    assert TF.rotation_matrix(-29.5, H, W) == TF.rand_augment_matrix(5, -29.5, H, W)


@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic"])
def test_rand_augment_numpy_with_an_interpolation_equals_the_pillow_chain(ptx, interpolation):
    """Every op code at both signs, one op per call, on a non-square frame; then the three-op sets."""
    TF = ptx.transforms
    H, W = 20, 27
    frames = synth_color_frames(1, 2, H, W, 7200)
    for code in range(14):
        for neg in ((False, True) if TF.RANDAUG_SIGNED[code] else (False,)):
            mag = WO.MG.magnitude(code, 14, H, W, neg)
            p = (np.array([[code]], np.int32), np.array([[mag]]))
            assert np.array_equal(TF.rand_augment_numpy(frames, p, FILL, interpolation=interpolation),
                                  WO.pil_randaug_clips(frames, p[0], p[1], interpolation)), (code, neg)
            if code not in range(1, 6):
                assert np.array_equal(TF.rand_augment_numpy(frames, p, FILL, interpolation=interpolation), TF.rand_augment_numpy(frames, p, FILL))
    frames = synth_color_frames(2, 1, 32, 40, 7201)
    for codes, mags in WO.RANDAUG_SETS:
        assert np.array_equal(TF.rand_augment_numpy(frames, (codes, mags), FILL, interpolation=interpolation),
                              WO.pil_randaug_clips(frames, codes, mags, interpolation))


# --------------------------------------------------------------------------------------------- the default is unchanged
def test_default_rows_are_unchanged_and_the_plan_rewrites_geometric_rows(ptx):
    TF, L = ptx.transforms, ptx._lib
    a, b = TF.RandAugment(3, generator=gen(5)), TF.RandAugment(3, generator=gen(5), interpolation="nearest")
    assert a.interpolation == b.interpolation == "nearest"
    c = TF.RandAugment(3, generator=gen(5), interpolation=2)       # Pillow's code for bilinear
    assert c.interpolation == "bilinear"
    pa, pb, pc = a.draw(4, 32, 40), b.draw(4, 32, 40), c.draw(4, 32, 40)
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(pa, pb, pc))         # draws do not depend on the filter
    ra, rb = a._rows_for(4, 32, 40, pa), b._rows_for(4, 32, 40, pa)
    assert isinstance(ra, np.ndarray) and np.array_equal(ra, rb) and np.array_equal(ra, TF.rand_augment_rows(pa, 32, 40))
    for codes, mags in WO.RANDAUG_SETS:
        plan = c._rows_for(2, 32, 40, (codes, mags))
        geo = np.isin(codes, range(1, 6))
        assert (plan.rows[..., 0][geo] == L.PTX_RANDAUG_IDENTITY).all() and not plan.rows[geo].any()
        assert np.array_equal(plan.rows[~geo], TF.rand_augment_rows((codes, mags), 32, 40)[~geo])
        for k in range(3):
            if not geo[:, k].any():
                assert plan.warps[k] is None
                continue
            kinds, coeffs = plan.warps[k]
            assert kinds.tolist() == [L.PTX_WARP_AFFINE if g else L.PTX_WARP_IDENTITY for g in geo[:, k]] and coeffs.dtype == np.float64
            for n in np.nonzero(geo[:, k])[0]:
                assert coeffs[n].tolist() == TF.rand_augment_matrix(int(codes[n, k]), float(mags[n, k]), 32, 40) + [0.0, 0.0]


# --------------------------------------------------------------------------------------------- the draws
def test_draws_are_seeded_per_clip_and_follow_the_stated_order(ptx):
    TF, L = ptx.transforms, ptx._lib
    H, W = 19, 23
    mk = lambda s: TF.RandomAffine(25, translate=(0.1, 0.2), scale=(0.8, 1.25), shear=(-10, 10, -5, 5), interpolation="bilinear", generator=gen(s))
    k1, c1 = mk(3).draw(4, H, W)
    k2, c2 = mk(3).draw(4, H, W)
    assert torch.equal(k1, k2) and torch.equal(c1, c2) and not torch.equal(c1, mk(4).draw(4, H, W)[1])
    assert k1.dtype == torch.int32 and k1.tolist() == [L.PTX_WARP_AFFINE] * 4 and c1.shape == (4, 8) and c1.dtype == torch.float64
    assert len({tuple(r.tolist()) for r in c1}) == 4 and not c1[:, 6:].any()
    g = gen(3)                                                      # torchvision's get_params order, restated
    u = lambda lo, hi: float(torch.empty(1).uniform_(lo, hi, generator=g).item())
    for n in range(4):
        angle = u(-25.0, 25.0)
        tx, ty = int(round(u(-0.1 * W, 0.1 * W))), int(round(u(-0.2 * H, 0.2 * H)))
        scale, sx, sy = u(0.8, 1.25), u(-10.0, 10.0), u(-5.0, 5.0)
        assert c1[n, :6].tolist() == TF._inverse_affine_matrix((W * 0.5, H * 0.5), angle, (tx, ty), (sx, sy), scale)
    m1 = TF._inverse_affine_matrix((3.0, 4.0), 12.0, (1, -2), (5.0, -3.0))
    m2 = TF._inverse_affine_matrix((3.0, 4.0), 12.0, (1, -2), (5.0, -3.0), 2.0)
    rot, sx, sy = math.radians(12.0), math.radians(5.0), math.radians(-3.0)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    assert m1[0] == d and m2[0] == d / 2.0 and m2[4] == m1[4] / 2.0                       # scale divides the entries
    # rotation: one uniform per clip, about a centre
    rot = TF.RandomRotation((-40, 75), center=(2.0, 3.0), generator=gen(8))
    kr, cr = rot.draw(3, H, W)
    g = gen(8)
    for n in range(3):
        assert cr[n, :6].tolist() == TF.rotation_matrix(u(-40.0, 75.0), H, W, (2.0, 3.0))
    assert torch.equal(rot.draw(3, H, W)[1], cr) is False         # the generator moves on
    # perspective: the p gate, then eight integers
    per = TF.RandomPerspective(0.6, p=0.6, generator=gen(61))
    kp, cp = per.draw(4, H, W)
    assert per.interpolation == "bilinear" and set(kp.tolist()) == {L.PTX_WARP_IDENTITY, L.PTX_WARP_PERSPECTIVE}
    g = gen(61)
    ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g).item())
    hw, hh = int(0.6 * (W // 2)), int(0.6 * (H // 2))
    for n in range(4):
        if not bool(torch.rand(1, generator=g) < 0.6):
            assert kp[n] == L.PTX_WARP_IDENTITY and not cp[n].any()
            continue
        ends = [[ri(0, hw + 1), ri(0, hh + 1)], [ri(W - hw - 1, W), ri(0, hh + 1)], [ri(W - hw - 1, W), ri(H - hh - 1, H)],
                [ri(0, hw + 1), ri(H - hh - 1, H)]]
        a = cp[n].tolist()
        assert kp[n] == L.PTX_WARP_PERSPECTIVE and a == [float(np.float32(v)) for v in a]              # float32 values, widened
        for (ex, ey), (sx_, sy_) in zip(ends, [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]]):      # the quad maps to the corners
            den = a[6] * ex + a[7] * ey + 1.0
            assert abs((a[0] * ex + a[1] * ey + a[2]) / den - sx_) < 1e-3 and abs((a[3] * ex + a[4] * ey + a[5]) / den - sy_) < 1e-3
    assert TF.RandomPerspective(0.5, p=0.0).draw(3, H, W)[0].tolist() == [0, 0, 0]
    assert TF.RandomPerspective(0.5, p=1.0, generator=gen(1)).draw(3, H, W)[0].tolist() == [2, 2, 2]


def test_params_replay_and_validation_errors(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    aff = TF.RandomAffine(10, interpolation="bicubic", generator=gen(2))
    p = aff.draw(2, 9, 11)
    k, c = aff.check_params(p, 2, 9, 11)
    assert torch.equal(k, p[0]) and torch.equal(c, p[1])
    assert aff.check_params((p[0].numpy(), p[1].tolist()), 2, 9, 11)[1].dtype == torch.float64
    with pytest.raises(E, match="pair"):
        aff.check_params(5)
    with pytest.raises(E, match=r"\[N, 8\]"):
        aff.check_params((p[0], p[1][:, :6]))
    with pytest.raises(E, match="N = 3"):
        aff.check_params(p, 3)
    with pytest.raises(E, match="integers"):
        aff.check_params((p[0].double(), p[1]))
    with pytest.raises(E, match="out of range"):
        aff.check_params((torch.tensor([1, 7]), p[1]), 2, 9, 11)
    bad = p[1].clone()
    bad[1, 2] = float("inf")
    with pytest.raises(E, match="not finite"):
        aff.check_params((p[0], bad), 2, 9, 11)
    with pytest.raises(E, match="fixed-point"):                  # nearest affine goes PIL's fixed-point way, with its range
        TF.RandomAffine(10).check_params((p[0], p[1] * 1e6), 2, 9, 11)
    with pytest.raises(E, match="share a launch"):
        TF.RandomAffine(10).check_params((torch.tensor([1, 2]), p[1]), 2, 9, 11)
    degenerate = torch.tensor([[1.0, 0, 0, 0, 1, 0, -0.2, 0]], dtype=torch.float64)           # 1 - 0.2 X vanishes at X = 5
    with pytest.raises(E, match="degenerate"):
        TF.RandomPerspective().check_params((torch.tensor([2]), degenerate), 1, 9, 11)
    with pytest.raises(E, match="uint8 CUDA"):
        aff(torch.zeros(2, 1, 9, 11, 3, dtype=torch.uint8))
    with pytest.raises(E, match="expected"):
        aff(torch.zeros(9, 11, 4, dtype=torch.uint8))
    with pytest.raises(E, match="expand"):
        TF.RandomRotation(10, expand=True)
    for make in (lambda: TF.RandomAffine(-1), lambda: TF.RandomAffine((1, 2, 3)), lambda: TF.RandomAffine(5, translate=(0.5, 1.5)),
                 lambda: TF.RandomAffine(5, scale=(0.0, 1.0)), lambda: TF.RandomAffine(5, shear=(1, 2, 3)),
                 lambda: TF.RandomRotation("x"), lambda: TF.RandomRotation(5, center=(1,)), lambda: TF.RandomPerspective(1.5),
                 lambda: TF.RandomPerspective(0.5, p=-0.1), lambda: TF.RandomAffine(5, fill=300), lambda: TF.RandomRotation(5, generator=7)):
        with pytest.raises(E):
            make()


def test_the_three_other_filters_are_refused(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    for bad in ("lanczos", "box", "hamming", 1):
        for make in (lambda f: TF.RandAugment(interpolation=f), lambda f: TF.RandomAffine(5, interpolation=f),
                     lambda f: TF.RandomRotation(5, interpolation=f), lambda f: TF.RandomPerspective(interpolation=f),
                     lambda f: TF.warp_numpy(np.zeros((1, 1, 2, 2, 3), np.uint8), [0], np.zeros((1, 8)), f)):
            with pytest.raises(E, match="'nearest', 'bilinear' or 'bicubic'"):
                make(bad)
    with pytest.raises(E, match="interpolation must be one of"):
        TF.RandAugment(interpolation="cubic")
    assert TF.WARP_INTERPOLATIONS == ("nearest", "bilinear", "bicubic") and TF.WARP_KINDS == ("identity", "affine", "perspective")
    with pytest.raises(E, match="RandAugment"):                  # augment= keeps accepting RandAugment only
        TF.TransformFrames(dict(input_space="RGB", input_range=[0, 1], mean=[0.5] * 3, std=[0.5] * 3, input_size=[3, 8, 8]),
                           augment=TF.RandomAffine(5))


# --------------------------------------------------------------------------------------------- the C ABI
def test_warp_supported_refuses_each_documented_reason(ptx):
    L = ptx._lib
    lib = L.lib()
    kinds0 = np.array([0, 1, 2], np.int32)
    coeffs0 = np.array([[np.nan] * 8, [1, 0.1, 2, 0, 1, -1, np.inf, np.nan], [1, 0, 0, 0, 1, 0, 0.02, -0.03]], np.float64)

    def ok(desc, kinds=kinds0, coeffs=coeffs0):
        k = None if kinds is None else np.ascontiguousarray(kinds, np.int32)
        c = None if coeffs is None else np.ascontiguousarray(coeffs, np.float64)
        return lib.ptx_warp_frames_supported(C.byref(desc) if desc is not None else None, C.c_void_p(k.ctypes.data) if k is not None else None,
                                             C.c_void_p(c.ctypes.data) if c is not None else None)

    err = lambda: lib.ptx_last_error().decode()
    base = dict(N=3, T=2, H=9, W=11, filter=L.PTX_RESAMPLE_BILINEAR, fill_r=0, fill_g=128, fill_b=255, reserved=0)
    D = lambda **kw: L.WarpDesc(**dict(base, **kw))
    assert ok(D()) == 1 and ok(D(filter=L.PTX_RESAMPLE_BICUBIC)) == 1          # an identity row and a6, a7 of an affine row are not read
    assert ok(D(filter=L.PTX_RESAMPLE_NEAREST), kinds=[0, 2, 2], coeffs=coeffs0[[0, 2, 2]]) == 1
    assert ok(None) == 0 and "null" in err()
    assert ok(D(), kinds=None) == 0 and "null" in err() and ok(D(), coeffs=None) == 0 and "null" in err()
    for k in ("N", "T", "H", "W"):
        assert ok(D(**{k: 0})) == 0 and "non-positive" in err()
    assert ok(D(N=1, H=26760, W=26760)) == 0 and "32-bit" in err()             # 3 * 26760^2 >= 2^31
    assert ok(D(N=1, H=26754, W=26754), kinds=[0], coeffs=coeffs0[:1]) == 1
    assert ok(D(T=70000)) == 0 and "grid" in err()
    for f in (L.PTX_RESAMPLE_LANCZOS, L.PTX_RESAMPLE_BOX, L.PTX_RESAMPLE_HAMMING, 6, -1):
        assert ok(D(filter=f)) == 0 and "filter" in err()
    assert ok(D(fill_b=256)) == 0 and "fill" in err()
    assert ok(D(), kinds=[0, 3, 2]) == 0 and "kind 3" in err() and ok(D(), kinds=[-1, 1, 2]) == 0 and "kind -1" in err()
    assert ok(D(filter=L.PTX_RESAMPLE_NEAREST)) == 0 and "nearest affine" in err() and "ptx_rand_augment_apply" in err()
    for n, i in ((1, 0), (1, 5), (2, 3), (2, 7)):
        for v in (np.nan, np.inf, -np.inf):
            c = coeffs0.copy()
            c[n, i] = v
            assert ok(D(), coeffs=c) == 0 and "not finite" in err() and "clip %d" % n in err() and "a%d" % i in err()
    for a6, a7 in ((-1.0 / 5.0, 0.0), (0.0, -1.0 / 4.5), (-0.1, -0.02), (-2.0, 0.0), (0.0, -1.0 / 0.5)):
        c = coeffs0.copy()                                          # zero inside, at a corner centre, or a sign change
        c[2, 6:] = a6, a7
        assert ok(D(), coeffs=c) == 0 and "denominator" in err(), (a6, a7)
    c = coeffs0.copy()
    c[2, 6:] = -3.0, -3.0                                           # strictly negative on the whole frame: accepted
    assert ok(D(), coeffs=c) == 1


def test_warp_header_bindings_and_exports_agree(ptx):
    """The two calls live in include/ptx_amd_warp.h: that header, _lib.SIGNATURES_WARP and the library's exports name the same
    functions with the same argument counts, disjoint from every other table, listed in INTEGRATION.md; the ctypes mirror of
    the descriptor matches field for field; the build hashes the header and the kernel file."""
    L = ptx._lib
    text = open(L.WARP_HEADER_PATH).read()
    declared = L.header_symbols(L.WARP_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_WARP) == NAMES
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.SIGNATURES_YUV16, L.SIGNATURES_COLOR,
                  L.SIGNATURES_RANDAUG, L.SIGNATURES_RESAMPLE, L.SIGNATURES_MIX, L.SIGNATURES_STEM_STRIDED, L.SIGNATURES_NL_KS,
                  L.SIGNATURES_LINEAR_BF16, L.SIGNATURES_BN, L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd_resample.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_WARP[name][0], list(L.SIGNATURES_WARP[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_WARP[name][1]), name
    root = os.path.dirname(os.path.dirname(L.HEADER_PATH))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    assert "ptx_amd_warp.h" in integ and all(n in integ for n in declared) and "### 1p." in integ
    assert "92 stable" in integ                                                    # ptx_amd.h's census does not move
    body = re.search(r"typedef struct ptx_warp_desc \{(.*?)\}", plain, flags=re.S).group(1)
    fields = [n.strip() for line in body.split(";") for n in line.replace("int32_t", "").split(",") if n.strip()]
    assert fields == [n for n, _ in L.WarpDesc._fields_] and all(t is C.c_int32 for _, t in L.WarpDesc._fields_)
    assert C.sizeof(L.WarpDesc) == 36
    for code, name in enumerate(ptx.transforms.WARP_KINDS):
        assert re.search(r"#define PTX_WARP_%s\s+%d\b" % (name.upper(), code), text) and getattr(L, "PTX_WARP_" + name.upper()) == code
    assert re.search(r"#define PTX_WARP_COEFFS\s+8\b", text) and L.PTX_WARP_COEFFS == 8
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "warp_frames.h" in build.HEADERS and any(h.endswith("ptx_amd_warp.h") for h in build.HEADERS)
    files = build.tu_files("pack_layout.hip")
    assert any(p.endswith("warp_frames.h") for p in files) and any(p.endswith("ptx_amd_warp.h") for p in files)
    assert L.binary_source_hash() == L.source_hash()
