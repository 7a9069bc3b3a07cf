"""GPU tests of the interpolated per-clip warps (`ptx_warp_frames`, include/ptx_amd_warp.h; `RandAugment(interpolation=..)`,
`RandomAffine`, `RandomRotation`, `RandomPerspective`).  Every comparison is byte equality, no tolerance: per-frame Pillow
(tests/warp_oracle.py), the numpy statement of the contract (`warp_numpy`, `rand_augment_numpy`), `FramesToTensor` of the
augmented bytes for the plane outputs.  The direct launches read their source one byte past an allocation and write into a
buffer pre-filled with a sentinel, guard bytes on both sides included, all of which is compared."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import warp_oracle as WO

from pretorched_x_amd.testing import synth_color_frames, synth_frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB01 = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
OPTS = dict(RGB01, input_size=[3, 32, 32])
FILL = WO.FILL
SENTINEL, GUARD = 0xAA, 64
assert SENTINEL not in FILL


def gen(seed):
    return torch.Generator().manual_seed(seed)


def run_warp(ptx, frames, kinds, coeffs, interpolation, fill=FILL):
    """ptx_warp_frames through ctypes on numpy frames [N,T,H,W,3]: the source one byte past an allocation, the output between
    two guards in a buffer of sentinels.  Returns the whole output buffer as numpy."""
    L, TF = ptx._lib, ptx.transforms
    lib = L.lib()
    N, T, H, W, _ = frames.shape
    kinds, coeffs = np.ascontiguousarray(kinds, np.int32), np.ascontiguousarray(coeffs, np.float64)
    desc = L.WarpDesc(N, T, H, W, TF.INTERPOLATIONS.index(interpolation), fill[0], fill[1], fill[2], 0)
    assert lib.ptx_warp_frames_supported(C.byref(desc), C.c_void_p(kinds.ctypes.data), C.c_void_p(coeffs.ctypes.data)) == 1, \
        lib.ptx_last_error().decode()
    src = torch.zeros(frames.size + 1, dtype=torch.uint8, device=DEV)
    src[1:].copy_(torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)).to(DEV))
    assert src[1:].data_ptr() % 2 == 1
    buf = torch.full((frames.size + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    d_kinds, d_coeffs = torch.from_numpy(kinds).to(DEV), torch.from_numpy(coeffs.reshape(-1)).to(DEV)
    L.check(lib.ptx_warp_frames(C.byref(desc), C.c_void_p(src[1:].data_ptr()), C.c_void_p(d_kinds.data_ptr()),
                                C.c_void_p(d_coeffs.data_ptr()), C.c_void_p(buf[GUARD:].data_ptr()),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ptx_warp_frames")
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def guarded(want):
    g = np.full(GUARD, SENTINEL, np.uint8)
    return np.concatenate([g, want.reshape(-1), g])


# --------------------------------------------------------------------------------------------- 1. the kernel against Pillow
@pytest.mark.parametrize("H,W", WO.SIZES + [(64, 48)], ids=lambda v: str(v))
@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic", "nearest"])
def test_warp_frames_equals_pillow_per_frame(ptx, interpolation, H, W):
    """N = 4 clips, T = 2: identity, affine, perspective, affine with different coefficients (bilinear / affine, bilinear /
    perspective, bicubic / affine, bicubic / perspective); nearest, which takes no affine clip, runs identity and three
    perspectives (nearest / perspective), one of them the strong one.  33 x 65 and 64 x 48 cross the 32 x 8 tile in both axes."""
    rng = np.random.default_rng(1000 * H + W)
    frames = synth_color_frames(4, 2, H, W, 8100 + H)
    kinds = [WO.IDENTITY, WO.AFFINE, WO.PERSPECTIVE, WO.AFFINE] if interpolation != "nearest" else [WO.IDENTITY] + [WO.PERSPECTIVE] * 3
    coeffs = [WO.random_coeffs(rng, k, H, W) for k in kinds]
    coeffs[0] = [float("nan")] * 8                                   # an identity clip's coefficients are not read
    if interpolation == "nearest":
        coeffs[3] = WO.strong_perspective(H, W)
    want = WO.pil_warp_clips(frames, kinds, coeffs, interpolation)
    got = run_warp(ptx, frames, kinds, coeffs, interpolation)
    assert np.array_equal(got, guarded(want))
    assert np.array_equal(ptx.transforms.warp_numpy(frames, kinds, np.nan_to_num(np.array(coeffs)), interpolation, FILL), want)


@pytest.mark.parametrize("H,W", [(9, 11), (33, 65)], ids=lambda v: str(v))
@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic", "nearest"])
def test_fixed_cases_equal_pillow(ptx, interpolation, H, W):
    """One clip per fixed case: identity, integer and half-pixel translations, one beyond the frame (all fill), scales 0.35 and
    3.0, a shear, Image.rotate's matrices, each as an affine clip AND as a perspective one with a6 = a7 = 0 (the division by 1.0
    is exact), and the strong perspective whose denominator spans about 0.5 .. 1.5.  Nearest takes the perspective forms."""
    TF = ptx.transforms
    cases = [a + [0.0, 0.0] for _, a in WO.fixed_affine(H, W)] + [TF.rotation_matrix(r, H, W) + [0.0, 0.0] for r in WO.ROTATIONS]
    kinds = ([] if interpolation == "nearest" else [WO.AFFINE] * len(cases)) + [WO.PERSPECTIVE] * (len(cases) + 1)
    coeffs = ([] if interpolation == "nearest" else cases) + cases + [WO.strong_perspective(H, W)]
    frames = synth_color_frames(len(kinds), 1, H, W, 8200 + H)
    want = WO.pil_warp_clips(frames, kinds, coeffs, interpolation)
    beyond = [a[2] == float(W + 5) for a in coeffs]
    assert any(beyond) and all((want[i] == np.array(FILL, np.uint8)).all() for i, b in enumerate(beyond) if b)
    if interpolation != "nearest":                                   # Image.rotate itself gives what its matrix gives
        for i, r in enumerate(WO.ROTATIONS):
            assert np.array_equal(want[len(WO.fixed_affine(H, W)) + i, 0], WO.pil_rotate(frames[len(WO.fixed_affine(H, W)) + i, 0], r, interpolation))
    assert np.array_equal(run_warp(ptx, frames, kinds, coeffs, interpolation), guarded(want))


# --------------------------------------------------------------------------------------------- 2. RandAugment(interpolation=)
@functools.lru_cache(None)
def ra_frames():
    return synth_color_frames(2, 2, 32, 40, 8300)


@pytest.mark.parametrize("which", range(len(WO.RANDAUG_SETS)))
@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic"])
def test_rand_augment_with_an_interpolation(ptx, interpolation, which):
    TF = ptx.transforms
    codes, mags = WO.RANDAUG_SETS[which]
    frames = ra_frames()
    ra = TF.RandAugment(num_ops=3, fill=FILL, interpolation=interpolation)
    y = ra(torch.from_numpy(frames).to(DEV), params=(codes, mags))
    assert ra.last_launches == WO.randaug_launches(codes)
    assert [i for i, s in enumerate(ra.last_launches) if s == "warp"] == \
        [i for i, s in enumerate(WO.randaug_launches(codes)) if s == "warp"] and ra.last_launches.count("warp") == \
        sum(bool(np.isin(codes[:, k], range(1, 6)).any()) for k in range(3))
    assert np.array_equal(y.cpu().numpy(), TF.rand_augment_numpy(frames, (codes, mags), FILL, interpolation=interpolation))
    assert np.array_equal(y.cpu().numpy(), WO.pil_randaug_clips(frames, codes, mags, interpolation))


def test_default_path_is_unchanged(ptx):
    """RandAugment() and RandAugment(interpolation="nearest") give the same bytes from the same launches, none of them a warp,
    and those bytes are the nearest contract's."""
    TF = ptx.transforms
    frames = ra_frames()
    dev = torch.from_numpy(frames).to(DEV)
    for codes, mags in WO.RANDAUG_SETS:
        a, b = TF.RandAugment(3, fill=FILL), TF.RandAugment(3, fill=FILL, interpolation="nearest")
        ya, yb = a(dev, params=(codes, mags)), b(dev, params=(codes, mags))
        assert torch.equal(ya, yb) and a.last_launches == b.last_launches and "warp" not in a.last_launches
        assert a.last_launches == tuple(s for k in range(3) for s in ((("stats",) if np.isin(codes[:, k], (8, 12, 13)).any() else ()) + ("apply",)))
        assert np.array_equal(ya.cpu().numpy(), TF.rand_augment_numpy(frames, (codes, mags), FILL))
    d0, d1 = TF.RandAugment(3, generator=gen(7)), TF.RandAugment(3, generator=gen(7), interpolation="bicubic")
    d0(dev), d1(dev)
    assert all(torch.equal(p, q) for p, q in zip(d0.last_params, d1.last_params))          # the draws do not depend on the filter


# --------------------------------------------------------------------------------------------- 3. pipeline outputs
AUG = (np.array([[5, 8], [1, 0]], np.int32), np.array([[20.0, 0.4], [-0.2, 0.0]]))
AUG_LAST = (np.array([[8, 5], [0, 3]], np.int32), np.array([[0.4, -20.0], [0.0, 5.0]]))


@functools.lru_cache(None)
def raw_frames():
    return torch.from_numpy(synth_frames(2 * 4, 60, 80, 4300).reshape(2, 4, 60, 80, 3)).to(DEV)


@pytest.mark.parametrize("params", [AUG, AUG_LAST], ids=["warp-first", "warp-last"])
def test_transform_frames_outputs_with_a_bilinear_augment(ptx, params):
    TF = ptx.transforms
    raw = raw_frames()
    kw = dict(random_resized_crop=True, random_hflip=True)
    ra = TF.RandAugment(2, 12, fill=5, interpolation="bilinear")
    tf = TF.TransformFrames(OPTS, out="frames", generator=gen(12), augment=ra, **kw)
    frames = tf(raw, augment_params=params)
    geo = tf.last_geometry
    assert "warp" in ra.last_launches
    plain = TF.TransformFrames(OPTS, out="frames", **kw)(raw, geometry=geo)
    assert np.array_equal(frames.cpu().numpy(), TF.rand_augment_numpy(plain.cpu().numpy(), params, 5, interpolation="bilinear"))
    for dtype in (torch.float32, torch.bfloat16):
        t = TF.TransformFrames(OPTS, dtype=dtype, augment=ra, **kw)(raw, geometry=geo, augment_params=params)
        want = TF.FramesToTensor(OPTS)(frames)
        assert t.dtype == dtype and torch.equal(t, want if dtype == torch.float32 else want.to(torch.bfloat16))


def test_sample_clips_outputs_with_a_bilinear_augment(ptx):
    TF = ptx.transforms
    videos = [torch.from_numpy(synth_frames(12, 60, 80, 4310)).to(DEV), torch.from_numpy(synth_frames(9, 50, 44, 4311)).to(DEV)]
    kw = dict(num_frames=4, frame_stride=2, clips=1, random_resized_crop=True, random_hflip=True)
    ra = TF.RandAugment(2, 12, interpolation="bilinear")
    sc = TF.SampleClips(OPTS, out="frames", generator=gen(22), augment=ra, **kw)
    frames = sc(videos, augment_params=AUG)
    assert frames.shape == (2, 4, 32, 32, 3) and "warp" in ra.last_launches
    plain = TF.SampleClips(OPTS, out="frames", **kw)(videos, indices=sc.last_indices, geometry=sc.last_geometry)
    assert np.array_equal(frames.cpu().numpy(), TF.rand_augment_numpy(plain.cpu().numpy(), AUG, 0, interpolation="bilinear"))
    for dtype in (torch.float32, torch.bfloat16):
        t = TF.SampleClips(OPTS, dtype=dtype, augment=ra, **kw)(videos, indices=sc.last_indices, geometry=sc.last_geometry, augment_params=AUG)
        want = TF.FramesToTensor(OPTS)(frames)
        assert torch.equal(t, want if dtype == torch.float32 else want.to(torch.bfloat16))


# --------------------------------------------------------------------------------------------- 4. the three classes
def make(TF, name, interpolation, seed):
    if name == "affine":
        return TF.RandomAffine(25, translate=(0.1, 0.2), scale=(0.8, 1.25), shear=(-10, 10, -5, 5), interpolation=interpolation, fill=FILL,
                               generator=gen(seed))
    if name == "rotation":
        return TF.RandomRotation(40, interpolation=interpolation, center=(7.5, 11.0), fill=FILL, generator=gen(seed))
    return TF.RandomPerspective(0.6, p=0.6, interpolation=interpolation, fill=FILL, generator=gen(seed))


@pytest.mark.parametrize("interpolation", ["bilinear", "bicubic"])
@pytest.mark.parametrize("name", ["affine", "rotation", "perspective"])
def test_classes_equal_pillow_on_their_draw_and_replay(ptx, name, interpolation):
    TF = ptx.transforms
    frames = synth_color_frames(4, 2, 19, 23, 8400)
    dev = torch.from_numpy(frames).to(DEV)
    tr = make(TF, name, interpolation, 61)
    y = tr(dev)
    kinds, coeffs = tr.last_params
    assert tr.last_launches == ("warp",) and kinds.shape == (4,) and coeffs.shape == (4, 8) and coeffs.dtype == torch.float64
    assert len({tuple(c.tolist()) for c in coeffs}) > 1                                    # one draw per clip
    if name == "perspective":
        assert set(kinds.tolist()) == {WO.IDENTITY, WO.PERSPECTIVE}                        # the p gate, both ways, at this seed
    assert np.array_equal(y.cpu().numpy(), WO.pil_warp_clips(frames, kinds.numpy(), coeffs.numpy(), interpolation))
    other = make(TF, name, interpolation, 999)
    assert torch.equal(other(dev, params=(kinds, coeffs)), y) and other.last_params is None        # a replay, byte for byte
    one = tr(dev[2], params=(kinds[2:3], coeffs[2:3]))
    assert one.shape == dev[2].shape and torch.equal(one, y[2])
    assert tr(dev[0, 0]).shape == (19, 23, 3) and tr.last_params[0].shape == (1,)


def test_nearest_rotation_and_affine_run_pils_fixed_point_walk(ptx):
    TF = ptx.transforms
    frames = synth_color_frames(3, 2, 19, 23, 8500)
    dev = torch.from_numpy(frames).to(DEV)
    rot = TF.RandomRotation((-40, 75), fill=FILL, generator=gen(62))
    y = rot(dev)
    assert rot.interpolation == "nearest" and rot.last_launches == ("apply",)
    g = gen(62)
    angles = [float(torch.empty(1).uniform_(-40.0, 75.0, generator=g).item()) for _ in range(3)]    # the stated draw
    assert len(set(angles)) == 3
    for n in range(3):
        for t in range(2):
            assert np.array_equal(y[n, t].cpu().numpy(), WO.pil_rotate(frames[n, t], angles[n], "nearest")), (n, t)
    aff = make(TF, "affine", "nearest", 63)
    ya = aff(dev)
    kinds, coeffs = aff.last_params
    assert aff.last_launches == ("apply",)
    assert np.array_equal(ya.cpu().numpy(), WO.pil_warp_clips(frames, kinds.numpy(), coeffs.numpy(), "nearest"))
    per = make(TF, "perspective", "nearest", 61)                       # a nearest perspective is the warp kernel's
    yp = per(dev)
    assert per.last_launches == ("warp",)
    assert np.array_equal(yp.cpu().numpy(), WO.pil_warp_clips(frames, per.last_params[0].numpy(), per.last_params[1].numpy(), "nearest"))
