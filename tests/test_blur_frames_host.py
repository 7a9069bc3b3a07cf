"""Host tests (no GPU) of the per-clip GaussianBlur (include/ptx_amd_blur.h; `pretorched.transforms.gaussian_kernel1d`,
`gaussian_blur_numpy`, `GaussianBlur`, `TransformFrames(.., blur=)`): torchvision's weights bit for bit; the numpy statement of
the arithmetic contract against a torch restatement of torchvision's fp32 conv2d route, which may differ by one level next to a
tie and nowhere else; identities; the draws; every argument error; the host-side check of the C ABI, one case per refusal; the
census of the header, the bindings and the exports."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def gen(seed):
    return torch.Generator().manual_seed(seed)


# --------------------------------------------------------------------------------------------- 1. the weights
@pytest.mark.parametrize("k", [1, 3, 9, 23])
def test_gaussian_kernel1d_is_torchvisions_bits(ptx, k):
    TF = ptx.transforms
    for sigma in (0.1, 0.37, 1.0, 1.5, 2.0, float(np.float32(0.73219))):
        half = (k - 1) * 0.5
        x = torch.linspace(-half, half, steps=k, dtype=torch.float32)
        pdf = torch.exp(-0.5 * (x / sigma).pow(2))
        want = pdf / pdf.sum()
        got = TF.gaussian_kernel1d(k, sigma)
        assert got.dtype == torch.float32 and got.shape == (k,) and torch.equal(got, want)
        if 0.5 * (half / sigma) ** 2 < 87.0:                        # exp() of the farthest tap is a normal fp32 number: positive
            assert bool((got > 0).all())
        assert bool((got >= 0).all()) and abs(float(got.double().sum()) - 1.0) < 1e-6          # (a far tap of a narrow sigma underflows to 0)
        assert torch.equal(got, got.flip(0))
    assert bool((TF.gaussian_kernel1d(k, 2.0) > 0).all())
    for bad in (0, 2, -3, 1.0, True):
        with pytest.raises(ptx._lib.PtxError, match="odd"):
            TF.gaussian_kernel1d(bad, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ptx._lib.PtxError, match="sigma"):
            TF.gaussian_kernel1d(3, bad)


# --------------------------------------------------------------------------------------------- 2. against torchvision's route
def torchvision_blur(img, wx, wy):
    """torchvision's F_t.gaussian_blur on a uint8 HWC image, restated: the fp32 2-D kernel mm(wy[:, None], wx[None, :]), reflect
    padding, a depthwise conv2d, torch.round, the cast back."""
    kx, ky = wx.shape[0], wy.shape[0]
    kernel = torch.mm(wy[:, None], wx[None, :]).expand(3, 1, ky, kx)
    x = torch.from_numpy(img).permute(2, 0, 1)[None].to(torch.float32)
    x = F.pad(x, [kx // 2, kx // 2, ky // 2, ky // 2], mode="reflect")
    y = torch.round(F.conv2d(x, kernel, groups=3)).to(torch.uint8)
    return y[0].permute(1, 2, 0).numpy()


@functools.lru_cache(None)
def tv_cases():
    """40 random and box-smoothed images of 40-46 x 48-52, k cycling through 3, 5, 9, 23, sigma ~ U(0.1, 2), seed 0."""
    rng = np.random.default_rng(0)
    cases = []
    for i in range(40):
        H, W = 40 + i % 7, 48 + i % 5
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        if i % 2:                                                   # box-smoothed: neighbouring values close, as in a photograph
            x = torch.from_numpy(img).permute(2, 0, 1)[None].float()
            x = F.avg_pool2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), 5, 1)
            img = np.ascontiguousarray(x.round().clamp(0, 255).to(torch.uint8)[0].permute(1, 2, 0).numpy())
        cases.append((img, (3, 5, 9, 23)[i % 4], float(rng.uniform(0.1, 2.0))))
    return cases


def test_numpy_contract_differs_from_torchvisions_route_next_to_ties_only(ptx):
    TF = ptx.transforms
    total = differing = 0
    worst = 0.0
    for img, k, sigma in tv_cases():
        w = TF.gaussian_kernel1d(k, sigma)
        out, v = TF.gaussian_blur_numpy(img[None, None], [1], w.numpy(), w.numpy(), return_real=True)
        assert np.array_equal(out, TF.gaussian_blur_numpy(img[None, None], [1], w.numpy(), w.numpy()))
        d = torchvision_blur(img, w, w).astype(np.int32) - out[0, 0].astype(np.int32)
        bad = d != 0
        total += d.size
        differing += int(bad.sum())
        if bad.any():
            assert np.abs(d[bad]).max() == 1                        # one level
            r = v[0, 0][bad]
            worst = max(worst, float(np.abs(r - np.floor(r) - 0.5).max()))
    print("samples %d, differing %d (share %.3g), farthest from a tie %.3g" % (total, differing, differing / total, worst))
    assert total > 250000
    assert worst < 2e-4
    assert differing / total <= 2e-4


# --------------------------------------------------------------------------------------------- 3. - 5. identities and axes
def test_one_tap_and_apply_zero_are_the_identity(ptx):
    TF = ptx.transforms
    frames = np.random.default_rng(1).integers(0, 256, (3, 2, 7, 9, 3), dtype=np.uint8)
    one = np.ones((3, 1), np.float32)
    assert np.array_equal(TF.gaussian_blur_numpy(frames, [1, 1, 1], one, one), frames)
    w = TF.gaussian_kernel1d(5, 1.0).numpy()
    out, v = TF.gaussian_blur_numpy(frames, [0, 1, 0], w, w, return_real=True)
    assert np.array_equal(out[[0, 2]], frames[[0, 2]]) and not np.array_equal(out[1], frames[1])
    assert np.array_equal(v[0], frames[0].astype(np.float64))
    gb = TF.GaussianBlur(1, sigma=1.0)
    assert torch.equal(gb.weights(gb.draw(2))[0], torch.ones(2, 1)) and gb.kernel_size == (1, 1)


def test_a_constant_image_stays_constant(ptx):
    TF = ptx.transforms
    for value in (0, 1, 127, 200, 255):
        frames = np.full((1, 1, 12, 14, 3), value, np.uint8)
        for k, sigma in ((3, 0.1), (9, 2.0), (23, 1.3)):
            wy = TF.gaussian_kernel1d(k, sigma).numpy()
            wx = TF.gaussian_kernel1d(min(k, 9), sigma).numpy()
            assert np.array_equal(TF.gaussian_blur_numpy(frames, [1], wx, wy), frames), (value, k, sigma)


def test_unequal_sizes_blur_their_own_axes_and_an_impulse_gives_the_outer_product(ptx):
    TF = ptx.transforms
    H, W, kx, ky = 21, 25, 9, 3
    wx, wy = TF.gaussian_kernel1d(kx, 1.7).numpy(), TF.gaussian_kernel1d(ky, 0.6).numpy()
    frames = np.zeros((1, 1, H, W, 3), np.uint8)
    frames[0, 0, 10, 12] = (255, 100, 7)
    out = TF.gaussian_blur_numpy(frames, [1], wx, wy)[0, 0]
    for ch, amp in enumerate((255, 100, 7)):
        want = np.zeros((H, W))
        h = np.float64(amp) * wx.astype(np.float64)                 # the impulse's row after the horizontal pass
        want[10 - ky // 2:10 + ky // 2 + 1, 12 - kx // 2:12 + kx // 2 + 1] = wy.astype(np.float64)[:, None] * h[None, :]
        assert np.array_equal(out[..., ch], np.rint(want).astype(np.uint8)), ch
    nz = np.argwhere(out[..., 0])
    assert nz[:, 1].max() - nz[:, 1].min() > nz[:, 0].max() - nz[:, 0].min()      # wider than tall: kx runs along W
    assert nz[:, 0].min() >= 10 - ky // 2 and nz[:, 0].max() <= 10 + ky // 2
    # reflect padding: an impulse in the corner folds back onto itself
    frames = np.zeros((1, 1, 5, 6, 3), np.uint8)
    frames[0, 0, 0, 0] = 255
    w3 = np.array([0.25, 0.5, 0.25], np.float32)
    out = TF.gaussian_blur_numpy(frames, [1], w3, w3)[0, 0, :, :, 0]
    assert out[0, 0] == 64 and out[0, 1] == 32 and out[1, 1] == 16 and out[0, 2] == 0          # 0.25 * 255 = 63.75; row 1 sees row 0 once
    a, b = TF.GaussianBlur((9, 3)), TF.GaussianBlur([9, 3])
    assert a.kernel_size == b.kernel_size == (9, 3)


# --------------------------------------------------------------------------------------------- 6. the draws
def test_draws_follow_the_stated_sequence(ptx):
    TF = ptx.transforms
    gb = TF.GaussianBlur(9, sigma=(0.1, 2.0), p=0.5, generator=gen(7))
    apply, sigma = gb.draw(8)
    assert apply.dtype == torch.int32 and sigma.dtype == torch.float64 and apply.shape == sigma.shape == (8,)
    g = gen(7)
    for n in range(8):
        if bool(torch.rand(1, generator=g) <= 0.5):
            assert apply[n] == 1 and float(sigma[n]) == torch.empty(1).uniform_(0.1, 2.0, generator=g).item()
        else:
            assert apply[n] == 0 and float(sigma[n]) == 0.0
    assert 0 < int(apply.sum()) < 8
    # the generator is where the restated sequence left it
    assert torch.equal(torch.rand(3, generator=g), torch.rand(3, generator=gb.generator))
    # p=None: one draw per clip, all blurred
    always = TF.GaussianBlur(5, generator=gen(8))
    apply, sigma = always.draw(4)
    g = gen(8)
    assert apply.tolist() == [1] * 4 and sigma.tolist() == [torch.empty(1).uniform_(0.1, 2.0, generator=g).item() for _ in range(4)]
    assert torch.equal(torch.rand(2, generator=g), torch.rand(2, generator=always.generator))
    # scalar sigma: nothing is consumed
    fixed = TF.GaussianBlur(5, sigma=1.5, generator=gen(9))
    apply, sigma = fixed.draw(3)
    assert apply.tolist() == [1] * 3 and sigma.tolist() == [1.5] * 3
    assert torch.equal(torch.rand(2, generator=gen(9)), torch.rand(2, generator=fixed.generator))
    gate = TF.GaussianBlur(5, sigma=1.5, p=0.3, generator=gen(10))          # the gate alone
    g = gen(10)
    assert gate.draw(6)[0].tolist() == [int(bool(torch.rand(1, generator=g) <= 0.3)) for _ in range(6)]
    assert TF.GaussianBlur(5, p=0.0, generator=gen(1)).draw(4)[0].tolist() == [0] * 4
    assert TF.GaussianBlur(5, p=1.0, generator=gen(1)).draw(4)[0].tolist() == [1] * 4
    # a seed reproduces the draw; the weights are torchvision's for the drawn sigma
    a, b = TF.GaussianBlur(9, p=0.5, generator=gen(11)), TF.GaussianBlur(9, p=0.5, generator=gen(11))
    pa, pb = a._params_for(5, 16, 16, None), b._params_for(5, 16, 16, None)
    assert torch.equal(pa[0], pb[0]) and torch.equal(pa[1], pb[1]) and torch.equal(a.last_params[1], pa[1])
    wx, wy = a.weights(pa)
    for n in range(5):
        want = TF.gaussian_kernel1d(9, float(pa[1][n])) if pa[0][n] else torch.eye(9)[4]
        assert torch.equal(wx[n], want) and torch.equal(wy[n], want)
    # params= replay draws nothing
    state = a.generator.get_state()
    again = a._params_for(5, 16, 16, (pa[0].numpy(), pa[1].tolist()))
    assert torch.equal(again[0], pa[0]) and torch.equal(again[1], pa[1]) and torch.equal(a.generator.get_state(), state)
    assert a.last_params[1] is not again[1] and torch.equal(a.last_params[1], pa[1])


# --------------------------------------------------------------------------------------------- 7. argument errors
def test_every_argument_error_raises_before_a_device_is_touched(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    for make in (lambda: TF.GaussianBlur(4), lambda: TF.GaussianBlur(0), lambda: TF.GaussianBlur(35), lambda: TF.GaussianBlur((3, 4)),
                 lambda: TF.GaussianBlur((3, 3, 3)), lambda: TF.GaussianBlur(3.0), lambda: TF.GaussianBlur("3"), lambda: TF.GaussianBlur(True)):
        with pytest.raises(E, match="kernel_size"):
            make()
    for make in (lambda: TF.GaussianBlur(3, sigma=0), lambda: TF.GaussianBlur(3, sigma=-1.0), lambda: TF.GaussianBlur(3, sigma=(2.0, 0.1)),
                 lambda: TF.GaussianBlur(3, sigma=(0.0, 1.0)), lambda: TF.GaussianBlur(3, sigma=(1.0, float("inf"))),
                 lambda: TF.GaussianBlur(3, sigma="x"), lambda: TF.GaussianBlur(3, sigma=(1, 2, 3)), lambda: TF.GaussianBlur(3, sigma=True)):
        with pytest.raises(E, match="sigma"):
            make()
    for bad in (-0.1, 1.5, "p", True):
        with pytest.raises(E, match="probability"):
            TF.GaussianBlur(3, p=bad)
    with pytest.raises(E, match="generator"):
        TF.GaussianBlur(3, generator=7)
    gb = TF.GaussianBlur((5, 13), generator=gen(3))
    p = gb.draw(3)
    assert all(torch.equal(a, b) for a, b in zip(gb.check_params(p, 3, 7, 9), p))
    with pytest.raises(E, match="pair"):
        gb.check_params(5)
    with pytest.raises(E, match="N = 2"):
        gb.check_params(p, 2)
    with pytest.raises(E, match="integers"):
        gb.check_params((p[0].double(), p[1]))
    with pytest.raises(E, match="like apply"):
        gb.check_params((p[0], p[1][:2]))
    with pytest.raises(E, match="0 or 1"):
        gb.check_params((torch.tensor([1, 2, 0]), p[1]))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(E, match="sigma must be finite"):
            gb.check_params((p[0], torch.tensor([1.0, bad, 1.0], dtype=torch.float64)))
    assert gb.check_params(([1, 0, 1], [1.0, float("nan"), 1.0]))[1].tolist() == [1.0, 0.0, 1.0]      # not read where apply is 0
    with pytest.raises(E, match="empty"):
        gb.check_params((np.zeros(0, np.int32), np.zeros(0)))
    # the reflect condition names kernel_size, H and W
    for H, W in ((6, 9), (7, 2)):
        with pytest.raises(E, match=r"kernel_size=\(5, 13\).*H=%d, W=%d" % (H, W)):
            gb.check_params(p, 3, H, W)
        with pytest.raises(E, match=r"kernel_size=\(5, 13\).*H=%d, W=%d" % (H, W)):
            gb(torch.zeros(3, 2, H, W, 3, dtype=torch.uint8))
    with pytest.raises(E, match="uint8 CUDA"):
        gb(torch.zeros(3, 2, 7, 9, 3, dtype=torch.uint8))
    with pytest.raises(E, match="uint8 CUDA"):
        gb(np.zeros((3, 2, 7, 9, 3), np.uint8))
    with pytest.raises(E, match="expected"):
        gb(torch.zeros(7, 9, 4, dtype=torch.uint8))
    with pytest.raises(E, match="empty"):
        gb(torch.zeros(0, 2, 7, 9, 3, dtype=torch.uint8))
    with pytest.raises(E, match="N = 3"):
        gb(torch.zeros(3, 2, 7, 9, 3, dtype=torch.uint8), params=([1], [1.0]))
    # the numpy statement refuses what the launch refuses
    w = np.array([0.25, 0.5, 0.25], np.float32)
    f = np.zeros((1, 1, 4, 4, 3), np.uint8)
    with pytest.raises(E, match="uint8"):
        TF.gaussian_blur_numpy(f.astype(np.float32), [1], w, w)
    with pytest.raises(E, match="apply"):
        TF.gaussian_blur_numpy(f, [1, 1], w, w)
    with pytest.raises(E, match="0 or 1"):
        TF.gaussian_blur_numpy(f, [2], w, w)
    with pytest.raises(E, match="finite and >= 0"):
        TF.gaussian_blur_numpy(f, [1], np.array([-0.25, 1.0, 0.25], np.float32), w)
    with pytest.raises(E, match="odd"):
        TF.gaussian_blur_numpy(f, [1], w[:2], w)
    with pytest.raises(E, match="float32 values"):
        TF.gaussian_blur_numpy(f, [1], np.array([0.1, 0.8, 0.1]), w)
    with pytest.raises(E, match="H=4, W=4"):
        TF.gaussian_blur_numpy(f, [1], np.full(9, 1 / 9, np.float32), w)


def test_blur_supported_refuses_each_documented_reason(ptx):
    L = ptx._lib
    lib = L.lib()
    apply0 = np.array([1, 0, 1], np.int32)

    def ok(desc, apply=apply0, wx=None, wy=None):
        kx, ky = (desc.kx, desc.ky) if desc is not None else (3, 3)
        a = None if apply is None else np.ascontiguousarray(apply, np.int32)
        x = np.full((3, max(kx, 1)), 0.2, np.float32) if wx is None else (None if wx is False else np.ascontiguousarray(wx, np.float32))
        y = np.full((3, max(ky, 1)), 0.2, np.float32) if wy is None else (None if wy is False else np.ascontiguousarray(wy, np.float32))
        ptr = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
        return lib.ptx_gaussian_blur_supported(C.byref(desc) if desc is not None else None, ptr(a), ptr(x), ptr(y))

    err = lambda: lib.ptx_last_error().decode()
    base = dict(N=3, T=2, H=9, W=11, kx=5, ky=3, out_mode=L.PTX_RESIZE_OUT_U8)
    D = lambda **kw: L.BlurDesc(**dict(base, **kw))
    assert ok(D()) == 1 and ok(D(out_mode=L.PTX_RESIZE_OUT_F32)) == 1 and ok(D(out_mode=L.PTX_RESIZE_OUT_BF16)) == 1
    assert ok(D(kx=1, ky=1)) == 1 and ok(D(kx=L.PTX_BLUR_MAX_TAPS, ky=17, H=9, W=17)) == 1 and L.PTX_BLUR_MAX_TAPS >= 33
    assert ok(None) == 0 and "null" in err()
    assert ok(D(), apply=None) == 0 and "null" in err()
    assert ok(D(), wx=False) == 0 and "null" in err() and ok(D(), wy=False) == 0 and "null" in err()
    for k in ("N", "T", "H", "W"):
        assert ok(D(**{k: 0})) == 0 and "non-positive" in err()
        assert ok(D(**{k: -2})) == 0 and "non-positive" in err()
    for kw in (dict(kx=4), dict(ky=2), dict(kx=0), dict(ky=-3), dict(kx=L.PTX_BLUR_MAX_TAPS + 2, W=64), dict(ky=L.PTX_BLUR_MAX_TAPS + 2, H=64)):
        assert ok(D(**kw)) == 0 and "odd" in err() and "PTX_BLUR_MAX_TAPS" in err(), kw
    assert ok(D(kx=23, W=11)) == 0 and "reflect" in err()           # kx / 2 = 11 = W
    assert ok(D(kx=21, W=11)) == 1                                  # kx / 2 = 10 = W - 1
    assert ok(D(ky=19, H=9)) == 0 and "reflect" in err() and ok(D(ky=17, H=9)) == 1
    for flag in (2, -1):
        assert ok(D(), apply=[1, flag, 0]) == 0 and "clip 1" in err() and "0 or 1" in err()
    for bad in (-1e-6, np.nan, np.inf, -np.inf):
        wx = np.full((3, 5), 0.2, np.float32)
        wx[2, 4] = bad
        assert ok(D(), wx=wx) == 0 and "wx[4]" in err() and "clip 2" in err()
        wy = np.full((3, 3), 0.2, np.float32)
        wy[0, 1] = bad
        assert ok(D(), wy=wy) == 0 and "wy[1]" in err() and "clip 0" in err()
    for mode in (3, -1):
        assert ok(D(out_mode=mode)) == 0 and "out_mode" in err()
    assert ok(D(N=1, H=26760, W=26760), apply=[1]) == 0 and "32-bit" in err()      # 3 * 26760^2 >= 2^31
    assert ok(D(N=1, H=26754, W=26754), apply=[1]) == 1
    assert ok(D(T=70000)) == 0 and "grid" in err()
    # the launch checks the descriptor and its pointers before it touches a device
    bad = lib.ptx_gaussian_blur_frames(C.byref(D(kx=4)), None, None, None, None, None, None, None)
    assert bad == 1 and "odd" in err()
    assert lib.ptx_gaussian_blur_frames(C.byref(D()), None, None, None, None, None, None, None) == 1 and "null" in err()
    buf = np.zeros(4096, np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.ptx_gaussian_blur_frames(C.byref(D()), p, p, p, p, p, None, None) == 1 and "must not be frames" in err()


# --------------------------------------------------------------------------------------------- 8. the census
def test_blur_header_bindings_and_exports_agree(ptx):
    """The two calls live in include/ptx_amd_blur.h: that header, _lib.SIGNATURES_BLUR and the library's exports name the same
    functions with the same argument counts, disjoint from every other table, listed in INTEGRATION.md under 1q.; the ctypes
    mirror of the descriptor matches field for field; the build hashes the header and the kernel file."""
    L = ptx._lib
    text = open(L.BLUR_HEADER_PATH).read()
    declared = L.header_symbols(L.BLUR_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_BLUR) == ["ptx_gaussian_blur_frames", "ptx_gaussian_blur_supported"]
    for other in (L.SIGNATURES, L.header_symbols(), L.SIGNATURES_WINO4, L.SIGNATURES_TFIR, L.SIGNATURES_YUV16, L.SIGNATURES_COLOR,
                  L.SIGNATURES_RANDAUG, L.SIGNATURES_RESAMPLE, L.SIGNATURES_MIX, L.SIGNATURES_STEM_STRIDED, L.SIGNATURES_NL_KS,
                  L.SIGNATURES_LINEAR_BF16, L.SIGNATURES_BN, L.SIGNATURES_WARP, L.EXPERIMENTAL):
        assert not set(declared) & set(other)
    assert '#include "ptx_amd.h"' in text
    lib = L.lib()
    plain = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_BLUR[name][0], list(L.SIGNATURES_BLUR[name][1]))
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_BLUR[name][1]), name
    root = os.path.dirname(os.path.dirname(L.HEADER_PATH))
    integ = open(os.path.join(root, "INTEGRATION.md")).read()
    section = integ.split("### 1q.", 1)[1].split("\n### ", 1)[0]
    assert "ptx_amd_blur.h" in section and all(n in section for n in declared) and "### 1p." in integ
    assert "92 stable" in integ                                                    # ptx_amd.h's census does not move
    body = re.search(r"typedef struct ptx_blur_desc \{(.*?)\}", plain, flags=re.S).group(1)
    fields = [n.strip() for line in body.split(";") for n in line.replace("int32_t", "").split(",") if n.strip()]
    assert fields == [n for n, _ in L.BlurDesc._fields_] == ["N", "T", "H", "W", "kx", "ky", "out_mode"]
    assert all(t is C.c_int32 for _, t in L.BlurDesc._fields_) and C.sizeof(L.BlurDesc) == 28
    taps = int(re.search(r"#define PTX_BLUR_MAX_TAPS\s+(\d+)\b", text).group(1))
    assert taps == L.PTX_BLUR_MAX_TAPS == ptx.transforms.BLUR_MAX_TAPS and taps >= 33
    import importlib.util
    spec = importlib.util.spec_from_file_location("ptx_build", os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "blur_frames.h" in build.HEADERS and any(h.endswith("ptx_amd_blur.h") for h in build.HEADERS)
    files = build.tu_files("pack_layout.hip")
    assert any(p.endswith("blur_frames.h") for p in files) and any(p.endswith("ptx_amd_blur.h") for p in files)
    before = build.source_hash()
    assert L.binary_source_hash() == L.source_hash() == before
    src = open(os.path.join(os.path.dirname(L.LIB_PATH), "csrc", "build.py")).read()       # ptx_version()'s hash names the header
    assert '"ptx_amd_blur.h"' in src.split("def source_hash", 1)[1].split("def obj_path", 1)[0]


# --------------------------------------------------------------------------------------------- 9. the pipeline's arguments
def test_transform_frames_and_sample_clips_check_blur(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    opts = dict(input_space="RGB", input_range=[0, 1], mean=[0.5] * 3, std=[0.5] * 3, input_size=[3, 8, 8])
    plain = TF.TransformFrames(opts)
    assert plain.blur is None and plain._resize is None
    assert TF.TransformFrames(opts, blur=None)._resize is None and TF.SampleClips(opts, blur=None)._resize is None
    gb = TF.GaussianBlur(3)
    tf = TF.TransformFrames(opts, blur=gb, out="frames")
    assert tf.blur is gb and tf._resize is not None and tf._resize.blur is None and tf._resize.out == "frames"
    sc = TF.SampleClips(opts, blur=gb)
    assert sc.blur is gb and sc._resize.blur is None and sc.spatial.blur is None
    for bad in ("blur", 3, TF.ColorJitter(0.4)):
        with pytest.raises(E, match="blur must be"):
            TF.TransformFrames(opts, blur=bad)
        with pytest.raises(E, match="blur must be"):
            TF.SampleClips(opts, blur=bad)
    with pytest.raises(E, match=r"kernel_size=\(17, 17\).*H=8, W=8"):         # 17 // 2 = 8 = S
        TF.TransformFrames(opts, blur=TF.GaussianBlur(17))
    assert TF.TransformFrames(opts, blur=TF.GaussianBlur(15)).blur.kernel_size == (15, 15)
    with pytest.raises(E, match="blur_params"):
        plain(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), blur_params=([1], [1.0]))
    with pytest.raises(E, match="blur_params"):
        TF.TransformFrames(opts, color=TF.ColorJitter(0.4))(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), blur_params=([1], [1.0]))
    with pytest.raises(E, match="blur_params"):
        TF.SampleClips(opts)(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), blur_params=([1], [1.0]))
    with pytest.raises(E, match="sigma must be finite"):            # a replayed draw is checked before the frames are looked at
        tf(torch.zeros(2, 8, 8, 3, dtype=torch.uint8), blur_params=([1], [0.0]))
    with pytest.raises(E, match="uint8 CUDA"):                      # host frames: refused by the resize, no fallback
        tf(torch.zeros(2, 8, 8, 3, dtype=torch.uint8))
