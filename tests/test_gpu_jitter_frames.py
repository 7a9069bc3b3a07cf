"""GPU tests of per-clip resize geometry: the device table builder (ptx_resize_build_tables), the per-clip tables launch
(ptx_resize_frames_u8_tables / _yuv420_tables) and `pretorched.transforms.TransformFrames` with `random_short_side` /
`random_resized_crop` / `geometry=`.  All references are exact: the host builder's tables (`geometry_tables`, float64 as PIL
builds them), PIL's stored outputs (tests/golden/jitter_frames.npz), the existing fixed-window launch per clip, and the RGB
call on the converted frames for YUV sources.  Output buffers are pre-filled (0x5A bytes / NaN) so an element a kernel does
not write fails."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

from pretorched_x_amd.testing import synth_frames, synth_state_dict, synth_yuv420, yuv420_source

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB01 = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
BGR255 = dict(input_space="BGR", input_range=[0, 255], mean=[104.0, 117.0, 123.0], std=[58.0, 57.0, 57.5])
OPTS = dict(RGB01, input_size=[3, 64, 64])
S = 64


@functools.lru_cache(None)
def golden():
    blob = load_golden("jitter_frames")
    return blob, json.loads(str(blob["cases"]))


CASE_NAMES = [c["name"] for c in golden()[1]]


def case_of(name):
    return {c["name"]: c for c in golden()[1]}[name]


@functools.lru_cache(None)
def case_frames(name):
    """The case's input, uint8 CUDA [N,T,H,W,3] (made once, never written)."""
    c = case_of(name)
    N, T = len(c["geometry"]), c["T"]
    return torch.from_numpy(synth_frames(N * T, c["H"], c["W"], c["seed"])).view(N, T, c["H"], c["W"], 3).to(DEV)


def prefilled(shape, dtype):
    if dtype == torch.uint8:
        return torch.full(shape, 0x5A, dtype=torch.uint8, device=DEV)
    if dtype == torch.int32:
        return torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def host_tables(TF, geometry, size, pitch=None):
    """The oracle: geometry_tables per clip, stacked with the coefficient rows zero-padded to the common pitch.
    Returns [row_lo, row_n, row_k, col_lo, col_n, col_k] as numpy int32 [N,size], [N,size], [N,size,taps]."""
    per = [TF.geometry_tables(row, size) for row in geometry]
    out = []
    for ax, axis in enumerate(("rows", "cols")):
        taps = max(t[axis][2].shape[1] for t in per) if pitch is None else pitch[ax]
        k = np.zeros((len(per), size, taps), np.int32)
        for n, t in enumerate(per):
            k[n, :, :t[axis][2].shape[1]] = t[axis][2]
        out += [np.stack([t[axis][0] for t in per]).astype(np.int32), np.stack([t[axis][1] for t in per]).astype(np.int32), k]
    return out


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_builder(ptx, geometry, H, W, size, taps_h, taps_w):
    """ptx_resize_build_tables through ctypes into pre-filled tables; returns the six device tensors."""
    L = ptx._lib
    N = len(geometry)
    geo = torch.tensor(geometry, dtype=torch.int32).to(DEV)
    assert geo.shape == (N, 10)
    tabs = [prefilled(s, torch.int32) for s in ((N, size), (N, size), (N, size, taps_h), (N, size), (N, size), (N, size, taps_w))]
    desc = L.ResizeDesc(N, 1, H, W, 3, size, size, taps_h, taps_w, L.PTX_RESIZE_OUT_U8)
    L.check(L.lib().ptx_resize_build_tables(C.byref(desc), C.c_void_p(geo.data_ptr()), *[C.c_void_p(t.data_ptr()) for t in tabs],
                                            stream()), "ptx_resize_build_tables")
    torch.cuda.synchronize()
    return tabs


def out_buffer(L, N, T, Cc, mode, Ho=S, Wo=S):
    if mode == L.PTX_RESIZE_OUT_U8:
        return prefilled((N, T, Ho, Wo, Cc), torch.uint8)
    return prefilled((N, Cc, T, Ho, Wo), torch.float32 if mode == L.PTX_RESIZE_OUT_F32 else torch.bfloat16)


def run_tables(ptx, frames, src, tabs, mode, opts=None):
    """ptx_resize_frames_u8_tables (frames [N,T,H,W,C]) or ptx_resize_frames_yuv420_tables (src) through ctypes with the
    per-clip tables `tabs` (numpy or device tensors), into a pre-filled buffer."""
    L = ptx._lib
    N, T, H, W, Cc = (src.N, src.T, src.H, src.W, 3) if src is not None else frames.shape
    dev = [t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t)).to(DEV) for t in tabs]
    assert dev[0].shape == (N, S) and dev[3].shape == (N, S)
    y = out_buffer(L, N, T, Cc, mode)
    norm = L.NormDesc.make(opts["mean"], opts["std"], opts["input_space"], opts["input_range"]) if opts else None
    desc = L.ResizeDesc(N, T, H, W, Cc, S, S, dev[2].shape[2], dev[5].shape[2], mode)
    args = [C.c_void_p(t.data_ptr()) for t in dev] + [C.c_void_p(y.data_ptr()), C.byref(norm) if norm is not None else None, stream()]
    if src is not None:
        ysrc, keep = src.source()
        assert L.lib().ptx_resize_frames_yuv420_tables_supported(C.byref(desc), C.byref(ysrc)) == 1
        L.check(L.lib().ptx_resize_frames_yuv420_tables(C.byref(desc), C.byref(ysrc), *args), "ptx_resize_frames_yuv420_tables")
    else:
        assert L.lib().ptx_resize_frames_u8_tables_supported(C.byref(desc)) == 1
        L.check(L.lib().ptx_resize_frames_u8_tables(C.byref(desc), C.c_void_p(frames.data_ptr()), *args), "ptx_resize_frames_u8_tables")
    torch.cuda.synchronize()
    return y


def run_fixed(ptx, clip, tables, mode, opts=None, size=S):
    """The existing fixed-window launch ptx_resize_frames_u8 on ONE clip [T,H,W,C] with that clip's own tables."""
    L = ptx._lib
    T, H, W, Cc = clip.shape
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in tuple(tables["rows"]) + tuple(tables["cols"])]
    y = out_buffer(L, 1, T, Cc, mode, size, size)
    norm = L.NormDesc.make(opts["mean"], opts["std"], opts["input_space"], opts["input_range"]) if opts else None
    desc = L.ResizeDesc(1, T, H, W, Cc, size, size, tables["rows"][2].shape[1], tables["cols"][2].shape[1], mode)
    L.check(L.lib().ptx_resize_frames_u8(C.byref(desc), C.c_void_p(clip.contiguous().data_ptr()), *[C.c_void_p(t.data_ptr()) for t in dev],
                                         C.c_void_p(y.data_ptr()), C.byref(norm) if norm is not None else None, stream()),
            "ptx_resize_frames_u8")
    torch.cuda.synchronize()
    return y[0]


def assert_tables_equal(got, want, what):
    """lo, n and every coefficient slot (zeros up to the pitch included) of both axes."""
    names = ("row_lo", "row_n", "row_k", "col_lo", "col_n", "col_k")
    for name, g, w in zip(names, got, want):
        g = g.cpu().numpy()
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        diff = int((g != w).sum())
        assert diff == 0, (what, name, "%d differing entries, first at %s" % (diff, np.argwhere(g != w)[0].tolist()))


# --------------------------------------------------------------------------------------------- 1. the builder
SWEEP_IN = 260


@pytest.mark.parametrize("n_out", [1, 2, 7, 64, 73, 224])
def test_builder_equals_the_host_tables_bit_for_bit_sweep(ptx, n_out):
    """Every n_in in 1..260 -> n_out as the clips of one launch: rows take the box [0, n_in), columns the box
    [260 - n_in, 260) mirrored, so both axes, a non-zero origin and the flip reversal are swept too.  Pairs above the tap
    cap are excluded and must be refused by the host."""
    TF, L, E = ptx.transforms, ptx._lib, ptx._lib.PtxError
    tf = TF.TransformFrames(dict(RGB01, input_size=[1, n_out, n_out]), out="frames")       # S = max(input_size) = n_out
    assert tf.size == n_out
    rows = [[0, SWEEP_IN - n_in, n_in, n_in, n_out, n_out, 0, 0, 1, 0] for n_in in range(1, SWEEP_IN + 1)]
    keep, dropped = [], []
    for row in rows:
        taps = int(TF.resize_axis_table(row[2], n_out)[1].max())
        (keep if taps <= L.PTX_RESIZE_MAX_TAPS else dropped).append(row)
    assert len(keep) >= 64 and (dropped or n_out >= 64)            # n_out = 1, 2, 7 reach the cap inside the sweep
    for row in dropped:
        with pytest.raises(E, match="PTX_RESIZE_MAX_TAPS"):
            tf.check_geometry([row], 1, SWEEP_IN, SWEEP_IN)
    _, taps_h, taps_w = tf._checked_geometry(keep, len(keep), SWEEP_IN, SWEEP_IN)
    want = host_tables(TF, keep, n_out)
    assert (taps_h, taps_w) == (want[2].shape[2], want[5].shape[2])                # the host's pitch is the exact one
    got = run_builder(ptx, keep, SWEEP_IN, SWEEP_IN, n_out, taps_h, taps_w)
    assert_tables_equal(got, want, "n_out=%d" % n_out)


def test_builder_on_large_down_scales_windows_origins_and_flips(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    tf = TF.TransformFrames(OPTS, out="frames")
    H, W = 1920, 2100
    geometry = [
        [0, 0, 540, 1080, 73, 256, 9, 192, 0, 0],                   # 540 -> 73 rows, 1080 -> 256 columns, corner window
        [0, 0, 1920, 1080, 455, 256, 391, 0, 1, 1],                 # 1920 -> 455, far window, both flips
        [1380, 1020, 540, 1080, 73, 256, 0, 100, 0, 1],             # the same scales from a box in the far corner
        [0, 2036, 64, 64, 73, 73, 9, 9, 1, 0],                      # 64-wide boxes of a 2100-wide frame: the last 64 columns,
        [7, 1000, 64, 64, 64, 64, 0, 0, 0, 1],                      # one that is not resampled (one tap),
        [0, 0, 64, 2100, 64, 73, 0, 0, 0, 0],                       # and the whole width -> 73 (58 taps)
        [1919, 2099, 1, 1, 64, 64, 0, 0, 0, 0],                     # the last pixel
    ]
    with pytest.raises(E, match="PTX_RESIZE_MAX_TAPS"):
        tf.check_geometry([[0, 0, 64, 2100, 64, 64, 0, 0, 0, 0]], 1, H, W)         # 2100 -> 64: 66 taps
    _, taps_h, taps_w = tf._checked_geometry(geometry, len(geometry), H, W)
    want = host_tables(TF, geometry, S)
    assert (taps_h, taps_w) == (want[2].shape[2], want[5].shape[2]) and taps_w >= 58
    assert_tables_equal(run_builder(ptx, geometry, H, W, S, taps_h, taps_w), want, "large")
    # a wider pitch than needed: the extra slots are zeros
    wide = host_tables(TF, geometry, S, pitch=(taps_h + 3, 64))
    assert_tables_equal(run_builder(ptx, geometry, H, W, S, taps_h + 3, 64), wide, "wide pitch")
    # garbage rows are clamped, never trusted: every entry stays inside the frame and the pitch
    junk = [[-5, 3000, 1 << 30, -7, 0, -3, 1 << 20, -9, 7, -1], [1 << 30, -1, 0, 1 << 30, 1 << 30, 1, -4, 5, 0, 0]]
    lo_r, n_r, _, lo_c, n_c, _ = [t.cpu().numpy() for t in run_builder(ptx, junk, 97, 131, S, 4, 5)]
    assert lo_r.min() >= 0 and (lo_r + n_r).max() <= 97 and n_r.min() >= 0 and n_r.max() <= 4
    assert lo_c.min() >= 0 and (lo_c + n_c).max() <= 131 and n_c.min() >= 0 and n_c.max() <= 5


# --------------------------------------------------------------------------------------------- 2. / 3. the tables launch
@pytest.mark.parametrize("name", CASE_NAMES)
def test_tables_launch_equals_pil_goldens(ptx, name):
    TF, L = ptx.transforms, ptx._lib
    c = case_of(name)
    frames = case_frames(name)
    tabs = host_tables(TF, c["geometry"], S)
    assert len({tuple(t) for t in c["taps"]}) > 1                                  # mixed tap counts meet in one launch
    want = torch.from_numpy(golden()[0]["out_" + name]).to(DEV)
    got = run_tables(ptx, frames, None, tabs, L.PTX_RESIZE_OUT_U8)
    assert got.shape == want.shape and torch.equal(got, want), name
    for opts in (RGB01, BGR255):                                                   # fp32 and bf16: FramesToTensor of the golden
        t = TF.FramesToTensor(opts)(want)
        got32 = run_tables(ptx, frames, None, tabs, L.PTX_RESIZE_OUT_F32, opts)
        assert got32.shape == t.shape and torch.equal(got32, t), (name, opts["input_space"])
        got16 = run_tables(ptx, frames, None, tabs, L.PTX_RESIZE_OUT_BF16, opts)
        assert got16.dtype == torch.bfloat16 and torch.equal(got16, t.to(torch.bfloat16)), (name, opts["input_space"])
    # and with the tables the device built
    _, taps_h, taps_w = TF.TransformFrames(OPTS)._checked_geometry(c["geometry"], len(c["geometry"]), c["H"], c["W"])
    built = run_builder(ptx, c["geometry"], c["H"], c["W"], S, taps_h, taps_w)
    assert_tables_equal(built, tabs, name)
    assert torch.equal(run_tables(ptx, frames, None, built, L.PTX_RESIZE_OUT_U8), want), name


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_clip_equals_the_fixed_window_launch(ptx, name):
    TF, L = ptx.transforms, ptx._lib
    c = case_of(name)
    frames = case_frames(name)
    tabs = host_tables(TF, c["geometry"], S)
    for mode, opts in ((L.PTX_RESIZE_OUT_U8, None), (L.PTX_RESIZE_OUT_F32, BGR255), (L.PTX_RESIZE_OUT_BF16, RGB01)):
        got = run_tables(ptx, frames, None, tabs, mode, opts)
        for n, row in enumerate(c["geometry"]):
            fixed = run_fixed(ptx, frames[n], TF.geometry_tables(row, S), mode, opts)
            assert not torch.isnan(fixed.float()).any() and torch.equal(fixed, got[n]), (name, mode, n)


def test_tables_with_the_coefficients_in_global_memory(ptx):
    TF = ptx.transforms
    # 1080 x 1920 -> 224 x 224: the row stages and the intermediate image leave no room for the coefficient tables in LDS,
    # so the kernel reads every clip's coefficients from its tables in global memory
    opts = dict(RGB01, input_size=[3, 224, 224])
    frames = torch.from_numpy(synth_frames(2, 1080, 1920, 301)).view(2, 1, 1080, 1920, 3).to(DEV)
    geometry = [[0, 0, 1080, 1920, 256, 455, 32, 231, 1, 1],       # short-side jitter R = 256, the far corner, both flips
                [100, 200, 800, 1100, 224, 224, 0, 0, 0, 0]]       # a RandomResizedCrop box
    tf = TF.TransformFrames(opts, out="frames")
    got = tf(frames, geometry=geometry)
    assert got.shape == (2, 1, 224, 224, 3)
    for n, row in enumerate(geometry):
        fixed = run_fixed(ptx, frames[n], TF.geometry_tables(row, 224), ptx._lib.PTX_RESIZE_OUT_U8, size=224)
        assert torch.equal(fixed, got[n]), n
    # the jitter row is expressible on the existing path as well
    old = TF.TransformFrames(opts, 224 / 256, crop=(32, 231), hflip=True, vflip=True, out="frames")
    assert TF.resized_size(1080, 1920, opts["input_size"], 224 / 256) == (256, 455)
    assert torch.equal(old(frames[0]), got[0])


# --------------------------------------------------------------------------------------------- 4. the class
@pytest.mark.parametrize("name", CASE_NAMES)
def test_transform_frames_with_a_given_geometry_equals_pil_goldens(ptx, name):
    TF = ptx.transforms
    c = case_of(name)
    frames = case_frames(name)
    want = torch.from_numpy(golden()[0]["out_" + name]).to(DEV)
    g = c["geometry"]
    got = TF.TransformFrames(OPTS, out="frames")(frames, geometry=g)
    assert torch.equal(got, want)
    for form in (np.array(g), torch.tensor(g, dtype=torch.int32)):
        assert torch.equal(TF.TransformFrames(OPTS, out="frames")(frames, geometry=form), want)
    bgr = dict(BGR255, input_size=[3, 64, 64])
    t32 = TF.TransformFrames(bgr)(frames, geometry=g)
    assert torch.equal(t32, TF.FramesToTensor(bgr)(want))
    t16 = TF.TransformFrames(bgr, dtype=torch.bfloat16)(frames, geometry=g)
    assert t16.dtype == torch.bfloat16 and torch.equal(t16, t32.to(torch.bfloat16))


def test_api_default_geometry_seeded_draws_and_ranks(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    frames = torch.from_numpy(synth_frames(16, 90, 120, 501)).view(8, 2, 90, 120, 3).to(DEV)
    plain = TF.TransformFrames(OPTS, out="frames")
    # the default-equivalent geometry ties the new path to the old one
    for kw in (dict(), dict(hflip=True, vflip=True), dict(crop=(9, 33)), dict(scale=1.0, preserve_aspect_ratio=False)):
        old = TF.TransformFrames(OPTS, out="frames", **kw)
        assert torch.equal(old(frames, geometry=old.draw_geometry(8, 90, 120)), old(frames)), kw
        assert old.last_geometry is None                                           # given rows: nothing is drawn or kept
    for out_kw in (dict(out="tensor"), dict(out="tensor", dtype=torch.bfloat16)):
        old = TF.TransformFrames(OPTS, **out_kw)
        assert torch.equal(old(frames, geometry=old.draw_geometry(8, 90, 120)), old(frames)), out_kw
    # seeded draws of both new switches
    for kw in (dict(random_short_side=(64, 96), random_crop=True, random_hflip=True, random_vflip=True),
               dict(random_short_side=(70, 80)),
               dict(random_resized_crop=True, random_hflip=True),
               dict(random_resized_crop=dict(scale=(0.3, 1.0), ratio=(0.5, 2.0)), vflip=True)):
        tf = TF.TransformFrames(OPTS, out="frames", generator=torch.Generator().manual_seed(5), **kw)
        assert tf.last_geometry is None
        got = tf(frames)
        g = tf.last_geometry
        assert g.shape == (8, 10) and g.dtype == torch.int32 and g.device.type == "cpu" and tf.last_params is None
        assert len(set(map(tuple, g.tolist()))) > 4, kw                             # the clips really differ
        assert torch.equal(g, TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(5), **kw).draw_geometry(8, 90, 120))
        assert got.shape == (8, 2, S, S, 3) and torch.equal(plain(frames, geometry=g), got), kw
        for n, row in enumerate(g.tolist()):                                        # the numpy model of PIL, clip by clip
            assert np.array_equal(got[n, 1].cpu().numpy(), TF.apply_tables_numpy(frames[n, 1].cpu().numpy(), TF.geometry_tables(row, S))), (kw, n)
        nxt = tf(frames)                                                           # the next call draws anew
        assert not torch.equal(tf.last_geometry, g) and not torch.equal(nxt, got)
        assert torch.equal(tf(frames, geometry=g), got)
        # ranks 4 and 3: one draw
        clip = tf(frames[3])
        assert clip.shape == (2, S, S, 3) and tf.last_geometry.shape == (1, 10)
        assert torch.equal(clip, plain(frames[3], geometry=tf.last_geometry))
        image = tf(frames[3, 1])
        assert image.shape == (S, S, 3) and tf.last_geometry.shape == (1, 10)
        assert torch.equal(image, plain(frames[3:4, 1:2], geometry=tf.last_geometry)[0, 0])
    # tensor outputs follow the ranks as before
    tt = TF.TransformFrames(OPTS, random_resized_crop=True, generator=torch.Generator().manual_seed(2))
    t5 = tt(frames)
    g5 = tt.last_geometry
    assert t5.shape == (8, 3, 2, S, S) and torch.equal(t5, TF.FramesToTensor(OPTS)(plain(frames, geometry=g5)))
    assert tt(frames[0]).shape == (3, 2, S, S) and tt(frames[0, 0]).shape == (3, S, S)
    # torch.manual_seed governs generator=None
    state = torch.get_rng_state()
    try:
        torch.manual_seed(123)
        d = TF.TransformFrames(OPTS, out="frames", random_short_side=(64, 96), random_crop=True)
        a = d(frames)
        torch.manual_seed(123)
        assert torch.equal(d.draw_geometry(8, 90, 120), d.last_geometry)
    finally:
        torch.set_rng_state(state)
    assert torch.equal(a, plain(frames, geometry=d.last_geometry))
    # errors on real device tensors
    with pytest.raises(E, match="CUDA tensor"):
        plain(frames, geometry=g5.to(DEV))
    with pytest.raises(E, match="N = 8"):
        plain(frames, geometry=g5[:7])
    with pytest.raises(E, match="cannot be combined"):
        plain(frames, params=[[0, 0, 0, 0]] * 8, geometry=g5)
    # params= stays on the windows launch and is what it was
    assert torch.equal(plain(frames, params=[[4, 16, 0, 0]] * 8), plain(frames))


# --------------------------------------------------------------------------------------------- 5. YUV sources
YUV_CASES = {   # name: H, W, layout, geometry per clip (T = 2 frames per clip)
    "nv12_pitched_90x120": (90, 120, "nv12_pitched", [[0, 0, 90, 120, 64, 85, 0, 21, 1, 0], [11, 13, 55, 52, 64, 64, 0, 0, 0, 1],
                                                      [89, 119, 1, 1, 64, 64, 0, 0, 0, 0], [0, 0, 90, 120, 96, 128, 32, 64, 1, 1]]),
    "i420_90x120": (90, 120, "i420", [[1, 1, 88, 117, 64, 64, 0, 0, 1, 1], [0, 0, 90, 120, 73, 97, 4, 16, 0, 0], [26, 56, 64, 64, 64, 64, 0, 0, 0, 1]]),
    "planes_odd_121x91": (121, 91, "planes", [[3, 5, 117, 85, 64, 64, 0, 0, 1, 0], [120, 90, 1, 1, 64, 64, 0, 0, 0, 0],
                                              [0, 0, 121, 91, 97, 73, 33, 9, 1, 1]]),
    "nv12_pitched_wide_64x2100": (64, 2100, "nv12_pitched", [[0, 2000, 64, 100, 64, 64, 0, 0, 0, 0], [0, 0, 64, 2100, 73, 2395, 9, 2331, 1, 0]]),
}


@pytest.mark.parametrize("name", sorted(YUV_CASES))
def test_yuv_sources_equal_the_rgb_call_on_converted_frames(ptx, name):
    TF, L = ptx.transforms, ptx._lib
    H, W, layout, geometry = YUV_CASES[name]
    N, T = len(geometry), 2
    kw = dict(matrix="bt601", color_range="limited")
    y, u, v = synth_yuv420(N * T, H, W, 41)
    src = yuv420_source((y, u, v), layout, DEV, lead_shape=(N, T), **kw)
    rgb = torch.from_numpy(src.to_rgb_numpy()).to(DEV)
    assert rgb.shape == (N, T, H, W, 3) and np.array_equal(rgb.cpu().numpy().reshape(N * T, H, W, 3), TF.yuv420_to_rgb_numpy(y, u, v, **kw))
    tabs = host_tables(TF, geometry, S)
    a = run_tables(ptx, None, src, tabs, L.PTX_RESIZE_OUT_U8)
    b = run_tables(ptx, rgb, None, tabs, L.PTX_RESIZE_OUT_U8)
    assert torch.equal(a, b), name
    for n, row in enumerate(geometry):                                             # and the numpy model of PIL on clip n
        assert np.array_equal(a[n, 1].cpu().numpy(), TF.apply_tables_numpy(rgb[n, 1].cpu().numpy(), TF.geometry_tables(row, S))), (name, n)
    for opts in (RGB01, BGR255):
        for mode in (L.PTX_RESIZE_OUT_F32, L.PTX_RESIZE_OUT_BF16):
            a, b = run_tables(ptx, None, src, tabs, mode, opts), run_tables(ptx, rgb, None, tabs, mode, opts)
            assert not torch.isnan(a.float()).any() and torch.equal(a, b), (name, mode)
    # the class: given rows, and a seeded draw on both kinds of source
    tf8 = TF.TransformFrames(OPTS, out="frames")
    assert torch.equal(tf8(src, geometry=geometry), tf8(rgb, geometry=geometry))
    if min(H, W) >= 64 and W < 2000:
        for kwr in (dict(random_short_side=(64, 90), random_crop=True, random_hflip=True), dict(random_resized_crop=True, random_vflip=True)):
            r1 = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(9), **kwr)
            r2 = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(9), **kwr)
            assert torch.equal(r1(src), r2(rgb)) and torch.equal(r1.last_geometry, r2.last_geometry) and r1.last_geometry.shape == (N, 10)
            one = TF.YUV420(src.y[0], src.u[0], src.v[0] if src.v is not None else None, **kw)   # [T,..] planes: one clip, one draw
            got = r1(one)
            assert got.shape == (3, T, S, S) and r1.last_geometry.shape == (1, 10)
            assert torch.equal(got, TF.TransformFrames(OPTS)(rgb[0], geometry=r1.last_geometry))


# --------------------------------------------------------------------------------------------- 7. end to end
def test_forward_frames_with_a_random_resized_crop_transform(ptx):
    TF = ptx.transforms
    frames = torch.from_numpy(synth_frames(16, 90, 120, 113)).view(2, 8, 90, 120, 3).to(DEV)
    model = ptx.__dict__["resnet3d18"](num_classes=400, pretrained=None)
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
    model = model.to(DEV).eval()
    model.engine().lanes = 1
    tf = TF.TransformFrames(OPTS, out="frames", random_resized_crop=True, random_hflip=True, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        got = model.forward_frames(frames, OPTS, transform=tf)
        g = tf.last_geometry
        assert g.shape == (2, 10) and len(set(map(tuple, g.tolist()))) == 2
        small = TF.TransformFrames(OPTS, out="frames")(frames, geometry=g)
        want = model.forward_frames(small, OPTS)
        assert got.shape == (2, 400) and torch.equal(got, want)
        assert torch.equal(model.engine().forward_frames(model, frames, OPTS, transform=tf),
                           model.forward_frames(TF.TransformFrames(OPTS, out="frames")(frames, geometry=tf.last_geometry), OPTS))
