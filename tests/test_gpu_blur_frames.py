"""GPU tests of the per-clip GaussianBlur on uint8 frames (`pretorched.transforms.GaussianBlur`, include/ptx_amd_blur.h).  Every
comparison is exact (`torch.equal`): the numpy statement of the contract (`gaussian_blur_numpy`) for the bytes, `FramesToTensor`
of the blurred bytes for the plane outputs, and the stages applied one after another for the composed transforms.  Output buffers
of the direct launches are pre-filled (0xAA bytes / NaN) so an element the kernel does not write fails."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pretorched_x_amd.testing import synth_color_frames, synth_frames, synth_state_dict, synth_yuv420, yuv420_source

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB01 = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
BGR255 = dict(input_space="BGR", input_range=[0, 255], mean=[104.0, 117.0, 123.0], std=[58.0, 57.0, 57.5])
OPTS = dict(RGB01, input_size=[3, 32, 32])
# (H, W), (kx, ky): ry = H - 1, every row reflects from both edges | one tile, unequal sizes | the 32 x 32 tile twice along H and
# five times along W with ragged last tiles (64 = 2 * 32 exactly, 130 = 4 * 32 + 2) and the longest halo the recipes use |
# the tap cap along W on a frame lower than one run of four rows
CASES = [((7, 9), (5, 13)), ((33, 70), (9, 3)), ((64, 130), (23, 23)), ((5, 300), (33, 1))]
IDS = ["7x9_k5x13", "33x70_k9x3", "64x130_k23", "5x300_k33x1"]
SIGMAS = (0.35, 1.0, 1.9)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def prefilled(shape, dtype, offset=0):
    """A pre-filled contiguous tensor whose first byte lies `offset` bytes past an allocation (uint8 only)."""
    if dtype == torch.uint8:
        n = int(np.prod(shape))
        return torch.full((n + offset,), 0xAA, dtype=torch.uint8, device=DEV)[offset:].view(shape)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def at_offset(frames, offset):
    """uint8 numpy frames as a contiguous device tensor whose first byte lies `offset` bytes past an allocation."""
    buf = torch.zeros(frames.size + offset, dtype=torch.uint8, device=DEV)
    view = buf[offset:].view(frames.shape)
    view.copy_(torch.from_numpy(frames).to(DEV))
    assert view.data_ptr() % 4 == offset % 4 and view.is_contiguous()
    return view


def run_kernel(ptx, frames, apply, wx, wy, mode=0, opts=None, out_offset=0):
    """ptx_gaussian_blur_frames through ctypes on device frames [N,T,H,W,3], into a pre-filled buffer."""
    L = ptx._lib
    lib = L.lib()
    N, T, H, W, _ = frames.shape
    apply = np.ascontiguousarray(apply, np.int32)
    wx, wy = np.ascontiguousarray(wx, np.float32), np.ascontiguousarray(wy, np.float32)
    desc = L.BlurDesc(N, T, H, W, wx.shape[1], wy.shape[1], mode)
    assert lib.ptx_gaussian_blur_supported(C.byref(desc), C.c_void_p(apply.ctypes.data), C.c_void_p(wx.ctypes.data),
                                           C.c_void_p(wy.ctypes.data)) == 1, lib.ptx_last_error().decode()
    d_apply, d_wx, d_wy = (torch.from_numpy(a).to(DEV) for a in (apply, wx, wy))
    if mode == L.PTX_RESIZE_OUT_U8:
        y = prefilled((N, T, H, W, 3), torch.uint8, out_offset)
    else:
        y = prefilled((N, 3, T, H, W), torch.float32 if mode == L.PTX_RESIZE_OUT_F32 else torch.bfloat16)
    norm = L.NormDesc.make(opts["mean"], opts["std"], opts["input_space"], opts["input_range"]) if opts else None
    L.check(lib.ptx_gaussian_blur_frames(C.byref(desc), C.c_void_p(frames.data_ptr()), C.c_void_p(d_apply.data_ptr()),
                                         C.c_void_p(d_wx.data_ptr()), C.c_void_p(d_wy.data_ptr()), C.c_void_p(y.data_ptr()),
                                         C.byref(norm) if norm else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "blur")
    torch.cuda.synchronize()
    return y


@functools.lru_cache(None)
def case(i):
    """(frames [3,2,H,W,3], apply, wx, wy, numpy's output) of CASES[i]: a sigma per clip, the middle clip not blurred.  Computed
    once, shared, never written."""
    import pretorched_x_amd as ptx
    TF = ptx.transforms
    (H, W), (kx, ky) = CASES[i]
    frames = synth_color_frames(3, 2, H, W, 8100 + i)
    apply = np.array([1, 0, 1], np.int32)
    wx = np.stack([TF.gaussian_kernel1d(kx, s).numpy() for s in SIGMAS])
    wy = np.stack([TF.gaussian_kernel1d(ky, s).numpy() for s in SIGMAS])
    want = TF.gaussian_blur_numpy(frames, apply, wx, wy)
    assert np.array_equal(want[1], frames[1]) and not np.array_equal(want[0], frames[0])
    return frames, apply, wx, wy, want


# --------------------------------------------------------------------------------------------- 1. the C ABI against the contract
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_kernel_equals_the_numpy_contract(ptx, i, offset):
    frames, apply, wx, wy, want = case(i)
    y = run_kernel(ptx, at_offset(frames, offset), apply, wx, wy, out_offset=offset)
    assert torch.equal(y.cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_plane_outputs_equal_frames_to_tensor_of_the_blurred_bytes(ptx, i):
    """fp32: FramesToTensor (ptx_frames_u8_to_ncdhw) of the blurred uint8 frames, bit for bit, under a BGR / 255-range norm (and
    an RGB / unit-range one); bf16: that value rounded once."""
    L, TF = ptx._lib, ptx.transforms
    frames, apply, wx, wy, want_u8 = case(i)
    dev = torch.from_numpy(frames).to(DEV)
    for opts in (BGR255, RGB01):
        want = TF.FramesToTensor(opts)(torch.from_numpy(want_u8).to(DEV))
        y32 = run_kernel(ptx, dev, apply, wx, wy, L.PTX_RESIZE_OUT_F32, opts)
        assert torch.equal(y32, want)
        y16 = run_kernel(ptx, dev, apply, wx, wy, L.PTX_RESIZE_OUT_BF16, opts)
        assert y16.dtype == torch.bfloat16 and torch.equal(y16, want.to(torch.bfloat16))


# --------------------------------------------------------------------------------------------- 2. the public call
def test_the_python_call_replay_and_one_clip(ptx):
    TF = ptx.transforms
    frames = synth_color_frames(4, 2, 37, 53, 8200)
    dev = torch.from_numpy(frames).to(DEV)
    gb = TF.GaussianBlur((9, 5), p=0.6, generator=gen(8201))
    y = gb(dev)
    p = gb.last_params
    assert 0 < int(p[0].sum()) < 4 and y.data_ptr() != dev.data_ptr() and y.shape == dev.shape and y.dtype == torch.uint8
    wx, wy = gb.weights(p)
    assert torch.equal(y.cpu(), torch.from_numpy(TF.gaussian_blur_numpy(frames, p[0], wx, wy)))
    assert torch.equal(gb(dev, params=p), y) and gb.last_params is p                 # a replay keeps the last draw
    assert torch.equal(TF.GaussianBlur((9, 5))(dev, params=(p[0].numpy(), p[1].tolist())), y)       # on any GaussianBlur of that size
    n = int(np.flatnonzero(p[0].numpy())[0])
    one = gb(dev[n], params=(p[0][n:n + 1], p[1][n:n + 1]))          # [T,H,W,3] is one clip
    assert one.shape == dev[n].shape and torch.equal(one, y[n])
    img = gb(dev[0, 0])                                             # [H,W,3]: one draw
    assert img.shape == (37, 53, 3) and gb.last_params[0].shape == (1,)
    always = TF.GaussianBlur(3, sigma=0.8)
    ya = always(dev)
    w = TF.gaussian_kernel1d(3, 0.8).numpy()
    assert always.last_params[0].tolist() == [1] * 4 and torch.equal(ya.cpu(), torch.from_numpy(TF.gaussian_blur_numpy(frames, [1] * 4, w, w)))
    assert torch.equal(TF.GaussianBlur(3, p=0.0)(dev), dev)         # no clip passes the gate: a copy
    with pytest.raises(ptx._lib.PtxError, match="uint8 CUDA"):
        gb(dev.cpu())


# --------------------------------------------------------------------------------------------- 3. the pipeline
@functools.lru_cache(None)
def raw_frames():
    return torch.from_numpy(synth_frames(3 * 4, 60, 80, 8300).reshape(3, 4, 60, 80, 3)).to(DEV)


def test_transform_frames_runs_the_stages_in_the_recipes_order(ptx):
    TF = ptx.transforms
    raw = raw_frames()
    kw = dict(random_resized_crop=True, random_hflip=True)

    def stages(seed):
        g = gen(seed)                                               # one generator for every draw of the call
        return (TF.ColorJitter(0.4, 0.4, 0.4, 0.1, grayscale=0.2, generator=g), TF.GaussianBlur(9, p=0.7, generator=g),
                TF.RandAugment(2, 9, generator=g), TF.BatchMix(generator=g), g)

    cj, gb, ra, bm, g = stages(41)
    tf = TF.TransformFrames(OPTS, generator=g, color=cj, blur=gb, augment=ra, mix=bm, **kw)
    y = tf(raw)
    geo, pc, pb, pa, pm = tf.last_geometry, cj.last_params, gb.last_params, ra.last_params, bm.last_params
    assert y.shape == (3, 3, 4, 32, 32) and y.dtype == torch.float32 and 0 < int(pb[0].sum())
    # the same stages one after another with the drawn parameters
    frames = TF.TransformFrames(OPTS, out="frames")(raw, geometry=geo)
    u8 = ra(gb(cj(frames, params=pc), params=pb), params=pa)
    assert torch.equal(y, bm(u8, params=pm, opts=OPTS))
    # one seed: the geometry and the colour lists are the same without blur=; the draws behind it move on
    cj2, _, ra2, bm2, g2 = stages(41)
    tf2 = TF.TransformFrames(OPTS, generator=g2, color=cj2, augment=ra2, mix=bm2, **kw)
    tf2(raw)
    assert torch.equal(tf2.last_geometry, geo) and all(torch.equal(a, b) for a, b in zip(cj2.last_params, pc))
    # out="frames" with the blur last: gb on the frames of the transform without it
    cj3, gb3, _, _, g3 = stages(42)
    tf3 = TF.TransformFrames(OPTS, out="frames", generator=g3, color=cj3, blur=gb3, **kw)
    y3 = tf3(raw)
    cj4, _, _, _, g4 = stages(42)
    plain = TF.TransformFrames(OPTS, out="frames", generator=g4, color=cj4, **kw)
    f4 = plain(raw)
    assert torch.equal(plain.last_geometry, tf3.last_geometry) and all(torch.equal(a, b) for a, b in zip(cj4.last_params, cj3.last_params))
    want = gb3(f4, params=gb3.last_params)
    assert y3.dtype == torch.uint8 and torch.equal(y3, want) and not torch.equal(y3, f4)
    # replay of every draw; the blur as the last stage writes fp32 and bf16
    assert torch.equal(tf3(raw, geometry=tf3.last_geometry, color_params=cj3.last_params, blur_params=gb3.last_params), want)
    for dtype in (torch.float32, torch.bfloat16):
        t = TF.TransformFrames(OPTS, dtype=dtype, color=cj3, blur=gb3, **kw)(raw, geometry=tf3.last_geometry, color_params=cj3.last_params,
                                                                              blur_params=gb3.last_params)
        assert t.dtype == dtype and torch.equal(t, TF.FramesToTensor(OPTS)(want).to(dtype))
    t = TF.TransformFrames(OPTS, dtype=torch.bfloat16, color=cj, blur=gb, augment=ra, mix=bm, **kw)(
        raw, geometry=geo, color_params=pc, blur_params=pb, augment_params=pa, mix_params=pm)
    assert t.dtype == torch.bfloat16 and torch.equal(t, bm(u8, params=pm, opts=OPTS, dtype=torch.bfloat16))
    # blur alone behind a fixed window, a lower rank, per-clip windows, a YUV 4:2:0 source
    only = TF.TransformFrames(OPTS, blur=gb)
    t4 = only(raw[0])
    assert t4.shape == (3, 4, 32, 32) and gb.last_params[0].shape == (1,)
    assert torch.equal(t4, TF.FramesToTensor(OPTS)(gb(TF.TransformFrames(OPTS, out="frames")(raw[0]), params=gb.last_params)))
    win = TF.TransformFrames(OPTS, out="frames", random_crop=True, generator=gen(43), blur=gb)
    yw = win(raw)
    assert torch.equal(yw, gb(TF.TransformFrames(OPTS, out="frames")(raw, params=win.last_params), params=gb.last_params))
    src = yuv420_source(synth_yuv420(3 * 4, 60, 80, 8301), "planes", DEV, lead_shape=(3, 4))
    ys = TF.TransformFrames(OPTS, out="frames", generator=gen(44), blur=gb, **kw)(src)
    assert torch.equal(ys, gb(TF.TransformFrames(OPTS, out="frames", generator=gen(44), **kw)(src), params=gb.last_params))


def test_sample_clips_with_blur_equals_transform_frames_on_the_gathered_frames(ptx):
    TF = ptx.transforms
    videos = [torch.from_numpy(synth_frames(12, 60, 80, 8310)).to(DEV), torch.from_numpy(synth_frames(9, 50, 44, 8311)).to(DEV)]
    kw = dict(random_resized_crop=True, random_hflip=True)
    g = gen(51)
    cj, gb = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, generator=g), TF.GaussianBlur((5, 9), p=0.7, generator=g)
    sc = TF.SampleClips(OPTS, num_frames=4, frame_stride=2, clips=2, generator=g, color=cj, blur=gb, **kw)
    y = sc(videos)
    idx, geo, pc, pb = sc.last_indices, sc.last_geometry, cj.last_params, gb.last_params
    assert y.shape == (4, 3, 4, 32, 32) and pb[0].shape == (4,) and 0 < int(pb[0].sum())
    tf = TF.TransformFrames(OPTS, color=cj, blur=gb, **kw)
    for j in range(4):                                              # output clip j comes from video j // clips
        gathered = videos[j // 2][idx[j]]
        one = tf(gathered, geometry=geo[j:j + 1], color_params=(pc[0][j:j + 1], pc[1][j:j + 1]), blur_params=(pb[0][j:j + 1], pb[1][j:j + 1]))
        assert torch.equal(y[j], one), j
    frames = TF.SampleClips(OPTS, num_frames=4, frame_stride=2, clips=2, out="frames", **kw)(videos, indices=idx, geometry=geo)
    assert torch.equal(y, TF.FramesToTensor(OPTS)(gb(cj(frames, params=pc), params=pb)))
    assert torch.equal(sc(videos, indices=idx, geometry=geo, color_params=pc, blur_params=pb), y)


def test_forward_frames_takes_a_transform_with_blur(ptx):
    TF = ptx.transforms
    with torch.no_grad():
        model = ptx.__dict__["resnet3d18"](num_classes=339, pretrained=None)
        model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
        model = model.to(DEV).eval()
        model.engine().lanes = 1
        raw = raw_frames()[:2]
        g = gen(61)
        cj, gb = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, generator=g), TF.GaussianBlur(9, generator=g)
        tf = TF.TransformFrames(OPTS, out="frames", random_resized_crop=True, generator=g, color=cj, blur=gb)
        got = model.forward_frames(raw, OPTS, transform=tf)
        frames = tf(raw, geometry=tf.last_geometry, color_params=cj.last_params, blur_params=gb.last_params)
        assert frames.dtype == torch.uint8 and got.shape == (2, 339) and torch.equal(got, model.forward_frames(frames, OPTS))


# --------------------------------------------------------------------------------------------- 4. blur=None is the path it was
def test_without_blur_the_colour_transform_gives_the_composed_stages_bits(ptx):
    """`TransformFrames(opts, color=cj)` for a fixed seed against the stage composition of the colour tests: the resize of the
    transform without colour on the same seed, then the colour call on the drawn lists."""
    TF = ptx.transforms
    raw = raw_frames()
    kw = dict(random_resized_crop=True, random_hflip=True)
    cj = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, grayscale=0.2, generator=gen(71))
    tf = TF.TransformFrames(OPTS, out="frames", generator=gen(72), color=cj, blur=None, **kw)
    assert tf.blur is None and tf._resize.blur is None
    y = tf(raw)
    plain = TF.TransformFrames(OPTS, out="frames", generator=gen(72), **kw)
    frames = plain(raw)
    assert plain._resize is None and torch.equal(plain.last_geometry, tf.last_geometry)
    want = cj(frames, params=cj.last_params)
    assert torch.equal(y, want)
    t = TF.TransformFrames(OPTS, color=cj, **kw)(raw, geometry=tf.last_geometry, color_params=cj.last_params)
    assert torch.equal(t, TF.FramesToTensor(OPTS)(want))
    assert torch.equal(t, TF.TransformFrames(OPTS, color=cj, blur=None, **kw)(raw, geometry=tf.last_geometry, color_params=cj.last_params))
