"""GPU tests of per-clip ColorJitter / RandomGrayscale on uint8 frames (`pretorched.transforms.ColorJitter`,
include/ptx_amd_color.h).  Every comparison is exact (`torch.equal`): PIL's stored outputs (tests/golden/color_jitter.npz),
the numpy statement of the contract (`color_jitter_numpy`), `FramesToTensor` of the jittered bytes for the plane outputs, and
the colour call on the `out="frames"` result for the composed transforms.  Output buffers of the direct launches are
pre-filled (0xA5 bytes / NaN) so an element the kernel does not write fails."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

from pretorched_x_amd.testing import synth_color_frames, synth_frames, synth_state_dict, synth_yuv420, yuv420_source

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB01 = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
BGR255 = dict(input_space="BGR", input_range=[0, 255], mean=[104.0, 117.0, 123.0], std=[58.0, 57.0, 57.5])
OPTS = dict(RGB01, input_size=[3, 32, 32])


def gen(seed):
    return torch.Generator().manual_seed(seed)


def prefilled(shape, dtype, offset=0):
    """A pre-filled contiguous tensor whose first byte lies `offset` bytes past an allocation (uint8 only)."""
    if dtype == torch.uint8:
        n = int(np.prod(shape))
        return torch.full((n + offset,), 0xA5, dtype=torch.uint8, device=DEV)[offset:].view(shape)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def at_offset(frames, offset):
    """uint8 numpy frames as a contiguous device tensor whose first byte lies `offset` bytes past an allocation."""
    buf = torch.zeros(frames.size + offset, dtype=torch.uint8, device=DEV)
    view = buf[offset:].view(frames.shape)
    view.copy_(torch.from_numpy(frames).to(DEV))
    assert view.data_ptr() % 4 == offset % 4 and view.is_contiguous()
    return view


def run_kernels(ptx, frames, codes, factors, mode=0, opts=None, out_offset=0):
    """ptx_color_jitter_stats (only when a list holds contrast) + ptx_color_jitter_apply through ctypes on device frames
    [N,T,H,W,3], into a pre-filled buffer.  Returns (y, launches)."""
    L = ptx._lib
    lib = L.lib()
    N, T, H, W, _ = frames.shape
    codes = np.ascontiguousarray(np.asarray(codes, np.int32))
    factors = np.ascontiguousarray(np.asarray(factors, np.float32))
    contrast = bool((codes == L.PTX_COLOR_CONTRAST).any())
    desc = L.ColorDesc(N, T, H, W, mode, int(contrast))
    assert lib.ptx_color_jitter_supported(C.byref(desc), C.c_void_p(codes.ctypes.data), C.c_void_p(factors.ctypes.data)) == 1, \
        lib.ptx_last_error().decode()
    d_codes, d_factors = torch.from_numpy(codes).to(DEV), torch.from_numpy(factors).to(DEV)
    if mode == L.PTX_RESIZE_OUT_U8:
        y = prefilled((N, T, H, W, 3), torch.uint8, out_offset)
    else:
        y = prefilled((N, 3, T, H, W), torch.float32 if mode == L.PTX_RESIZE_OUT_F32 else torch.bfloat16)
    norm = L.NormDesc.make(opts["mean"], opts["std"], opts["input_space"], opts["input_range"]) if opts else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sums = torch.full((N * T,), -1, dtype=torch.int64, device=DEV)          # the statistics call zeroes them itself
    launches = 0
    if contrast:
        L.check(lib.ptx_color_jitter_stats(C.byref(desc), C.c_void_p(frames.data_ptr()), C.c_void_p(d_codes.data_ptr()),
                                           C.c_void_p(d_factors.data_ptr()), C.c_void_p(sums.data_ptr()), stream), "stats")
        launches += 1
    L.check(lib.ptx_color_jitter_apply(C.byref(desc), C.c_void_p(frames.data_ptr()), C.c_void_p(d_codes.data_ptr()),
                                       C.c_void_p(d_factors.data_ptr()), C.c_void_p(sums.data_ptr()) if contrast else None,
                                       C.c_void_p(y.data_ptr()), C.byref(norm) if norm else None, stream), "apply")
    torch.cuda.synchronize()
    return y, launches + 1


@functools.lru_cache(None)
def golden_group(name):
    blob = load_golden("color_jitter")
    N, T, H, W, seed = (int(v) for v in blob[name + "_shape"])
    return synth_color_frames(N, T, H, W, seed), blob[name + "_codes"], blob[name + "_factors"], blob[name + "_out"]


@functools.lru_cache(None)
def random_case(N, T, seed):
    """Random frames of 37 x 53 and lists drawn by a ColorJitter with every op on: (frames, codes, factors, numpy's output).
    Computed once, shared, never written."""
    import pretorched_x_amd as ptx
    TF = ptx.transforms
    frames = synth_color_frames(N, T, 37, 53, seed)
    cj = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, grayscale=0.3, generator=gen(seed))
    codes, factors = (t.numpy() for t in cj.draw(N))
    return frames, codes, factors, TF.color_jitter_numpy(frames, (codes, factors))


# --------------------------------------------------------------------------------------------- 1. golden, restatement
@pytest.mark.parametrize("group", ["small", "chunks"])
def test_kernel_equals_pil_golden(ptx, group):
    frames, codes, factors, want = golden_group(group)
    y, launches = run_kernels(ptx, torch.from_numpy(frames).to(DEV), codes, factors)
    assert launches == 2
    assert torch.equal(y.cpu(), torch.from_numpy(want))
    if group == "small":                                            # the empty list gives the input back
        empty = int(np.flatnonzero((codes == 0).all(axis=1))[0])
        assert torch.equal(y[empty].cpu(), torch.from_numpy(frames[empty]))


@pytest.mark.parametrize("N,T,offset,out_offset", [(2, 3, 0, 0), (2, 3, 1, 0), (2, 3, 2, 1), (2, 3, 3, 3), (1, 3, 0, 0), (2, 1, 1, 2)])
def test_kernel_equals_numpy_on_random_lists(ptx, N, T, offset, out_offset):
    """37 x 53 frames (5883 bytes: frame t starts at another byte phase than frame t - 1), the input and the output at any
    byte offset: the dword groups, the byte heads and tails, the whole-dword and the byte stores."""
    frames, codes, factors, want = random_case(N, T, 500 + N * 10 + T)
    assert len({tuple(r) for r in codes.tolist()}) == N            # the clips' lists differ
    y, _ = run_kernels(ptx, at_offset(frames, offset), codes, factors, out_offset=out_offset)
    assert torch.equal(y.cpu(), torch.from_numpy(want))


# --------------------------------------------------------------------------------------------- 2. tensor output
@pytest.mark.parametrize("opts", [RGB01, BGR255], ids=["rgb01", "bgr255"])
@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (2, 2, 16, 24)], ids=["scalar_stores", "vector_stores"])
def test_plane_outputs_equal_frames_to_tensor_of_the_jittered_bytes(ptx, opts, shape):
    """fp32: FramesToTensor(opts) of the jittered uint8 frames, bit for bit; bf16: that value rounded once.  37 x 53 planes
    are no multiple of four elements (element stores); 16 x 24 planes are (16- and 8-byte pieces)."""
    L, TF = ptx._lib, ptx.transforms
    N, T, H, W = shape
    if (H, W) == (37, 53):
        frames, codes, factors, want_u8 = random_case(N, T, 500 + N * 10 + T)
    else:
        frames = synth_color_frames(N, T, H, W, 77)
        codes, factors = (t.numpy() for t in TF.ColorJitter(0.4, 0.4, 0.4, 0.1, generator=gen(78)).draw(N))
        want_u8 = TF.color_jitter_numpy(frames, (codes, factors))
    dev = torch.from_numpy(frames).to(DEV)
    want = TF.FramesToTensor(opts)(torch.from_numpy(want_u8).to(DEV))
    y32, _ = run_kernels(ptx, dev, codes, factors, L.PTX_RESIZE_OUT_F32, opts)
    assert torch.equal(y32, want)
    y16, _ = run_kernels(ptx, dev, codes, factors, L.PTX_RESIZE_OUT_BF16, opts)
    assert y16.dtype == torch.bfloat16 and torch.equal(y16, want.to(torch.bfloat16))


# --------------------------------------------------------------------------------------------- 3. determinism, edge cases
def test_two_runs_are_bit_equal(ptx):
    frames, codes, factors, want = golden_group("chunks")           # several statistics workgroups per frame
    dev = torch.from_numpy(frames).to(DEV)
    a, _ = run_kernels(ptx, dev, codes, factors)
    b, _ = run_kernels(ptx, dev, codes, factors)
    assert torch.equal(a, b) and torch.equal(a.cpu(), torch.from_numpy(want))


def test_no_contrast_means_no_statistics_launch(ptx):
    TF = ptx.transforms
    frames = synth_color_frames(2, 2, 19, 23, 91)
    dev = torch.from_numpy(frames).to(DEV)
    cj = TF.ColorJitter(brightness=0.4, saturation=0.4, hue=0.1, grayscale=0.5, generator=gen(92))
    y = cj(dev)
    assert cj.last_launches == ("apply",) and not (cj.last_params[0] == ptx._lib.PTX_COLOR_CONTRAST).any()
    assert torch.equal(y.cpu(), torch.from_numpy(TF.color_jitter_numpy(frames, cj.last_params)))
    y2, launches = run_kernels(ptx, dev, cj.last_params[0].numpy(), cj.last_params[1].numpy())
    assert launches == 1 and torch.equal(y2, y)
    both = TF.ColorJitter(contrast=0.4, generator=gen(93))
    yc = both(dev)
    assert both.last_launches == ("stats", "apply")
    assert torch.equal(yc.cpu(), torch.from_numpy(TF.color_jitter_numpy(frames, both.last_params)))


def test_empty_lists_and_the_python_call(ptx):
    TF = ptx.transforms
    frames = synth_color_frames(2, 2, 19, 23, 94)
    dev = torch.from_numpy(frames).to(DEV)
    off = TF.ColorJitter()                                          # every op off: empty lists, the input comes back
    y = off(dev)
    assert not off.last_params[0].any() and torch.equal(y, dev) and y.data_ptr() != dev.data_ptr()
    cj = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, grayscale=0.3, generator=gen(95))
    y = cj(dev)
    p = cj.last_params
    assert torch.equal(y.cpu(), torch.from_numpy(TF.color_jitter_numpy(frames, p)))
    assert torch.equal(cj(dev, params=p), y) and cj.last_params is p             # a replay keeps the last draw
    assert torch.equal(TF.ColorJitter()(dev, params=(p[0].numpy(), p[1].tolist())), y)      # on any ColorJitter
    one = cj(dev[0], params=(p[0][1:], p[1][1:]))                   # [T,H,W,3] is one clip
    assert one.shape == dev[0].shape and torch.equal(one.cpu(), torch.from_numpy(TF.color_jitter_numpy(frames[:1], (p[0][1:], p[1][1:]))[0]))
    img = cj(dev[1, 0])                                             # [H,W,3]: one draw
    assert img.shape == (19, 23, 3) and cj.last_params[0].shape == (1, 5)
    with pytest.raises(ptx._lib.PtxError, match="uint8 CUDA"):
        cj(dev.cpu())


# --------------------------------------------------------------------------------------------- 4. composition
@functools.lru_cache(None)
def raw_frames():
    return torch.from_numpy(synth_frames(2 * 4, 60, 80, 4300).reshape(2, 4, 60, 80, 3)).to(DEV)


def test_transform_frames_with_colour(ptx):
    TF = ptx.transforms
    raw = raw_frames()
    kw = dict(random_resized_crop=True, random_hflip=True)
    cj = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, grayscale=0.2, generator=gen(11))
    tf = TF.TransformFrames(OPTS, out="frames", generator=gen(12), color=cj, **kw)
    y = tf(raw)
    geo, p = tf.last_geometry, cj.last_params
    plain = TF.TransformFrames(OPTS, out="frames", generator=gen(12), **kw)
    frames = plain(raw)
    assert torch.equal(plain.last_geometry, geo)                    # the same seed gives the same geometry without colour
    want = cj(frames, params=p)
    assert torch.equal(y, want) and not torch.equal(y, frames)
    assert torch.equal(tf(raw, geometry=geo, color_params=p), want)                 # replay of both draws
    assert torch.equal(cj.last_params[0], p[0])
    for dtype in (torch.float32, torch.bfloat16):
        t = TF.TransformFrames(OPTS, dtype=dtype, color=cj, **kw)(raw, geometry=geo, color_params=p)
        assert t.dtype == dtype and torch.equal(t, TF.FramesToTensor(OPTS)(want).to(dtype))
    # per-clip windows (params=), the fixed window, lower ranks
    win = TF.TransformFrames(OPTS, out="frames", random_crop=True, generator=gen(13), color=cj)
    yw = win(raw)
    assert torch.equal(yw, cj(TF.TransformFrames(OPTS, out="frames")(raw, params=win.last_params), params=cj.last_params))
    fixed = TF.TransformFrames(OPTS, color=cj)
    t4 = fixed(raw[0])
    assert t4.shape == (3, 4, 32, 32) and cj.last_params[0].shape == (1, 5)
    assert torch.equal(t4, TF.FramesToTensor(OPTS)(cj(TF.TransformFrames(OPTS, out="frames")(raw[0]), params=cj.last_params)))
    # a YUV 4:2:0 source goes the same way
    src = yuv420_source(synth_yuv420(2 * 4, 60, 80, 4301), "planes", DEV, lead_shape=(2, 4))
    ys = TF.TransformFrames(OPTS, out="frames", generator=gen(14), color=cj, **kw)(src)
    assert torch.equal(ys, cj(TF.TransformFrames(OPTS, out="frames", generator=gen(14), **kw)(src), params=cj.last_params))
    with pytest.raises(ptx._lib.PtxError, match="color_params"):
        plain(raw, color_params=p)
    with pytest.raises(ptx._lib.PtxError, match="color must be"):
        TF.TransformFrames(OPTS, color="jitter")


def test_sample_clips_with_colour(ptx):
    TF = ptx.transforms
    videos = [torch.from_numpy(synth_frames(12, 60, 80, 4310)).to(DEV), torch.from_numpy(synth_frames(9, 50, 44, 4311)).to(DEV)]
    kw = dict(num_frames=4, frame_stride=2, clips=2, random_resized_crop=True, random_hflip=True)
    cj = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, grayscale=0.2, generator=gen(21))
    sc = TF.SampleClips(OPTS, out="frames", generator=gen(22), color=cj, **kw)
    y = sc(videos)
    p = cj.last_params
    assert y.shape == (4, 4, 32, 32, 3) and p[0].shape == (4, 5)
    plain = TF.SampleClips(OPTS, out="frames", generator=gen(22), **kw)
    frames = plain(videos)
    assert torch.equal(plain.last_indices, sc.last_indices) and torch.equal(plain.last_geometry, sc.last_geometry)
    want = cj(frames, params=p)
    assert torch.equal(y, want)
    for dtype in (torch.float32, torch.bfloat16):
        t = TF.SampleClips(OPTS, dtype=dtype, color=cj, **kw)(videos, indices=sc.last_indices, geometry=sc.last_geometry, color_params=p)
        assert torch.equal(t, TF.FramesToTensor(OPTS)(want).to(dtype))
    with pytest.raises(ptx._lib.PtxError, match="color_params"):
        plain(videos, color_params=p)


def test_forward_frames_takes_a_transform_with_colour(ptx):
    TF = ptx.transforms
    with torch.no_grad():
        model = ptx.__dict__["resnet3d18"](num_classes=339, pretrained=None)
        model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
        model = model.to(DEV).eval()
        model.engine().lanes = 1
        raw = raw_frames()
        cj = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, generator=gen(31))
        tf = TF.TransformFrames(OPTS, out="frames", random_resized_crop=True, generator=gen(32), color=cj)
        got = model.forward_frames(raw, OPTS, transform=tf)
        tensor = TF.TransformFrames(OPTS, random_resized_crop=True, color=cj)(raw, geometry=tf.last_geometry, color_params=cj.last_params)
        assert got.shape == (2, 339) and torch.equal(got, model(tensor))
