"""GPU tests of per-clip RandAugment on uint8 frames (`pretorched.transforms.RandAugment`, include/ptx_amd_randaug.h).  Every
comparison is exact (`torch.equal`): Pillow's stored outputs and inputs (tests/golden/rand_augment.npz), the numpy statement of
the contract (`rand_augment_numpy`), `FramesToTensor` of the augmented bytes for the plane outputs, and the stand-alone call on
the `out="frames"` result for the composed transforms.  Output buffers of the direct launches are pre-filled (0xAA bytes / NaN)
so an element the kernel does not write fails.  Neither Pillow nor the generator of the goldens is imported."""
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
STATS = (8, 12, 13)


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(None)
def golden():
    blob = load_golden("rand_augment")
    return {k: blob[k] for k in blob.files}


def fill_of():
    return tuple(int(v) for v in golden()["fill"])


def at_offset(frames, offset):
    """uint8 numpy frames as a contiguous device tensor whose first byte lies `offset` bytes past an allocation."""
    buf = torch.zeros(frames.size + offset, dtype=torch.uint8, device=DEV)
    view = buf[offset:].view(frames.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(frames)).to(DEV))
    assert view.data_ptr() % 4 == offset % 4 and view.is_contiguous()
    return view


def run_kernels(ptx, frames, params, fill, mode=0, opts=None, out_offset=0):
    """The launches through ctypes on device frames [N,T,H,W,3], position by position, into pre-filled buffers (scratch, the
    statistics and the output).  Returns (y, launches)."""
    L, TF = ptx._lib, ptx.transforms
    lib = L.lib()
    N, T, H, W, _ = frames.shape
    rows = np.ascontiguousarray(TF.rand_augment_rows(params, H, W, N))
    K = rows.shape[1]
    d_rows = torch.from_numpy(rows.reshape(-1)).to(DEV)
    n = N * T * H * W * 3
    if mode == L.PTX_RESIZE_OUT_U8:
        y = torch.full((n + out_offset,), 0xAA, dtype=torch.uint8, device=DEV)[out_offset:].view(N, T, H, W, 3)
    else:
        y = torch.full((N, 3, T, H, W), float("nan"), dtype=torch.float32 if mode == L.PTX_RESIZE_OUT_F32 else torch.bfloat16, device=DEV)
    scratch = [torch.full((N, T, H, W, 3), 0xAA, dtype=torch.uint8, device=DEV) for _ in range(2)]
    stats = torch.full((N * T * L.PTX_RANDAUG_STATS_WORDS,), -1, dtype=torch.int32, device=DEV)   # the statistics call zeroes them itself
    norm = L.NormDesc.make(opts["mean"], opts["std"], opts["input_space"], opts["input_range"]) if opts else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    launches, cur = [], frames
    for k in range(K):
        last = k == K - 1
        need = bool(np.isin(rows[:, k, 0], STATS).any())
        desc = L.RandAugDesc(N, T, H, W, mode if last else L.PTX_RESIZE_OUT_U8, K, k, int(need), fill[0], fill[1], fill[2], 0)
        assert lib.ptx_rand_augment_supported(C.byref(desc), C.c_void_p(rows.ctypes.data)) == 1, lib.ptx_last_error().decode()
        if need:
            L.check(lib.ptx_rand_augment_stats(C.byref(desc), C.c_void_p(cur.data_ptr()), C.c_void_p(d_rows.data_ptr()),
                                               C.c_void_p(stats.data_ptr()), stream), "stats")
            launches.append("stats")
        dst = y if last else scratch[k % 2]
        L.check(lib.ptx_rand_augment_apply(C.byref(desc), C.c_void_p(cur.data_ptr()), C.c_void_p(d_rows.data_ptr()),
                                           C.c_void_p(stats.data_ptr()) if need else None, C.c_void_p(dst.data_ptr()),
                                           C.byref(norm) if (last and norm) else None, stream), "apply")
        launches.append("apply")
        cur = dst
    torch.cuda.synchronize()
    return y, tuple(launches)


# --------------------------------------------------------------------------------------------- 1. goldens, restatement
@pytest.mark.parametrize("launch", range(8))
def test_every_op_at_both_signs_equals_pil_golden(ptx, launch):
    """[3,2,9,11,3] frames, three one-op cases per launch (clip j of the launch runs case 3 * launch + j): mixed op codes over
    the clips, 99 pixels per frame (a partial tile, an odd frame size in bytes)."""
    g, TF = golden(), ptx.transforms
    sl = slice(3 * launch, 3 * launch + 3)
    params = (g["every_codes"][sl], g["every_mags"][sl])
    y, launches = run_kernels(ptx, torch.from_numpy(g["every_in"]).to(DEV), params, fill_of())
    assert launches == (("stats", "apply") if np.isin(params[0], STATS).any() else ("apply",))
    assert torch.equal(y.cpu(), torch.from_numpy(g["every_out"][sl]))
    assert np.array_equal(TF.rand_augment_numpy(g["every_in"], params, fill_of()), g["every_out"][sl])


@pytest.mark.parametrize("group,want", [("chain2", ("stats", "apply", "stats", "apply")), ("chain4", ("apply", "stats", "apply", "stats", "apply", "apply"))])
def test_chains_with_mixed_codes_equal_pil_golden(ptx, group, want):
    """[2,2,32,20,3]: at every position the two clips run different ops and at most one of them needs the statistics
    (its workgroups alone count; the other clip's leave the statistics kernel)."""
    g, TF = golden(), ptx.transforms
    params = (g[group + "_codes"], g[group + "_mags"])
    assert all(np.isin(params[0][:, k], STATS).sum() <= 1 for k in range(params[0].shape[1]))
    y, launches = run_kernels(ptx, torch.from_numpy(g[group + "_in"]).to(DEV), params, fill_of())
    assert launches == want
    assert torch.equal(y.cpu(), torch.from_numpy(g[group + "_out"]))
    ra = TF.RandAugment(fill=fill_of())
    y2 = ra(torch.from_numpy(g[group + "_in"]).to(DEV), params=params)          # the Python call: the same launches
    assert ra.last_launches == want and torch.equal(y2, y) and ra.last_params is None


@pytest.mark.parametrize("case", range(3), ids=["equalize", "autocontrast", "contrast"])
def test_statistics_ops_on_224x224_frames(ptx, case):
    """[1,2,224,224,3]: 13 tiles per frame flush into one histogram; frame 0 is constant (one bin holds all 50176 pixels, the
    degenerate branches), frame 1 a ramp."""
    g = golden()
    params = (g["big_codes"][case:case + 1], g["big_mags"][case:case + 1])
    y, launches = run_kernels(ptx, torch.from_numpy(g["big_in"]).to(DEV), params, fill_of())
    assert launches == ("stats", "apply") and torch.equal(y.cpu(), torch.from_numpy(g["big_out"][case:case + 1]))
    y2, _ = run_kernels(ptx, torch.from_numpy(g["big_in"]).to(DEV), params, fill_of())       # integer atomics: deterministic
    assert torch.equal(y2, y)


@functools.lru_cache(None)
def random_case(seed, K):
    """Random 37 x 53 frames [3,2,..] and a seeded draw of K ops: (frames, codes, magnitudes, numpy's output).  Computed once."""
    import pretorched_x_amd as ptx
    TF = ptx.transforms
    frames = synth_color_frames(3, 2, 37, 53, seed)
    codes, mags = (t.numpy() for t in TF.RandAugment(K, 14, generator=gen(seed)).draw(3, 37, 53))
    return frames, codes, mags, TF.rand_augment_numpy(frames, (codes, mags), (3, 99, 201))


@pytest.mark.parametrize("offset,out_offset,K", [(1, 0, 2), (2, 1, 3), (3, 3, 4), (0, 2, 1)])
def test_frames_and_output_at_odd_byte_offsets(ptx, offset, out_offset, K):
    frames, codes, mags, want = random_case(700 + K, K)
    y, _ = run_kernels(ptx, at_offset(frames, offset), (codes, mags), (3, 99, 201), out_offset=out_offset)
    assert torch.equal(y.cpu(), torch.from_numpy(want))


# --------------------------------------------------------------------------------------------- 2. tensor output
@pytest.mark.parametrize("opts", [RGB01, BGR255], ids=["rgb01", "bgr255"])
def test_plane_outputs_equal_frames_to_tensor_of_the_augmented_bytes(ptx, opts):
    L, TF = ptx._lib, ptx.transforms
    for K in (1, 3):
        frames, codes, mags, want_u8 = random_case(700 + K, K)
        dev = torch.from_numpy(frames).to(DEV)
        want = TF.FramesToTensor(opts)(torch.from_numpy(want_u8).to(DEV))
        y32, _ = run_kernels(ptx, dev, (codes, mags), (3, 99, 201), L.PTX_RESIZE_OUT_F32, opts)
        assert torch.equal(y32, want)
        y16, _ = run_kernels(ptx, dev, (codes, mags), (3, 99, 201), L.PTX_RESIZE_OUT_BF16, opts)
        assert y16.dtype == torch.bfloat16 and torch.equal(y16, want.to(torch.bfloat16))
    ident = (np.zeros((3, 2), np.int32), np.zeros((3, 2)))            # identity positions: copied, then final-converted
    y32, launches = run_kernels(ptx, dev, ident, (0, 0, 0), L.PTX_RESIZE_OUT_F32, opts)
    assert launches == ("apply", "apply") and torch.equal(y32, TF.FramesToTensor(opts)(dev))


# --------------------------------------------------------------------------------------------- 3. the Python call
def test_python_call_draws_replays_and_lists_its_launches(ptx):
    TF = ptx.transforms
    frames = synth_color_frames(3, 2, 19, 23, 94)
    dev = torch.from_numpy(frames).to(DEV)
    ra = TF.RandAugment(3, 12, fill=(9, 8, 7), generator=gen(95))
    y = ra(dev)
    p = ra.last_params
    assert p[0].shape == (3, 3) and y.data_ptr() != dev.data_ptr()
    assert torch.equal(y.cpu(), torch.from_numpy(TF.rand_augment_numpy(frames, p, (9, 8, 7))))
    want = tuple(s for k in range(3) for s in ((("stats",) if np.isin(p[0][:, k].numpy(), STATS).any() else ()) + ("apply",)))
    assert ra.last_launches == want
    assert torch.equal(ra(dev, params=p), y) and ra.last_params is p              # a replay keeps the last draw
    assert torch.equal(TF.RandAugment(fill=(9, 8, 7))(dev, params=(p[0].numpy(), p[1].tolist())), y)     # on any RandAugment
    one = ra(dev[1], params=(p[0][1:2], p[1][1:2]))                  # [T,H,W,3] is one clip
    assert one.shape == dev[1].shape and torch.equal(one, y[1])
    img = ra(dev[1, 0])                                              # [H,W,3]: one draw
    assert img.shape == (19, 23, 3) and ra.last_params[0].shape == (1, 3)
    # no statistics launch when no list needs one
    geo = (np.array([[1, 5], [6, 10], [3, 0]], np.int32), np.array([[0.1, -20.0], [0.3, 5.0], [4.0, 0.0]]))
    yg = ra(dev, params=geo)
    assert ra.last_launches == ("apply", "apply") and torch.equal(yg.cpu(), torch.from_numpy(TF.rand_augment_numpy(frames, geo, (9, 8, 7))))
    with pytest.raises(ptx._lib.PtxError, match="uint8 CUDA"):
        ra(dev.cpu())


# --------------------------------------------------------------------------------------------- 4. composition
@functools.lru_cache(None)
def raw_frames():
    return torch.from_numpy(synth_frames(2 * 4, 60, 80, 4300).reshape(2, 4, 60, 80, 3)).to(DEV)


def test_transform_frames_with_augment(ptx):
    TF = ptx.transforms
    raw = raw_frames()
    kw = dict(random_resized_crop=True, random_hflip=True)
    ra = TF.RandAugment(2, 12, fill=5, generator=gen(41))
    tf = TF.TransformFrames(OPTS, out="frames", generator=gen(12), augment=ra, **kw)
    y = tf(raw)
    geo, p = tf.last_geometry, ra.last_params
    plain = TF.TransformFrames(OPTS, out="frames", generator=gen(12), **kw)
    frames = plain(raw)
    assert torch.equal(plain.last_geometry, geo)                    # the same seed gives the same geometry without it
    want = ra(frames, params=p)
    assert torch.equal(y, want) and p[0].shape == (2, 2)
    assert torch.equal(want.cpu(), torch.from_numpy(TF.rand_augment_numpy(frames.cpu().numpy(), p, 5)))
    assert torch.equal(tf(raw, geometry=geo, augment_params=p), want)
    for dtype in (torch.float32, torch.bfloat16):
        t = TF.TransformFrames(OPTS, dtype=dtype, augment=ra, **kw)(raw, geometry=geo, augment_params=p)
        assert t.dtype == dtype and torch.equal(t, TF.FramesToTensor(OPTS)(want).to(dtype))
    # behind colour: resize -> colour (uint8 scratch) -> augment writes the output
    cj = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, generator=gen(42))
    both = TF.TransformFrames(OPTS, generator=gen(12), color=cj, augment=ra, **kw)
    t = both(raw)
    assert torch.equal(both.last_geometry, geo)
    want2 = ra(cj(frames, params=cj.last_params), params=ra.last_params)
    assert torch.equal(t, TF.FramesToTensor(OPTS)(want2))
    assert torch.equal(both(raw, geometry=geo, color_params=cj.last_params, augment_params=ra.last_params), t)
    # lower ranks, a YUV 4:2:0 source
    t4 = TF.TransformFrames(OPTS, augment=ra)(raw[0])
    assert t4.shape == (3, 4, 32, 32) and ra.last_params[0].shape == (1, 2)
    assert torch.equal(t4, TF.FramesToTensor(OPTS)(ra(TF.TransformFrames(OPTS, out="frames")(raw[0]), params=ra.last_params)))
    src = yuv420_source(synth_yuv420(2 * 4, 60, 80, 4301), "planes", DEV, lead_shape=(2, 4))
    ys = TF.TransformFrames(OPTS, out="frames", generator=gen(14), augment=ra, **kw)(src)
    assert torch.equal(ys, ra(TF.TransformFrames(OPTS, out="frames", generator=gen(14), **kw)(src), params=ra.last_params))
    with pytest.raises(ptx._lib.PtxError, match="augment_params"):
        plain(raw, augment_params=p)


def test_sample_clips_with_augment(ptx):
    TF = ptx.transforms
    videos = [torch.from_numpy(synth_frames(12, 60, 80, 4310)).to(DEV), torch.from_numpy(synth_frames(9, 50, 44, 4311)).to(DEV)]
    kw = dict(num_frames=4, frame_stride=2, clips=2, random_resized_crop=True, random_hflip=True)
    ra = TF.RandAugment(2, 12, generator=gen(51))
    sc = TF.SampleClips(OPTS, out="frames", generator=gen(22), augment=ra, **kw)
    y = sc(videos)
    p = ra.last_params
    assert y.shape == (4, 4, 32, 32, 3) and p[0].shape == (4, 2)
    plain = TF.SampleClips(OPTS, out="frames", generator=gen(22), **kw)
    frames = plain(videos)
    assert torch.equal(plain.last_indices, sc.last_indices) and torch.equal(plain.last_geometry, sc.last_geometry)
    want = ra(frames, params=p)
    assert torch.equal(y, want)
    for dtype in (torch.float32, torch.bfloat16):
        t = TF.SampleClips(OPTS, dtype=dtype, augment=ra, **kw)(videos, indices=sc.last_indices, geometry=sc.last_geometry, augment_params=p)
        assert torch.equal(t, TF.FramesToTensor(OPTS)(want).to(dtype))
    with pytest.raises(ptx._lib.PtxError, match="augment_params"):
        plain(videos, augment_params=p)


def test_forward_frames_takes_a_transform_with_augment(ptx):
    TF = ptx.transforms
    with torch.no_grad():
        model = ptx.__dict__["resnet3d18"](num_classes=339, pretrained=None)
        model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
        model = model.to(DEV).eval()
        model.engine().lanes = 1
        raw = raw_frames()
        ra = TF.RandAugment(generator=gen(31))
        tf = TF.TransformFrames(OPTS, out="frames", random_resized_crop=True, generator=gen(32), augment=ra)
        got = model.forward_frames(raw, OPTS, transform=tf)
        tensor = TF.TransformFrames(OPTS, random_resized_crop=True, augment=ra)(raw, geometry=tf.last_geometry, augment_params=ra.last_params)
        assert got.shape == (2, 339) and torch.equal(got, model(tensor))
