"""GPU tests of the per-clip windows launch (ptx_resize_frames_u8_windows / _yuv420_windows) and of
`pretorched.transforms.TransformFrames` with `random_crop` / `random_hflip` / `random_vflip` / `vflip` / `params=`.  Three
references, all exact: PIL's stored outputs (tests/golden/random_frames.npz), the existing fixed-window launch per clip, and
the RGB windows call on the converted frames for YUV sources.  Output buffers are pre-filled (0x5A bytes / NaN) so an element
the kernel does not write fails."""
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
    blob = load_golden("random_frames")
    return blob, json.loads(str(blob["cases"]))


CASE_NAMES = [c["name"] for c in golden()[1]]


def case_of(name):
    return {c["name"]: c for c in golden()[1]}[name]


@functools.lru_cache(None)
def case_frames(name):
    """The case's input, uint8 CUDA [N,T,H,W,3] (made once, never written)."""
    c = case_of(name)
    N, T = len(c["params"]), c["T"]
    return torch.from_numpy(synth_frames(N * T, c["H"], c["W"], c["seed"])).view(N, T, c["H"], c["W"], 3).to(DEV)


def prefilled(shape, dtype):
    if dtype == torch.uint8:
        return torch.full(shape, 0x5A, dtype=torch.uint8, device=DEV)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def run_windows(ptx, frames, src, full, params, mode, opts=None):
    """ptx_resize_frames_u8_windows (frames [N,T,H,W,C]) or ptx_resize_frames_yuv420_windows (src) through ctypes, with the
    whole-frame tables `full` and params [N][4], into a pre-filled buffer."""
    L = ptx._lib
    N, T, H, W, Cc = (src.N, src.T, src.H, src.W, 3) if src is not None else frames.shape
    h, w = full["resized"]
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in tuple(full["rows"]) + tuple(full["cols"])]
    wins = torch.tensor(params, dtype=torch.int32).to(DEV)
    assert wins.shape == (N, 4)
    y = prefilled((N, T, S, S, Cc), torch.uint8) if mode == L.PTX_RESIZE_OUT_U8 else \
        prefilled((N, Cc, T, S, S), torch.float32 if mode == L.PTX_RESIZE_OUT_F32 else torch.bfloat16)
    norm = L.NormDesc.make(opts["mean"], opts["std"], opts["input_space"], opts["input_range"]) if opts else None
    desc = L.ResizeDesc(N, T, H, W, Cc, S, S, full["rows"][2].shape[1], full["cols"][2].shape[1], mode)
    args = [C.c_void_p(t.data_ptr()) for t in dev] + [h, w, C.c_void_p(wins.data_ptr()), C.c_void_p(y.data_ptr()),
                                                      C.byref(norm) if norm is not None else None,
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)]
    if src is not None:
        ysrc, keep = src.source()
        assert L.lib().ptx_resize_frames_yuv420_windows_supported(C.byref(desc), C.byref(ysrc), h, w) == 1
        L.check(L.lib().ptx_resize_frames_yuv420_windows(C.byref(desc), C.byref(ysrc), *args), "ptx_resize_frames_yuv420_windows")
    else:
        assert L.lib().ptx_resize_frames_u8_windows_supported(C.byref(desc), h, w) == 1
        L.check(L.lib().ptx_resize_frames_u8_windows(C.byref(desc), C.c_void_p(frames.data_ptr()), *args),
                "ptx_resize_frames_u8_windows")
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("name", CASE_NAMES)
def test_windows_kernel_equals_pil_goldens(ptx, name):
    TF, L = ptx.transforms, ptx._lib
    c = case_of(name)
    frames = case_frames(name)
    full = TF.build_frame_tables(c["H"], c["W"], c["input_size"])
    want = torch.from_numpy(golden()[0]["out_" + name]).to(DEV)
    got = run_windows(ptx, frames, None, full, c["params"], L.PTX_RESIZE_OUT_U8)
    assert got.shape == want.shape and torch.equal(got, want), name
    # fp32 and bf16: FramesToTensor of the golden, rounded once for bf16
    for opts in (RGB01, BGR255):
        t = TF.FramesToTensor(opts)(want)                                          # [N,3,T,S,S]
        got32 = run_windows(ptx, frames, None, full, c["params"], L.PTX_RESIZE_OUT_F32, opts)
        assert got32.shape == t.shape and torch.equal(got32, t), (name, opts["input_space"])
        got16 = run_windows(ptx, frames, None, full, c["params"], L.PTX_RESIZE_OUT_BF16, opts)
        assert got16.dtype == torch.bfloat16 and torch.equal(got16, t.to(torch.bfloat16)), (name, opts["input_space"])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_clip_equals_the_fixed_window_launch(ptx, name):
    """Ties the new launch to the existing one: clip n == TransformFrames(crop=(top, left), hflip=.., vflip=..) on clip n."""
    TF = ptx.transforms
    c = case_of(name)
    frames = case_frames(name)
    want = torch.from_numpy(golden()[0]["out_" + name]).to(DEV)
    for kw in (dict(out="frames"), dict(out="tensor"), dict(out="tensor", dtype=torch.bfloat16)):
        opts = OPTS if kw["out"] == "frames" else dict(BGR255, input_size=[3, 64, 64])
        got = TF.TransformFrames(opts, **kw)(frames, params=c["params"])
        if kw["out"] == "frames":
            assert torch.equal(got, want)
        for n, (top, left, hf, vf) in enumerate(c["params"]):
            fixed = TF.TransformFrames(opts, crop=(top, left), hflip=bool(hf), vflip=bool(vf), **kw)
            assert torch.equal(fixed(frames[n]), got[n]), (name, kw, n)


def test_windows_with_the_coefficients_in_global_memory_and_other_channel_counts(ptx):
    TF, L = ptx.transforms, ptx._lib
    # 1080 x 1920 -> 224 x 224 out of 256 x 455: the row stages and the intermediate image leave no room for the
    # coefficient tables in LDS, so the kernel reads them from global memory through the clip's window
    opts = dict(RGB01, input_size=[3, 224, 224])
    frames = torch.from_numpy(synth_frames(2, 1080, 1920, 301)).view(2, 1, 1080, 1920, 3).to(DEV)
    params = [[32, 231, 1, 1], [0, 0, 0, 0]]
    got = TF.TransformFrames(opts, out="frames")(frames, params=params)
    assert got.shape == (2, 1, 224, 224, 3)
    for n, (top, left, hf, vf) in enumerate(params):
        fixed = TF.TransformFrames(opts, out="frames", crop=(top, left), hflip=bool(hf), vflip=bool(vf))
        assert torch.equal(fixed(frames[n]), got[n]), n
    # 1, 2 and 4 interleaved channels, against the numpy model on the reversed slices
    rgb = synth_frames(2, 97, 131, 31)
    full = TF.build_frame_tables(97, 131, [3, 64, 64])
    params = [[9, 22, 1, 1], [0, 0, 0, 1]]
    for ch in (1, 2, 4):
        f = np.ascontiguousarray(np.concatenate([rgb, rgb[..., ::-1]], -1)[..., :ch])
        got = run_windows(ptx, torch.from_numpy(f).view(2, 1, 97, 131, ch).to(DEV), None, full, params, L.PTX_RESIZE_OUT_U8).cpu()
        for n, (top, left, hf, vf) in enumerate(params):
            tables = TF.build_tables(97, 131, [3, 64, 64], crop=(top, left), hflip=bool(hf), vflip=bool(vf))
            assert np.array_equal(got[n, 0].numpy(), TF.apply_tables_numpy(f[n], tables)), (ch, n)


YUV_CASES = {   # name: H, W, layout, params per clip (T = 2 frames per clip)
    "nv12_pitched_odd_91x121": (91, 121, "nv12_pitched", [[0, 0, 0, 0], [9, 33, 1, 0], [4, 17, 0, 1], [9, 1, 1, 1]]),
    "i420_90x120": (90, 120, "i420", [[9, 33, 1, 1], [0, 32, 0, 1], [5, 0, 1, 0]]),
    "planes_odd_121x91": (121, 91, "planes", [[33, 9, 1, 1], [0, 0, 0, 0]]),
    "nv12_pitched_wide_64x2100": (64, 2100, "nv12_pitched", [[0, 2331, 1, 0], [9, 1100, 0, 1]]),
}


@pytest.mark.parametrize("name", sorted(YUV_CASES))
def test_yuv_windows_equal_the_rgb_windows_on_converted_frames(ptx, name):
    TF, L = ptx.transforms, ptx._lib
    H, W, layout, params = YUV_CASES[name]
    N, T = len(params), 2
    kw = dict(matrix="bt601", color_range="limited")
    y, u, v = synth_yuv420(N * T, H, W, 41)
    src = yuv420_source((y, u, v), layout, DEV, lead_shape=(N, T), **kw)
    rgb = torch.from_numpy(TF.yuv420_to_rgb_numpy(y, u, v, **kw)).view(N, T, H, W, 3).to(DEV)
    full = TF.build_frame_tables(H, W, [3, 64, 64])
    assert (src.N, src.T, src.H, src.W) == (N, T, H, W)
    assert tuple(full["resized"]) == (TF.resized_size(H, W, [3, 64, 64]))
    a = run_windows(ptx, None, src, full, params, L.PTX_RESIZE_OUT_U8)
    b = run_windows(ptx, rgb, None, full, params, L.PTX_RESIZE_OUT_U8)
    assert torch.equal(a, b), name
    for n, (top, left, hf, vf) in enumerate(params):                               # and the numpy model of PIL on clip n
        tables = TF.build_tables(H, W, [3, 64, 64], crop=(top, left), hflip=bool(hf), vflip=bool(vf))
        assert np.array_equal(a[n, 0].cpu().numpy(), TF.apply_tables_numpy(rgb[n, 0].cpu().numpy(), tables)), (name, n)
    for opts in (RGB01, BGR255):
        for mode in (L.PTX_RESIZE_OUT_F32, L.PTX_RESIZE_OUT_BF16):
            a, b = run_windows(ptx, None, src, full, params, mode, opts), run_windows(ptx, rgb, None, full, params, mode, opts)
            assert not torch.isnan(a.float()).any() and torch.equal(a, b), (name, mode)
    # the class: given parameters, and a seeded draw on both kinds of source
    tf8 = TF.TransformFrames(OPTS, out="frames")
    assert torch.equal(tf8(src, params=params), tf8(rgb, params=params))
    kwr = dict(random_crop=True, random_hflip=True, random_vflip=True)
    r1 = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(9), **kwr)
    r2 = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(9), **kwr)
    assert torch.equal(r1(src), r2(rgb)) and torch.equal(r1.last_params, r2.last_params) and r1.last_params.shape == (N, 4)
    one = TF.YUV420(src.y[0], src.u[0], src.v[0] if src.v is not None else None, **kw)      # [T,..] planes: one clip, one draw
    got = r1(one)
    assert got.shape == (3, T, S, S) and r1.last_params.shape == (1, 4)
    assert torch.equal(got, TF.TransformFrames(OPTS)(rgb[0], params=r1.last_params))


def test_api_ranks_params_and_seeded_draws(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    frames = torch.from_numpy(synth_frames(16, 90, 120, 501)).view(8, 2, 90, 120, 3).to(DEV)
    kw = dict(random_crop=True, random_hflip=True, random_vflip=True)
    tf = TF.TransformFrames(OPTS, out="frames", generator=torch.Generator().manual_seed(5), **kw)
    assert tf.last_params is None
    got = tf(frames)
    p = tf.last_params
    assert p.shape == (8, 4) and p.dtype == torch.int32 and p.device.type == "cpu"
    # the draw exercises both hflip values, a vflip and more than one window (otherwise this test would prove nothing)
    assert set(p[:, 2].tolist()) == {0, 1} and 1 in p[:, 3].tolist() and len(set(map(tuple, p[:, :2].tolist()))) > 1
    assert torch.equal(p, TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(5), **kw).draw(8, 90, 120))
    assert got.shape == (8, 2, S, S, 3)
    for n, (top, left, hf, vf) in enumerate(p.tolist()):
        fixed = TF.TransformFrames(OPTS, out="frames", crop=(top, left), hflip=bool(hf), vflip=bool(vf))
        assert torch.equal(fixed(frames[n]), got[n]), n
        tables = TF.build_tables(90, 120, [3, 64, 64], crop=(top, left), hflip=bool(hf), vflip=bool(vf))
        assert np.array_equal(got[n, 1].cpu().numpy(), TF.apply_tables_numpy(frames[n, 1].cpu().numpy(), tables)), n
    # the same seed reproduces, the next call draws anew, params= applies a given draw on any transform (numpy or tensor)
    again = TF.TransformFrames(OPTS, out="frames", generator=torch.Generator().manual_seed(5), **kw)
    assert torch.equal(again(frames), got) and torch.equal(again.last_params, p)
    nxt = tf(frames)
    assert not torch.equal(tf.last_params, p) and not torch.equal(nxt, got)
    plain = TF.TransformFrames(OPTS, out="frames")
    assert torch.equal(plain(frames, params=p), got) and torch.equal(plain(frames, params=p.numpy()), got)
    assert plain.last_params is None
    assert torch.equal(tf(frames, params=p), got)                                 # given parameters: nothing is drawn
    # torch.manual_seed governs generator=None
    state = torch.get_rng_state()
    try:
        torch.manual_seed(123)
        d = TF.TransformFrames(OPTS, out="frames", **kw)
        a = d(frames)
        torch.manual_seed(123)
        assert torch.equal(d.draw(8, 90, 120), d.last_params)
    finally:
        torch.set_rng_state(state)
    assert torch.equal(a, plain(frames, params=d.last_params))
    # ranks 4 and 3: one draw; an image batch augmented per image is [N,1,H,W,3]
    clip = tf(frames[3])
    assert clip.shape == (2, S, S, 3) and tf.last_params.shape == (1, 4)
    assert torch.equal(clip, plain(frames[3], params=tf.last_params))
    image = tf(frames[3, 1])
    assert image.shape == (S, S, 3) and tf.last_params.shape == (1, 4)
    assert torch.equal(image, plain(frames[3:4, 1:2], params=tf.last_params)[0, 0])
    batch = frames[:, :1]
    per_image = tf(batch)
    assert per_image.shape == (8, 1, S, S, 3) and tf.last_params.shape == (8, 4)
    assert torch.equal(per_image, plain(batch.contiguous(), params=tf.last_params))
    # tensor outputs follow the ranks as before
    tt = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(2), **kw)
    t5 = tt(frames)
    p5 = tt.last_params                                                          # the calls below draw anew
    assert t5.shape == (8, 3, 2, S, S) and torch.equal(t5, TF.FramesToTensor(OPTS)(plain(frames, params=p5)))
    assert tt(frames[0]).shape == (3, 2, S, S) and tt(frames[0, 0]).shape == (3, S, S)
    t16 = TF.TransformFrames(OPTS, dtype=torch.bfloat16)(frames, params=p5)
    assert t16.dtype == torch.bfloat16 and torch.equal(t16, t5.to(torch.bfloat16))
    # deterministic vflip stays on the fixed-window entry point; a non-random call without params is today's path
    v = TF.TransformFrames(OPTS, out="frames", vflip=True)
    assert torch.equal(v(frames), plain(frames).flip(-3)) and v.last_params is None
    assert torch.equal(plain(frames), plain(frames, params=[[4, 16, 0, 0]] * 8))   # the centre window of 73 x 97
    # errors
    with pytest.raises(E, match="does not fit"):
        plain(frames, params=[[10, 0, 0, 0]] * 8)
    with pytest.raises(E, match="flip"):
        plain(frames, params=[[0, 0, 0, 2]] * 8)
    with pytest.raises(E, match="N = 8"):
        plain(frames, params=[[0, 0, 0, 0]] * 7)
    with pytest.raises(E, match="N = 1"):
        plain(frames[0], params=[[0, 0, 0, 0]] * 2)
    with pytest.raises(E, match="CUDA"):
        plain(frames, params=p.to(DEV))


def test_forward_frames_with_a_random_transform(ptx):
    TF = ptx.transforms
    frames = torch.from_numpy(synth_frames(16, 90, 120, 113)).view(2, 8, 90, 120, 3).to(DEV)
    model = ptx.__dict__["resnet3d18"](num_classes=400, pretrained=None)
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
    model = model.to(DEV).eval()
    model.engine().lanes = 1
    tf = TF.TransformFrames(OPTS, out="frames", random_crop=True, random_hflip=True, random_vflip=True,
                            generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        got = model.forward_frames(frames, OPTS, transform=tf)
        p = tf.last_params
        assert p.shape == (2, 4) and len(set(map(tuple, p.tolist()))) == 2
        small = TF.TransformFrames(OPTS, out="frames")(frames, params=p)
        want = model.forward_frames(small, OPTS)
        assert got.shape == (2, 400) and torch.equal(got, want)
        assert torch.equal(model.engine().forward_frames(model, frames, OPTS, transform=tf),
                           model.forward_frames(TF.TransformFrames(OPTS, out="frames")(frames, params=tf.last_params), OPTS))
