"""GPU tests of `pretorched.transforms.SampleClips` (ptx_resize_clips_u8 / _yuv420, ptx_resize_build_tables_clips): training
clips from videos of different sizes and lengths in one launch.  Every comparison is bit-exact (`torch.equal`): per clip
against `TransformFrames` on the clip's gathered frames, against PIL's stored outputs (tests/golden/sample_clips.npz), YUV
sources against the RGB call on the converted frames, and the fixed-start form against `SampleViews`.

Batch R (S = 32, T = 4, frame_stride = 2) is the smallest that reaches every path: odd row bytes and an up-scale (37x53), a
portrait video, a video shorter than the span of 7 (indices clamp; 5-6 taps), an axis that is not resampled (32x32) and
3090-byte rows, past the 3 KiB a lane prefetches in registers (24x1030) -- the row stages are sized from W = 1030 while most
clips are narrow.  Batch G (S = 224, T = 2) pairs a 1080x1920 video (10 taps: the plan reads the coefficients from global
memory) with a 240x320 one that runs under that same plan."""
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
OPTS = dict(BGR255, input_size=[3, 32, 32])
OPTS224 = dict(RGB01, input_size=[3, 224, 224])
R_SHAPES = [(5, 37, 53), (12, 64, 48), (3, 90, 160), (9, 32, 32), (2, 24, 1030)]
SWITCHES = {"jitter": dict(random_short_side=(32, 40), random_crop=True, random_hflip=True),
            "rrc": dict(random_resized_crop=True, random_vflip=True),
            "crop": dict(random_crop=True)}
OUTPUTS = [("frames", torch.float32), ("tensor", torch.float32), ("tensor", torch.bfloat16)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(None)
def batch_r():
    return [torch.from_numpy(synth_frames(Tv, H, W, 600 + i)).to(DEV) for i, (Tv, H, W) in enumerate(R_SHAPES)]


@functools.lru_cache(None)
def batch_g():
    return [torch.from_numpy(synth_frames(2, 1080, 1920, 611)).to(DEV), torch.from_numpy(synth_frames(3, 240, 320, 612)).to(DEV)]


def per_clip_reference(TF, opts, videos, clips, idx, geo, out, dtype):
    """Every clip through TransformFrames on its gathered frames with its own geometry row."""
    tf = TF.TransformFrames(opts, out=out, dtype=dtype)
    return torch.cat([tf(videos[j // clips][idx[j].to(DEV)][None], geometry=geo[j][None]) for j in range(idx.shape[0])])


# --------------------------------------------------------------------------------------------- 1. per-clip equivalence
@pytest.mark.parametrize("clips", [1, 2])
@pytest.mark.parametrize("switches", list(SWITCHES))
def test_every_clip_of_batch_r_equals_transform_frames_on_its_gathered_frames(ptx, switches, clips):
    TF = ptx.transforms
    videos = batch_r()
    for sampling in ("dense", "segments"):
        for out, dtype in OUTPUTS:
            sc = TF.SampleClips(OPTS, num_frames=4, frame_stride=2, clips=clips, sampling=sampling, out=out, dtype=dtype,
                                generator=gen(31), **SWITCHES[switches])
            got = sc(videos)
            idx, geo = sc.last_indices, sc.last_geometry
            assert idx.shape == (5 * clips, 4) and idx.dtype == torch.int64 and geo.shape == (5 * clips, 10) and geo.dtype == torch.int32
            assert got.shape == ((5 * clips, 4, 32, 32, 3) if out == "frames" else (5 * clips, 3, 4, 32, 32))
            assert got.dtype == (torch.uint8 if out == "frames" else dtype)
            want = per_clip_reference(TF, OPTS, videos, clips, idx, geo, out, dtype)
            for j in range(5 * clips):
                assert torch.equal(got[j], want[j]), (sampling, out, dtype, j, idx[j].tolist(), geo[j].tolist())
            if sampling == "dense":
                assert idx[2 * clips].tolist() == [0, 2, 2, 2]                      # the 3-frame video clamps


def test_batch_g_runs_the_small_video_under_the_large_videos_plan(ptx):
    TF = ptx.transforms
    videos = batch_g()
    for out, dtype in OUTPUTS:
        sc = TF.SampleClips(OPTS224, num_frames=2, frame_stride=1, out=out, dtype=dtype)
        got = sc(videos)
        idx, geo = sc.last_indices, sc.last_geometry
        assert geo.tolist() == [[0, 0, 1080, 1920, 256, 455, 16, 116, 0, 0], [0, 0, 240, 320, 256, 341, 16, 58, 0, 0]]
        assert sc._checked(idx, geo, [(2, 1080, 1920), (3, 240, 320)])[2:] == (9, 9)
        want = per_clip_reference(TF, OPTS224, videos, 1, idx, geo, out, dtype)
        assert torch.equal(got, want)
    # The widest entry of the 224-entry window has 9 taps (1080 -> 256: at most floor(2 * 4.22) + 1), and at that pitch
    # resize_plan still copies the coefficients to LDS (64 592 B).  At a pitch of 10 -- PIL's own allocation is 11 -- the copy
    # would need 68 912 B, above the 64 KiB cap, and the plan reads them from global memory: the same batch through the C ABI
    # at that pitch (the builder zero-fills the unused slots), so the small video runs under the global-coefficients plan too.
    L = ptx._lib
    buf, first, n = run_abi(ptx, videos, idx.tolist(), geo.tolist(), OPTS224, L.PTX_RESIZE_OUT_U8, taps=(10, 10))
    want = per_clip_reference(TF, OPTS224, videos, 1, idx, geo, "frames", torch.float32)
    assert torch.equal(buf[first:first + n].view(want.shape), want) and (buf[first + n:] == 0xA5).all()


# --------------------------------------------------------------------------------------------- 2. PIL's stored clips
def test_given_rows_reproduce_the_stored_pil_clips(ptx):
    TF = ptx.transforms
    blob = load_golden("sample_clips")
    meta = json.loads(str(blob["meta"]))
    videos = [torch.from_numpy(synth_frames(*v["shape"], v["seed"])).to(DEV) for v in meta["videos"]]
    sc = TF.SampleClips(OPTS, num_frames=meta["T"], clips=meta["clips"], out="frames")
    got = sc(videos, indices=meta["indices"], geometry=meta["geometry"])
    assert torch.equal(got.cpu(), torch.from_numpy(blob["out"]))
    assert sc.last_indices is None and sc.last_geometry is None                    # a replay keeps no draw


# --------------------------------------------------------------------------------------------- 3. YUV sources
@pytest.mark.parametrize("layouts", [("nv12_pitched",) * 5, ("planes",) * 5, ("planes", "nv12_pitched", "planes_uv", "planes", "nv12_pitched")])
def test_yuv_batches_equal_the_rgb_call_on_the_converted_frames(ptx, layouts):
    TF = ptx.transforms
    srcs = [yuv420_source(synth_yuv420(Tv, H, W, 700 + i), layouts[i], DEV, "bt601" if i % 2 else "bt709", "full" if i == 2 else "limited")
            for i, (Tv, H, W) in enumerate(R_SHAPES)]
    rgb = [torch.from_numpy(s.to_rgb_numpy()).to(DEV) for s in srcs]
    assert [tuple(v.shape) for v in rgb] == [s + (3,) for s in R_SHAPES]
    draw = TF.SampleClips(OPTS, 4, 2, 2, generator=gen(41), **SWITCHES["jitter"])
    idx, geo = draw.draw(R_SHAPES)
    for out, dtype in OUTPUTS:
        sc = TF.SampleClips(OPTS, 4, 2, 2, out=out, dtype=dtype)
        assert torch.equal(sc(srcs, indices=idx, geometry=geo), sc(rgb, indices=idx, geometry=geo))
    # one YUV420 with planes [N,Tv,H,W] is N videos
    both = yuv420_source(synth_yuv420(6, 37, 53, 77), "planes", DEV, lead_shape=(2, 3))
    sc = TF.SampleClips(OPTS, 4, 2, 2, out="frames", generator=gen(42), random_crop=True)
    got = sc(both)
    assert got.shape == (4, 4, 32, 32, 3)
    assert torch.equal(got, sc(torch.from_numpy(both.to_rgb_numpy()).to(DEV), indices=sc.last_indices, geometry=sc.last_geometry))


# --------------------------------------------------------------------------------------------- 4. the test-time path
@pytest.mark.parametrize("sampling", ["dense", "segments"])
def test_fixed_starts_and_the_centre_crop_are_sample_views(ptx, sampling):
    TF = ptx.transforms
    video = torch.from_numpy(synth_frames(22, 45, 80, 88)).view(2, 11, 45, 80, 3).to(DEV)
    for out, dtype in OUTPUTS:
        sc = TF.SampleClips(OPTS, num_frames=4, frame_stride=2, clips=3, sampling=sampling, random_start=False, out=out, dtype=dtype)
        views = TF.SampleViews(OPTS, num_frames=4, frame_stride=2, clips=3, crops=1, sampling=sampling, out=out, dtype=dtype)(video)
        got = sc(video)
        assert torch.equal(got, views.reshape((6,) + tuple(views.shape[2:])))
        assert torch.equal(sc(list(video)), got) and torch.equal(sc(video[1])[:3], got[3:])


# --------------------------------------------------------------------------------------------- 5. in place
def test_a_strided_view_is_read_in_place_and_other_views_are_copied(ptx):
    TF = ptx.transforms
    big = torch.from_numpy(synth_frames(12, 40, 56, 91)).to(DEV)
    wide = torch.from_numpy(synth_frames(4, 40, 70, 92)).to(DEV)
    views = [big[1::2], big[3:9], wide[:, :, 7:63], wide.transpose(1, 2)]              # stepped, sliced, cut rows, transposed
    sc = TF.SampleClips(OPTS, 4, 2, 2, out="frames", generator=gen(51), random_crop=True, random_hflip=True)
    got = sc(views)
    assert torch.equal(got, sc([v.contiguous() for v in views], indices=sc.last_indices, geometry=sc.last_geometry))
    assert big[1::2].stride(0) == 2 * 40 * 56 * 3 and not big[1::2].is_contiguous()


# --------------------------------------------------------------------------------------------- 6 / 7. the C ABI directly
OPTS30 = dict(RGB01, input_size=[3, 30, 30])
ABI_GEO = [[0, 0, 37, 53, 30, 42, 0, 5, 0, 0], [0, 0, 64, 48, 40, 30, 4, 0, 1, 1]]


def run_abi(ptx, videos, idx_rows, geo_rows, opts, mode, guard=96, taps=None):
    """ptx_resize_build_tables_clips + ptx_resize_clips_u8 through ctypes, one clip per video, into the middle of a pre-filled
    buffer: y starts one element (uint8: two bytes) past the allocation.  Returns (buffer, first element of y, elements of y)."""
    L, TF = ptx._lib, ptx.transforms
    S, N, T = int(max(opts["input_size"])), len(videos), len(idx_rows[0])
    shapes = [tuple(v.shape[:3]) for v in videos]
    _, _, taps_h, taps_w = TF.SampleClips(opts, num_frames=T)._checked(np.zeros((N, T), np.int64), geo_rows, shapes)
    if taps is not None:                                             # a wider pitch than the widest entry
        assert taps[0] >= taps_h and taps[1] >= taps_w
        taps_h, taps_w = taps
    src = (L.ClipSrc * N)()
    for i, v in enumerate(videos):
        src[i].base, src[i].stride_t, src[i].H, src[i].W, src[i].Tv = v.data_ptr(), v.stride(0), v.shape[1], v.shape[2], v.shape[0]
    d_src = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to(DEV)
    d_idx = torch.tensor(idx_rows, dtype=torch.int32, device=DEV)
    d_geo = torch.tensor(geo_rows, dtype=torch.int32, device=DEV)
    sizes = [N * S, N * S, N * S * taps_h, N * S, N * S, N * S * taps_w]
    tab = torch.zeros(sum(sizes), dtype=torch.int32, device=DEV)
    tabs = [C.c_void_p(tab.data_ptr() + int(o) * 4) for o in np.cumsum([0] + sizes[:-1])]
    n = N * T * S * S * 3
    if mode == L.PTX_RESIZE_OUT_U8:
        first, buf = 2, torch.full((2 + n + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    else:
        first, buf = 1, torch.full((1 + n + guard,), float("nan"), device=DEV,
                                   dtype=torch.float32 if mode == L.PTX_RESIZE_OUT_F32 else torch.bfloat16)
    desc = L.ResizeDesc(N, T, max(s[1] for s in shapes), max(s[2] for s in shapes), 3, S, S, taps_h, taps_w, mode)
    norm = L.NormDesc.make(opts["mean"], opts["std"], opts["input_space"], opts["input_range"])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.lib().ptx_resize_clips_u8_supported(C.byref(desc)) == 1
    L.check(L.lib().ptx_resize_build_tables_clips(C.byref(desc), C.c_void_p(d_src.data_ptr()), C.c_void_p(d_geo.data_ptr()), *tabs,
                                                  stream), "ptx_resize_build_tables_clips")
    L.check(L.lib().ptx_resize_clips_u8(C.byref(desc), C.c_void_p(d_src.data_ptr()), C.c_void_p(d_idx.data_ptr()), *tabs,
                                        C.c_void_p(buf.data_ptr() + first * buf.element_size()), C.byref(norm), stream),
            "ptx_resize_clips_u8")
    torch.cuda.synchronize()
    return buf, first, n


def abi_reference(ptx, videos, idx_rows, geo_rows, opts, out, dtype):
    TF = ptx.transforms
    return per_clip_reference(TF, opts, videos, 1, torch.tensor(idx_rows), torch.tensor(geo_rows, dtype=torch.int32), out, dtype)


@pytest.mark.parametrize("out,dtype", OUTPUTS)
def test_every_element_is_written_and_nothing_around_it(ptx, out, dtype):
    """S = 30: rows are no multiple of 4 elements, so every output takes the scalar-store path.  y starts 2 bytes into the
    buffer for uint8 and bf16; the fp32 output starts one float in (a float pointer 2 bytes off its alignment is not a
    tensor any caller can hold), which is as far from the 16-byte alignment of the vector path."""
    L = ptx._lib
    mode = {("frames", torch.float32): L.PTX_RESIZE_OUT_U8, ("tensor", torch.float32): L.PTX_RESIZE_OUT_F32,
            ("tensor", torch.bfloat16): L.PTX_RESIZE_OUT_BF16}[(out, dtype)]
    videos = batch_r()[:2]
    idx_rows = [[4, 0, 2], [11, 3, 3]]
    buf, first, n = run_abi(ptx, videos, idx_rows, ABI_GEO, OPTS30, mode)
    want = abi_reference(ptx, videos, idx_rows, ABI_GEO, OPTS30, out, dtype)
    assert want.numel() == n
    y = buf[first:first + n]
    if mode == L.PTX_RESIZE_OUT_U8:
        assert (buf[:first] == 0xA5).all() and (buf[first + n:] == 0xA5).all()    # the guard bytes are untouched
    else:
        assert not torch.isnan(y.float()).any()                                    # every element was written
        assert torch.isnan(buf[:first].float()).all() and torch.isnan(buf[first + n:].float()).all()
    assert torch.equal(y.view(want.shape), want)


def test_frame_indices_outside_the_video_give_the_clamped_frames(ptx):
    L = ptx._lib
    videos = batch_r()[:2]
    buf, first, n = run_abi(ptx, videos, [[-3, 1, 5 + 7], [12 + 7, -3, 6]], ABI_GEO, OPTS30, L.PTX_RESIZE_OUT_U8)
    want = abi_reference(ptx, videos, [[0, 1, 4], [11, 0, 6]], ABI_GEO, OPTS30, "frames", torch.float32)
    assert torch.equal(buf[first:first + n].view(want.shape), want)


# --------------------------------------------------------------------------------------------- 8. replay, determinism
def test_replay_and_equally_seeded_samplers(ptx):
    TF = ptx.transforms
    videos = batch_r()
    for sampling in ("dense", "segments"):
        a = TF.SampleClips(OPTS, 4, 2, 2, sampling, generator=gen(61), **SWITCHES["jitter"])
        b = TF.SampleClips(OPTS, 4, 2, 2, sampling, generator=gen(61), **SWITCHES["jitter"])
        ya, yb = a(videos), b(tuple(videos))
        assert torch.equal(ya, yb) and torch.equal(a.last_indices, b.last_indices) and torch.equal(a.last_geometry, b.last_geometry)
        idx, geo = a.last_indices, a.last_geometry
        assert torch.equal(a(videos, indices=idx, geometry=geo), ya)
        assert torch.equal(TF.SampleClips(OPTS, 4, 2, 2)(videos, indices=idx.numpy(), geometry=geo.tolist()), ya)   # on any sampler
        assert torch.equal(a.last_indices, idx)                                    # a replay keeps the last draw
        assert not torch.equal(a(videos), ya)                                      # the next call draws again


# --------------------------------------------------------------------------------------------- 9. models
def test_forward_frames_takes_a_sampler_as_its_transform(ptx):
    TF = ptx.transforms
    with torch.no_grad():
        model = ptx.__dict__["resnet3d18"](num_classes=339, pretrained=None)
        model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
        model = model.to(DEV).eval()
        model.engine().lanes = 1
        videos = batch_r()[:2]
        kw = dict(num_frames=4, frame_stride=2, clips=2, out="frames", **SWITCHES["jitter"])
        sc, ref = TF.SampleClips(OPTS, generator=gen(71), **kw), TF.SampleClips(OPTS, generator=gen(71), **kw)
        got = model.forward_frames(videos, OPTS, transform=sc)
        assert got.shape == (4, 339) and torch.equal(got, model.forward_frames(ref(videos), OPTS))
        assert torch.equal(sc.last_geometry, ref.last_geometry) and len(set(map(tuple, sc.last_geometry.tolist()))) > 1
        assert torch.equal(model.engine().forward_frames(model, videos, OPTS, transform=sc), model.forward_frames(ref(videos), OPTS))
        with pytest.raises(ptx._lib.PtxError, match="transform must be"):
            model.forward_frames(videos, OPTS, transform=TF.SampleClips(OPTS, 4, 2))

        sf = ptx.slowfast.resnet18(mode="sf", num_classes=10)
        sf.load_state_dict(synth_state_dict(sf.state_dict(), 1234))
        sf = sf.to(DEV).eval()
        sf.engine().lanes = 1
        o64 = dict(BGR255, input_size=[3, 64, 64])
        videos = [torch.from_numpy(synth_frames(40, 90, 120, 4242)).to(DEV), torch.from_numpy(synth_frames(33, 80, 72, 4243)).to(DEV)]
        kw = dict(num_frames=32, frame_stride=1, out="frames", random_crop=True, random_hflip=True)
        sc, ref = TF.SampleClips(o64, generator=gen(72), **kw), TF.SampleClips(o64, generator=gen(72), **kw)
        got = sf.forward_frames(videos, o64, transform=sc)
        assert got.shape == (2, 10) and torch.equal(got, sf.forward_frames(ref(videos), o64))
