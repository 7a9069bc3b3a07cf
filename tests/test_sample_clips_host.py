"""No-GPU tests of `pretorched.transforms.SampleClips` (training clips from videos of any sizes and lengths): the temporal
draw rules, the draw order against `TransformFrames.draw_geometry`, determinism, `check` and the call's host-side validation
(each naming the clip or the video), the two ctypes structs and the host checks of the five C entry points, and the numpy
model (`geometry_tables` + `apply_tables_numpy` on the indexed frames) against the stored PIL outputs
(tests/golden/sample_clips.npz, written by tests/golden/make_sample_clips_golden.py with PIL only)."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

from pretorched_x_amd.testing import synth_frames

OPTS = dict(input_size=[3, 32, 32], input_space="RGB", input_range=[0, 1], mean=[0.4, 0.4, 0.4], std=[0.2, 0.2, 0.2])
SHAPES = [(5, 37, 53), (12, 64, 48), (3, 90, 160), (9, 32, 32), (2, 24, 1030)]
SWITCHES = [dict(random_short_side=(32, 40), random_crop=True, random_hflip=True), dict(random_resized_crop=True, random_vflip=True),
            dict(random_crop=True), dict()]


def gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("Tv", [1, 3, 4, 6, 7, 8, 30])
def test_dense_starts_stay_in_range_and_short_videos_consume_nothing(ptx, Tv):
    T, stride = 4, 2
    span = (T - 1) * stride + 1                                                    # 7
    g = gen(5)
    sc = ptx.transforms.SampleClips(OPTS, num_frames=T, frame_stride=stride, generator=g)
    before = g.get_state()
    rows = [sc.draw_indices(Tv) for _ in range(40)]
    if Tv < span:
        assert torch.equal(g.get_state(), before)                                 # nothing drawn
        assert all(r == [min(i * stride, Tv - 1) for i in range(T)] for r in rows)
    else:
        g2 = gen(5)
        for r in rows:                                                             # one randint per clip, the literal call
            start = int(torch.randint(0, Tv - span + 1, (1,), generator=g2))
            assert r == [start + i * stride for i in range(T)] and 0 <= start and r[-1] <= Tv - 1
        assert torch.equal(g.get_state(), g2.get_state())
        if Tv > span:
            assert len({r[0] for r in rows}) > 1


@pytest.mark.parametrize("Tv", [1, 3, 4, 5, 12, 31])                              # Tv < T, Tv == T, Tv = 1, uneven segments
def test_every_segments_index_lies_in_its_segment(ptx, Tv):
    T = 4
    g, g2 = gen(9), gen(9)
    sc = ptx.transforms.SampleClips(OPTS, num_frames=T, sampling="segments", generator=g)
    seen = set()
    for _ in range(30):
        row = sc.draw_indices(Tv)
        r = torch.randint(0, 2 ** 30, (T,), generator=g2).tolist()                 # one call per clip
        for i in range(T):
            lo = (i * Tv) // T
            hi = max(((i + 1) * Tv) // T, lo + 1)
            assert lo <= row[i] < hi <= max(Tv, lo + 1) and row[i] < Tv and row[i] == lo + r[i] % (hi - lo)
        seen.add(tuple(row))
    assert torch.equal(g.get_state(), g2.get_state())
    assert len(seen) > 1 or Tv <= T


@pytest.mark.parametrize("sampling", ["dense", "segments"])
@pytest.mark.parametrize("kw", SWITCHES)
def test_fixed_starts_take_the_test_time_rows_and_the_geometry_is_draw_geometrys(ptx, kw, sampling):
    TF = ptx.transforms
    sc = TF.SampleClips(OPTS, num_frames=4, frame_stride=2, clips=3, sampling=sampling, random_start=False, generator=gen(21), **kw)
    idx, geo = sc.draw(SHAPES)
    assert idx.dtype == torch.int64 and geo.dtype == torch.int32 and idx.shape == (15, 4) and geo.shape == (15, 10)
    assert not idx.is_cuda and not geo.is_cuda
    tf = TF.TransformFrames(OPTS, generator=gen(21), **kw)
    want = torch.cat([tf.draw_geometry(1, H, W) for _, H, W in SHAPES for _ in range(3)])
    assert torch.equal(geo, want)
    for i, (Tv, _, _) in enumerate(SHAPES):
        assert np.array_equal(idx[3 * i:3 * i + 3].numpy(), TF.clip_frame_indices(Tv, 4, 2, 3, sampling))
    if not kw:                                                                     # a fixed transform: one row per video
        assert all(torch.equal(geo[3 * i], geo[3 * i + 2]) for i in range(len(SHAPES)))
    a, b = sc.check(idx, geo, SHAPES)
    assert torch.equal(a, idx) and torch.equal(b, geo)                             # a draw is always valid


def test_the_order_is_video_by_video_clip_by_clip_temporal_then_spatial(ptx):
    TF = ptx.transforms
    kw = dict(random_crop=True, random_hflip=True)
    g, g2 = gen(4), gen(4)
    sc = TF.SampleClips(OPTS, num_frames=4, frame_stride=2, clips=2, generator=g, **kw)
    idx, geo = sc.draw(SHAPES)
    tf = TF.TransformFrames(OPTS, generator=g2, **kw)
    for j in range(2 * len(SHAPES)):
        Tv, H, W = SHAPES[j // 2]
        start = int(torch.randint(0, Tv - 7 + 1, (1,), generator=g2)) if Tv >= 7 else 0
        assert idx[j].tolist() == [min(start + 2 * i, Tv - 1) for i in range(4)]
        assert torch.equal(geo[j], tf.draw_geometry(1, H, W)[0])
    assert torch.equal(g.get_state(), g2.get_state())


def test_equally_seeded_samplers_draw_the_same_rows(ptx):
    TF = ptx.transforms
    for kw in SWITCHES:
        for sampling in ("dense", "segments"):
            a = TF.SampleClips(OPTS, 4, 2, 2, sampling, generator=gen(8), **kw).draw(SHAPES)
            b = TF.SampleClips(OPTS, 4, 2, 2, sampling, generator=gen(8), **kw).draw(SHAPES)
            c = TF.SampleClips(OPTS, 4, 2, 2, sampling, generator=gen(9), **kw).draw(SHAPES)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            if kw:
                assert not torch.equal(a[1], c[1])
    state = torch.get_rng_state()                                                  # generator=None: torch's default generator
    try:
        torch.manual_seed(3)
        a = TF.SampleClips(OPTS, 4, 2, random_crop=True).draw(SHAPES)
        torch.manual_seed(3)
        b = TF.SampleClips(OPTS, 4, 2, random_crop=True).draw(SHAPES)
    finally:
        torch.set_rng_state(state)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_check_and_the_call_refuse_bad_rows_and_bad_batches_and_name_the_clip(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    sc = TF.SampleClips(OPTS, num_frames=4, frame_stride=2, clips=2, generator=gen(1), random_crop=True)
    idx, geo = sc.draw(SHAPES)
    with pytest.raises(E, match=r"indices holds 9 clips, 5 videos x 2 clips need 10"):
        sc.check(idx[:9], geo, SHAPES)
    with pytest.raises(E, match=r"geometry holds 11 clips"):
        sc.check(idx, torch.cat([geo, geo[:1]]), SHAPES)
    with pytest.raises(E, match=r"indices must be \[N\*clips, 4\]"):
        sc.check(idx[:, :3], geo, SHAPES)
    bad = idx.clone()
    bad[5, 2] = 3                                                                  # clip 5 is video 2 (Tv = 3); 3 fits video 1
    with pytest.raises(E, match=re.escape("clip 5 (videos[2]): frame index 3 (position 2) is outside [0, 3)")):
        sc.check(bad, geo, SHAPES)
    bad[5, 2] = -1
    with pytest.raises(E, match=r"clip 5 \(videos\[2\]\): frame index -1"):
        sc.check(bad, geo, SHAPES)
    # a box outside video 0's 37x53 frame that fits video 2's 90x160
    box = geo.clone()
    box[1] = torch.tensor([0, 0, 60, 100, 32, 53, 0, 0, 0, 0], dtype=torch.int32)
    with pytest.raises(E, match=r"clip 1 \(videos\[0\], 37x53\): .*geometry\[0\]: the 60x100 box at \(0, 0\) is empty or does not lie "
                                r"inside the 37x53 frame"):
        sc.check(idx, box, SHAPES)
    box[5] = box[1]
    sc.check(idx, torch.cat([geo[:5], box[5:6], geo[6:]]), SHAPES)                # the same row on the larger video is fine
    with pytest.raises(E, match=r"must hold integers"):
        sc.check(idx.float(), geo, SHAPES)
    for shapes in ([], [(3, 4)], [(0, 4, 4)], None):
        with pytest.raises(E, match="shapes must be a non-empty list|is empty"):
            sc.draw(shapes)
    with pytest.raises(E, match=r"clip 2 \(videos\[1\], 20x64\): .*does not fit the resized 36x115 frame"):   # a window that leaves it
        TF.SampleClips(OPTS, 4, 2, 2, crop=(10, 0)).draw([(4, 80, 64), (4, 20, 64)])

    # the call: everything is validated before a device is needed
    vids = [torch.zeros(s + (3,), dtype=torch.uint8) for s in SHAPES]
    meta = torch.device("meta")
    for kind, tensor in (("indices", idx), ("geometry", geo)):
        if torch.cuda.is_available():
            args = dict(indices=idx, geometry=geo)
            args[kind] = tensor.cuda()
            with pytest.raises(E, match="%s must be an integer array or a CPU tensor .* got a CUDA tensor" % kind):
                sc(vids, **args)
    with pytest.raises(E, match="given together"):
        sc(vids, indices=idx)
    with pytest.raises(E, match=r"videos\[3\] is on meta, videos\[0\] on cpu"):
        sc(vids[:3] + [torch.zeros((9, 32, 32, 3), dtype=torch.uint8, device=meta)] + vids[4:])
    with pytest.raises(E, match=r"videos\[1\] must be a uint8 tensor, got torch.float32"):
        sc([vids[0], vids[1].float()])
    with pytest.raises(E, match=r"videos\[1\]: expected \[Tv,H,W,3\]"):
        sc([vids[0], vids[1][0]])
    with pytest.raises(E, match="empty batch"):
        sc([])
    with pytest.raises(E, match="videos must be a list"):
        sc(None)
    with pytest.raises(E, match=r"videos\[0\] is empty"):
        sc([vids[0][:0]])
    frame = TF.YUV420(torch.zeros(36, 52, dtype=torch.uint8), torch.zeros(18, 26, 2, dtype=torch.uint8))
    with pytest.raises(E, match=r"expected a YUV420 source with planes \[N,Tv,H,W\] or \[Tv,H,W\], got 0 leading"):
        sc(frame)
    video = TF.YUV420(torch.zeros(2, 5, 36, 52, dtype=torch.uint8), torch.zeros(2, 5, 18, 26, 2, dtype=torch.uint8))
    with pytest.raises(E, match=r"videos\[0\]: expected a YUV420 source with planes \[Tv,H,W\], got 2 leading"):
        sc([video])
    with pytest.raises(E, match=r"videos\[1\]: a batch is all tensors or all YUV420"):
        sc([vids[0], frame])
    with pytest.raises(E, match=r"clip 5 \(videos\[2\]\): frame index 7"):        # replayed rows are checked against the batch
        far = idx.clone()
        far[5, 0] = 7
        sc(vids, indices=far, geometry=geo)
    with pytest.raises(E, match="CUDA"):                                           # valid rows: only then the device
        sc(vids, indices=idx, geometry=geo)
    with pytest.raises(E, match="CUDA"):
        sc(video)
    assert sc.last_indices is None and sc.last_geometry is None
    for kw, match in ((dict(num_frames=0), "num_frames must be a positive integer"), (dict(clips=True), "clips must be"),
                      (dict(sampling="uniform"), "sampling must be"), (dict(random_crop=True, crop=(0, 0)), "cannot be combined"),
                      (dict(random_short_side=(31, 40)), "a >= 32"), (dict(out="frames", dtype=torch.bfloat16), "out='frames'")):
        with pytest.raises(E, match=match):
            TF.SampleClips(OPTS, **kw)


def test_apply_frames_transform_takes_a_sampler_with_frames_output_only(ptx):
    TF, E = ptx.transforms, ptx._lib.PtxError
    vids = [torch.zeros((3, 40, 40, 3), dtype=torch.uint8)]
    for bad in (TF.SampleClips(OPTS, 4, 2), TF.SampleViews(OPTS, 4, 2, 1, 1), object()):
        with pytest.raises(E, match="transform must be a pretorched.transforms.TransformFrames with out='frames'"):
            TF.apply_frames_transform(bad, vids)
    with pytest.raises(E, match="SampleClips: videos must be uint8 CUDA tensors"):   # accepted: it reaches the sampler's call
        TF.apply_frames_transform(TF.SampleClips(OPTS, 4, 2, out="frames"), vids)


def test_the_structs_mirror_the_header_and_the_census_holds(ptx):
    L = ptx._lib
    assert C.sizeof(L.ClipSrc) == 32 and [n for n, _ in L.ClipSrc._fields_] == ["base", "stride_t", "H", "W", "Tv", "reserved"]
    assert [(L.ClipSrc.base.offset, L.ClipSrc.stride_t.offset, L.ClipSrc.H.offset, L.ClipSrc.Tv.offset)] == [(0, 8, 16, 24)]
    assert C.sizeof(L.ClipSrcYuv420) == C.sizeof(L.Yuv420Src) + 16 == 112
    assert [n for n, _ in L.ClipSrcYuv420._fields_] == ["planes", "H", "W", "Tv", "reserved"] and L.ClipSrcYuv420.H.offset == 96
    assert ptx.transforms._CLIP_SRC.itemsize == 32 and list(ptx.transforms._CLIP_SRC.names) == [n for n, _ in L.ClipSrc._fields_]
    header = re.sub(r"/\*.*?\*/", "", open(L.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"typedef struct ptx_clip_src \{(.*?)\} ptx_clip_src;", header, re.S)
    assert re.findall(r"(\w+)\s*[;,]", m.group(1)) == ["base", "stride_t", "H", "W", "Tv", "reserved"]
    m = re.search(r"typedef struct ptx_clip_src_yuv420 \{(.*?)\} ptx_clip_src_yuv420;", header, re.S)
    assert re.findall(r"(\w+)\s*[;,]", m.group(1)) == ["planes", "H", "W", "Tv", "reserved"]
    new = ["ptx_resize_build_tables_clips", "ptx_resize_clips_u8", "ptx_resize_clips_u8_supported", "ptx_resize_clips_yuv420",
           "ptx_resize_clips_yuv420_supported"]
    declared = set(L.header_symbols())
    assert set(new) <= declared == set(L.SIGNATURES) and not set(new) & set(L.EXPERIMENTAL)
    assert len(declared - set(L.EXPERIMENTAL)) == 117 and len(L.EXPERIMENTAL) == 10
    integ = open(L.HEADER_PATH.replace("include/ptx_amd.h", "INTEGRATION.md")).read()
    assert "117 stable" in integ and "10 experimental" in integ and "92 stable" in integ


def test_the_entry_points_check_on_the_host(ptx):
    """Null pointers, extents and the tap cap are refused before a device is needed."""
    L = ptx._lib
    lib = L.lib()
    d = L.ResizeDesc(10, 4, 90, 1030, 3, 32, 32, 6, 6, L.PTX_RESIZE_OUT_U8)
    assert lib.ptx_resize_clips_u8_supported(C.byref(d)) == 1 and lib.ptx_resize_clips_yuv420_supported(C.byref(d)) == 1
    one = C.c_void_p(16)
    tabs = [one] * 6
    assert lib.ptx_resize_clips_u8(C.byref(d), None, one, *tabs, one, None, None) == 1
    assert b"ptx_resize_clips_u8: null pointer" in lib.ptx_last_error()
    assert lib.ptx_resize_clips_u8(C.byref(d), one, None, *tabs, one, None, None) == 1
    assert lib.ptx_resize_clips_u8(C.byref(d), one, one, *tabs, None, None, None) == 1
    assert lib.ptx_resize_clips_u8(C.byref(d), one, one, one, one, None, one, one, one, one, None, None) == 1
    assert lib.ptx_resize_clips_u8(None, one, one, *tabs, one, None, None) == 1
    assert b"null descriptor" in lib.ptx_last_error()
    assert lib.ptx_resize_clips_yuv420(C.byref(d), None, one, *tabs, one, None, None) == 1
    assert b"ptx_resize_clips_yuv420: null pointer" in lib.ptx_last_error()
    assert lib.ptx_resize_clips_yuv420(C.byref(d), one, None, *tabs, one, None, None) == 1
    assert lib.ptx_resize_build_tables_clips(C.byref(d), None, one, *tabs, None) == 1
    assert b"ptx_resize_build_tables_clips: null pointer" in lib.ptx_last_error()
    assert lib.ptx_resize_build_tables_clips(C.byref(d), one, None, *tabs, None) == 1
    assert lib.ptx_resize_build_tables_clips(C.byref(d), one, one, one, one, one, one, one, None, None) == 1
    f32 = L.ResizeDesc(10, 4, 90, 1030, 3, 32, 32, 6, 6, L.PTX_RESIZE_OUT_F32)
    assert lib.ptx_resize_clips_u8(C.byref(f32), one, one, *tabs, one, None, None) == 1
    assert b"null norm descriptor" in lib.ptx_last_error()
    for bad, status, text in ((L.ResizeDesc(10, 4, 0, 1030, 3, 32, 32, 6, 6, 0), 1, b"non-positive extent"),
                              (L.ResizeDesc(10, 4, 90, 1030, 3, 32, 32, 6, L.PTX_RESIZE_MAX_TAPS + 1, 0), 2, b"PTX_RESIZE_MAX_TAPS"),
                              (L.ResizeDesc(10, 4, 90, 1030, 3, 32, 32, 6, 6, 7), 1, b"out_mode"),
                              (L.ResizeDesc(10, 4, 90, 30000, 3, 32, 32, 6, 6, 0), 2, b"LDS staging")):
        assert lib.ptx_resize_clips_u8_supported(C.byref(bad)) == 0 and lib.ptx_resize_clips_yuv420_supported(C.byref(bad)) == 0
        assert lib.ptx_resize_clips_u8(C.byref(bad), one, one, *tabs, one, None, None) == status
        assert text in lib.ptx_last_error()
        assert lib.ptx_resize_clips_yuv420(C.byref(bad), one, one, *tabs, one, None, None) == status
        assert lib.ptx_resize_build_tables_clips(C.byref(bad), one, one, *tabs, None) == status
    c4 = L.ResizeDesc(10, 4, 90, 1030, 4, 32, 32, 6, 6, 0)
    assert lib.ptx_resize_clips_u8_supported(C.byref(c4)) == 1 and lib.ptx_resize_clips_yuv420_supported(C.byref(c4)) == 0
    assert lib.ptx_resize_clips_yuv420(C.byref(c4), one, one, *tabs, one, None, None) == 1
    assert b"converts to 3 channels" in lib.ptx_last_error()
    # batch G's plan: 1080x1920 -> 224 with 10 taps does not fit the coefficients in LDS, and still runs
    g = L.ResizeDesc(2, 2, 1080, 1920, 3, 224, 224, 10, 10, L.PTX_RESIZE_OUT_U8)
    assert lib.ptx_resize_clips_u8_supported(C.byref(g)) == 1


def test_the_numpy_model_reproduces_the_stored_pil_clips(ptx):
    TF = ptx.transforms
    blob = load_golden("sample_clips")
    meta = json.loads(str(blob["meta"]))
    S, T, K = meta["S"], meta["T"], meta["clips"]
    assert (S, T, K) == (32, 4, 2) and [v["shape"] for v in meta["videos"]] == [[5, 37, 53], [12, 64, 48], [3, 90, 160]]
    want = blob["out"]
    assert want.shape == (6, T, S, S, 3) and want.dtype == np.uint8
    videos = [synth_frames(*v["shape"], v["seed"]) for v in meta["videos"]]
    sc = TF.SampleClips(OPTS, num_frames=T, clips=K, out="frames")
    idx, geo = sc.check(meta["indices"], meta["geometry"], [tuple(v["shape"]) for v in meta["videos"]])
    for j in range(6):
        tables = TF.geometry_tables(geo[j].tolist(), S)
        for t in range(T):
            assert np.array_equal(TF.apply_tables_numpy(videos[j // K][int(idx[j, t])], tables), want[j, t]), (j, t)
    assert {tuple(g[8:]) for g in meta["geometry"]} == {(0, 0), (1, 0), (0, 1), (1, 1)}
