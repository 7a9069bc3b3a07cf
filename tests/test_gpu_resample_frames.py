"""GPU tests of the resize filters other than bilinear (`interpolation=`; include/ptx_amd_resample.h): negative coefficients in
every resize entry point, and the filter-aware device table builder.  References, all exact: Pillow's stored outputs
(tests/golden/resample_frames.npz: every case has a clip of noise and a saturated clip whose bicubic / Lanczos sums leave
[0, 255] on both sides), the host tables bit for bit, the fixed-window launch per clip, the RGB call on converted frames for
YUV sources.  Output buffers are pre-filled (0xFF bytes / NaN) so an element the kernel does not write fails."""
import ctypes as C
import functools
import json
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden

sys.path.insert(0, GOLDEN)
import make_resample_golden as MG                        # noqa: E402   (the cases, the inputs)

from pretorched_x_amd.testing import (synth_frames, synth_state_dict, synth_yuv420, synth_yuv420p16, yuv420_source,  # noqa: E402
                                      yuv420p16_source)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB01 = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
BGR255 = dict(input_space="BGR", input_range=[0, 255], mean=[104.0, 117.0, 123.0], std=[58.0, 57.0, 57.5])
OPTS = dict(RGB01, input_size=[3, 32, 32])
S = 32
FILTERS = MG.FILTERS


@functools.lru_cache(None)
def golden():
    blob = load_golden("resample_frames")
    return blob, json.loads(str(blob["cases"]))


CASE_NAMES = [c["name"] for c in MG.CASES]


def case_of(name):
    return {c["name"]: c for c in golden()[1]}[name]


@functools.lru_cache(None)
def case_frames(name):
    """The case's input, uint8 CUDA [2,T,H,W,3]: clip 0 noise, clip 1 saturated (made once, never written)."""
    return torch.from_numpy(MG.case_frames(case_of(name))).to(DEV)


def want_of(name, f):
    return torch.from_numpy(golden()[0]["out_%s_%s" % (name, f)]).to(DEV)


def prefilled(shape, dtype):
    if dtype == torch.uint8:
        return torch.full(shape, 0xFF, dtype=torch.uint8, device=DEV)
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def output(L, N, T, Cc, mode):
    return prefilled((N, T, S, S, Cc), torch.uint8) if mode == L.PTX_RESIZE_OUT_U8 else \
        prefilled((N, Cc, T, S, S), torch.float32 if mode == L.PTX_RESIZE_OUT_F32 else torch.bfloat16)


def run_fixed(ptx, frames, tables, mode=0, opts=None):
    """ptx_resize_frames_u8 through ctypes: frames [N,T,H,W,C] with one pair of host tables, into a pre-filled buffer."""
    L = ptx._lib
    N, T, H, W, Cc = frames.shape
    dev = [torch.from_numpy(np.array(a)).to(DEV) for a in tuple(tables["rows"]) + tuple(tables["cols"])]
    y = output(L, N, T, Cc, mode)
    norm = L.NormDesc.make(opts["mean"], opts["std"], opts["input_space"], opts["input_range"]) if opts else None
    desc = L.ResizeDesc(N, T, H, W, Cc, S, S, tables["rows"][2].shape[1], tables["cols"][2].shape[1], mode)
    assert L.lib().ptx_resize_frames_u8_supported(C.byref(desc)) == 1
    L.check(L.lib().ptx_resize_frames_u8(C.byref(desc), C.c_void_p(frames.data_ptr()), *[C.c_void_p(t.data_ptr()) for t in dev],
                                         C.c_void_p(y.data_ptr()), C.byref(norm) if norm is not None else None,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ptx_resize_frames_u8")
    torch.cuda.synchronize()
    return y


def case_transform(TF, c, f, **kw):
    return TF.TransformFrames(dict(RGB01, input_size=c["input_size"]), scale=c["scale"], preserve_aspect_ratio=False,
                              crop=(c["top"], c["left"]), hflip=bool(c["hflip"]), vflip=bool(c["vflip"]), interpolation=f, **kw)


# --------------------------------------------------------------------------------------------- 1. the fixtures
@pytest.mark.parametrize("f", FILTERS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_filter_equals_the_pil_fixtures(ptx, name, f):
    TF, L = ptx.transforms, ptx._lib
    c, frames, want = case_of(name), case_frames(name), want_of(name, f)
    tables = TF.geometry_tables(MG.geometry_row(c), S, f)
    got = run_fixed(ptx, frames, tables)
    assert got.shape == want.shape and torch.equal(got[0], want[0]), (name, f, "noise")
    assert torch.equal(got[1], want[1]), (name, f, "saturated")
    tf = case_transform(TF, c, f, out="frames")
    assert tf.interpolation == f and torch.equal(tf(frames), want), (name, f)
    if name == "down_90x160":                            # the normalised outputs: one rounding of the uint8 result
        for opts in (RGB01, BGR255):
            t = TF.FramesToTensor(opts)(want)
            got32 = run_fixed(ptx, frames, tables, L.PTX_RESIZE_OUT_F32, opts)
            assert got32.shape == t.shape and torch.equal(got32, t), (f, opts["input_space"])
            got16 = run_fixed(ptx, frames, tables, L.PTX_RESIZE_OUT_BF16, opts)
            assert got16.dtype == torch.bfloat16 and torch.equal(got16, t.to(torch.bfloat16)), (f, opts["input_space"])
        t = TF.FramesToTensor(RGB01)(want)
        assert torch.equal(case_transform(TF, c, f)(frames), t)
        assert torch.equal(case_transform(TF, c, f, dtype=torch.bfloat16)(frames), t.to(torch.bfloat16))


# --------------------------------------------------------------------------------------------- 2. the device builder
FRAME = 208                                              # frame extent of the builder sweep (every box lies inside)
BS = 8                                                   # entries per axis of the builder sweep


@functools.lru_cache(None)
def builder_rows():
    """Geometry rows of the sweep n_in 1..200 x n_out in {1, 2, 7, 32, 64} (both axes of a row take the pair, with their own
    box origin, window start and flip), fixed by a seed."""
    rng = np.random.RandomState(5)
    rows = []
    for n_in in range(1, 201):
        for n_out in (1, 2, 7, 32, 64):
            o = rng.randint(0, FRAME - n_in + 1, 2)
            s = rng.randint(0, max(n_out - BS, 0) + 1, 2)
            fl = rng.randint(0, 2, 2)
            rows.append([o[0], o[1], n_in, n_in, n_out, n_out, s[0], s[1], fl[0], fl[1]])
    return np.array(rows, np.int32)


def host_entries(TF, row, f, taps):
    """What the builder must write for one row: (lo, n, k) of both axes at pitch `taps`, with the builder's clamps of a
    window that does not fit (n_out < BS: the index stops at the last entry)."""
    out = []
    for origin, n_in, n_out, start, flip in ((row[0], row[2], row[4], row[6], row[9]), (row[1], row[3], row[5], row[7], row[8])):   # rows: vflip
        lo, n, k = TF.resize_axis_table(int(n_in), int(n_out), f)
        idx = np.minimum(start + (BS - 1 - np.arange(BS) if flip else np.arange(BS)), n_out - 1)
        kk = np.zeros((BS, taps), np.int32)
        kk[:, :k.shape[1]] = k[idx]
        out += [lo[idx] + origin, n[idx], kk]
    return out


def run_builder(ptx, rows, code, taps, clips=False, plain=False):
    L = ptx._lib
    N = len(rows)
    geo = torch.from_numpy(np.ascontiguousarray(rows)).to(DEV)
    sizes = [N * BS, N * BS, N * BS * taps] * 2
    tabs = [torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in sizes]
    desc = L.ResizeDesc(N, 1, FRAME, FRAME, 3, BS, BS, taps, taps, L.PTX_RESIZE_OUT_U8)
    ptrs = [C.c_void_p(t.data_ptr()) for t in tabs]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if clips:
        src = np.zeros(N, ptx.transforms._CLIP_SRC)
        src["H"], src["W"], src["Tv"] = FRAME, FRAME, 1
        srcs = torch.from_numpy(src.view(np.uint8)).to(DEV)
        status = L.lib().ptx_resize_build_tables_clips_filter(C.byref(desc), C.c_void_p(srcs.data_ptr()), C.c_void_p(geo.data_ptr()),
                                                              code, *ptrs, stream)
    elif plain:
        status = L.lib().ptx_resize_build_tables(C.byref(desc), C.c_void_p(geo.data_ptr()), *ptrs, stream)
    else:
        status = L.lib().ptx_resize_build_tables_filter(C.byref(desc), C.c_void_p(geo.data_ptr()), code, *ptrs, stream)
    torch.cuda.synchronize()
    return status, tabs


@pytest.mark.parametrize("f", ["nearest", "box", "bilinear", "bicubic"])
def test_device_builder_equals_the_host_tables(ptx, f):
    TF, L = ptx.transforms, ptx._lib
    code = TF.INTERPOLATIONS.index(f)
    rows = builder_rows()
    n_in, n_out = rows[:, 2].astype(np.int64), rows[:, 4].astype(np.int64)
    need = np.maximum(TF._axis_taps(n_in, n_out, rows[:, 6].astype(np.int64), BS, f), TF._axis_taps(n_in, n_out, rows[:, 7].astype(np.int64), BS, f))
    full = np.array([TF.resize_axis_table(int(a), int(b), f)[2].shape[1] for a, b in zip(n_in, n_out)])
    rows = rows[full <= L.PTX_RESIZE_MAX_TAPS]           # a pair whose table is wider than the cap is refused by the host too
    assert len(rows) >= 600 and (f == "nearest" or int(need.max()) > 1)
    taps = int(min(full.max(), L.PTX_RESIZE_MAX_TAPS))
    status, tabs = run_builder(ptx, rows, code, taps)
    assert status == 0, L.lib().ptx_last_error()
    got = [t.cpu().numpy() for t in tabs]
    want = [np.concatenate([np.asarray(e[i]).reshape(-1) for e in (host_entries(TF, r, f, taps) for r in rows)]) for i in range(6)]
    for i, name in enumerate(("row_lo", "row_n", "row_k", "col_lo", "col_n", "col_k")):
        bad = np.flatnonzero(got[i] != want[i])
        assert bad.size == 0, (f, name, bad[:5], got[i][bad[:5]], want[i][bad[:5]])
    if f == "bicubic":
        assert (want[2] < 0).any() and (want[5] < 0).any()                       # negative coefficients were compared
    status, again = run_builder(ptx, rows, code, taps, clips=True)                # the per-clip-extent form: the same bits
    assert status == 0 and all(torch.equal(a, b) for a, b in zip(again, tabs))
    if f == "bilinear":                                                          # and what the existing builder writes
        status, old = run_builder(ptx, rows, code, taps, plain=True)
        assert status == 0 and all(torch.equal(a, b) for a, b in zip(old, tabs))


def test_device_builder_refuses_the_trigonometric_filters(ptx):
    L = ptx._lib
    for code, word in ((L.PTX_RESAMPLE_HAMMING, "hamming"), (L.PTX_RESAMPLE_LANCZOS, "lanczos")):
        for clips in (False, True):
            status, tabs = run_builder(ptx, builder_rows()[:4], code, 8, clips=clips)
            assert status == 2 and word in L.lib().ptx_last_error().decode()
            assert all(bool((t == -7).all()) for t in tabs)                      # nothing was launched


# --------------------------------------------------------------------------------------------- 3. the per-clip tables launch
@pytest.mark.parametrize("f", ["bicubic", "box", "nearest"])
@pytest.mark.parametrize("name", ["down_90x160", "deep_200x120"])
def test_per_clip_tables_launch_with_mixed_geometries(ptx, name, f):
    TF = ptx.transforms
    c, frames = case_of(name), case_frames(name)
    four = torch.cat([frames, frames.flip(0)])                                   # noise, saturated, saturated, noise
    H, W = c["H"], c["W"]
    rows = [MG.geometry_row(c), MG.geometry_row(c),
            [H // 4, W // 5, H // 2, W // 2, 40, 35, 8, 3, 1, 1],                # a box, other extents, both flips
            [1, 0, H - 1, W, 32, 47, 0, 15, 0, 1]]
    tf = TF.TransformFrames(OPTS, interpolation=f, out="frames")
    got = tf(four, geometry=rows)
    assert got.shape == (4, MG.T, S, S, 3) and tf.last_geometry is None
    assert torch.equal(got[:2], want_of(name, f)), (name, f)
    for n, row in enumerate(rows):
        fixed = run_fixed(ptx, four[n:n + 1], TF.geometry_tables(row, S, f))
        assert torch.equal(fixed[0], got[n]), (name, f, n)
    t = TF.TransformFrames(dict(BGR255, input_size=[3, 32, 32]), interpolation=f)(four, geometry=rows)
    assert torch.equal(t, TF.FramesToTensor(BGR255)(got))


def test_drawn_geometries_with_bicubic(ptx):
    TF = ptx.transforms
    frames = torch.from_numpy(synth_frames(8, 90, 120, 511)).view(4, 2, 90, 120, 3).to(DEV)
    for kw in (dict(random_short_side=(32, 48), random_crop=True, random_hflip=True), dict(random_resized_crop=True, random_vflip=True)):
        tf = TF.TransformFrames(OPTS, interpolation="bicubic", out="frames", generator=torch.Generator().manual_seed(3), **kw)
        got = tf(frames)
        bil = TF.TransformFrames(OPTS, out="frames", generator=torch.Generator().manual_seed(3), **kw)
        bil(frames)
        assert torch.equal(tf.last_geometry, bil.last_geometry)                  # the draw does not depend on the filter
        for n, row in enumerate(tf.last_geometry.tolist()):
            assert np.array_equal(got[n, 1].cpu().numpy(),
                                  TF.apply_tables_numpy(frames[n, 1].cpu().numpy(), TF.geometry_tables(row, S, "bicubic"))), (kw, n)


# --------------------------------------------------------------------------------------------- 4. the per-clip windows launch
def test_per_clip_windows_launch_with_lanczos(ptx):
    TF = ptx.transforms
    c = case_of("down_90x160")
    frames = torch.cat([case_frames("down_90x160")] * 2)                          # noise, saturated, noise, saturated
    kw = dict(scale=0.75, interpolation="lanczos")                                # 90 x 160 -> 42 x 74
    tf = TF.TransformFrames(OPTS, out="frames", random_crop=True, random_hflip=True, random_vflip=True,
                            generator=torch.Generator().manual_seed(12), **kw)
    got = tf(frames)
    p = tf.last_params
    assert p.shape == (4, 4) and len(set(map(tuple, p[:, :2].tolist()))) == 4 and set(p[:, 2].tolist()) == set(p[:, 3].tolist()) == {0, 1}
    for n, (top, left, hf, vf) in enumerate(p.tolist()):
        fixed = TF.TransformFrames(OPTS, out="frames", crop=(top, left), hflip=bool(hf), vflip=bool(vf), **kw)
        assert torch.equal(fixed(frames[n]), got[n]), n
        tables = TF.build_tables(c["H"], c["W"], [3, 32, 32], 0.75, crop=(top, left), hflip=bool(hf), vflip=bool(vf), interpolation="lanczos")
        assert np.array_equal(got[n, 0].cpu().numpy(), TF.apply_tables_numpy(frames[n, 0].cpu().numpy(), tables)), n


# --------------------------------------------------------------------------------------------- 5. coefficients in global memory
def test_lanczos_with_the_coefficients_in_global_memory(ptx):
    """1080 x 1920 -> 224 x 224 out of 256 x 455: 26 taps per axis; the row stages and the intermediate image leave no room
    for the coefficient tables in LDS (k_in_lds is false), so both passes read negative coefficients from global memory."""
    TF = ptx.transforms
    opts = dict(RGB01, input_size=[3, 224, 224])
    noise = synth_frames(1, 1080, 1920, 301)[0]
    sat = MG.saturated_frames(1, 1080, 1920, 256, 455)[0]
    frames = torch.from_numpy(np.stack([noise, sat])).view(2, 1, 1080, 1920, 3).to(DEV)
    tf = TF.TransformFrames(opts, out="frames", interpolation="lanczos")
    tables = tf.tables(1080, 1920)
    assert tables["rows"][2].shape[1] == 26 and tables["cols"][2].shape[1] == 26 and (tables["rows"][2] < 0).any()
    got = tf(frames)
    assert got.shape == (2, 1, 224, 224, 3)
    for n, frame in enumerate((noise, sat)):
        assert np.array_equal(got[n, 0].cpu().numpy(), TF.apply_tables_numpy(frame, tables)), n


# --------------------------------------------------------------------------------------------- 6. SampleViews
@pytest.mark.parametrize("share", ["always", "never"])
def test_sample_views_with_bicubic_equal_transform_frames_per_view(ptx, share):
    TF = ptx.transforms
    video = torch.cat([case_frames("down_90x160")[0], case_frames("down_90x160")[1]] * 2)      # [8,90,160,3], noise and saturated
    sv = TF.SampleViews(OPTS, num_frames=2, frame_stride=3, clips=2, crops=3, interpolation="bicubic", share=share, out="frames")
    assert sv.describe(90, 160) == ("shared" if share == "always" else "per-window")
    views = sv(video)
    assert views.shape == (6, 2, S, S, 3)
    idx, wins = sv.frame_indices(8), sv.windows(90, 160)
    assert len(set(wins)) == 3
    for v in range(6):
        clip, crop = divmod(v, 3)
        tf = TF.TransformFrames(OPTS, crop=wins[crop], interpolation="bicubic", out="frames")
        assert torch.equal(views[v], tf(video[torch.from_numpy(idx[clip]).to(DEV)])), (share, v)
    t = TF.SampleViews(OPTS, num_frames=2, frame_stride=3, clips=2, crops=3, interpolation="bicubic", share=share, out="tensor")(video)
    assert torch.equal(t, TF.FramesToTensor(OPTS)(views.view(1, 12, S, S, 3)).view(3, 6, 2, S, S).transpose(0, 1))


# --------------------------------------------------------------------------------------------- 7. SampleClips
def test_sample_clips_with_bicubic_equal_transform_frames_on_gathered_frames(ptx):
    TF = ptx.transforms
    vids = [torch.cat([case_frames("down_90x160")[0], case_frames("down_90x160")[1]] * 2),      # [8,90,160,3]
            torch.cat(list(case_frames("up_31x29")) * 3)]                                       # [12,31,29,3]
    for kw in (dict(random_resized_crop=True, random_hflip=True), dict(random_short_side=(32, 40), random_crop=True, random_vflip=True)):
        sc = TF.SampleClips(OPTS, num_frames=3, frame_stride=2, clips=2, interpolation="bicubic", out="frames",
                            generator=torch.Generator().manual_seed(20), **kw)
        got = sc(vids)
        assert got.shape == (4, 3, S, S, 3) and sc.last_geometry.shape == (4, 10)
        assert set(sc.last_geometry[:, 8:].sum(1).tolist()) == {0, 1}                 # the draw holds flipped and unflipped clips
        tf = TF.TransformFrames(OPTS, interpolation="bicubic", out="frames")
        for j in range(4):
            gathered = vids[j // 2][sc.last_indices[j].to(DEV)]
            assert torch.equal(tf(gathered, geometry=sc.last_geometry[j:j + 1]), got[j]), (kw, j)
        row = sc.last_geometry[3].tolist()
        frame = vids[1][int(sc.last_indices[3, 1])].cpu().numpy()
        assert np.array_equal(got[3, 1].cpu().numpy(), TF.apply_tables_numpy(frame, TF.geometry_tables(row, S, "bicubic")))


# --------------------------------------------------------------------------------------------- 8. YUV sources
def test_nv12_and_p010_sources_with_lanczos_equal_the_rgb_call(ptx):
    TF = ptx.transforms
    H, W, N, T = 90, 122, 2, 2
    kw = dict(scale=0.75, interpolation="lanczos", out="frames")
    tf = TF.TransformFrames(OPTS, **kw)
    rnd = dict(random_crop=True, random_hflip=True, random_vflip=True)
    col = dict(matrix="bt601", color_range="limited")
    y, u, v = synth_yuv420(N * T, H, W, 41)
    src = yuv420_source((y, u, v), "nv12_pitched", DEV, lead_shape=(N, T), **col)
    rgb = torch.from_numpy(TF.yuv420_to_rgb_numpy(y, u, v, **col)).view(N, T, H, W, 3).to(DEV)
    planes = synth_yuv420p16(N * T, H, W, 43, 10, "msb")
    src16 = yuv420p16_source(planes, "p010_pitched", DEV, 10, "msb", lead_shape=(N, T), **col)
    rgb16 = torch.from_numpy(TF.yuv420p16_to_rgb_numpy(*planes, bits=10, align="msb", **col)).view(N, T, H, W, 3).to(DEV)
    for s, r in ((src, rgb), (src16, rgb16)):
        want = tf(r)
        assert torch.equal(tf(s), want), type(s).__name__
        assert np.array_equal(want[1, 1].cpu().numpy(), TF.apply_tables_numpy(r[1, 1].cpu().numpy(), tf.tables(H, W)))
        a = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(4), **rnd, **kw)
        b = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(4), **rnd, **kw)
        assert torch.equal(a(s), b(r)) and torch.equal(a.last_params, b.last_params)
        sv = TF.SampleViews(OPTS, num_frames=2, frame_stride=1, clips=1, crops=3, interpolation="lanczos")
        assert torch.equal(sv(s), sv(r))


# --------------------------------------------------------------------------------------------- 9. models
def test_forward_frames_with_a_bicubic_transform(ptx):
    TF = ptx.transforms
    opts = dict(RGB01, input_size=[3, 64, 64])
    raw = torch.from_numpy(synth_frames(16, 90, 120, 113)).view(2, 8, 90, 120, 3).to(DEV)
    model = ptx.__dict__["resnet3d18"](num_classes=400, pretrained=None)
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
    model = model.to(DEV).eval()
    model.engine().lanes = 1
    tf = TF.TransformFrames(opts, out="frames", interpolation="bicubic")
    with torch.no_grad():
        got = model.forward_frames(raw, opts, transform=tf)
        small = tf(raw)
        assert small.shape == (2, 8, 64, 64, 3) and not torch.equal(small, TF.TransformFrames(opts, out="frames")(raw))
        assert got.shape == (2, 400) and torch.equal(got, model.forward_frames(small, opts))
        assert torch.equal(got, model(TF.TransformFrames(opts, interpolation="bicubic")(raw)))
