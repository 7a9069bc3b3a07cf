"""GPU tests of BatchMix (`pretorched.transforms.BatchMix`, include/ptx_amd_mix.h): RandomErasing per clip and MixUp / CutMix across
the clips of a batch in one launch.  Every comparison is exact (`torch.equal`) against `batch_mix_torch`, the torch-on-CPU statement
of the contract, of the CPU copy of `FramesToTensor(opts)(frames)` (bf16: rounded once) or of the input clip.  The direct launches
go through ctypes into NaN-filled outputs, so an element the kernel does not write fails.  The shapes are chosen for where the
kernel can go wrong: a width with no vector-friendly factor (heads and tails, groups that cross rows), T * H * W not a multiple of
four (no whole-group stores), one clip that is its own partner, a frame of more than one workgroup, sources at odd byte / element
offsets."""
import ctypes as C

import numpy as np
import pytest
import torch

from pretorched_x_amd.testing import synth_color_frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RGB01 = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
BGR255 = dict(input_space="BGR", input_range=[0, 255], mean=[104.0, 117.0, 123.0], std=[58.0, 57.0, 57.5])
OPTS = dict(RGB01, input_size=[3, 32, 32])
VALUE = (0.25, -1.5, 3.0)
SHAPES = [(3, 2, 9, 13), (4, 3, 16, 20), (1, 2, 9, 13), (2, 1, 66, 67)]      # the last: two workgroups per frame, every pass of a lane
SOURCES = ["u8_f32", "u8_bf16", "f32", "bf16"]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def row(partner, mode=0, lam=1.0, box=(0, 0, 0, 0), erase=None):
    return [partner, mode] + list(box) + ([1] + list(erase) if erase is not None else [0, 0, 0, 0, 0]), lam


def params_of(entries):
    return np.array([e[0] for e in entries], np.int64), np.array([e[1] for e in entries], np.float64)


def hand_draws(N, H, W):
    """Hand-written draws for N clips of H x W frames, by name."""
    cyc = [(i - 1) % N for i in range(N)]
    rev = [(N - 1 - i) for i in range(N)] if N > 2 else cyc      # a partner permutation that is no roll (N = 4: two swaps)
    if N == 3:
        rev = [1, 0, 2]
    d = {}
    # CutMix boxes touching each edge, an empty box and the whole frame, under the cyclic partner
    boxes = [(0, 3, 4, W - 2), (2, 0, H - 1, 5), (H - 3, 2, H, W - 1), (1, W - 4, H - 2, W), (4, 6, 4, 6), (0, 0, H, W), (3, 5, 3, W), (0, 0, 1, 1)]
    for k in range(0, len(boxes), max(N, 1)):
        chunk = [boxes[(k + i) % len(boxes)] for i in range(N)]
        d["cutmix_boxes_%d" % k] = params_of([row(cyc[i], 2, 0.5, chunk[i]) for i in range(N)])
    # erase rectangles that straddle the CutMix box boundary in the clip and in its partner (constant and noise fills use these)
    d["cutmix_erase_straddle"] = params_of([row(cyc[i], 2, 0.4, (2, 3, H - 2, W - 3), (1 + i % 2, 1, 3, 4 + i % 3)) for i in range(N)])
    # MixUp with every clip erased; lam 0 and 1 and an ordinary one; a non-cyclic permutation
    lams = [0.0, 1.0, 0.3, 0.7231]
    d["mixup_erased"] = params_of([row(cyc[i], 1, lams[(i + 2) % 4], erase=(i % 3, (2 * i) % 4, H - 3, W - 5)) for i in range(N)])
    d["mixup_lam_edges"] = params_of([row(cyc[i], 1, lams[i % 4]) for i in range(N)])
    d["permutation"] = params_of([row(rev[i], 1 + i % 2, 0.6, (1, 1, H - 1, W - 2), (0, 0, 2, W - 1) if i % 2 else None) for i in range(N)])
    # every kind in one batch: an unmixed erased clip, an untouched clip, an erase of zero extent, a whole-frame erase
    kinds = [row(0 if N == 1 else i, 0, 1.0, erase=(2, 2, 4, 7)) if i % 4 == 0 else row(cyc[i], 1, 0.25, erase=(H, W, 0, 0)) if i % 4 == 1 else
             row(i, 0, 1.0) if i % 4 == 2 else row(cyc[i], 2, 0.5, (0, 0, H // 2, W), (0, 0, H, W)) for i in range(N)]
    d["every_kind"] = params_of(kinds)
    return d


def seeded_draws(ptx, N, H, W):
    TF = ptx.transforms
    out = {}
    for seed in range(3):
        for mode in ("batch", "clip"):
            bm = TF.BatchMix(prob=0.9, erase_prob=0.7, mode=mode, generator=gen(100 + seed))
            out["seed%d_%s" % (seed, mode)] = tuple(t.numpy() for t in bm.draw(N, H, W))
    return out


def make_source(ptx, kind, N, T, H, W, opts, seed):
    """(device source for the kernel, CPU clip that `batch_mix_torch` takes, src_mode, dtype, norm)."""
    L, TF = ptx._lib, ptx.transforms
    if kind.startswith("u8"):
        frames = torch.from_numpy(synth_color_frames(N, T, H, W, seed))
        buf = torch.zeros(frames.numel() + 1, dtype=torch.uint8, device=DEV)          # viewed at byte offset 1 of a larger buffer
        src = buf[1:].view(frames.shape)
        src.copy_(frames)
        assert src.data_ptr() % 4 == 1 and src.is_contiguous()
        dtype = torch.float32 if kind == "u8_f32" else torch.bfloat16
        ref = TF.FramesToTensor(opts)(src).cpu().to(dtype)
        return src, ref, L.PTX_MIX_SRC_U8, dtype, L.NormDesc.make(opts["mean"], opts["std"], opts["input_space"], opts["input_range"])
    dtype = torch.float32 if kind == "f32" else torch.bfloat16
    clip = torch.randn(N, 3, T, H, W, generator=gen(seed)).to(dtype)
    buf = torch.zeros(clip.numel() + 3, dtype=dtype, device=DEV)                      # viewed at element offset 3
    src = buf[3:].view(clip.shape)
    src.copy_(clip)
    assert src.data_ptr() % 8 != 0 and src.is_contiguous()
    return src, clip, L.PTX_MIX_SRC_F32 if kind == "f32" else L.PTX_MIX_SRC_BF16, dtype, None


def run_kernel(ptx, src, src_mode, dtype, norm, params, value=0, noise=None):
    """ptx_batch_mix_apply through ctypes into a NaN-filled output."""
    L, TF = ptx._lib, ptx.transforms
    lib = L.lib()
    if src_mode == L.PTX_MIX_SRC_U8:
        N, T, H, W, _ = src.shape
    else:
        N, _, T, H, W = src.shape
    out_mode = L.PTX_RESIZE_OUT_F32 if dtype == torch.float32 else L.PTX_RESIZE_OUT_BF16
    rows, noise_elems = TF.batch_mix_rows(params, T, value, N)
    desc = L.MixDesc(N, T, H, W, src_mode, out_mode, noise_elems)
    rows = np.ascontiguousarray(rows)
    assert lib.ptx_batch_mix_supported(C.byref(desc), C.c_void_p(rows.ctypes.data)) == 1, lib.ptx_last_error()
    d_rows = torch.from_numpy(rows.reshape(-1)).to(DEV)
    y = torch.full((N, 3, T, H, W), float("nan"), dtype=dtype, device=DEV)
    assert noise_elems == (0 if noise is None else noise.numel())
    L.check(lib.ptx_batch_mix_apply(C.byref(desc), C.c_void_p(src.data_ptr()), C.c_void_p(d_rows.data_ptr()),
                                    C.c_void_p(noise.data_ptr()) if noise is not None else None, C.c_void_p(y.data_ptr()),
                                    C.byref(norm) if norm is not None else None, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "ptx_batch_mix_apply")
    torch.cuda.synchronize()
    return y.cpu()


@pytest.mark.parametrize("kind", SOURCES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_draw_equals_the_torch_statement(ptx, shape, kind):
    TF = ptx.transforms
    N, T, H, W = shape
    for opts in ((RGB01, BGR255) if kind == "u8_f32" else (RGB01,)):
        src, ref, src_mode, dtype, norm = make_source(ptx, kind, N, T, H, W, opts, 7000 + N)
        draws = dict(hand_draws(N, H, W), **seeded_draws(ptx, N, H, W))
        for name, params in draws.items():
            got = run_kernel(ptx, src, src_mode, dtype, norm, params, VALUE)
            want = TF.batch_mix_torch(ref, params, VALUE)
            assert not torch.isnan(got.float()).any(), name
            assert torch.equal(got, want), (name, kind, shape)


@pytest.mark.parametrize("kind", SOURCES)
def test_noise_erase_equals_the_same_randn_calls(ptx, kind):
    """erase_value="random": the reference draws the same torch.randn calls from an equally seeded CUDA generator."""
    TF = ptx.transforms
    N, T, H, W = 4, 3, 16, 20
    src, ref, src_mode, dtype, norm = make_source(ptx, kind, N, T, H, W, RGB01, 7100)
    draws = hand_draws(N, H, W)
    for name in ("cutmix_erase_straddle", "mixup_erased", "permutation", "every_kind"):
        params = draws[name]
        g = torch.Generator(device=DEV).manual_seed(55)
        noise = [torch.randn((3, T, int(r[9]), int(r[10])), device=DEV, generator=g).cpu() for r in params[0] if r[6]]
        bm = TF.BatchMix(erase_value="random", noise_generator=torch.Generator(device=DEV).manual_seed(55))
        got = bm(src, params=params, opts=RGB01, dtype=dtype) if kind.startswith("u8") else bm(src, params=params)
        want = TF.batch_mix_torch(ref, params, "random", noise)
        assert got.dtype == dtype and torch.equal(got.cpu(), want), (name, kind)
        assert bm.last_noise.dtype == dtype and bm.last_noise.numel() == sum(n.numel() for n in noise)
        # the packed buffer, replayed into a NaN-filled output through the C ABI
        assert torch.equal(run_kernel(ptx, src, src_mode, dtype, norm, params, "random", bm.last_noise), want), (name, kind)


def test_public_call_draws_keeps_and_replays(ptx):
    TF = ptx.transforms
    frames = torch.from_numpy(synth_color_frames(4, 3, 16, 20, 7200)).to(DEV)
    ref = TF.FramesToTensor(RGB01)(frames)
    bm = TF.BatchMix(erase_prob=0.8, mode="clip", erase_value=VALUE, generator=gen(21))
    got = bm(frames, opts=RGB01)
    want_params = TF.BatchMix(erase_prob=0.8, mode="clip", generator=gen(21)).draw(4, 16, 20)
    assert torch.equal(bm.last_params[0], want_params[0]) and torch.equal(bm.last_params[1], want_params[1])
    want = TF.batch_mix_torch(ref.cpu(), bm.last_params, VALUE)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    assert torch.equal(bm(ref, params=bm.last_params).cpu(), want)                     # the same draw on the normalised clip
    assert torch.equal(bm(frames, params=bm.last_params, opts=RGB01, dtype=torch.bfloat16).cpu(),
                       TF.batch_mix_torch(ref.cpu().bfloat16(), bm.last_params, VALUE))
    nc = ref.permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3)                # a non-contiguous clip costs one copy
    assert not nc.is_contiguous() and torch.equal(bm(nc, params=bm.last_params).cpu(), want)


def test_fused_routes_equal_the_stand_alone_call(ptx):
    TF = ptx.transforms
    frames = torch.from_numpy(synth_color_frames(2, 4, 40, 52, 7300)).to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        g = gen(31)
        cj, ra = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, generator=g), TF.RandAugment(generator=g)
        bm = TF.BatchMix(erase_prob=1.0, erase_value=VALUE, generator=g)
        tf = TF.TransformFrames(OPTS, random_crop=True, color=cj, augment=ra, mix=bm, generator=g, dtype=dtype)
        got = tf(frames)
        u8 = TF.TransformFrames(OPTS, random_crop=True, color=cj, augment=ra, out="frames")(
            frames, params=tf.last_params, color_params=cj.last_params, augment_params=ra.last_params)
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (2, 4, 32, 32, 3)
        want = bm(u8, opts=OPTS, params=bm.last_params, dtype=dtype)
        assert got.dtype == dtype and tuple(got.shape) == (2, 3, 4, 32, 32) and torch.equal(got, want)
        assert torch.equal(got.cpu(), TF.batch_mix_torch(TF.FramesToTensor(OPTS)(u8).cpu().to(dtype), bm.last_params, VALUE))
        assert bm.last_params[0][:, 6].all() and bm.last_params[0][:, 1].all()         # every clip erased and mixed
        assert torch.equal(tf(frames, params=tf.last_params, color_params=cj.last_params, augment_params=ra.last_params,
                              mix_params=bm.last_params), got)                          # the replay
    # mix alone behind the resize, on one clip of rank 4: it is its own partner
    bm = TF.BatchMix(erase_prob=1.0, erase_value=VALUE, generator=gen(33))
    tf = TF.TransformFrames(OPTS, mix=bm)
    got = tf(frames[0])
    u8 = TF.TransformFrames(OPTS, out="frames")(frames[0])
    assert tuple(got.shape) == (3, 4, 32, 32) and torch.equal(got, bm(u8[None], opts=OPTS, params=bm.last_params)[0])
    # SampleClips on two videos of different sizes
    videos = [torch.from_numpy(synth_color_frames(1, 12, 48, 60, 7301)[0]).to(DEV), torch.from_numpy(synth_color_frames(1, 9, 40, 44, 7302)[0]).to(DEV)]
    g = gen(35)
    bm = TF.BatchMix(erase_prob=1.0, erase_value=VALUE, mode="clip", generator=g)
    kw = dict(num_frames=4, frame_stride=2, clips=2, random_resized_crop=True, random_hflip=True)
    sc = TF.SampleClips(OPTS, mix=bm, generator=g, **kw)
    got = sc(videos)
    u8 = TF.SampleClips(OPTS, out="frames", **kw)(videos, indices=sc.last_indices, geometry=sc.last_geometry)
    assert tuple(got.shape) == (4, 3, 4, 32, 32) and torch.equal(got, bm(u8, opts=OPTS, params=bm.last_params))
    assert torch.equal(sc(videos, indices=sc.last_indices, geometry=sc.last_geometry, mix_params=bm.last_params), got)


def test_targets_on_the_device_equal_the_host_restatement(ptx):
    TF = ptx.transforms
    labels = torch.tensor([3, 0, 299, 3, 17])
    for seed, mode in ((0, "batch"), (1, "clip"), (2, "clip")):
        bm = TF.BatchMix(prob=0.7, mode=mode, generator=gen(40 + seed))
        bm(torch.randn(5, 3, 1, 9, 13, device=DEV))
        for smoothing in (0.0, 0.1):
            got = bm.targets(labels.to(DEV), 300, smoothing)
            assert got.dtype == torch.float32 and torch.equal(got.cpu(), TF.batch_mix_targets_torch(labels, 300, bm.last_params, smoothing))
    params = params_of([row(1, 1, 0.3), row(0, 2, 0.75, (0, 0, 2, 2)), row(2), row(4, 1, 0.0), row(3, 1, 1.0)])
    got = bm.targets(labels.to(DEV), 300, 0.1, params=params)
    want = TF.batch_mix_targets_torch(labels, 300, params, 0.1)
    assert torch.equal(got.cpu(), want) and float((want.sum(1) - 1).abs().max()) <= 1e-6


def test_apply_refuses_on_the_device_what_supported_refuses(ptx):
    """A status, no launch, no fault: the NaN-filled output stays as it is."""
    L, TF, E = ptx._lib, ptx.transforms, ptx._lib.PtxError
    lib = L.lib()
    src = torch.zeros(4, 2, 9, 13, 3, dtype=torch.uint8, device=DEV)
    y = torch.full((4, 3, 2, 9, 13), float("nan"), device=DEV)
    rows, _ = TF.batch_mix_rows(params_of([row(i) for i in range(4)]), 2)
    d_rows = torch.from_numpy(rows.reshape(-1)).to(DEV)
    norm = L.NormDesc.make(RGB01["mean"], RGB01["std"])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())                  # noqa: E731
    for desc, args, what in ((L.MixDesc(4, 2, 9, 0, 0, 1, 0), (P(src), P(d_rows), None, P(y), C.byref(norm)), "non-positive extent"),
                             (L.MixDesc(4, 2, 9, 13, 0, 0, 0), (P(src), P(d_rows), None, P(y), C.byref(norm)), "out_mode=0 must be"),
                             (L.MixDesc(4, 2, 9, 13, 1, 2, 0), (P(src), P(d_rows), None, P(y), None), "writes its own type"),
                             (L.MixDesc(4, 2, 9, 13, 0, 1, 8), (P(src), P(d_rows), None, P(y), C.byref(norm)), "null pointer"),
                             (L.MixDesc(4, 2, 9, 13, 0, 1, 0), (P(src), P(d_rows), None, P(y), None), "null norm descriptor"),
                             (L.MixDesc(4, 2, 9, 13, 0, 1, 0), (P(src), None, None, P(y), C.byref(norm)), "null pointer")):
        assert lib.ptx_batch_mix_apply(C.byref(desc), *args, stream) in (1, 2) and what in lib.ptx_last_error().decode()
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
    # rows that the host check refuses never reach a launch through the public call
    bm = TF.BatchMix()
    for bad, what in ((params_of([row(4, 1, 0.5)] + [row(i) for i in range(1, 4)]), "partner 4 out of range"),
                      (params_of([row(0, 2, 0.5, (0, 0, 10, 13))] + [row(i) for i in range(1, 4)]), "leaves the 9x13 frame"),
                      (params_of([row(0, erase=(8, 0, 2, 3))] + [row(i) for i in range(1, 4)]), "erase rectangle"),
                      (params_of([row(0, 1, 1.5)] + [row(i) for i in range(1, 4)]), "must be finite and in")):
        with pytest.raises(E, match=what):
            bm(src, params=bad, opts=RGB01)
