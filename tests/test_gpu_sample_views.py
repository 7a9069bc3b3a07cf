"""GPU tests of multi-view inference: `transforms.SampleViews` (ptx_resize_views_u8) against PIL's stored outputs and
against `TransformFrames` on the same frame and window (exact equality, every output mode, both workgroup shapes),
`forward_views` against the same views pushed through the existing API in the same chunks (exact equality),
`TRN.forward_frames` against `TRN.forward`, and ptx_views_mean against a float64 softmax-mean (1e-6, the bar of
tests/test_gpu_kernels.py::test_softmax_and_bgemm)."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

from pretorched_x_amd.testing import I3D_RECIPE, synth_frames, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPTS = dict(input_size=[3, 64, 64], input_space="RGB", input_range=[0, 1], mean=[0.45, 0.40, 0.35], std=[0.2, 0.25, 0.3])
BGR255 = dict(input_size=[3, 64, 64], input_space="BGR", input_range=[0, 255], mean=[104.0, 117.0, 123.0], std=[1.0, 1.0, 1.0])


def golden_cases():
    blob = load_golden("sample_views")
    return blob, json.loads(str(blob["cases"]))


def sampler(TF, c, opts=OPTS, **kw):
    return TF.SampleViews(opts, num_frames=c["num_frames"], frame_stride=c["frame_stride"], clips=c["clips"],
                          crops=c["crops"], sampling=c["sampling"], **kw)


def video_of(c, seed_shift=0):
    return torch.from_numpy(synth_frames(c["Tv"], c["H"], c["W"], c["seed"] + seed_shift, c["content"]))


def compose(TF, vs, video, opts, **kw):
    """The views through the existing API: per clip an index_select of the frames, per crop one TransformFrames launch."""
    N, Tv, H, W, _ = video.shape
    idx, wins = vs.frame_indices(Tv), vs.windows(H, W)
    out = []
    for clip in range(vs.clips):
        frames = video.index_select(1, torch.from_numpy(idx[clip]).to(video.device))
        for crop in range(vs.crops):
            out.append(TF.TransformFrames(opts, crop=wins[crop], **kw)(frames))
    return torch.stack(out, 1)                      # [N, V, ...]


def test_sample_views_equal_pil_and_transform_frames(ptx):
    TF = ptx.transforms
    blob, cases = golden_cases()
    for c in cases:
        want = torch.from_numpy(blob["out_" + c["name"]]).to(DEV)                # PIL: [V,T,64,64,3]
        video = torch.stack([video_of(c), video_of(c, 1000)]).to(DEV)             # batch of 2: [2,Tv,H,W,3]
        for share in ("auto", "always", "never"):
            if share == "always" and c["crops"] == 1:
                continue
            vs = sampler(TF, c, share=share)
            got = vs(video)
            assert got.dtype == torch.uint8 and got.shape == (2, vs.num_views, c["num_frames"], 64, 64, 3)
            assert torch.equal(got[0], want), (c["name"], share)
            assert torch.equal(got, compose(TF, vs, video, OPTS, out="frames")), (c["name"], share)
            assert torch.equal(vs(video[0]), want), (c["name"], share)            # the [Tv,H,W,3] rank
            for opts in (OPTS, BGR255):
                v32, v16 = sampler(TF, c, opts, share=share, out="tensor"), sampler(TF, c, opts, share=share, out="tensor", dtype=torch.bfloat16)
                g32, g16 = v32(video), v16(video)
                assert g32.dtype == torch.float32 and g32.shape == (2, vs.num_views, 3, c["num_frames"], 64, 64)
                assert torch.equal(g32, compose(TF, v32, video, opts)), (c["name"], share)
                assert g16.dtype == torch.bfloat16 and torch.equal(g16, compose(TF, v16, video, opts, dtype=torch.bfloat16))
                assert torch.equal(g32[0], TF.FramesToTensor(opts)(want)), (c["name"], share)      # PIL + the tensor half
    # which workgroup shape serves which case is the library's answer, and both were run above
    assert sampler(TF, cases[0]).describe(90, 120) in ("shared", "per-window")


def test_view_ranges_strided_videos_and_odd_sizes(ptx):
    TF = ptx.transforms
    blob, cases = golden_cases()
    by = {c["name"]: c for c in cases}
    for name in ("landscape_90x120", "portrait_120x90"):
        c = by[name]
        want = torch.from_numpy(blob["out_" + name]).to(DEV)
        video = torch.stack([video_of(c), video_of(c, 1000)]).to(DEV)
        for share in ("always", "never"):
            for out_kw in (dict(), dict(out="tensor"), dict(out="tensor", dtype=torch.bfloat16)):
                vs = sampler(TF, c, share=share, **out_kw)
                full = vs(video)
                # ranges that split a clip's three crops across chunks: [0,2) [2,4) [4,6), [1,5), single views
                for v0, nv in ((0, 2), (2, 2), (4, 2), (1, 4), (0, 1), (5, 1), (3, 3)):
                    assert torch.equal(vs.sample(video, v0, nv), full[:, v0:v0 + nv]), (name, share, v0, nv)
                assert torch.equal(vs.sample(video[1], 2), full[1, 2:])
        vs = sampler(TF, c)
        # non-contiguous videos read in place: every second frame of a longer buffer, a slice of a bigger batch, and a
        # frame-interior slice (columns of a wider buffer: copied once)
        long = torch.zeros(3, 2 * c["Tv"], c["H"], c["W"], 3, dtype=torch.uint8, device=DEV)
        long[1:, ::2] = video
        view = long[1:, ::2]
        assert not view.is_contiguous() and torch.equal(vs(view), vs(video))
        wide = torch.zeros(2, c["Tv"], c["H"], c["W"] + 30, 3, dtype=torch.uint8, device=DEV)
        wide[:, :, :, 20:20 + c["W"]] = video
        assert torch.equal(vs(wide[:, :, :, 20:20 + c["W"]]), vs(video))
        assert torch.equal(vs(video[0].expand(2, -1, -1, -1, -1))[1], want)       # stride 0 over the batch: copied
        with pytest.raises(ptx._lib.PtxError, match="view range"):
            vs.sample(video, 4, 3)
    # an output width that is not a multiple of 4 takes the narrow stores (S = 50)
    c = by["landscape_90x120"]
    o50 = dict(OPTS, input_size=[3, 50, 50])
    video = video_of(c).unsqueeze(0).to(DEV)
    for share in ("always", "never"):
        for out_kw in (dict(), dict(out="tensor"), dict(out="tensor", dtype=torch.bfloat16)):
            vs = sampler(TF, c, o50, share=share, **out_kw)
            ref = dict(out_kw) if out_kw else dict(out="frames")
            assert torch.equal(vs(video), compose(TF, vs, video, o50, **ref)), (share, out_kw)


def test_union_too_big_for_lds_takes_one_window_per_workgroup(ptx):
    """An 8:1 panorama at 224: the union of the three windows is 3 x 224 columns, 2016 bytes per intermediate row; next to
    the staging of four 3600-pixel input rows (43 KiB) that leaves the shared pass a band of one row, below the library's
    floor, and the per-window shape runs.  It gives TransformFrames' bits."""
    TF = ptx.transforms
    opts = dict(OPTS, input_size=[3, 224, 224])
    vs = TF.SampleViews(opts, num_frames=2, frame_stride=1, clips=2, crops=3)
    H, W = 450, 3600
    assert vs.describe(H, W) == "per-window"
    assert TF.SampleViews(opts, num_frames=2, clips=2, crops=3).describe(640, 360) == "shared"
    video = torch.from_numpy(synth_frames(4, H, W, 77)).unsqueeze(0).to(DEV)
    got = vs(video)
    assert torch.equal(got, compose(TF, vs, video, opts, out="frames"))
    f = TF.SampleViews(opts, num_frames=2, frame_stride=1, clips=2, crops=3, share="never")
    assert torch.equal(f(video), got)


def _fp32_reference(model, vs, video, opts, chunks, run=None):
    """The same views through the existing API in the same chunks: forward_frames on the stacked uint8 views."""
    views = vs(video)                                                            # [N,V,T,S,S,3]
    N, V = views.shape[:2]
    run = run or (lambda fr: model.forward_frames(fr, opts))
    out = [run(views[:, v0:v0 + nv].reshape((N * nv,) + tuple(views.shape[2:]))).reshape(N, nv, -1) for v0, nv in chunks]
    return torch.cat(out, 1)


def test_forward_views_resnet3d18_fp32_and_bf16(ptx):
    TF, E = ptx.transforms, ptx.engine
    blob, cases = golden_cases()
    c = {c["name"]: c for c in cases}["landscape_90x120"]
    video = torch.stack([video_of(c), video_of(c, 1000)]).to(DEV)                # [2,24,90,120,3]
    model = ptx.__dict__["resnet3d18"](num_classes=400, pretrained=None)
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
    model = model.to(DEV).eval()
    model.engine().lanes = 1
    vs = TF.SampleViews(OPTS, num_frames=4, frame_stride=2, clips=2, crops=3)    # 6 views of 4 frames
    with torch.no_grad():
        one = model.forward_views(video, OPTS, views=vs, reduce=None)            # one chunk: 2 x 6 clips
        assert one.shape == (2, 6, 400) and one.dtype == torch.float32
        assert torch.equal(one, _fp32_reference(model, vs, video, OPTS, [(0, 6)]))
        # chunk=4 splits the second clip's crops across chunks: views [0,4) then [4,6)
        several = model.forward_views(video, OPTS, views=vs, reduce=None, chunk=4)
        assert torch.equal(several, _fp32_reference(model, vs, video, OPTS, [(0, 4), (4, 2)]))
        assert torch.equal(model.engine().forward_views(model, video, OPTS, vs, None, 4), several)
        # the reductions are ptx_views_mean applied to the reduce=None output, bit for bit
        probs = model.forward_views(video, OPTS, views=vs)
        assert probs.shape == (2, 400) and probs.dtype == torch.float32
        assert torch.equal(probs, E.views_mean(one, 2, 6, "softmax"))
        assert torch.equal(model.forward_views(video, OPTS, views=vs, reduce="logits"), E.views_mean(one, 2, 6, "logits"))
        assert float((probs.double().sum(1) - 1).abs().max()) <= 1e-6
        single = model.forward_views(video[0], OPTS, views=vs, reduce=None, chunk=6)     # [Tv,H,W,3]: one video
        assert single.shape == (1, 6, 400)
        # misuse
        with pytest.raises(ptx._lib.PtxError, match="out='frames'"):
            model.forward_views(video, OPTS, views=TF.SampleViews(OPTS, num_frames=4, clips=2, out="tensor"))
        two_d = ptx.__dict__["resnet18"](num_classes=10, pretrained=None).to(DEV).eval()
        with pytest.raises(ptx._lib.PtxError, match="2-D model"):
            two_d.forward_views(video, OPTS, views=vs)

        # bf16: the views as the normalised bf16 tensor through model(clip)
        m16 = ptx.__dict__["resnet3d18"](num_classes=400, pretrained=None)
        m16.load_state_dict(synth_state_dict(m16.state_dict(), 1234))
        m16 = m16.eval().to(torch.bfloat16).to(DEV)
        m16.engine().lanes = 1
        v16 = TF.SampleViews(OPTS, num_frames=4, frame_stride=2, clips=2, crops=3, out="tensor", dtype=torch.bfloat16)
        clips = v16(video)                                                       # [2,6,3,4,64,64]
        got = m16.forward_views(video, views=v16, reduce=None)
        assert got.dtype == torch.bfloat16 and got.shape == (2, 6, 400)
        assert torch.equal(got, m16(clips.reshape((12,) + tuple(clips.shape[2:]))).reshape(2, 6, 400))
        got4 = m16.forward_views(video, views=v16, reduce=None, chunk=4)
        want4 = torch.cat([m16(clips[:, a:b].reshape((2 * (b - a),) + tuple(clips.shape[2:]))).reshape(2, b - a, 400)
                           for a, b in ((0, 4), (4, 6))], 1)
        assert torch.equal(got4, want4)
        p16 = m16.forward_views(video, views=v16)
        assert p16.dtype == torch.float32 and torch.equal(p16, E.views_mean(got, 2, 6, "softmax"))
        with pytest.raises(ptx._lib.PtxError, match="bfloat16"):
            m16.forward_views(video, views=vs)                                   # a frames-out sampler on a bf16 model
        with pytest.raises(ptx._lib.PtxError, match="bfloat16"):
            m16.forward_views(video, views=TF.SampleViews(OPTS, num_frames=4, clips=2, out="tensor"))
        with pytest.raises(ptx._lib.PtxError):
            m16.forward_frames(vs(video)[:, 0], OPTS)                            # forward_frames on a bf16 model keeps raising


def test_forward_views_slowfast_i3d_trn(ptx):
    TF = ptx.transforms
    with torch.no_grad():
        # a small SlowFast: 32-frame clips at 64 x 64
        sf = ptx.slowfast.resnet18(mode="sf", num_classes=10)
        sf.load_state_dict(synth_state_dict(sf.state_dict(), 1234))
        sf = sf.to(DEV).eval()
        sf.engine().lanes = 1
        video = torch.from_numpy(synth_frames(40, 90, 120, 4242)).unsqueeze(0).to(DEV)
        vs = TF.SampleViews(BGR255, num_frames=32, frame_stride=1, clips=2, crops=3)
        one = sf.forward_views(video, BGR255, views=vs, reduce=None)
        assert one.shape == (1, 6, 10) and torch.equal(one, _fp32_reference(sf, vs, video, BGR255, [(0, 6)]))
        assert torch.equal(sf.forward_views(video, BGR255, views=vs, reduce=None, chunk=2),
                           _fp32_reference(sf, vs, video, BGR255, [(0, 2), (2, 2), (4, 2)]))

        # I3D at its own input size: 16 x 224 x 224
        i3d = ptx.i3d(400)
        i3d.load_state_dict(synth_state_dict(i3d.state_dict(), 1234, **I3D_RECIPE))
        i3d = i3d.to(DEV).eval()
        i3d.engine().lanes = 1
        o224 = dict(mean=[0.5, 0.5, 0.5], std=[0.5, 0.5, 0.5], input_space="RGB", input_range=[0, 1], input_size=[3, 224, 224])
        video = torch.from_numpy(synth_frames(20, 240, 320, 808)).unsqueeze(0).to(DEV)
        vs = TF.SampleViews(o224, num_frames=16, frame_stride=1, clips=2, crops=1)
        assert torch.equal(i3d.forward_views(video, o224, views=vs, reduce=None), _fp32_reference(i3d, vs, video, o224, [(0, 2)]))
        assert torch.equal(i3d.forward_views(video, o224, views=vs, reduce=None, chunk=1),
                           _fp32_reference(i3d, vs, video, o224, [(0, 1), (1, 1)]))

        # TRN: a 2-D backbone on the frames of a clip
        trn = ptx.zoo.TRN(10, num_segments=4, arch="resnet18", consensus="TRN", pretrained=None)
        trn.load_state_dict(synth_state_dict(trn.state_dict(), 1234))
        trn = trn.to(DEV).eval()
        trn.base_model.engine().lanes = 1
        video = torch.from_numpy(synth_frames(20, 90, 120, 515)).view(2, 10, 90, 120, 3).to(DEV)
        vs = TF.SampleViews(OPTS, num_frames=4, clips=2, crops=3, sampling="segments")
        frames = vs(video)                                                       # [2,6,4,64,64,3]
        flat = frames.reshape(12, 4, 64, 64, 3)
        want = trn(TF.FramesToTensor(OPTS)(flat).permute(0, 2, 1, 3, 4).contiguous())       # [12,4,3,64,64]
        got = trn.forward_frames(flat, OPTS)
        assert got.shape == (12, 10) and torch.equal(got, want)                  # forward_frames == forward, bit for bit
        run = lambda fr: trn.forward_frames(fr, OPTS)
        assert torch.equal(trn.forward_views(video, OPTS, views=vs, reduce=None), got.reshape(2, 6, 10))
        assert torch.equal(trn.forward_views(video, OPTS, views=vs, reduce=None, chunk=4),
                           _fp32_reference(trn, vs, video, OPTS, [(0, 4), (4, 2)], run))
        dense = TF.SampleViews(OPTS, num_frames=4, frame_stride=2, clips=2, crops=1)
        probs = trn.forward_views(video, OPTS, views=dense)
        assert probs.shape == (2, 10) and float((probs.double().sum(1) - 1).abs().max()) <= 1e-6
        with pytest.raises(ptx._lib.PtxError, match="num_segments"):
            trn.forward_views(video, OPTS, views=TF.SampleViews(OPTS, num_frames=8, clips=2, sampling="segments"))
        with pytest.raises(ptx._lib.PtxError, match="out='frames'"):
            trn.forward_views(video, OPTS, views=TF.SampleViews(OPTS, num_frames=4, clips=2, out="tensor"))


def close(got, want, tol):
    scale = max(1.0, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert got.shape == want.shape
    assert err <= tol * scale, "max err %.3e (scale %.3e)" % (err, scale)


def test_views_mean(ptx):
    E = ptx.engine
    g = torch.Generator().manual_seed(42)
    for K in (339, 400, 37):
        for V in (1, 3, 30):
            for dtype in (torch.float32, torch.bfloat16):
                N, ld = 3, K + 5                                                  # a padded row stride
                x = (torch.randn(N * V, ld, generator=g) * 3.0).to(dtype)
                xd = x.to(DEV)[:, :K]
                assert xd.stride(0) == ld
                ref = x[:, :K].double().view(N, V, K)
                soft = E.views_mean(xd, N, V, "softmax")
                torch.cuda.synchronize()
                assert soft.dtype == torch.float32
                close(soft.cpu().double(), torch.softmax(ref, -1).mean(1), 1e-6)
                assert float((soft.cpu().double().sum(1) - 1).abs().max()) <= 1e-6
                close(E.views_mean(xd, N, V, "logits").cpu().double(), ref.mean(1), 1e-6)
                assert torch.equal(E.views_mean(xd.contiguous().view(N, V, K), N, V, "softmax"), soft)   # dense rows, [N,V,K]
    with pytest.raises(ptx._lib.PtxError, match="mode"):
        E.views_mean(xd, 3, 30, "max")
    with pytest.raises(ptx._lib.PtxError, match="CUDA"):
        E.views_mean(x, 3, 30)
