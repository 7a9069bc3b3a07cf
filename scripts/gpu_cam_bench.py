"""Class activation maps on the GPU: the three launches of include/ptx_amd_cam.h, `model.cam(x)` against `model(x)`, and the
overlay against the torch route it replaces on the same GPU.

    python scripts/gpu_cam_bench.py [--out profiles/cam.json] [--quick]

Shape: config 2's batch -- 8 clips, a final feature map of 2048 x 2 x 7 x 7, k = 1 and 5 classes per clip, overlays onto 8 x 16
frames of 224 x 224.  The launches are timed with HIP events around `--iters` back-to-back launches (through ctypes, buffers
allocated once), every variant warmed, the variants alternating inside every round; the median of the rounds is reported, the
spread of a variant is (max - min) / median of its rounds.  `model.cam(x)` and `model(x)` (resnet3d50, 8 x 3 x 16 x 224 x 224,
fp32 and bf16) are timed the same way, whole calls back to back.  The torch route is what a user writes without the kernels:
`model.features`' NCDHW copy aside, einsum of the chosen classifier rows, amin / amax, the stretch to 0 .. 255,
`F.interpolate(trilinear)` to 16 x 224 x 224 in fp32, a colour-table gather, the blend with the fp32 frames and the cast -- six
full-size passes with fp32 intermediates.  Its image is not Pillow's; the kernel's is compared with `cam_overlay_numpy` on one clip
before anything is timed.  Bytes are the algorithm's: N T H W 3 read (once per class) and N k T H W 3 written.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pretorched_x_amd as ptx                                   # noqa: E402
from pretorched_x_amd.testing import synth_state_dict            # noqa: E402

TF, L = ptx.transforms, ptx._lib
DEV = "cuda:0"
N, T, S = 8, 16, 224
CF, TM, HM = 2048, 2, 7
CLASSES = 339


def event_timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def alternate(variants, iters, rounds):
    """{name: fn} -> {name: {"ms": median, "spread": (max - min) / median, "rounds": [...]}}, variants alternating."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(event_timed(fn, iters))
    return {k: dict(ms=round(statistics.median(v), 4), spread=round((max(v) - min(v)) / statistics.median(v), 4),
                    rounds=[round(x, 4) for x in v]) for k, v in got.items()}


def ptr(t):
    return C.c_void_p(t.data_ptr())


def torch_route(feats, w, b, cls, frames_f32, lut, alpha):
    """features NCDHW fp32 [N,C,Tm,h,w] -> overlays uint8 [N,k,T,H,W,3] with torch ops alone."""
    scores = torch.einsum("nkc,ncthw->nkthw", w[cls], feats) + b[cls][:, :, None, None, None]
    mn, mx = scores.amin(dim=(2, 3, 4), keepdim=True), scores.amax(dim=(2, 3, 4), keepdim=True)
    q = 255.0 * ((scores - mn) / (mx - mn))
    big = F.interpolate(q, size=(T, S, S), mode="trilinear", align_corners=False)
    heat = lut[big.clamp(0, 255).long()].float()                 # [N,k,T,H,W,3]
    return (frames_f32[:, None] + alpha * (heat - frames_f32[:, None])).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-model", action="store_true", help="skip the model.cam / model(x) rows")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_cam_bench: no GPU (there is no CPU path to time)")
    iters, rounds = (5, 2) if args.quick else (args.iters, args.rounds)
    lib = L.lib()
    g = torch.Generator(device=DEV).manual_seed(1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    frames = torch.randint(0, 256, (N, T, S, S, 3), dtype=torch.uint8, device=DEV, generator=g)
    feats_cl = torch.randn((N, TM * HM * HM, CF), device=DEV, generator=g).relu_()      # channels-last, as the plan holds it
    feats_bf = feats_cl.to(torch.bfloat16)
    w = torch.randn((CLASSES, CF), device=DEV, generator=g) * 0.02
    b = torch.randn((CLASSES,), device=DEV, generator=g)
    lut_np = TF.jet_colormap()
    lut = torch.from_numpy(lut_np).to(DEV)
    Sm = TM * HM * HM
    variants, routes, keep, checks = {}, {}, [], {}
    rows_t, cols_t = TF.resize_axis_table(HM, S), TF.resize_axis_table(HM, S)
    tabs = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV) for a in rows_t + cols_t]
    step = torch.from_numpy(TF.cam_default_steps(T, TM)).to(DEV)
    for k in (1, 5):
        cls = torch.randint(0, CLASSES, (N, k), device=DEV, generator=g)
        cls32 = cls.to(torch.int32)
        scores = torch.empty((N, k, Sm), device=DEV)
        maps = torch.empty((N, k, TM, HM, HM), dtype=torch.uint8, device=DEV)
        out = torch.empty((N, k, T, S, S, 3), dtype=torch.uint8, device=DEV)
        desc = L.CamOverlayDesc(N, k, TM, HM, HM, T, S, S, rows_t[2].shape[1], cols_t[2].shape[1], L.PTX_CAM_OUT_OVERLAY, 0.4)
        keep.append((cls32, desc))

        def f_scores(x=feats_cl, bf=0, cls32=cls32, scores=scores, k=k):
            L.check(lib.ptx_cam_scores(ptr(x), bf, ptr(w), ptr(b), ptr(cls32), ptr(scores), N, Sm, CF, CF, k, CLASSES, stream), "scores")

        def f_quant(scores=scores, maps=maps, k=k):
            L.check(lib.ptx_cam_quantize(ptr(scores), ptr(maps), N * k, Sm, stream), "quantize")

        def f_overlay(desc=desc, maps=maps, out=out):
            L.check(lib.ptx_cam_overlay(C.byref(desc), ptr(maps), ptr(frames), ptr(lut), *[ptr(t) for t in tabs], ptr(step), ptr(out),
                                        stream), "overlay")

        variants["scores_f32_k%d" % k] = f_scores
        variants["scores_bf16_k%d" % k] = lambda f=f_scores: f(x=feats_bf, bf=1)
        variants["quantize_k%d" % k] = f_quant
        variants["overlay_k%d" % k] = f_overlay
        f_scores(), f_quant(), f_overlay()
        torch.cuda.synchronize()
        want = TF.cam_overlay_numpy(maps[:1].cpu().numpy(), frames[:1].cpu().numpy(), lut_np, 0.4)
        assert np.array_equal(out[:1].cpu().numpy(), want), k
        assert np.array_equal(maps.cpu().numpy().reshape(N, k, Sm), TF.cam_quantize_numpy(scores.cpu().numpy()))
        feats_nc = feats_cl.view(N, TM, HM, HM, CF).permute(0, 4, 1, 2, 3).contiguous()
        frames_f32 = frames.float()
        routes["torch_k%d" % k] = lambda cls=cls, feats_nc=feats_nc, frames_f32=frames_f32: torch_route(feats_nc, w, b, cls, frames_f32, lut, 0.4)
        ref = routes["torch_k%d" % k]()
        diff = (ref.int() - out.int()).abs()
        checks["k%d" % k] = dict(samples=diff.numel(), differ_from_torch_route=int((diff != 0).sum().item()), largest_step=int(diff.max().item()))
        del ref, diff
    kernels = alternate(variants, iters, rounds)
    px = N * T * S * S
    for k in (1, 5):
        row = kernels["overlay_k%d" % k]
        row["compulsory_bytes"] = px * 3 + px * 3 * k
        row["GBps_compulsory"] = round(row["compulsory_bytes"] / row["ms"] / 1e6, 1)
        row["GBps_issued"] = round(px * 6 * k / row["ms"] / 1e6, 1)           # the frames are read once per class (L2 serves the repeats)
        for name in ("scores_f32_k%d" % k, "scores_bf16_k%d" % k):
            kernels[name]["GBps"] = round(N * Sm * CF * (2 if "bf16" in name else 4) / kernels[name]["ms"] / 1e6, 1)
    slow_iters = max(iters // 10, 2)
    torch_events = alternate(routes, slow_iters, rounds)
    ratios = {"torch_route_over_three_launches_k%d" % k: round(
        torch_events["torch_k%d" % k]["ms"] / sum(kernels["%s_k%d" % (n, k)]["ms"] for n in ("scores_f32", "quantize", "overlay")), 1)
        for k in (1, 5)}
    models = {}
    if not args.no_model:
        m = ptx.resnet3d50(num_classes=CLASSES, pretrained=None)
        m.load_state_dict(synth_state_dict(m.state_dict(), 1234))
        m = m.eval().to(DEV)
        x = torch.randn((N, 3, T, S, S), device=DEV, generator=g)
        with torch.no_grad():
            for tag, mm, xx in (("fp32", m, x), ("bf16", None, None)):
                if tag == "bf16":
                    mm, xx = m.to(torch.bfloat16), x.to(torch.bfloat16)
                r = mm.cam(xx, topk=5)
                assert torch.equal(r.logits, mm(xx))
                rows = alternate({"forward": lambda: mm(xx), "cam_top1": lambda: mm.cam(xx, topk=1), "cam_top5": lambda: mm.cam(xx, topk=5)},
                                 max(iters // 10, 2), rounds)
                rows["feature_map"] = list(r.scores.shape[2:])
                rows["cam_top5_over_forward"] = round(rows["cam_top5"]["ms"] / rows["forward"]["ms"], 4)
                models["resnet3d50_" + tag] = rows
    out = dict(device=torch.cuda.get_device_name(0), binary=lib.ptx_version().decode(), clips=N, features=[CF, TM, HM, HM],
               frames=[N, T, S, S, 3], iters=iters, rounds=rounds, slow_iters=slow_iters,
               clock="HIP events around back-to-back launches / calls, warmed, alternating rounds, median",
               kernels=kernels, torch_route_events=torch_events, against_torch_route=checks, ratios=ratios, model_calls=models)
    print(json.dumps(dict(ratios=ratios, ms={k: v["ms"] for k, v in list(kernels.items()) + list(torch_events.items())},
                          overlay_GBps={k: kernels["overlay_k%d" % k]["GBps_compulsory"] for k in (1, 5)},
                          models={k: {n: (v[n]["ms"] if isinstance(v[n], dict) else v[n]) for n in v} for k, v in models.items()})), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
