"""Multi-view sampling on the GPU: `transforms.SampleViews` (one ptx_resize_views_u8 launch) against the composition it
replaces (per clip an index_select of the frames, per crop one TransformFrames launch), and `forward_views` against a
Python loop over that composition + forward_frames + torch softmax-mean.

    python scripts/gpu_views_bench.py [--out profiles/sample_views.json] [--quick] [--no-e2e]

HIP events around blocks of `--iters` calls, after a warm-up of every variant; the variants alternate inside every round
and the spread of a variant is (max - min) / median of its rounds, all in one process.  Outputs are compared
(torch.equal) before anything is timed.  Bytes are the algorithm's: every sampled frame read once, every view written once.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pretorched_x_amd as ptx                                   # noqa: E402
from pretorched_x_amd.testing import synth_state_dict            # noqa: E402

TF = ptx.transforms
DEV = "cuda:0"
OPTS = dict(input_size=[3, 224, 224], input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def alternate(variants, iters, rounds):
    """{name: fn} -> {name: {"ms": median, "spread": (max - min) / median, "rounds": [...]}}, variants alternating."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(timed(fn, iters))
    return {k: dict(ms=round(statistics.median(v), 4), spread=round((max(v) - min(v)) / statistics.median(v), 4),
                    rounds=[round(x, 4) for x in v]) for k, v in got.items()}


def composition(vs, video, **kw):
    N, Tv, H, W, _ = video.shape
    idx = [torch.from_numpy(i).to(video.device) for i in vs.frame_indices(Tv)]
    tfs = [TF.TransformFrames(OPTS, crop=w, **kw) for w in vs.windows(H, W)]

    def run():
        out = []
        for i in idx:
            frames = video.index_select(1, i)
            out += [tf(frames) for tf in tfs]
        return out
    return run


def kernel_rows(args):
    rows = []
    shapes = [(360, 640)] if args.quick else [(360, 640), (720, 1280), (640, 360)]
    for H, W in shapes:
        g = torch.Generator(device=DEV).manual_seed(H * 10000 + W)
        video = torch.randint(0, 256, (2, 300, H, W, 3), dtype=torch.uint8, device=DEV, generator=g)
        for mode in ("frames", "bf16"):
            kw = dict(out="frames") if mode == "frames" else dict(out="tensor", dtype=torch.bfloat16)
            vs = {s: TF.SampleViews(OPTS, share=s, **kw) for s in ("auto", "always", "never")}
            comp = composition(vs["auto"], video, **kw)
            want = torch.stack(comp(), 1)
            for s, v in vs.items():
                assert torch.equal(v(video), want), (H, W, mode, s)
            del want
            res = alternate(dict(composition=comp, auto=lambda: vs["auto"](video), shared=lambda: vs["always"](video),
                                 per_window=lambda: vs["never"](video)), args.iters, args.rounds)
            t = vs["auto"].tables(H, W)
            read = 2 * 10 * 16 * H * W * 3
            written = 2 * 30 * 16 * 224 * 224 * 3 * (1 if mode == "frames" else 2)
            spread = max(r["spread"] for r in res.values())
            row = dict(H=H, W=W, out=mode, videos=2, frames=300, views=30, clip_frames=16, resized=list(t["resized"]),
                       union=[len(t["rows"][0]), len(t["cols"][0])], auto_path=vs["auto"].describe(H, W),
                       bytes_read=read, bytes_written=written, spread=spread,
                       speedup_auto=round(res["composition"]["ms"] / res["auto"]["ms"], 3),
                       tb_per_s_auto=round((read + written) / res["auto"]["ms"] / 1e9, 3), **{k: v for k, v in res.items()})
            print(json.dumps(row), flush=True)
            rows.append(row)
        del video
        torch.cuda.empty_cache()
    return rows


def end_to_end(args):
    model = ptx.__dict__["resnet3d50"](num_classes=400, pretrained=None)
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
    model = model.to(DEV).eval()
    model.engine().lanes = 1
    g = torch.Generator(device=DEV).manual_seed(7)
    video = torch.randint(0, 256, (1, 300, 360, 640, 3), dtype=torch.uint8, device=DEV, generator=g)
    vs = TF.SampleViews(OPTS)
    mb = model.engine().max_batch(model, (3, 16, 224, 224))
    nv = ptx.engine.views_chunk(1, vs.num_views, mb)
    comp = composition(vs, video, out="frames")

    def loop():
        views = torch.cat(comp(), 0)                                       # [30,16,224,224,3]
        logits = torch.cat([model.forward_frames(views[i:i + nv], OPTS) for i in range(0, views.shape[0], nv)], 0)
        return torch.softmax(logits, -1).mean(0, keepdim=True)

    new = lambda: model.forward_views(video, OPTS, views=vs)
    with torch.no_grad():
        a, b = loop(), new()
        err = float((a - b).abs().max())
        same_logits = torch.equal(model.forward_views(video, OPTS, views=vs, reduce=None)[0],
                                  torch.cat([model.forward_frames(torch.cat(comp(), 0)[i:i + nv], OPTS) for i in range(0, 30, nv)], 0))
        res = alternate(dict(loop=loop, forward_views=new), max(2, args.iters // 5), args.rounds)
    row = dict(model="resnet3d50", video=[1, 300, 360, 640, 3], views=30, max_batch=mb, chunk=nv, logits_equal=same_logits,
               max_abs_diff_probs=err, spread=max(r["spread"] for r in res.values()),
               ratio=round(res["forward_views"]["ms"] / res["loop"]["ms"], 4), **res)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_views_bench: no GPU (there is no CPU path to time)")
    out = dict(device=torch.cuda.get_device_name(0), binary=ptx._lib.lib().ptx_version().decode(), iters=args.iters,
               rounds=args.rounds, kernel=kernel_rows(args))
    if not args.no_e2e:
        out["end_to_end"] = end_to_end(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
