"""10- / 12-bit YUV 4:2:0 sources on the GPU: `TransformFrames` / `SampleViews` on a P010 source (one launch, the colour
conversion inside the row staging) against the same call on the RGB frames, on an NV12 source of the same size, and against
what a user had to run before -- a torch-op P010 -> RGB uint8 conversion followed by the RGB launch.

    python scripts/gpu_yuv16_bench.py [--out profiles/yuv16_frames.json] [--quick]

One process; every variant is warmed, the variants alternate inside every round, and a round of a variant is `--iters` calls
between two device synchronises timed with the host clock.  The spread of a variant is (max - min) / median of its rounds.
Outputs are compared (torch.equal) before anything is timed.  Bytes are the algorithm's: every referenced frame read once
(3 B per pixel as P010 or RGB, 1.5 B as NV12), every output written once.  The P010 / NV12 ratio is the figure of interest:
the source reads twice the bytes and the kernel is LDS-issue-bound, so it is expected between 1x and 2x.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pretorched_x_amd as ptx                                   # noqa: E402

TF = ptx.transforms
DEV = "cuda:0"
OPTS = dict(input_size=[3, 224, 224], input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def alternate(variants, iters, rounds):
    """{name: fn} -> {name: {"ms": median, "spread": (max - min) / median, "rounds": [...]}}, variants alternating."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(timed(fn, iters))
    return {k: dict(ms=round(statistics.median(v), 4), spread=round((max(v) - min(v)) / statistics.median(v), 4),
                    rounds=[round(x, 4) for x in v]) for k, v in got.items()}


def torch_p010_to_rgb(src):
    """The colour contract in torch ops (int32), P010 planes -> uint8 [..,H,W,3]: widen, shift, multiply, clamp, cast,
    interleave -- what a user had to run before."""
    y_off, ky, krv, kgu, kgv, kbu = src.coefficients
    d, mask, H, W = src.bits - 8, (1 << src.bits) - 1, src.H, src.W
    sample = lambda p: (p.to(torch.int32) >> src.shift) & mask          # int16 planes: the sign extension is masked off
    yy = (sample(src.y) - y_off) * ky + (1 << (15 + d))
    c = sample(src.u) - (128 << d)
    c = c.repeat_interleave(2, -3).repeat_interleave(2, -2)[..., :H, :W, :]
    cb, cr = c[..., 0], c[..., 1]
    rgb = torch.stack([yy + krv * cr, yy - kgu * cb - kgv * cr, yy + kbu * cb], -1)
    return (rgb >> (16 + d)).clamp_(0, 255).to(torch.uint8)


def videos(N, T, H, W, seed):
    """(P010 source, NV12 source) of the same size; independent seeded noise."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    words = torch.randint(-32768, 32768, (N, T, H * 3 // 2, W), dtype=torch.int16, device=DEV, generator=g)
    nv12 = torch.randint(0, 256, (N, T, H * 3 // 2, W), dtype=torch.uint8, device=DEV, generator=g)
    return TF.YUV420P16.from_p010(words), TF.YUV420.from_nv12(nv12)


def report(res, bytes_):
    return dict(bytes=bytes_, spread=max(r["spread"] for r in res.values()),
                p010_over_nv12=round(res["p010"]["ms"] / res["nv12"]["ms"], 4),
                p010_over_rgb=round(res["p010"]["ms"] / res["rgb"]["ms"], 4),
                p010_over_torch_then_rgb=round(res["p010"]["ms"] / res["torch_then_rgb"]["ms"], 4), **res)


def check_contract(src):
    one = TF.YUV420P16(src.y[0, :1], src.u[0, :1], None, src.bits, src.align, src.matrix, src.color_range)
    assert torch.equal(torch_p010_to_rgb(one).cpu(), torch.from_numpy(one.to_rgb_numpy()))       # the torch ops follow the contract


def frames_rows(args):
    rows = []
    shapes = [(360, 640)] if args.quick else [(360, 640), (720, 1280), (1080, 1920)]
    for H, W in shapes:
        src, nv12 = videos(8, 16, H, W, H * 10000 + W)
        check_contract(src)
        rgb = torch_p010_to_rgb(src)
        for mode in ("frames", "tensor"):
            tf = TF.TransformFrames(OPTS, out=mode)
            assert torch.equal(tf(src), tf(rgb)), (H, W, mode)
            res = alternate(dict(rgb=lambda: tf(rgb), nv12=lambda: tf(nv12), p010=lambda: tf(src),
                                 torch_then_rgb=lambda: tf(torch_p010_to_rgb(src))), args.iters, args.rounds)
            px, out = 8 * 16 * H * W, 8 * 16 * 224 * 224 * 3 * (1 if mode == "frames" else 4)
            row = dict(what="TransformFrames", H=H, W=W, out=mode, frames=[8, 16],
                       **report(res, dict(rgb=px * 3 + out, nv12=px * 3 // 2 + out, p010=px * 3 + out,
                                          torch_then_rgb=px * 3 + px * 3 + px * 3 + out)))
            print(json.dumps(row), flush=True)
            rows.append(row)
        del src, nv12, rgb
        torch.cuda.empty_cache()
    return rows


def views_rows(args):
    rows = []
    shapes = [(360, 640)] if args.quick else [(360, 640), (720, 1280), (1080, 1920)]
    for H, W in shapes:
        src, nv12 = videos(2, 64, H, W, H * 10000 + W + 1)
        rgb = torch_p010_to_rgb(src)
        vs = TF.SampleViews(OPTS, num_frames=16, frame_stride=2, clips=10, crops=3, out="frames")
        assert torch.equal(vs(src), vs(rgb)), (H, W)
        res = alternate(dict(rgb=lambda: vs(rgb), nv12=lambda: vs(nv12), p010=lambda: vs(src),
                             torch_then_rgb=lambda: vs(torch_p010_to_rgb(src))), args.iters, args.rounds)
        sampled, whole = 2 * 10 * 16 * H * W, 2 * 64 * H * W
        out = 2 * 30 * 16 * 224 * 224 * 3
        row = dict(what="SampleViews", H=H, W=W, out="frames", videos=2, frames=64, views=30, clip_frames=16, path=vs.describe(H, W),
                   **report(res, dict(rgb=sampled * 3 + out, nv12=sampled * 3 // 2 + out, p010=sampled * 3 + out,
                                      torch_then_rgb=whole * 3 + whole * 3 + sampled * 3 + out)))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del src, nv12, rgb
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_yuv16_bench: no GPU (there is no CPU path to time)")
    out = dict(device=torch.cuda.get_device_name(0), binary=ptx._lib.lib().ptx_version().decode(), iters=args.iters,
               rounds=args.rounds, clock="host clock around device synchronises", frames=frames_rows(args), views=views_rows(args))
    ratios = [r["p010_over_nv12"] for r in out["frames"] + out["views"]]
    out["p010_over_nv12_range"] = [min(ratios), max(ratios)]
    print(json.dumps(dict(p010_over_nv12_range=out["p010_over_nv12_range"])), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
