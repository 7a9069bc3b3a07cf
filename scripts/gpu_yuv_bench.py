"""YUV 4:2:0 sources on the GPU: `TransformFrames` / `SampleViews` on an NV12 source (one launch, the colour conversion
inside the row staging) against what the library offered before -- a torch-op NV12 -> RGB uint8 conversion of everything
that must be converted, then the RGB launch -- and against the RGB launch alone on frames converted beforehand.

    python scripts/gpu_yuv_bench.py [--out profiles/yuv_frames.json] [--quick] [--no-e2e]

Method of scripts/gpu_views_bench.py: HIP events around blocks of `--iters` calls, after a warm-up of every variant; the
variants alternate inside every round and the spread of a variant is (max - min) / median of its rounds, all in one
process.  Outputs are compared (torch.equal) before anything is timed.  Bytes are the algorithm's: every referenced frame
read once (1.5 B per pixel as NV12, 3 B as RGB), every output written once; the torch conversion reads 1.5 B and writes
3 B per pixel of everything it converts (its int32 temporaries are not counted).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pretorched_x_amd as ptx                                   # noqa: E402
from pretorched_x_amd.testing import synth_state_dict            # noqa: E402
from gpu_views_bench import alternate                            # noqa: E402

TF = ptx.transforms
DEV = "cuda:0"
OPTS = dict(input_size=[3, 224, 224], input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])


def torch_nv12_to_rgb(src):
    """The colour contract in torch ops (int32), NV12 planes -> uint8 [..,H,W,3]: what a user had to run before."""
    y_off, ky, krv, kgu, kgv, kbu = src.coefficients
    H, W = src.H, src.W
    yy = (src.y.to(torch.int32) - y_off) * ky + 32768
    c = src.u.to(torch.int32) - 128
    c = c.repeat_interleave(2, -3).repeat_interleave(2, -2)[..., :H, :W, :]
    cb, cr = c[..., 0], c[..., 1]
    rgb = torch.stack([yy + krv * cr, yy - kgu * cb - kgv * cr, yy + kbu * cb], -1)
    return (rgb >> 16).clamp_(0, 255).to(torch.uint8)


def nv12_video(N, T, H, W, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return TF.YUV420.from_nv12(torch.randint(0, 256, (N, T, H * 3 // 2, W), dtype=torch.uint8, device=DEV, generator=g))


def report(res, bytes_):
    spread = max(r["spread"] for r in res.values())
    return dict(bytes=bytes_, spread=spread, nv12_over_torch_then_rgb=round(res["nv12"]["ms"] / res["torch_then_rgb"]["ms"], 4),
                nv12_over_rgb_alone=round(res["nv12"]["ms"] / res["rgb_alone"]["ms"], 4), **res)


def frames_rows(args):
    rows = []
    shapes = [(360, 640)] if args.quick else [(360, 640), (720, 1280), (1080, 1920)]
    for H, W in shapes:
        src = nv12_video(8, 16, H, W, H * 10000 + W)
        rgb = torch_nv12_to_rgb(src)
        one = TF.YUV420(src.y[0, :1], src.u[0, :1])
        assert torch.equal(rgb[0, :1].cpu(), torch.from_numpy(one.to_rgb_numpy()))          # the torch ops follow the contract
        for mode in ("frames", "bf16"):
            tf = TF.TransformFrames(OPTS, out="frames") if mode == "frames" else TF.TransformFrames(OPTS, dtype=torch.bfloat16)
            assert torch.equal(tf(src), tf(rgb)), (H, W, mode)
            res = alternate(dict(nv12=lambda: tf(src), torch_then_rgb=lambda: tf(torch_nv12_to_rgb(src)), rgb_alone=lambda: tf(rgb)),
                            args.iters, args.rounds)
            px, out = 8 * 16 * H * W, 8 * 16 * 224 * 224 * 3 * (1 if mode == "frames" else 2)
            row = dict(what="TransformFrames", H=H, W=W, out=mode, frames=[8, 16],
                       **report(res, dict(nv12=px * 3 // 2 + out, torch_then_rgb=px * 3 // 2 + px * 3 + px * 3 + out, rgb_alone=px * 3 + out)))
            print(json.dumps(row), flush=True)
            rows.append(row)
        del src, rgb
        torch.cuda.empty_cache()
    return rows


def views_rows(args):
    rows = []
    H, W = 360, 640
    src = nv12_video(2, 300, H, W, 77)
    rgb = torch_nv12_to_rgb(src)
    for mode in ("frames", "bf16"):
        vs = TF.SampleViews(OPTS, out="frames") if mode == "frames" else TF.SampleViews(OPTS, out="tensor", dtype=torch.bfloat16)
        assert torch.equal(vs(src), vs(rgb)), mode
        res = alternate(dict(nv12=lambda: vs(src), torch_then_rgb=lambda: vs(torch_nv12_to_rgb(src)), rgb_alone=lambda: vs(rgb)),
                        args.iters, args.rounds)
        sampled, whole = 2 * 10 * 16 * H * W, 2 * 300 * H * W
        out = 2 * 30 * 16 * 224 * 224 * 3 * (1 if mode == "frames" else 2)
        row = dict(what="SampleViews", H=H, W=W, out=mode, videos=2, frames=300, views=30, clip_frames=16,
                   path=vs.describe(H, W),
                   **report(res, dict(nv12=sampled * 3 // 2 + out, torch_then_rgb=whole * 3 // 2 + whole * 3 + sampled * 3 + out,
                                      rgb_alone=sampled * 3 + out)))
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def end_to_end(args):
    model = ptx.__dict__["resnet3d50"](num_classes=400, pretrained=None)
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
    model = model.to(DEV).eval()
    model.engine().lanes = 1
    src = nv12_video(1, 300, 360, 640, 7)
    rgb = torch_nv12_to_rgb(src)
    vs = TF.SampleViews(OPTS)
    with torch.no_grad():
        same = torch.equal(model.forward_views(src, OPTS, views=vs), model.forward_views(rgb, OPTS, views=vs))
        res = alternate(dict(nv12=lambda: model.forward_views(src, OPTS, views=vs),
                             torch_then_rgb=lambda: model.forward_views(torch_nv12_to_rgb(src), OPTS, views=vs),
                             rgb_alone=lambda: model.forward_views(rgb, OPTS, views=vs)), max(2, args.iters // 5), args.rounds)
    row = dict(model="resnet3d50", video=[1, 300, 360, 640], views=30, equal=same, spread=max(r["spread"] for r in res.values()),
               nv12_over_torch_then_rgb=round(res["nv12"]["ms"] / res["torch_then_rgb"]["ms"], 4),
               nv12_over_rgb_alone=round(res["nv12"]["ms"] / res["rgb_alone"]["ms"], 4), **res)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_yuv_bench: no GPU (there is no CPU path to time)")
    out = dict(device=torch.cuda.get_device_name(0), binary=ptx._lib.lib().ptx_version().decode(), iters=args.iters,
               rounds=args.rounds, frames=frames_rows(args), views=views_rows(args))
    if not args.no_e2e:
        out["end_to_end"] = end_to_end(args)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
