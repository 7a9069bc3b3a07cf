"""Per-clip GaussianBlur on the GPU: the launch of `pretorched.transforms.GaussianBlur` at 9 and 23 taps with uint8 and fp32
output, the public call by the host clock, and the torch route it replaces on the same GPU.

    python scripts/gpu_blur_bench.py [--out profiles/blur_frames.json] [--quick]

Shape: 8 clips x 16 frames of 224 x 224, every clip blurred with a sigma of its own.  The launches are timed with HIP events
around `--iters` back-to-back launches (through ctypes, buffers allocated once), every variant warmed, the variants alternating
inside every round; the median of the rounds is reported, the spread of a variant is (max - min) / median of its rounds.  The
19 MB of frames stay cache-resident between back-to-back launches.  The public call `gb(frames, params=p)` (weights built on the
host, one upload, one launch) is timed by the host clock around a synchronised loop.  The torch route is what a user writes
without the kernel: permute + float + F.pad(reflect) + a depthwise F.conv2d with the clip's fp32 outer-product kernel + round +
to(uint8) + permute, clip by clip (every clip has its own sigma), timed the same two ways.  The uint8 output is compared with
the numpy statement of the contract on one frame of every clip before anything is timed, the fp32 output with FramesToTensor of
the uint8 one.  Bytes are the algorithm's: 3 B read and 3 B (uint8) or 12 B (fp32) written per pixel; fp64 operations are
counted from the tile arithmetic of DESIGN.md 3.41.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pretorched_x_amd as ptx                                   # noqa: E402

TF, L = ptx.transforms, ptx._lib
DEV = "cuda:0"
OPTS = dict(input_size=[3, 224, 224], input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
N, T, S = 8, 16, 224
TILE = 32


def event_timed(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def host_timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def alternate(variants, iters, rounds, clock=event_timed):
    """{name: fn} -> {name: {"ms": median, "spread": (max - min) / median, "rounds": [...]}}, variants alternating."""
    for fn in variants.values():
        for _ in range(3):
            fn()
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(clock(fn, iters))
    return {k: dict(ms=round(statistics.median(v), 4), spread=round((max(v) - min(v)) / statistics.median(v), 4),
                    rounds=[round(x, 4) for x in v]) for k, v in got.items()}


def launch(frames, params, gb, mode):
    """(launch fn, output) on device frames [N,T,S,S,3] through ctypes, buffers allocated once."""
    lib = L.lib()
    kx, ky = gb.kernel_size
    wx, wy = gb.weights(params)
    d_apply, d_wx, d_wy = params[0].to(DEV), wx.to(DEV), wy.to(DEV)
    desc = L.BlurDesc(N, T, S, S, kx, ky, mode)
    norm = L.NormDesc.make(OPTS["mean"], OPTS["std"], OPTS["input_space"], OPTS["input_range"])
    y = torch.empty((N, T, S, S, 3), dtype=torch.uint8, device=DEV) if mode == L.PTX_RESIZE_OUT_U8 else \
        torch.empty((N, 3, T, S, S), dtype=torch.float32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = (d_apply, d_wx, d_wy, desc, norm)

    def run(_keep=keep):
        L.check(lib.ptx_gaussian_blur_frames(C.byref(desc), C.c_void_p(frames.data_ptr()), C.c_void_p(d_apply.data_ptr()),
                                             C.c_void_p(d_wx.data_ptr()), C.c_void_p(d_wy.data_ptr()), C.c_void_p(y.data_ptr()),
                                             C.byref(norm), stream), "ptx_gaussian_blur_frames")

    return run, y


def torch_route(frames, kernels2d, k):
    """The route the kernel replaces, on the same GPU: fp32 NCHW copy, reflect pad, depthwise conv2d, round, cast, back to NHWC."""
    out = torch.empty_like(frames)
    for n in range(N):
        x = frames[n].permute(0, 3, 1, 2).float()
        x = F.pad(x, [k // 2] * 4, mode="reflect")
        out[n] = torch.round(F.conv2d(x, kernels2d[n], groups=3)).to(torch.uint8).permute(0, 2, 3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_blur_bench: no GPU (there is no CPU path to time)")
    iters, rounds = (5, 2) if args.quick else (args.iters, args.rounds)
    g = torch.Generator(device=DEV).manual_seed(1)
    frames = torch.randint(0, 256, (N, T, S, S, 3), dtype=torch.uint8, device=DEV, generator=g)
    variants, calls, routes, checks, work = {}, {}, {}, {}, {}
    for k in (9, 23):
        gb = TF.GaussianBlur(k, sigma=(0.1, 2.0), generator=torch.Generator().manual_seed(k))
        params = gb.check_params(gb.draw(N), N, S, S)
        wx, wy = gb.weights(params)
        outs = {}
        for mname, mode in (("u8", L.PTX_RESIZE_OUT_U8), ("f32", L.PTX_RESIZE_OUT_F32)):
            run, y = launch(frames, params, gb, mode)
            variants["blur_k%d_%s" % (k, mname)] = run
            run()
            outs[mname] = y
        want = TF.gaussian_blur_numpy(frames[:, :1].cpu().numpy(), params[0], wx, wy)
        assert np.array_equal(outs["u8"][:, :1].cpu().numpy(), want), k
        assert torch.equal(outs["f32"], TF.FramesToTensor(OPTS)(outs["u8"])), k
        calls["call_k%d" % k] = lambda gb=gb, params=params: gb(frames, params=params)
        k2 = [torch.mm(wy[n][:, None], wx[n][None, :]).expand(3, 1, k, k).contiguous().to(DEV) for n in range(N)]
        routes["torch_k%d" % k] = lambda k2=k2, k=k: torch_route(frames, k2, k)
        ref = routes["torch_k%d" % k]()
        differ = (ref != outs["u8"])
        step = (ref.int() - outs["u8"].int()).abs().max().item()
        checks["k%d" % k] = dict(samples=differ.numel(), differ_from_torch_route=int(differ.sum().item()), largest_step=int(step))
        halo = (TILE + k - 1) / TILE
        work["k%d" % k] = dict(lds_bytes=2 * 33 * 8 + (TILE + k - 1) * (TILE * 3 * 8 + (TILE + k - 1) * 3) + 16,
                               bytes_staged_per_output_byte=round(halo * halo, 3),
                               fp64_instructions_per_sample=round(k * halo + 2 * k + k * halo / 4 + 4, 1))   # FMAs, mul + add, conversions + rounding
    kernels = alternate(variants, iters, rounds)
    px = N * T * S * S
    for name, row in kernels.items():
        k = int(name.split("_")[1][1:])
        row["GBps"] = round(px * (6 if name.endswith("u8") else 15) / row["ms"] / 1e6, 1)
        row["fp64_Ginstr_per_s"] = round(px * 3 * work["k%d" % k]["fp64_instructions_per_sample"] / row["ms"] / 1e6, 1)
    slow_iters = max(iters // 10, 2)
    public = alternate(calls, slow_iters, rounds, host_timed)
    torch_events = alternate(routes, slow_iters, rounds)
    torch_host = alternate(routes, slow_iters, rounds, host_timed)
    ratios = {}
    for k in (9, 23):
        ratios["torch_route_over_launch_k%d" % k] = round(torch_events["torch_k%d" % k]["ms"] / kernels["blur_k%d_u8" % k]["ms"], 1)
        ratios["torch_route_over_call_k%d_host_clock" % k] = round(torch_host["torch_k%d" % k]["ms"] / public["call_k%d" % k]["ms"], 1)
    out = dict(device=torch.cuda.get_device_name(0), binary=L.lib().ptx_version().decode(), shape=[N, T, S, S], iters=iters,
               rounds=rounds, clock="HIP events around back-to-back launches; the host clock around synchronised loops where said",
               kernels=kernels, public_call_host_clock=public, torch_route_events=torch_events, torch_route_host_clock=torch_host,
               slow_iters=slow_iters, tile=work, against_torch_route=checks, ratios=ratios)
    print(json.dumps(dict(ratios=ratios, ms={k: v["ms"] for k, v in list(kernels.items()) + list(public.items()) +
                                             list(torch_events.items())}, checks=checks)), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
