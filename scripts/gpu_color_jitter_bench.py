"""Per-clip ColorJitter / RandomGrayscale on the GPU: the two launches of `pretorched.transforms.ColorJitter` against the plain
uint8 -> fp32 conversion at the same shape, and `TransformFrames(random_resized_crop, color=cj)` against the same call without
colour.

    python scripts/gpu_color_jitter_bench.py [--out profiles/color_jitter.json] [--quick]

Shape: 8 clips x 16 frames of 224 x 224.  The launches are timed with HIP events around `--iters` back-to-back launches
(through ctypes, buffers allocated once), every variant warmed, the variants alternating inside every round; the end-to-end
calls the same way around the Python calls (their host work included).  The spread of a variant is (max - min) / median of
its rounds.  The colour outputs are compared with the numpy statement of the contract on the first clip before anything is
timed.  Bytes are the algorithm's: the statistics launch reads 3 B per pixel; an apply launch reads 3 B and writes 3 B
(uint8) or 12 B (fp32) per pixel, as the plain conversion does.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pretorched_x_amd as ptx                                   # noqa: E402

TF, L = ptx.transforms, ptx._lib
DEV = "cuda:0"
OPTS = dict(input_size=[3, 224, 224], input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
N, T, S = 8, 16, 224


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


def lists(names, seed):
    """[N, 5] rows with the ops `names` in a per-clip random order and factors as ColorJitter(0.4, 0.4, 0.4, 0.1) draws them."""
    cj = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, grayscale=1.0 if "grayscale" in names else 0.0,
                        generator=torch.Generator().manual_seed(seed))
    codes, factors = cj.draw(N)
    keep = torch.tensor([[TF.COLOR_OPS[int(c)] in names for c in row] for row in codes])
    out_c, out_f = torch.zeros_like(codes), torch.zeros_like(factors)
    for n in range(N):
        k = int(keep[n].sum())
        out_c[n, :k], out_f[n, :k] = codes[n][keep[n]], factors[n][keep[n]]
    return TF.check_color_params((out_c, out_f), N)


def launches(frames, params, mode):
    """(stats fn or None, apply fn, output) on device frames [N,T,S,S,3] through ctypes, buffers allocated once."""
    lib = L.lib()
    codes, factors = params
    contrast = bool((codes == L.PTX_COLOR_CONTRAST).any())
    d_codes, d_factors = codes.to(DEV), factors.to(DEV)
    desc = L.ColorDesc(N, T, S, S, mode, int(contrast))
    norm = L.NormDesc.make(OPTS["mean"], OPTS["std"], OPTS["input_space"], OPTS["input_range"])
    y = torch.empty((N, T, S, S, 3), dtype=torch.uint8, device=DEV) if mode == L.PTX_RESIZE_OUT_U8 else \
        torch.empty((N, 3, T, S, S), dtype=torch.float32, device=DEV)
    sums = torch.zeros(N * T, dtype=torch.int64, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (C.byref(desc), C.c_void_p(frames.data_ptr()), C.c_void_p(d_codes.data_ptr()), C.c_void_p(d_factors.data_ptr()))
    keep = (d_codes, d_factors, desc, norm, sums)

    def stats(_keep=keep):
        L.check(lib.ptx_color_jitter_stats(*args, C.c_void_p(sums.data_ptr()), stream), "ptx_color_jitter_stats")

    def apply(_keep=keep):
        L.check(lib.ptx_color_jitter_apply(*args, C.c_void_p(sums.data_ptr()) if contrast else None, C.c_void_p(y.data_ptr()),
                                           C.byref(norm), stream), "ptx_color_jitter_apply")

    return (stats if contrast else None), apply, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_color_jitter_bench: no GPU (there is no CPU path to time)")
    iters, rounds = (5, 2) if args.quick else (args.iters, args.rounds)
    g = torch.Generator(device=DEV).manual_seed(1)
    frames = torch.randint(0, 256, (N, T, S, S, 3), dtype=torch.uint8, device=DEV, generator=g)
    bcs, all5 = lists(("brightness", "contrast", "saturation"), 2), lists(TF.COLOR_OPS[1:], 3)
    variants, outs = {}, {}
    for tag, params in (("bcs", bcs), ("all5", all5)):
        for mname, mode in (("u8", L.PTX_RESIZE_OUT_U8), ("f32", L.PTX_RESIZE_OUT_F32)):
            stats, apply, y = launches(frames, params, mode)
            if mname == "u8":
                variants["stats_" + tag] = stats
            variants["apply_%s_%s" % (tag, mname)] = apply
            stats()
            apply()
            outs[(tag, mname)] = y
        want = TF.color_jitter_numpy(frames[:1].cpu().numpy(), (params[0][:1], params[1][:1]))
        assert np.array_equal(outs[(tag, "u8")][:1].cpu().numpy(), want), tag
        assert torch.equal(outs[(tag, "f32")], TF.FramesToTensor(OPTS)(outs[(tag, "u8")])), tag
    plain = torch.empty((N, 3, T, S, S), dtype=torch.float32, device=DEV)
    norm = L.NormDesc.make(OPTS["mean"], OPTS["std"], OPTS["input_space"], OPTS["input_range"])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    variants["frames_u8_to_ncdhw"] = lambda: L.check(L.lib().ptx_frames_u8_to_ncdhw(
        C.c_void_p(frames.data_ptr()), C.c_void_p(plain.data_ptr()), N, T, S, S, 3, C.byref(norm), stream), "ptx_frames_u8_to_ncdhw")
    kernels = alternate(variants, iters, rounds)
    px = N * T * S * S
    for k, row in kernels.items():
        nbytes = px * (3 if k.startswith("stats") else 6 if k.endswith("u8") else 15)
        row["GBps"] = round(nbytes / row["ms"] / 1e6, 1)
    base = kernels["frames_u8_to_ncdhw"]["ms"]
    ratios = {k: round(kernels[k]["ms"] / base, 3) for k in ("apply_bcs_f32", "apply_all5_f32")}
    ratios["stats_plus_apply_bcs_f32"] = round((kernels["stats_bcs"]["ms"] + kernels["apply_bcs_f32"]["ms"]) / base, 3)
    ratios["stats_plus_apply_all5_f32"] = round((kernels["stats_all5"]["ms"] + kernels["apply_all5_f32"]["ms"]) / base, 3)

    # end to end: raw 8 x 16 frames of 256 x 340 -> RandomResizedCrop -> (colour) -> fp32 clip
    raw = torch.randint(0, 256, (N, T, 256, 340, 3), dtype=torch.uint8, device=DEV, generator=g)
    cj = TF.ColorJitter(0.4, 0.4, 0.4, 0.1, grayscale=0.2, generator=torch.Generator().manual_seed(5))
    tf_plain = TF.TransformFrames(OPTS, random_resized_crop=True, random_hflip=True, generator=torch.Generator().manual_seed(6))
    tf_color = TF.TransformFrames(OPTS, random_resized_crop=True, random_hflip=True, generator=torch.Generator().manual_seed(6), color=cj)
    tf_bcs = TF.TransformFrames(OPTS, random_resized_crop=True, random_hflip=True, generator=torch.Generator().manual_seed(6),
                                color=TF.ColorJitter(0.4, 0.4, 0.4, generator=torch.Generator().manual_seed(5)))
    e2e = alternate({"transform_frames": lambda: tf_plain(raw), "transform_frames_color_bcs": lambda: tf_bcs(raw),
                     "transform_frames_color_all5": lambda: tf_color(raw)}, max(iters // 2, 2), rounds)
    ratios["e2e_color_bcs_over_plain"] = round(e2e["transform_frames_color_bcs"]["ms"] / e2e["transform_frames"]["ms"], 3)
    ratios["e2e_color_all5_over_plain"] = round(e2e["transform_frames_color_all5"]["ms"] / e2e["transform_frames"]["ms"], 3)
    out = dict(device=torch.cuda.get_device_name(0), binary=L.lib().ptx_version().decode(), shape=[N, T, S, S], iters=iters,
               rounds=rounds, clock="HIP events around back-to-back launches / calls", kernels=kernels, end_to_end=e2e,
               end_to_end_source=[N, T, 256, 340], ratios=ratios)
    print(json.dumps(dict(ratios=ratios, ms={k: v["ms"] for k, v in list(kernels.items()) + list(e2e.items())})), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
