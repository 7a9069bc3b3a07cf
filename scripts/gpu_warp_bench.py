"""Interpolated per-clip warps on the GPU: the `ptx_warp_frames` launch for bilinear / bicubic x affine / perspective, the
nearest apply launch of `ptx_rand_augment_apply` and a same-size `copy_` in the same run, `RandAugment(num_ops=2,
interpolation="bilinear")` through the public call, and the per-frame Pillow loop on one host core that the call replaces.

    python scripts/gpu_warp_bench.py [--out profiles/warp_frames.json] [--quick]

Shape: 8 clips x 16 frames of 224 x 224.  The launches are timed with HIP events around `--iters` back-to-back launches (through
ctypes, buffers allocated once), every variant warmed, the variants alternating inside every round; the public call the same
way around the Python call (its host work and uploads included).  The spread of a variant is (max - min) / median of its
rounds.  Every warp's output is compared with the numpy statement of the contract on the first clip before anything is timed.
Bytes are the algorithm's: 3 B read and 3 B written per pixel.  The clips of a launch rotate by different angles (and, for a
perspective, lean differently), so the source footprints of the tiles are not axis-aligned.  The Pillow loop (when Pillow is
installed) runs bilinear rotations frame by frame on `--pil-frames` frames and is reported per frame.
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pretorched_x_amd as ptx                                   # noqa: E402

TF, L = ptx.transforms, ptx._lib
DEV = "cuda:0"
N, T, S = 8, 16, 224
FILL = (0, 0, 0)


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


def clip_coeffs(kind):
    """Per clip a rotation by 5 + 7 n degrees about the centre; a perspective also leans (denominator about 0.8 .. 1.2)."""
    rows = []
    for n in range(N):
        a = TF.rotation_matrix(5.0 + 7.0 * n, S, S) + [0.0, 0.0]
        if kind == L.PTX_WARP_PERSPECTIVE:
            a[6], a[7] = (0.2 if n % 2 else -0.2) / S, 0.1 / S
        rows.append(a)
    return np.full(N, kind, np.int32), np.array(rows, np.float64)


def warp_launch(frames, interpolation, kind):
    lib = L.lib()
    kinds, coeffs = clip_coeffs(kind)
    desc = L.WarpDesc(N, T, S, S, TF.INTERPOLATIONS.index(interpolation), FILL[0], FILL[1], FILL[2], 0)
    assert lib.ptx_warp_frames_supported(C.byref(desc), C.c_void_p(kinds.ctypes.data), C.c_void_p(coeffs.ctypes.data)) == 1
    d_kinds, d_coeffs = torch.from_numpy(kinds).to(DEV), torch.from_numpy(coeffs.reshape(-1)).to(DEV)
    y = torch.empty_like(frames)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = (desc, d_kinds, d_coeffs)

    def run(_keep=keep):
        L.check(lib.ptx_warp_frames(C.byref(desc), C.c_void_p(frames.data_ptr()), C.c_void_p(d_kinds.data_ptr()),
                                    C.c_void_p(d_coeffs.data_ptr()), C.c_void_p(y.data_ptr()), stream), "ptx_warp_frames")

    run()
    want = TF.warp_numpy(frames[:1].cpu().numpy(), kinds[:1], coeffs[:1], interpolation, FILL)
    assert np.array_equal(y[:1].cpu().numpy(), want), (interpolation, kind)
    return run


def nearest_launch(frames):
    """The nearest rotate of ptx_rand_augment_apply (one position, uint8 out), the launch the warp stands next to."""
    lib = L.lib()
    params = (np.full((N, 1), L.PTX_RANDAUG_ROTATE, np.int32), np.array([[5.0 + 7.0 * n] for n in range(N)]))
    rows = np.ascontiguousarray(TF.rand_augment_rows(params, S, S, N))
    d_rows = torch.from_numpy(rows.reshape(-1)).to(DEV)
    desc = L.RandAugDesc(N, T, S, S, L.PTX_RESIZE_OUT_U8, 1, 0, 0, FILL[0], FILL[1], FILL[2], 0)
    y = torch.empty_like(frames)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = (desc, d_rows)

    def run(_keep=keep):
        L.check(lib.ptx_rand_augment_apply(C.byref(desc), C.c_void_p(frames.data_ptr()), C.c_void_p(d_rows.data_ptr()), None,
                                           C.c_void_p(y.data_ptr()), None, stream), "ptx_rand_augment_apply")

    return run


def pil_loop(raw_frames, frames):
    """Seconds per frame of the host loop the call replaces: one bilinear Image.rotate per frame, one core.  None without Pillow."""
    try:
        from PIL import Image
    except ImportError:
        return None
    torch.set_num_threads(1)
    t0 = time.perf_counter()
    for i in range(frames):
        img = Image.fromarray(raw_frames[i % len(raw_frames)], "RGB")
        np.asarray(img.rotate(5.0 + 7.0 * (i % N), Image.BILINEAR, fillcolor=FILL))
    return (time.perf_counter() - t0) / frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pil-frames", type=int, default=64)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_warp_bench: no GPU (there is no CPU path to time)")
    iters, rounds = (5, 2) if args.quick else (args.iters, args.rounds)
    g = torch.Generator(device=DEV).manual_seed(1)
    frames = torch.randint(0, 256, (N, T, S, S, 3), dtype=torch.uint8, device=DEV, generator=g)
    variants = {}
    for interpolation in ("bilinear", "bicubic"):
        for kind, name in ((L.PTX_WARP_AFFINE, "affine"), (L.PTX_WARP_PERSPECTIVE, "perspective")):
            variants["warp_%s_%s" % (interpolation, name)] = warp_launch(frames, interpolation, kind)
    variants["warp_nearest_perspective"] = warp_launch(frames, "nearest", L.PTX_WARP_PERSPECTIVE)
    variants["apply_nearest_rotate"] = nearest_launch(frames)
    dst = torch.empty_like(frames)
    variants["copy"] = lambda: dst.copy_(frames)
    kernels = alternate(variants, iters, rounds)
    px = N * T * S * S
    for row in kernels.values():
        row["GBps"] = round(px * 6 / row["ms"] / 1e6, 1)
    ratios = {k + "_over_copy": round(v["ms"] / kernels["copy"]["ms"], 2) for k, v in kernels.items() if k != "copy"}

    # the public call: a 2-op draw per clip, geometric ops interpolated; host work and uploads included
    ra = TF.RandAugment(2, 9, generator=torch.Generator().manual_seed(5), interpolation="bilinear")
    ra_nearest = TF.RandAugment(2, 9, generator=torch.Generator().manual_seed(5))
    draw = ra.draw(N, S, S)
    geo = (np.array([[5, 6]] * N, np.int32), np.array([[5.0 + 7.0 * n, 0.3] for n in range(N)]))       # rotate, then brightness
    calls = alternate({"rand_augment_bilinear_draw": lambda: ra(frames, params=draw),
                       "rand_augment_nearest_draw": lambda: ra_nearest(frames, params=draw),
                       "rand_augment_bilinear_rotate_brightness": lambda: ra(frames, params=geo),
                       "rand_augment_nearest_rotate_brightness": lambda: ra_nearest(frames, params=geo)}, max(iters // 4, 2), rounds)
    ra(frames, params=draw)
    launches = dict(draw=list(ra.last_launches), draw_codes=draw[0].tolist())
    per_frame = pil_loop(frames[0].cpu().numpy(), 4 if args.quick else args.pil_frames)
    pil = None
    if per_frame is not None:
        pil = dict(ms_per_frame=round(per_frame * 1e3, 4), ms_per_batch=round(per_frame * 1e3 * N * T, 2),
                   frames_timed=4 if args.quick else args.pil_frames,
                   what="Pillow on one host core, one bilinear Image.rotate per 224 x 224 frame already in host memory (no copies counted)")
        ratios["pil_batch_over_warp_bilinear_affine"] = round(pil["ms_per_batch"] / kernels["warp_bilinear_affine"]["ms"], 1)
    out = dict(device=torch.cuda.get_device_name(0), binary=L.lib().ptx_version().decode(), shape=[N, T, S, S], iters=iters,
               rounds=rounds, clock="HIP events around back-to-back launches / calls", kernels=kernels, calls=calls, launches=launches,
               pil_loop=pil, ratios=ratios)
    print(json.dumps(dict(ratios=ratios, pil=pil, ms={k: v["ms"] for k, v in list(kernels.items()) + list(calls.items())})), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
