"""Per-clip RandAugment on the GPU: the launches of one position of `pretorched.transforms.RandAugment` per op family, with and
without the statistics launch, `TransformFrames(random_resized_crop, augment=ra)` against the same call without it, and the
per-frame PIL loop on one host core that the call replaces.

    python scripts/gpu_rand_augment_bench.py [--out profiles/rand_augment.json] [--quick]

Shape: 8 clips x 16 frames of 224 x 224.  The launches are timed with HIP events around `--iters` back-to-back launches (through
ctypes, buffers allocated once), every variant warmed, the variants alternating inside every round; the end-to-end calls the
same way around the Python calls (their host work included).  The spread of a variant is (max - min) / median of its rounds.
Every op's uint8 output is compared with the numpy statement of the contract on the first clip before anything is timed.  Bytes
are the algorithm's: a statistics launch reads 3 B per pixel; an apply launch reads 3 B and writes 3 B (uint8) or 12 B (fp32)
per pixel.  The PIL loop (Pillow on the host, when it is installed) runs the same two-op draw frame by frame on `--pil-frames`
frames and is reported per frame; it is left out, and said so, where Pillow is missing.
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
OPTS = dict(input_size=[3, 224, 224], input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
N, T, S = 8, 16, 224
FILL = (0, 0, 0)
STATS = (L.PTX_RANDAUG_CONTRAST, L.PTX_RANDAUG_AUTOCONTRAST, L.PTX_RANDAUG_EQUALIZE)


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


def one_op(code, bin_=9):
    """Every clip runs op `code` at `bin_`, the signed ones with alternating signs: (codes [N, 1], magnitudes [N, 1])."""
    table = TF.rand_augment_space(31, S, S)[code]
    mag = float(table[bin_].item()) if table is not None else 0.0
    return (np.full((N, 1), code, np.int32), np.array([[-mag if (TF.RANDAUG_SIGNED[code] and n % 2) else mag] for n in range(N)]))


def launches(frames, params, mode):
    """(stats fn or None, apply fn, output) of position 0 on device frames [N,T,S,S,3] through ctypes, buffers allocated once."""
    lib = L.lib()
    rows = TF.rand_augment_rows(params, S, S, N)
    need = bool(np.isin(rows[:, 0, 0], STATS).any())
    d_rows = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)).to(DEV)
    desc = L.RandAugDesc(N, T, S, S, mode, rows.shape[1], 0, int(need), FILL[0], FILL[1], FILL[2], 0)
    assert lib.ptx_rand_augment_supported(C.byref(desc), C.c_void_p(np.ascontiguousarray(rows).ctypes.data)) == 1
    norm = L.NormDesc.make(OPTS["mean"], OPTS["std"], OPTS["input_space"], OPTS["input_range"])
    y = torch.empty((N, T, S, S, 3), dtype=torch.uint8, device=DEV) if mode == L.PTX_RESIZE_OUT_U8 else \
        torch.empty((N, 3, T, S, S), dtype=torch.float32, device=DEV)
    st = torch.zeros(N * T * L.PTX_RANDAUG_STATS_WORDS, dtype=torch.int32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (C.byref(desc), C.c_void_p(frames.data_ptr()), C.c_void_p(d_rows.data_ptr()))
    keep = (d_rows, desc, norm, st)

    def stats(_keep=keep):
        L.check(lib.ptx_rand_augment_stats(*args, C.c_void_p(st.data_ptr()), stream), "ptx_rand_augment_stats")

    def apply(_keep=keep):
        L.check(lib.ptx_rand_augment_apply(*args, C.c_void_p(st.data_ptr()) if need else None, C.c_void_p(y.data_ptr()),
                                           C.byref(norm), stream), "ptx_rand_augment_apply")

    return (stats if need else None), apply, y


def pil_loop(raw_frames, params, frames):
    """Seconds per frame of the host loop the call replaces: PIL images through the same ops, one core.  None without Pillow."""
    try:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
        import make_rand_augment_golden as MG
    except ImportError:
        return None
    torch.set_num_threads(1)
    codes, mags = params
    t0 = time.perf_counter()
    for i in range(frames):
        MG.pil_chain(raw_frames[i % len(raw_frames)], codes[i % len(codes)], mags[i % len(mags)], FILL)
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
        raise SystemExit("gpu_rand_augment_bench: no GPU (there is no CPU path to time)")
    iters, rounds = (5, 2) if args.quick else (args.iters, args.rounds)
    g = torch.Generator(device=DEV).manual_seed(1)
    frames = torch.randint(0, 256, (N, T, S, S, 3), dtype=torch.uint8, device=DEV, generator=g)
    first = frames[:1].cpu().numpy()
    variants = {}
    for code, name in enumerate(TF.RANDAUG_OPS):
        params = one_op(code)
        stats, apply, y = launches(frames, params, L.PTX_RESIZE_OUT_U8)
        if stats is not None:
            stats()
            variants["stats_" + name] = stats
        apply()
        want = TF.rand_augment_numpy(first, (params[0][:1], params[1][:1]), FILL)
        assert np.array_equal(y[:1].cpu().numpy(), want), name
        variants["apply_%s_u8" % name] = apply
        if name in ("identity", "rotate", "sharpness", "equalize"):
            stats32, apply32, y32 = launches(frames, params, L.PTX_RESIZE_OUT_F32)
            if stats32 is not None:
                stats32()
            apply32()
            assert torch.equal(y32, TF.FramesToTensor(OPTS)(y)), name
            variants["apply_%s_f32" % name] = apply32
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

    # end to end: raw 8 x 16 frames of 256 x 340 -> RandomResizedCrop -> (RandAugment) -> fp32 clip
    raw = torch.randint(0, 256, (N, T, 256, 340, 3), dtype=torch.uint8, device=DEV, generator=g)
    kw = dict(random_resized_crop=True, random_hflip=True)
    ra = TF.RandAugment(2, 9, generator=torch.Generator().manual_seed(5))
    tf_plain = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(6), **kw)
    tf_aug = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(6), augment=ra, **kw)
    e2e = alternate({"transform_frames": lambda: tf_plain(raw), "transform_frames_augment": lambda: tf_aug(raw)},
                    max(iters // 4, 2), rounds)
    ratios = {"e2e_augment_over_plain": round(e2e["transform_frames_augment"]["ms"] / e2e["transform_frames"]["ms"], 3)}
    draw = ra.draw(N, S, S)
    per_frame = pil_loop(frames[0].cpu().numpy(), (draw[0].numpy(), draw[1].numpy()), 4 if args.quick else args.pil_frames)
    pil = None
    if per_frame is not None:
        pil = dict(ms_per_frame=round(per_frame * 1e3, 4), ms_per_batch=round(per_frame * 1e3 * N * T, 2), frames_timed=4 if args.quick else args.pil_frames,
                   what="Pillow on one host core, the same 2-op draws, 224 x 224 frames already in host memory (no copies counted)")
        ratios["pil_batch_over_e2e_augment"] = round(pil["ms_per_batch"] / e2e["transform_frames_augment"]["ms"], 1)
    out = dict(device=torch.cuda.get_device_name(0), binary=L.lib().ptx_version().decode(), shape=[N, T, S, S], iters=iters,
               rounds=rounds, clock="HIP events around back-to-back launches / calls", kernels=kernels, end_to_end=e2e,
               end_to_end_source=[N, T, 256, 340], pil_loop=pil, ratios=ratios)
    print(json.dumps(dict(ratios=ratios, pil=pil, ms={k: v["ms"] for k, v in list(kernels.items()) + list(e2e.items())})), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
