"""BatchMix on the GPU: the fused erase + mix launch from uint8 frames against the route it replaces, and `TransformFrames` of the
jitter recipe with and without `mix=`.

    python scripts/gpu_batch_mix_bench.py [--out profiles/batch_mix.json] [--quick]

Shape: 8 clips x 16 frames of 224 x 224.  Everything is timed with HIP events on one stream around `--iters` back-to-back
launches / calls, every variant warmed, the variants alternating inside every round; a variant's time is the median of its
`--rounds` (5) rounds and its spread (max - min) / median of them.

 (a) `fused_*`: ptx_batch_mix_apply through ctypes (buffers allocated once) for a MixUp draw, a CutMix draw and an erase-only
     draw (every clip erased), to fp32 and to bf16.
 (b) `replaced_*`: the route a user of the parent commit takes, built from what exists there plus torch: `FramesToTensor(opts)
     (frames)`, then the Python loop of slice assignments for the erase boxes, then torch's roll / mul / add (MixUp) or the
     roll and one slice assignment per clip (CutMix).  Its host work is part of it, as it is in a training loop.
     `replaced_*_public` times (a)'s draw through the public call `bm(frames, opts=.., params=..)` the same way, host work
     included, for a like-for-like comparison.
 (c) `TransformFrames(opts, random_short_side=(256, 320), random_crop=True, random_hflip=True)` on 8 x 16 frames of 256 x 340 with
     and without `mix=bm`, and without it followed by the same host draw and the hand-written torch erase and mix of its fp32
     clip (`transform_frames_then_torch_mix`); `draw_alone` is the host draw, which both routes with a mix pay.
 (d) bytes: the fused launch must read one byte per sample of the clip, one of the partner where it is used, and write the
     output element; GBps is that count over the time.

Every fused output is compared with the replaced route's (and with `batch_mix_torch` on the first two clips) before anything is
timed.
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
VALUE = (0.0, 0.0, 0.0)


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


def draws():
    """The three draws of (a): per clip an erase box as RandomErasing draws it (MixUp / CutMix: a quarter of the clips; erase-only:
    every clip), one lam per batch."""
    out = {}
    for name, kw in (("mixup", dict(mixup_alpha=0.8, cutmix_alpha=0.0, erase_prob=0.25)), ("cutmix", dict(mixup_alpha=0.0, cutmix_alpha=1.0, erase_prob=0.25)),
                     ("erase", dict(mixup_alpha=0.0, cutmix_alpha=0.0, erase_prob=1.0))):
        seed = 0
        while True:                                                  # a draw that holds what its name says
            rows, lam = TF.BatchMix(generator=torch.Generator().manual_seed(seed), **kw).draw(N, S, S)
            erased = int(rows[:, 6].sum())
            if (name == "erase" and erased == N) or (name != "erase" and erased == N // 4 and 0.2 < float(lam[0]) < 0.8):
                break
            seed += 1
        out[name] = (rows, lam)
    return out


def fused(frames, params, dtype):
    """(launch fn, output, compulsory bytes) of ptx_batch_mix_apply on device frames through ctypes, buffers allocated once."""
    lib = L.lib()
    mode = L.PTX_RESIZE_OUT_F32 if dtype == torch.float32 else L.PTX_RESIZE_OUT_BF16
    rows, noise = TF.batch_mix_rows(params, T, VALUE, N)
    desc = L.MixDesc(N, T, S, S, L.PTX_MIX_SRC_U8, mode, noise)
    assert lib.ptx_batch_mix_supported(C.byref(desc), C.c_void_p(np.ascontiguousarray(rows).ctypes.data)) == 1
    d_rows = torch.from_numpy(rows.reshape(-1)).to(DEV)
    norm = L.NormDesc.make(OPTS["mean"], OPTS["std"], OPTS["input_space"], OPTS["input_range"])
    y = torch.empty((N, 3, T, S, S), dtype=dtype, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = (d_rows, desc, norm)

    def launch(_keep=keep):
        L.check(lib.ptx_batch_mix_apply(C.byref(desc), C.c_void_p(frames.data_ptr()), C.c_void_p(d_rows.data_ptr()), None,
                                        C.c_void_p(y.data_ptr()), C.byref(norm), stream), "ptx_batch_mix_apply")

    # per clip and channel sample: the output element; the clip's byte unless a CutMix box covers it; the partner's byte for MixUp
    # or inside the box
    px, esz = T * S * S * 3, (4 if dtype == torch.float32 else 2)
    nbytes = 0
    for r in params[0].tolist():
        box = (r[4] - r[2]) * (r[5] - r[3]) / float(S * S) if r[1] == L.PTX_MIX_CUTMIX else 0.0
        nbytes += px * esz + px * (1.0 - box) + px * (1.0 if r[1] == L.PTX_MIX_MIXUP else box)
    return launch, y, int(nbytes)


def torch_mix(x, params, fill):
    """The hand-written erase and mix of a normalised clip x (changed in place where torch allows it)."""
    rows, lam = params[0].tolist(), [float(v) for v in params[1]]
    for i, r in enumerate(rows):
        if r[6]:
            x[i, :, :, r[7]:r[7] + r[9], r[8]:r[8] + r[10]] = fill.to(x.dtype)
    if rows[0][1] == L.PTX_MIX_MIXUP:
        return x.roll(1, 0).mul(1.0 - lam[0]).add_(x.mul(lam[0]))
    if rows[0][1] == L.PTX_MIX_CUTMIX:
        rolled = x.roll(1, 0)
        for i, r in enumerate(rows):
            x[i, :, :, r[2]:r[4], r[3]:r[5]] = rolled[i, :, :, r[2]:r[4], r[3]:r[5]]
    return x


def replaced(frames, params, dtype):
    """The route on the parent commit: FramesToTensor, the Python erase loop, torch's roll / mul / add (or the CutMix slices)."""
    to_tensor = TF.FramesToTensor(OPTS)
    fill = torch.tensor(VALUE, device=DEV).view(3, 1, 1, 1)

    def run():
        x = to_tensor(frames)
        return torch_mix(x if dtype == torch.float32 else x.to(dtype), params, fill)

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_batch_mix_bench: no GPU (there is no CPU path to time)")
    iters, rounds = (3, 2) if args.quick else (args.iters, args.rounds)
    g = torch.Generator(device=DEV).manual_seed(1)
    frames = torch.randint(0, 256, (N, T, S, S, 3), dtype=torch.uint8, device=DEV, generator=g)
    variants, nbytes = {}, {}
    bm = TF.BatchMix(erase_value=VALUE)
    for name, params in draws().items():
        for dname, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            tag = "%s_%s" % (name, dname)
            launch, y, nbytes["fused_" + tag] = fused(frames, params, dtype)
            route = replaced(frames, params, dtype)
            launch()
            want = route()
            assert torch.equal(y, want), tag                         # the replaced route is the same arithmetic: the same bits
            ref = TF.FramesToTensor(OPTS)(frames).cpu().to(dtype)
            assert torch.equal(y[:2].cpu(), TF.batch_mix_torch(ref, params, VALUE)[:2]), tag
            variants["fused_" + tag] = launch
            variants["replaced_" + tag] = route
            variants["fused_%s_public" % tag] = lambda p=params, d=dtype: bm(frames, params=p, opts=OPTS, dtype=d)
            del want
    kernels = alternate(variants, iters, rounds)
    for k, b in nbytes.items():
        kernels[k]["bytes"] = b
        kernels[k]["GBps"] = round(b / kernels[k]["ms"] / 1e6, 1)
    ratios = {}
    for k in nbytes:
        r = "replaced_" + k[len("fused_"):]
        ratios[r + "_over_fused"] = round(kernels[r]["ms"] / kernels[k]["ms"], 2)
        ratios[r + "_over_fused_public"] = round(kernels[r]["ms"] / kernels[k + "_public"]["ms"], 2)

    # (c) end to end: raw 8 x 16 frames of 256 x 340 -> scale jitter, random crop, flip -> (erase + mix) -> fp32 clip
    raw = torch.randint(0, 256, (N, T, 256, 340, 3), dtype=torch.uint8, device=DEV, generator=g)
    kw = dict(random_short_side=(256, 320), random_crop=True, random_hflip=True)
    tf_plain = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(6), **kw)
    tf_mix = TF.TransformFrames(OPTS, generator=torch.Generator().manual_seed(6), mix=TF.BatchMix(generator=torch.Generator().manual_seed(7)), **kw)
    bm_host = TF.BatchMix(generator=torch.Generator().manual_seed(7))
    fill = torch.tensor(VALUE, device=DEV).view(3, 1, 1, 1)
    e2e = alternate({"transform_frames": lambda: tf_plain(raw), "transform_frames_mix": lambda: tf_mix(raw),
                     "transform_frames_then_torch_mix": lambda: torch_mix(tf_plain(raw), bm_host.draw(N, S, S), fill),
                     "draw_alone": lambda: bm_host.draw(N, S, S)}, max(iters // 2, 2), rounds)
    ratios["e2e_mix_over_plain"] = round(e2e["transform_frames_mix"]["ms"] / e2e["transform_frames"]["ms"], 3)
    ratios["e2e_torch_mix_over_mix"] = round(e2e["transform_frames_then_torch_mix"]["ms"] / e2e["transform_frames_mix"]["ms"], 3)
    out = dict(device=torch.cuda.get_device_name(0), binary=L.lib().ptx_version().decode(), shape=[N, T, S, S], iters=iters,
               rounds=rounds, clock="HIP events on one stream around back-to-back launches / calls; median of the rounds",
               kernels=kernels, end_to_end=e2e, end_to_end_source=[N, T, 256, 340], ratios=ratios)
    print(json.dumps(dict(ratios=ratios, ms={k: [v["ms"], v["spread"]] for k, v in list(kernels.items()) + list(e2e.items())},
                          GBps={k: kernels[k]["GBps"] for k in nbytes})), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
