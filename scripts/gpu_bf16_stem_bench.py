"""The two bf16 stems side by side, in one process: Engine.bf16_stem = "fold" (ptx_im2col_hw_bf16 + a (kT,1,1) conv on the
generic bf16 tiles) against "direct" (ptx_conv_stem_bf16_fwd, from the bf16 clip and from uint8 frames).

    python scripts/gpu_bf16_stem_bench.py [--iters 20] [--rounds 3] [--out logs/bf16_stem.json]

resnet3d50 at config 2 (8x3x16x224x224) and r2plus1d18 at 8x3x32x112x112, synthetic weights.  Stem times come from
Engine.profile_steps (event chain inside ordinary passes); whole forwards are timed with device events, warmed up, the two
settings alternating `rounds` times (two model objects with the same weights, so no plan is rebuilt between rounds); the
median round is reported.  Also the logit error of both stems against an fp32 twin for the two small test models.
The committed copy of the output is profiles/bf16_stem.json."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pretorched_x_amd as ptx  # noqa: E402
from pretorched_x_amd import _lib as L  # noqa: E402
from pretorched_x_amd.engine import StemBf16Step, _ptr  # noqa: E402
from pretorched_x_amd.testing import synth_state_dict  # noqa: E402

DEV = "cuda:0"
OPTS = dict(input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])


def zoo(name, classes=400):
    try:
        return ptx.__dict__[name](num_classes=classes, pretrained=None)
    except TypeError:
        return ptx.__dict__[name](num_classes=classes)


def weights(name):
    sd = synth_state_dict(zoo(name).state_dict(), 1234)
    return {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}


def bf16_model(name, sd, mode):
    m = zoo(name)
    m.load_state_dict(sd)
    m = m.eval().to(torch.bfloat16).to(DEV)
    m.engine().lanes = 1
    m.engine().bf16_stem = mode
    return m


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def stem_rows(model, plan, x, iters):
    """Per-launch ms of the stem's steps of one plan: the im2col pass and the stem conv, or the one direct launch."""
    plan.in_ptr = _ptr(x)
    rows = model.engine().profile_steps(plan, iters)
    out = {}
    for i, (label, kind, nb, macs, ms, kernel) in enumerate(r[:6] for r in rows):
        if label == "im2col_hw_bf16" or kind == "stem" or (plan.stem_bf16_step is not None and plan.steps[i] is plan.stem_bf16_step):
            out[label if label == "im2col_hw_bf16" else "stem_conv"] = round(ms, 4)
    out["total_ms"] = round(sum(out.values()), 4)
    return out


def measure(name, shape, iters, rounds):
    n, _, t, h, w = shape
    sd = weights(name)
    fold, direct = bf16_model(name, sd, "fold"), bf16_model(name, sd, "direct")
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (n, t, h, w, 3), dtype=torch.uint8, generator=g).to(DEV)
    opts = dict(OPTS, input_size=[3, h, w])
    tf16 = ptx.transforms.TransformFrames(opts, dtype=torch.bfloat16)
    res = {"model": name, "shape": list(shape)}
    with torch.no_grad():
        clip = ptx.transforms.FramesToTensor(opts)(frames).to(torch.bfloat16)
        for m in (fold, direct):
            m(clip)
        direct.forward_frames(frames, opts)
        fold(tf16(frames))
        torch.cuda.synchronize()
        norm = L.NormDesc.make(opts["mean"], opts["std"], opts["input_space"], opts["input_range"])
        p_fold, p_clip = fold.engine().plan_for(fold, clip), direct.engine().plan_for(direct, clip)
        p_u8 = direct.engine().plan_for(direct, frames, shape=shape, norm=norm)
        res["stem_ms"] = {"fold": stem_rows(fold, p_fold, clip, iters), "direct_clip": stem_rows(direct, p_clip, clip, iters),
                          "direct_uint8": stem_rows(direct, p_u8, frames, iters)}
        st = next(s for s in p_clip.steps if isinstance(s, StemBf16Step))
        st8 = next(s for s in p_u8.steps if isinstance(s, StemBf16Step))
        for key, s in (("direct_clip", st), ("direct_uint8", st8)):
            ms = res["stem_ms"][key]["stem_conv"]
            res["stem_ms"][key].update(issued_tflops=round(s.issued_flop() / ms / 1e9, 1),
                                       algorithmic_tflops=round(2.0 * s.macs / ms / 1e9, 1),
                                       algorithmic_MB=round(s.hbm_bytes / 1e6, 1),
                                       algorithmic_GBps=round(s.hbm_bytes / ms / 1e6, 1))
        runs = {"fold_forward": lambda: fold(clip), "direct_forward": lambda: direct(clip),
                "direct_forward_frames": lambda: direct.forward_frames(frames, opts),
                "fold_transform_then_forward": lambda: fold(tf16(frames))}
        ms = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                ms[k].append(timed(fn, iters))
        res["forward"] = {k: {"ms": round(statistics.median(v), 4), "clips_per_s": round(n / statistics.median(v) * 1e3, 1),
                              "rounds_ms": [round(x, 4) for x in v]} for k, v in ms.items()}
    return res


def accuracy(name):
    """max |logits - fp32 twin's logits| of both stems on 2 clips of 4 frames, 64x64 (the quantities of
    tests/test_gpu_bf16_stem.py::test_direct_accuracy_not_worse_than_fold)."""
    opts = dict(input_size=[3, 64, 64], input_space="RGB", input_range=[0, 1], mean=[0.45, 0.40, 0.35], std=[0.2, 0.25, 0.3])
    sd = weights(name)
    m16 = bf16_model(name, sd, "direct")
    m32 = zoo(name)
    m32.load_state_dict(sd)
    m32 = m32.eval().to(DEV)
    g = torch.Generator().manual_seed(71)
    frames = torch.randint(0, 256, (2, 4, 64, 64, 3), dtype=torch.uint8, generator=g).to(DEV)
    with torch.no_grad():
        ref = m32.forward_frames(frames, opts).float()
        d = m16.forward_frames(frames, opts).float()
        m16.engine().bf16_stem = "fold"
        f = m16(ptx.transforms.FramesToTensor(opts)(frames).to(torch.bfloat16)).float()
    return {"model": name, "e_fold": float((f - ref).abs().max()), "e_direct": float((d - ref).abs().max()),
            "max_abs_logit": float(ref.abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "logs", "bf16_stem.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "library": L.lib().ptx_version().decode(), "iters": a.iters, "rounds": a.rounds,
           "cases": [measure("resnet3d50", (8, 3, 16, 224, 224), a.iters, a.rounds),
                     measure("r2plus1d18", (8, 3, 32, 112, 112), a.iters, a.rounds)],
           "accuracy": [accuracy("resnet3d18"), accuracy("r2plus1d18")]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
