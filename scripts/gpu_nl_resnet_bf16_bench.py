"""bf16 non-local ResNets on the direct bf16 stem against their fp32 twins, in one process.

    python scripts/gpu_nl_resnet_bf16_bench.py [--iters 5] [--rounds 5] [--only NAME] [--out logs/nl_resnet_bf16.json]

nonlocal_r2plus1d50 and nonlocalresnet3d50 at 8x3x32x112x112 (BASELINE config 3's shape) and nonlocalresnet3d50 at
8x3x16x224x224, synthetic weights rounded to bf16 (the fp32 twin holds the same values).  Whole forwards are timed with
device events after a warm-up of every variant, the variants alternating `rounds` times; the median round and the range are
reported.  Variants: the fp32 plan, the bf16 plan with the attention's single-group form (PTX_NL_BF16_KSPLIT=0), the bf16 plan
with the key split forced on where it is supported (=1), forward_frames from uint8 frames, and FramesToTensor + .to(bf16) +
forward.  Per-launch attention times come from Engine.profile_steps under either form.  Also max |bf16 logits - fp32 logits|
and argmax agreement.  The output is rewritten after every model, so a run cut short keeps what it measured.
The committed copy of the output is profiles/nl_resnet_bf16.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pretorched_x_amd as ptx  # noqa: E402
from pretorched_x_amd import _lib as L  # noqa: E402
from pretorched_x_amd.engine import _ptr  # noqa: E402
from pretorched_x_amd.testing import synth_state_dict  # noqa: E402

DEV = "cuda:0"
OPTS = dict(input_space="BGR", input_range=[0, 255], mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
CASES = [
    ("nonlocal_r2plus1d50@8x3x32x112x112", lambda: ptx.nonlocal_r2plus1d50(339), dict(inner_bn_damp=0.9, nl_bn_damp=0.05), (8, 3, 32, 112, 112)),
    ("nonlocalresnet3d50@8x3x32x112x112", lambda: ptx.nonlocalresnet3d50(pretrained=None), dict(last_bn_damp=0.65, nl_bn_damp=0.05), (8, 3, 32, 112, 112)),
    ("nonlocalresnet3d50@8x3x16x224x224", lambda: ptx.nonlocalresnet3d50(pretrained=None), dict(last_bn_damp=0.65, nl_bn_damp=0.05), (8, 3, 16, 224, 224)),
]


def timed(fn, iters, warmup=0):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(runs, iters, rounds, warmup=2):
    """{name: fn} -> {name: {median ms, min, max, rounds}}: every fn warmed up, then `rounds` passes over all of them, in
    reverse order on every second pass."""
    for fn in runs.values():
        timed(fn, warmup)
    ms = {k: [] for k in runs}
    for r in range(rounds):
        for k in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
            ms[k].append(timed(runs[k], iters))
    return {k: {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "rounds_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def with_ksplit(value, fn):
    """fn under PTX_NL_BF16_KSPLIT=value (the attention dispatcher reads it at every launch)."""
    def run():
        os.environ["PTX_NL_BF16_KSPLIT"] = value
        try:
            return fn()
        finally:
            del os.environ["PTX_NL_BF16_KSPLIT"]
    return run


def attention_launches(m16, clip16, iters):
    """[{Nq, Nk, d, dv, default variant, us under the single-group form, us under the key split (or None)}] per launch."""
    eng = m16.engine()
    plan = eng.plan_for(m16, clip16)
    plan.in_ptr = _ptr(clip16)
    idx = [i for i, s in enumerate(plan.steps) if getattr(s, "label", None) == "nonlocal_attention"]
    lib = L.lib()
    rows = {v: with_ksplit(v, lambda: eng.profile_steps(plan, iters))() for v in ("0", "1")}
    out = []
    for k, (i, d) in enumerate(zip(idx, plan.attn_descs)):
        sup = bool(lib.ptx_nonlocal_bf16_variant_supported(C.byref(d), 1))
        out.append({"Nq": d.Nq, "Nk": d.Nk, "d": d.d, "dv": d.dv, "plan_variant": plan.attn_variants[k],
                    "single_group_us": round(rows["0"][i][4] * 1e3, 1),
                    "key_split_us": round(rows["1"][i][4] * 1e3, 1) if sup else None})
    return out


def one(name, factory, recipe, shape, iters, rounds):
    n, _, t, h, w = shape
    sd = synth_state_dict(factory().state_dict(), 1234, **recipe)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    m32, m16 = factory(), factory()
    for m in (m32, m16):
        m.load_state_dict(sd)
    m32 = m32.eval().to(DEV)
    m16 = m16.eval().to(torch.bfloat16).to(DEV)
    m16.engine().bf16_stem = "direct"
    for m in (m32, m16):
        m.engine().lanes = 1
    frames = torch.randint(0, 256, (n, t, h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(5)).to(DEV)
    opts = dict(OPTS, input_size=[3, h, w])
    to_tensor = ptx.transforms.FramesToTensor(opts)
    res = {"model": name, "shape": list(shape)}
    with torch.no_grad():
        clip32 = to_tensor(frames)
        clip16 = clip32.to(torch.bfloat16)
        ref = m32(clip16.float()).float()
        out0 = with_ksplit("0", lambda: m16(clip16))().float()
        out1 = with_ksplit("1", lambda: m16(clip16))().float()
        res["logits"] = {"max_abs_fp32_logit": float(ref.abs().max()),
                         "max_abs_delta_bf16_vs_fp32": {"single_group": float((out0 - ref).abs().max()), "key_split": float((out1 - ref).abs().max())},
                         "argmax_equal": {"single_group": bool(torch.equal(out0.argmax(1), ref.argmax(1))),
                                          "key_split": bool(torch.equal(out1.argmax(1), ref.argmax(1)))},
                         "frames_equal_clip_bits": bool(torch.equal(m16.forward_frames(frames, opts), m16(clip16)))}
        fwd = alternate({"fp32_forward": lambda: m32(clip32),
                         "bf16_forward_single_group": with_ksplit("0", lambda: m16(clip16)),
                         "bf16_forward_key_split": with_ksplit("1", lambda: m16(clip16)),
                         "bf16_forward_frames": lambda: m16.forward_frames(frames, opts),
                         "bf16_to_tensor_then_forward": lambda: m16(to_tensor(frames).to(torch.bfloat16))}, iters, rounds)
        for v in fwd.values():
            v["clips_per_s"] = round(n / v["ms"] * 1e3, 1)
        res["forward"] = fwd
        res["speedup_bf16_over_fp32"] = {k: round(fwd["fp32_forward"]["ms"] / fwd["bf16_forward_" + k]["ms"], 3) for k in ("single_group", "key_split")}
        res["attention_launches"] = attention_launches(m16, clip16, iters)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="run the cases whose name contains this")
    ap.add_argument("--out", default=os.path.join(ROOT, "logs", "nl_resnet_bf16.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("at least 5 rounds")
    out = {"device": torch.cuda.get_device_name(0), "library": L.lib().ptx_version().decode(), "iters": a.iters, "rounds": a.rounds,
           "models": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name, factory, recipe, shape in CASES:
        if a.only and a.only not in name:
            continue
        out["models"].append(one(name, factory, recipe, shape, a.iters, a.rounds))
        print(json.dumps(out["models"][-1]), flush=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
