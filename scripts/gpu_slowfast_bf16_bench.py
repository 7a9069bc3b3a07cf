"""bf16 SlowFast on the frame-strided direct bf16 stem against the fp32 default plan, in one process.

    python scripts/gpu_slowfast_bf16_bench.py [--iters 10] [--rounds 5] [--parent-lib libptx_amd.so of the parent commit]
                                              [--out logs/slowfast_bf16.json]

SlowFast-50 (mode SF) at 8x3x64x224x224, synthetic weights rounded to bf16 (the fp32 twin holds the same values).  Whole
forwards are timed with device events after a warm-up of every shape, the variants alternating `rounds` times; the median
round and the range are reported.  Stem times come from Engine.profile_steps (event chain inside ordinary passes).
Also: forward_frames from uint8 frames against FramesToTensor + .to(bf16) + forward, max |bf16 logits - fp32 logits|, and
the plain entry point ptx_conv_stem_bf16_fwd at resnet3d50's config-2 stem -- on this build and, with --parent-lib, on the
parent commit's library loaded next to it, alternating, with the parent's own run-to-run spread as the margin.
The committed copy of the output is profiles/slowfast_bf16.json."""
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
from pretorched_x_amd.engine import StemBf16Step, _ptr  # noqa: E402
from pretorched_x_amd.testing import synth_state_dict  # noqa: E402

DEV = "cuda:0"
OPTS = dict(input_space="BGR", input_range=[0, 255], mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375])
SHAPE = (8, 3, 64, 224, 224)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


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


def alternate(runs, iters, rounds, warmup=3):
    """{name: fn} -> {name: {median ms, min, max, rounds}}: every fn warmed up, then `rounds` passes over all of them, in
    reverse order on every second pass (no variant always runs behind the same other one)."""
    for fn in runs.values():
        timed(fn, warmup)
    ms = {k: [] for k in runs}
    for r in range(rounds):
        for k in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
            ms[k].append(timed(runs[k], iters))
    return {k: {"ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "rounds_ms": [round(x, 4) for x in v]} for k, v in ms.items()}


def models():
    sd = synth_state_dict(ptx.slowfast.resnet50(mode="SF", num_classes=400).state_dict(), 1234)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    m32 = ptx.slowfast.resnet50(mode="SF", num_classes=400)
    m32.load_state_dict(sd)
    m32 = m32.eval().to(DEV)
    m16 = ptx.slowfast.resnet50(mode="SF", num_classes=400)
    m16.load_state_dict(sd)
    m16 = m16.eval().to(torch.bfloat16).to(DEV)
    m16.engine().bf16_stem = "direct"
    for m in (m32, m16):
        m.engine().lanes = 1
    return m32, m16


def slowfast(iters, rounds):
    n, _, t, h, w = SHAPE
    m32, m16 = models()
    g = torch.Generator().manual_seed(5)
    frames = torch.randint(0, 256, (n, t, h, w, 3), dtype=torch.uint8, generator=g).to(DEV)
    opts = dict(OPTS, input_size=[3, h, w])
    to_tensor = ptx.transforms.FramesToTensor(opts)
    res = {"model": "slowfast.resnet50 SF", "shape": list(SHAPE)}
    with torch.no_grad():
        clip32 = to_tensor(frames)
        clip16 = clip32.to(torch.bfloat16)
        ref = m32(clip16.float()).float()
        out = m16(clip16).float()
        res["logits"] = {"max_abs_delta_bf16_vs_fp32": float((out - ref).abs().max()), "max_abs_fp32_logit": float(ref.abs().max()),
                         "argmax_equal": bool(torch.equal(out.argmax(1), ref.argmax(1))),
                         "frames_equal_clip_bits": bool(torch.equal(m16.forward_frames(frames, opts), m16(clip16)))}
        fwd = alternate({"fp32_forward": lambda: m32(clip32), "bf16_forward": lambda: m16(clip16),
                         "bf16_forward_frames": lambda: m16.forward_frames(frames, opts),
                         "bf16_to_tensor_then_forward": lambda: m16(to_tensor(frames).to(torch.bfloat16))}, iters, rounds)
        for v in fwd.values():
            v["clips_per_s"] = round(n / v["ms"] * 1e3, 1)
        res["forward"] = fwd
        res["speedup_bf16_over_fp32"] = round(fwd["fp32_forward"]["ms"] / fwd["bf16_forward"]["ms"], 3)
        # the two stem launches inside the bf16 step
        plan = m16.engine().plan_for(m16, clip16)
        plan.in_ptr = _ptr(clip16)
        rows = m16.engine().profile_steps(plan, iters)
        stems = {}
        for i, r in enumerate(rows):
            if isinstance(plan.steps[i], StemBf16Step):
                s = plan.steps[i]
                ms = r[4]
                stems[s.label] = {"ms": round(ms, 4), "frame_step": s.frame_step, "frames_read": s.d.Ti, "Co": s.d.Co,
                                  "issued_tflops": round(s.issued_flop() / ms / 1e9, 1),
                                  "algorithmic_tflops": round(2.0 * s.macs / ms / 1e9, 1),
                                  "algorithmic_GBps": round(s.hbm_bytes / ms / 1e6, 1)}
        step_ms = sum(r[4] for r in rows)
        for v in stems.values():
            v["share_of_step"] = round(v["ms"] / step_ms, 4)
        res["stems"] = stems
        res["profiled_step_ms"] = round(step_ms, 4)
    return res


def plain_entry(iters, rounds, parent_path):
    """ptx_conv_stem_bf16_fwd at resnet3d50's config-2 stem (8x3x16x224x224 -> 64 channels, bf16 clip), called directly."""
    lib = L.lib()
    n, T, H, W, Co = 8, 16, 224, 224, 64
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci = n, T, H, W, 3
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = 7, 7, 7, 1, 2, 2, 3, 3, 3
    d.To, d.Ho, d.Wo, d.Co, d.ldy, d.Co_pad = T, H // 2, W // 2, Co, Co, 128
    d.flags = L.PTX_EPI_RELU
    torch.manual_seed(1)
    K = 7 * 7 * 3
    w = (torch.randn(Co, K, 7, 1, 1) * 0.03).to(DEV)
    dpk = L.PackDesc(Co, K, 7, 1, 1, (K + 31) // 32 * 32, 128, 0, 0, 0, 0, 0, 0, L.PTX_PACK_BF16)
    wp = torch.empty(lib.ptx_packed_weight_elems(C.byref(dpk)), device=DEV, dtype=torch.bfloat16)
    bp = torch.zeros(128, device=DEV)
    null = C.c_void_p(0)
    L.check(lib.ptx_pack_conv_weight(C.byref(dpk), _ptr(w), null, null, null, null, null, C.c_float(0), _ptr(wp), _ptr(bp), stream()), "pack")
    ws = torch.empty(lib.ptx_stem_bf16_weight_elems(C.byref(d)), device=DEV, dtype=torch.bfloat16)
    L.check(lib.ptx_pack_stem_bf16_weight(C.byref(d), _ptr(wp), _ptr(ws), stream()), "relay")
    x = torch.randn(n, 3, T, H, W, device=DEV).to(torch.bfloat16)
    y = torch.empty(n, T, H // 2, W // 2, Co, device=DEV, dtype=torch.bfloat16)

    def call(fn):
        def run():
            if fn(C.byref(d), _ptr(x), L.PTX_STEM_SRC_BF16_NCDHW, None, _ptr(ws), _ptr(bp), _ptr(y), stream()) != 0:
                raise RuntimeError("ptx_conv_stem_bf16_fwd failed")
        return run
    runs = {"branch": call(lib.ptx_conv_stem_bf16_fwd)}
    out = {"problem": "resnet3d50 config 2 stem, bf16 clip", "recorded_ms": 0.37}
    if parent_path:
        parent = C.CDLL(parent_path)
        res, args = L.SIGNATURES["ptx_conv_stem_bf16_fwd"]
        parent.ptx_conv_stem_bf16_fwd.restype, parent.ptx_conv_stem_bf16_fwd.argtypes = res, args
        parent.ptx_version.restype = C.c_char_p
        out["parent_library"] = parent.ptx_version().decode()
        runs = {"parent": call(parent.ptx_conv_stem_bf16_fwd), "branch": runs["branch"]}
        runs["parent"]()
        torch.cuda.synchronize()
        y_parent = y.clone()
        runs["branch"]()
        torch.cuda.synchronize()
        out["bits_equal"] = bool(torch.equal(y, y_parent))
    out.update(alternate(runs, iters, rounds, warmup=30))
    if parent_path:
        spread = out["parent"]["max_ms"] - out["parent"]["min_ms"]
        out["parent_spread_ms"] = round(spread, 4)
        out["branch_not_slower"] = bool(out["branch"]["ms"] <= out["parent"]["ms"] + spread)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "logs", "slowfast_bf16.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("at least 5 rounds")
    out = {"device": torch.cuda.get_device_name(0), "library": L.lib().ptx_version().decode(), "iters": a.iters, "rounds": a.rounds,
           "plain_entry_point": plain_entry(100, max(a.rounds, 10), a.parent_lib),
           "slowfast": slowfast(a.iters, a.rounds)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
