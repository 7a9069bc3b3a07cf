"""bf16 vs fp32 forward throughput of one model in ONE process (BASELINE config 2 by default: resnet3d50, 8 x 3 x 16 x 224 x 224).

    python scripts/bf16_throughput.py [--model resnet3d50] [--shape 8 3 16 224 224] [--iters 20] [--out profiles/bf16_cfg2.json]

Both runs use synth_state_dict weights rounded to bf16 (so both models hold the same values) and the same bf16-exact clips.
fp32: the single-plan forward (Engine.lanes = 1); bf16: the same model cast to torch.bfloat16 (lanes = 1).  Each is warmed up
(plan compiled, untuned conv problems timed) and then timed over `iters` forwards between two synchronisations.  Prints one
JSON line: clips/s of both, the ratio, and max|bf16 - fp32| of the logits with max|fp32| for scale."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet3d50")
    ap.add_argument("--shape", type=int, nargs=5, default=[8, 3, 16, 224, 224])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("fp32", "bf16"), default=None, help="time one arm only (profiler runs)")
    ap.add_argument("--save-tuned", default=None, help="write the tuned tile table after the run (a profiled run then reads it "
                    "through PTX_TUNED_TABLE and times no candidate tiles)")
    a = ap.parse_args()
    import pretorched_x_amd as ptx
    from pretorched_x_amd.testing import synth_clips, synth_state_dict
    dev = torch.device("cuda:0")
    m = ptx.__dict__[a.model](num_classes=339, pretrained=None)
    sd = synth_state_dict(m.state_dict(), 1234)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    m.load_state_dict(sd)
    m32 = m.eval().to(dev)
    N, _, T, H, W = a.shape
    x = synth_clips(N, T, H, 99).to(torch.bfloat16).to(dev)
    rows = {}
    outs = {}
    for prec in ((a.only,) if a.only else ("fp32", "bf16")):
        model = m32 if prec == "fp32" else ptx.__dict__[a.model](num_classes=339, pretrained=None)
        if prec == "bf16":
            model.load_state_dict(sd)
            model = model.eval().to(torch.bfloat16).to(dev)
        model.engine().lanes = 1
        xin = x.float() if prec == "fp32" else x
        with torch.no_grad():
            for _ in range(a.warmup):
                out = model(xin)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                out = model(xin)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / a.iters
        outs[prec] = out.float()
        rows[prec] = dict(ms=1e3 * dt, clips_per_s=N / dt)
        if prec == "fp32":
            del model
    if a.save_tuned:
        from pretorched_x_amd.engine import save_tuned_table
        save_tuned_table(a.save_tuned)
    if a.only:
        print(json.dumps(dict(model=a.model, shape=a.shape, precision=a.only, **rows[a.only])))
        return
    res = dict(model=a.model, shape=a.shape, iters=a.iters, lanes=1,
               fp32_clips_per_s=round(rows["fp32"]["clips_per_s"], 1), fp32_ms=round(rows["fp32"]["ms"], 3),
               bf16_clips_per_s=round(rows["bf16"]["clips_per_s"], 1), bf16_ms=round(rows["bf16"]["ms"], 3),
               speedup=round(rows["bf16"]["clips_per_s"] / rows["fp32"]["clips_per_s"], 3),
               max_abs_diff_vs_fp32=float((outs["bf16"] - outs["fp32"]).abs().max()),
               max_abs_fp32=float(outs["fp32"].abs().max()),
               argmax_agree=int((outs["bf16"].argmax(1) == outs["fp32"].argmax(1)).sum()),
               device=torch.cuda.get_device_name(dev), version=ptx._lib.lib().ptx_version().decode())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
