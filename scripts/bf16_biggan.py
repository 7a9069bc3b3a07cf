"""BigGAN-deep generator throughput in fp32, fp16 and bf16 on the same weights, in ONE process (BASELINE config 5 by default:
resolution 256, ch 128, batch 64).

    python scripts/bf16_biggan.py [--res 256] [--ch 128] [--batch 64] [--iters 10] [--check 4] [--out profiles/bf16_biggan.json]
                                  [--only bf16] [--ab]

The three generators hold the same synth_state_dict weights rounded to bf16 and get the same bf16-exact z / class
embeddings.  fp32: the default plan; fp16: precision="fp16"; bf16: the generator cast with .to(torch.bfloat16).  Each is
warmed up and timed over `iters` calls between two synchronisations.  max|d image| of each against the fp32 CPU stand-in
(oracle/biggan_standin.py) is taken over the first `check` samples (samples are independent; the CPU stand-in is slow).
--ab adds bf16 runs with PTX_CONV3X3_BF16=0 / PTX_CONV1X1_BF16=0 (the patch kernels against the generic bf16 tiles).
Prints one JSON line.  Profiled runs: `--only bf16 --check 0 --save-tuned T` first, then the traced run under
PTX_TUNED_TABLE=T, so the trace holds the forwards and no candidate tiles."""
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
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--ch", type=int, default=128)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=4, help="samples compared against the CPU stand-in (0: none)")
    ap.add_argument("--only", choices=("fp32", "fp16", "bf16"), default=None, help="time one arm only (profiler runs)")
    ap.add_argument("--ab", action="store_true", help="also time bf16 with each patch kernel switched off")
    ap.add_argument("--out", default=None)
    ap.add_argument("--save-tuned", default=None, help="write the tuned tile table after the run (a profiled run then reads it "
                    "through PTX_TUNED_TABLE and times no candidate tiles)")
    a = ap.parse_args()
    import pretorched_x_amd as ptx
    from pretorched_x_amd.testing import BIGGAN_RECIPE, synth_state_dict
    from oracle import biggan_standin as BG
    dev = torch.device("cuda:0")
    G0 = ptx.biggan_deep(a.res, ch=a.ch)
    sd = synth_state_dict(G0.state_dict(), 1234, **BIGGAN_RECIPE)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    g = torch.Generator().manual_seed(3)
    z = torch.randn(a.batch, G0.dim_z, generator=g).to(torch.bfloat16).float()
    lab = torch.randint(0, G0.n_classes, (a.batch,), generator=g)
    y = sd["shared.weight"][lab]
    ref = BG.forward(sd, z[:a.check], y[:a.check]) if a.check else None
    arms = [a.only] if a.only else ["fp32", "fp16", "bf16"]
    if a.ab and not a.only:
        arms += ["bf16:PTX_CONV3X3_BF16=0", "bf16:PTX_CONV1X1_BF16=0", "bf16:PTX_CONV3X3_BF16=0,PTX_CONV1X1_BF16=0"]
    rows = {}
    for arm in arms:
        prec, _, env = arm.partition(":")
        saved = {}
        for kv in filter(None, env.split(",")):
            k, v = kv.split("=")
            saved[k] = os.environ.get(k)
            os.environ[k] = v
        G = ptx.biggan_deep(a.res, ch=a.ch, precision="fp16" if prec == "fp16" else "fp32")
        G.load_state_dict(sd)
        G = G.eval().to(dev)
        dt = torch.float32
        if prec == "bf16":
            G, dt = G.to(torch.bfloat16), torch.bfloat16
        zd, yd = z.to(dev, dt), y.to(dev, dt)
        with torch.no_grad():
            for _ in range(a.warmup):
                img = G(zd, yd)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.iters):
                img = G(zd, yd)
            torch.cuda.synchronize()
            sec = (time.perf_counter() - t0) / a.iters
        row = dict(img_per_s=round(a.batch / sec, 1), ms=round(sec * 1e3, 3))
        if ref is not None:
            row["max_abs_d_image_vs_fp32_standin"] = float((img[:a.check].float().cpu() - ref).abs().max())
        rows[arm] = row
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        del G
        torch.cuda.empty_cache()
    out = dict(model="biggan_deep", res=a.res, ch=a.ch, batch=a.batch, iters=a.iters, checked_samples=a.check, arms=rows)
    if "bf16" in rows and "fp16" in rows:
        out["bf16_over_fp16"] = round(rows["bf16"]["img_per_s"] / rows["fp16"]["img_per_s"], 3)
    if "bf16" in rows and "fp32" in rows:
        out["bf16_over_fp32"] = round(rows["bf16"]["img_per_s"] / rows["fp32"]["img_per_s"], 3)
    line = json.dumps(out)
    print(line)
    if a.save_tuned:
        from pretorched_x_amd.engine import save_tuned_table
        save_tuned_table(a.save_tuned)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
