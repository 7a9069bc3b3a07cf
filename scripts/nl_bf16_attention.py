"""fp32 ptx_nonlocal_fwd vs bf16 ptx_nonlocal_bf16_fwd at the attention shapes of the video non-local nets, timed with HIP
events through ctypes, plus a bf16 NonLocalBlock3D(1024) forward.

    python scripts/nl_bf16_attention.py [--iters 50] [--out profiles/nl_bf16_attention.json] [--only bf16]

Shapes (8 clips each): config 3 (nonlocal_r2plus1d50 at 8x3x16x112x112: N = 1568, d = dv = 256; N = 196, d = dv = 512),
nonlocalresnet3d50 at 16x224^2 (N = 3136, d = dv = 256; N = 392, d = dv = 512) and the 'gaussian' mode at C = 1024
(d = 1024, dv = 512, N = 392).  Softmax mode, random operands with moderate logits.  Prints one JSON line per shape and
writes them all to --out.

    python scripts/nl_bf16_attention.py --ab [--rounds 7] [--out profiles/nl_bf16_ksplit.json]

A/B of the bf16 kernel's two forms through ptx_nonlocal_bf16_variant_fwd (include/ptx_amd_nl_ks.h): variant 0 (single group)
against variant 1 (key split) in one process, on the same inputs, HIP events around --iters launches, the two forms
alternating for --rounds rounds; per form the median and the spread (min, max) of the rounds.  Shapes: the five above, N = 784
at d = dv = 256 (nonlocalresnet3d50 at 8 x 224^2) and N = 128 / 144 at d = dv = 256 (the model tests' layer2 shapes)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("cfg3.layer2", 8, 1568, 256, 256), ("cfg3.layer3", 8, 196, 512, 512), ("nl3d50.layer2", 8, 3136, 256, 256),
          ("nl3d50.layer3", 8, 392, 512, 512), ("gaussian.c1024", 8, 392, 1024, 512)]


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters        # us per launch


AB_SHAPES = SHAPES + [("nl3d50_8f.layer2", 8, 784, 256, 256), ("test.n128", 8, 128, 256, 256), ("test.n144", 8, 144, 256, 256)]


def ab(a, lib, L, dev, st):
    """variant 0 against variant 1, alternating; us per launch: median, min, max over the rounds."""
    rows = []
    for name, B, N, d, dv in AB_SHAPES:
        gen = torch.Generator().manual_seed(N + d)
        amp = (2.0 / d ** 0.5) ** 0.5
        th = (torch.randn(B, N, d, generator=gen) * amp).to(torch.bfloat16).to(dev)
        ph = (torch.randn(B, N, d, generator=gen) * amp).to(torch.bfloat16).to(dev)
        g = torch.randn(B, N, dv, generator=gen).to(torch.bfloat16).to(dev)
        desc = L.NonlocalDesc()
        desc.batch, desc.Nq, desc.Nk, desc.d, desc.dv = B, N, N, d, dv
        desc.ld_theta = desc.ld_phi = d
        desc.ld_g = desc.ld_y = dv
        desc.bs_theta = desc.bs_phi = N * d
        desc.bs_g = desc.bs_y = N * dv
        desc.mode = L.PTX_NL_BF16 | L.PTX_NL_SOFTMAX
        row = {"shape": name, "batch": B, "N": N, "d": d, "dv": dv, "default_variant": int(lib.ptx_nonlocal_bf16_variant(C.byref(desc)))}
        variants = [v for v in (0, 1) if lib.ptx_nonlocal_bf16_variant_supported(C.byref(desc), v)]
        ys = {v: torch.empty(B, N, dv, device=dev, dtype=torch.bfloat16) for v in variants}

        def fn(v):
            rc = lib.ptx_nonlocal_bf16_variant_fwd(C.byref(desc), v, *[C.c_void_p(t.data_ptr()) for t in (th, ph, g, ys[v])], st)
            if rc:
                raise RuntimeError(lib.ptx_last_error().decode())
        times = {v: [] for v in variants}
        for _ in range(a.rounds):
            for v in variants:
                times[v].append(_time(lambda: fn(v), a.iters, a.warmup))
        for v in variants:
            t = sorted(times[v])
            row["v%d_us" % v] = {"median": round(t[len(t) // 2], 1), "min": round(t[0], 1), "max": round(t[-1], 1)}
        if 1 in variants:
            row["v1_over_v0_time"] = round(row["v1_us"]["median"] / row["v0_us"]["median"], 3)
            row["max_abs_diff"] = float((ys[1].float() - ys[0].float()).abs().max())
        else:
            row["v1_us"] = "unsupported (d > 256 stays single-group)"
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=("fp32", "bf16"), default=None, help="time one arm only (profiler runs)")
    ap.add_argument("--ab", action="store_true", help="variant 0 against variant 1 of the bf16 kernel (the key split)")
    ap.add_argument("--rounds", type=int, default=7, help="--ab: alternating rounds per form (median of these)")
    a = ap.parse_args()
    import pretorched_x_amd as ptx
    from pretorched_x_amd import _lib as L
    lib = L.lib()
    dev = torch.device("cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    if a.ab:
        rows = ab(a, lib, L, dev, st)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
                f.write("\n")
        return
    for name, B, N, d, dv in SHAPES:
        gen = torch.Generator().manual_seed(N + d)
        amp = (2.0 / d ** 0.5) ** 0.5
        th = (torch.randn(B, N, d, generator=gen) * amp).to(torch.bfloat16).to(dev)
        ph = (torch.randn(B, N, d, generator=gen) * amp).to(torch.bfloat16).to(dev)
        g = torch.randn(B, N, dv, generator=gen).to(torch.bfloat16).to(dev)
        row = {"shape": name, "batch": B, "N": N, "d": d, "dv": dv, "gflop": round(2.0 * B * N * N * (d + dv) / 1e9, 2)}
        outs = {}
        for prec in ((a.only,) if a.only else ("fp32", "bf16")):
            desc = L.NonlocalDesc()
            desc.batch, desc.Nq, desc.Nk, desc.d, desc.dv = B, N, N, d, dv
            desc.ld_theta = desc.ld_phi = d
            desc.ld_g = desc.ld_y = dv
            desc.bs_theta = desc.bs_phi = N * d
            desc.bs_g = desc.bs_y = N * dv
            if prec == "fp32":
                desc.mode = L.PTX_NL_SOFTMAX
                ops = [th.float(), ph.float(), g.float()]
                y = torch.empty(B, N, dv, device=dev, dtype=torch.float32)
                call = lib.ptx_nonlocal_fwd
            else:
                desc.mode = L.PTX_NL_BF16 | L.PTX_NL_SOFTMAX
                ops = [th, ph, g]
                y = torch.empty(B, N, dv, device=dev, dtype=torch.bfloat16)
                call = lib.ptx_nonlocal_bf16_fwd
            ptrs = [C.c_void_p(t.data_ptr()) for t in ops + [y]]

            def fn():
                rc = call(C.byref(desc), *ptrs, st)
                if rc:
                    raise RuntimeError(lib.ptx_last_error().decode())
            us = _time(fn, a.iters, a.warmup)
            row[prec + "_us"] = round(us, 1)
            row[prec + "_tflops"] = round(2.0 * B * N * N * (d + dv) / us / 1e6, 1)
            outs[prec] = y.float()
        if len(outs) == 2:
            row["bf16_over_fp32_time"] = round(row["bf16_us"] / row["fp32_us"], 3)
            row["max_abs_diff"] = float((outs["bf16"] - outs["fp32"]).abs().max())
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.only in (None, "bf16"):
        # a bf16 NonLocalBlock3D(1024) forward ('embedded_gaussian', sub_sample, BN): nonlocalresnet3d50's layer3 block at
        # 8 x 1024 x 4 x 14 x 14 (N = 784 queries, 196 keys)
        from pretorched_x_amd.testing import synth_state_dict
        m = ptx.NonLocalBlock3D(1024, sub_sample=True)
        sd = synth_state_dict(m.state_dict(), 1234)
        m.load_state_dict({k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()})
        m = m.eval().to(torch.bfloat16).to(dev)
        x = torch.randn(8, 1024, 4, 14, 14, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16).to(dev)
        with torch.no_grad():
            us = _time(lambda: m(x), a.iters, a.warmup)
        row = {"shape": "NonLocalBlock3D(1024) bf16 forward", "input": [8, 1024, 4, 14, 14], "us": round(us, 1)}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
