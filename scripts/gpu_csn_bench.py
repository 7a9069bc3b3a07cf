"""The depthwise 3-D convolution (include/ptx_amd_dw.h) and the channel-separated networks on the GPU.

    python scripts/gpu_csn_bench.py [--out profiles/csn.json] [--part kernels|models|all] [--quick]

Kernels: the depthwise launches of an 8 x 3 x 32 x 224 x 224 batch of ir-CSN / ip-CSN -- 64 channels at 32 x 56 x 56; 128 from
32 x 56 x 56 to 16 x 28 x 28 (stride 2) and at 16 x 28 x 28; 256 and 512 likewise -- each against `F.conv3d(groups=C)` on the same
GPU, on contiguous (NCDHW) and on `channels_last_3d` tensors, under MIOpen's default find mode and under
`torch.backends.cudnn.benchmark = True`, with BN and ReLU left OUT of the torch side (it is charged the conv alone).  Next to the
library's own rule every form is forced through `ptx_conv3d_dw_f32_force_form`: strips of 4 and 8 columns, and the LDS-staged tile.  Bytes are the algorithm's: the input read once, the output written once, 4 bytes each; the rate is those bytes over the
launch time.  The stem's max pool (8 x 64 x 32 x 112 x 112 -> 56 x 56, `ptx_maxpool3d_fwd`) runs in the same process as the
streaming yardstick: what this library's own streaming kernel of the same kind reaches on this device, on this day.

Models: `ir_csn152` and `ip_csn152` at that batch in clips/s, against the same model's torch.nn children in eval mode on the GPU
(`eager.resnet_forward` under no_grad: MIOpen convolutions, BatchNorm, ReLU as separate ops).

Clock: HIP events around `iters` back-to-back launches / calls, every variant warmed, the variants alternating inside every round;
the median of 5 rounds is reported, the spread of a variant is (max - min) / median of its rounds.  `iters` is sized per variant to a
window of about 100 ms (at least 2 calls; --iters fixes it).  Results are written after every shape, so a cut-off run keeps what it has.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import pretorched_x_amd as ptx                                   # noqa: E402
from pretorched_x_amd import eager                               # noqa: E402
from pretorched_x_amd.testing import synth_state_dict            # noqa: E402

L = ptx._lib
DEV = "cuda:0"
N = 8
# (channels, input (T, H, W), stride)
SHAPES = [(64, (32, 56, 56), 1), (128, (32, 56, 56), 2), (128, (16, 28, 28), 1), (256, (16, 28, 28), 2), (256, (8, 14, 14), 1),
          (512, (8, 14, 14), 2), (512, (4, 7, 7), 1)]


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
    """{name: fn} -> {name: {"ms": median, "spread": (max - min) / median, "rounds": [...], "iters": n}}, variants alternating."""
    per = {}
    for k, fn in variants.items():
        fn()
        fn()
        once = max(event_timed(fn, 1), 1e-3)
        per[k] = iters if iters else (1 if once > 2000.0 else max(2, min(2000, int(100.0 / once))))     # ~100 ms windows
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(event_timed(fn, per[k]))
    return {k: dict(ms=round(statistics.median(v), 5), spread=round((max(v) - min(v)) / statistics.median(v), 4),
                    rounds=[round(x, 5) for x in v], iters=per[k]) for k, v in got.items()}


def ptr(t):
    return C.c_void_p(t.data_ptr())


def save(out, path):
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


def bench_kernels(out, args, iters, rounds):
    lib = L.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device=DEV).manual_seed(1)
    rows = out.setdefault("kernels", {})
    # the streaming yardstick: the CSN stem pool on the library's own max-pool kernel
    px = torch.randn((N, 32, 112, 112, 64), device=DEV, generator=g)
    py = torch.empty((N, 32, 56, 56, 64), device=DEV)
    pd = L.PoolDesc(N, 32, 112, 112, 64, 64, 32, 56, 56, 1, 3, 3, 1, 2, 2, 0, 1, 1, 64, 0)
    r = alternate({"maxpool": lambda: L.check(lib.ptx_maxpool3d_fwd(C.byref(pd), ptr(px), ptr(py), stream), "maxpool")}, iters, rounds)["maxpool"]
    r["compulsory_bytes"] = 4 * (px.numel() + py.numel())
    r["GBps"] = round(r["compulsory_bytes"] / r["ms"] / 1e6, 1)
    rows["maxpool_stem_1x3x3_s2_64ch_32x112x112"] = r
    del px, py
    save(out, args.out)
    for Cc, dims, s in SHAPES:
        T, H, W = dims
        To, Ho, Wo = [(v - 1) // s + 1 for v in dims]
        x = torch.randn((N, T, H, W, Cc), device=DEV, generator=g)
        w = torch.randn((Cc, 1, 3, 3, 3), device=DEV, generator=g) * 0.2
        bn = [torch.rand(Cc, device=DEV, generator=g) + 0.5, torch.randn(Cc, device=DEV, generator=g) * 0.1,
              torch.randn(Cc, device=DEV, generator=g) * 0.1, torch.rand(Cc, device=DEV, generator=g) + 0.5]
        wp, bp = torch.empty((27, Cc), device=DEV), torch.empty(Cc, device=DEV)
        L.check(lib.ptx_pack_dw_weight_f32(Cc, 3, 3, 3, ptr(w), None, ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), ptr(bn[3]), C.c_float(1e-3),
                                           ptr(wp), ptr(bp), stream), "pack")
        y = torch.empty((N, To, Ho, Wo, Cc), device=DEV)
        d = L.ConvDesc()
        d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx, d.To, d.Ho, d.Wo, d.Co, d.ldy = N, T, H, W, Cc, Cc, To, Ho, Wo, Cc, Cc
        d.kT = d.kH = d.kW = 3
        d.sT = d.sH = d.sW = s
        d.pT = d.pH = d.pW = 1
        d.groups, d.flags = Cc, L.PTX_EPI_RELU
        assert lib.ptx_conv3d_dw_f32_supported(C.byref(d)) == 1, lib.ptx_last_error().decode()

        def ours():
            L.check(lib.ptx_conv3d_dw_f32_fwd(C.byref(d), ptr(x), ptr(wp), ptr(bp), ptr(y), stream), "dw")

        def forced(form):
            def run():
                L.check(lib.ptx_conv3d_dw_f32_force_form(form), "force_form")
                try:
                    ours()
                finally:
                    lib.ptx_conv3d_dw_f32_force_form(0)
            return run

        def tuned(fn):                                                  # MIOpen's exhaustive find (torch.backends.cudnn.benchmark)
            def run():
                torch.backends.cudnn.benchmark = True
                try:
                    return fn()
                finally:
                    torch.backends.cudnn.benchmark = False
            return run

        x_nc = x.permute(0, 4, 1, 2, 3).contiguous()                    # NCDHW, contiguous
        x_cl = x.permute(0, 4, 1, 2, 3)                                 # the same values, channels_last_3d strides
        assert x_cl.is_contiguous(memory_format=torch.channels_last_3d)
        w_cl = w.contiguous(memory_format=torch.channels_last_3d)
        t_nc, t_cl = (lambda: F.conv3d(x_nc, w, None, s, 1, 1, Cc)), (lambda: F.conv3d(x_cl, w_cl, None, s, 1, 1, Cc))
        variants = {"ptx_dw": ours, "ptx_dw_strip4": forced(L.PTX_DW_FORM_STRIP4), "ptx_dw_strip8": forced(L.PTX_DW_FORM_STRIP8),
                    "ptx_dw_lds": forced(L.PTX_DW_FORM_LDS), "torch_contiguous": t_nc, "torch_channels_last_3d": t_cl,
                    "torch_contiguous_benchmark": tuned(t_nc), "torch_channels_last_3d_benchmark": tuned(t_cl)}
        # the same numbers first: the folded pack against torch's conv + eval BN + ReLU on the same device
        ours()
        scale = bn[0] / torch.sqrt(bn[3] + 1e-3)
        ref = F.relu(F.conv3d(x_nc, w, None, s, 1, 1, Cc) * scale.view(1, -1, 1, 1, 1) + (bn[1] - bn[2] * scale).view(1, -1, 1, 1, 1))
        err = (y.permute(0, 4, 1, 2, 3) - ref).abs().max().item()
        del ref
        with torch.no_grad():
            r = alternate(variants, iters, rounds)
        nbytes = 4 * Cc * N * (T * H * W + To * Ho * Wo)
        row = dict(channels=Cc, input=[T, H, W], stride=s, output=[To, Ho, Wo], compulsory_bytes=nbytes, max_abs_diff_vs_torch=err)
        for k, v in r.items():
            v["GBps_compulsory"] = round(nbytes / v["ms"] / 1e6, 1)
            row[k] = v
        best = min(r[k]["ms"] for k in r if k.startswith("torch_"))
        row["best_torch_over_ptx"] = round(best / r["ptx_dw"]["ms"], 2)
        rows["dw_%dch_%dx%dx%d_s%d" % (Cc, T, H, W, s)] = row
        print(json.dumps({"dw_%dch_%dx%dx%d_s%d" % (Cc, T, H, W, s): {k: (v["ms"] if isinstance(v, dict) else v) for k, v in row.items()}}),
              flush=True)
        save(out, args.out)
        del x, y, x_nc, x_cl


def bench_models(out, args, iters, rounds):
    rows = out.setdefault("models", {})
    g = torch.Generator(device=DEV).manual_seed(2)
    T, S = (8, 64) if args.quick else (32, 224)
    x = torch.randn((N, 3, T, S, S), device=DEV, generator=g)
    for name in ("ir_csn152", "ip_csn152"):
        m = ptx.__dict__[name](num_classes=400, pretrained=None)
        m.load_state_dict(synth_state_dict(m.state_dict(), 1234))
        m = m.eval().to(DEV)
        with torch.no_grad():
            a = m(x)                                                     # plan build, weight pack, first-use tuning
            b = eager.resnet_forward(m, x)
            diff = (a - b).abs().max().item()
            r = alternate({"ptx": lambda: m(x), "torch_nn_eval": lambda: eager.resnet_forward(m, x)}, iters, rounds)
            eng = m.engine()
            plan = eng.plan_for(m, x)                                    # the whole batch as one plan, for the per-launch rows
            eng._maybe_tune(m, plan, x)
            with plan.exclusive():
                plan.bind(m)
                plan.run_features(x)
                prof = eng.profile_steps(plan, 3)
        row = dict(batch=[N, 3, T, S, S], max_abs_diff_logits=diff, max_abs_logit=a.abs().max().item())
        for k, v in r.items():
            v["clips_per_s"] = round(N / v["ms"] * 1e3, 1)
            row[k] = v
        row["speedup"] = round(r["torch_nn_eval"]["ms"] / r["ptx"]["ms"], 2)
        kinds = {}
        for p in prof:
            key = "depthwise" if p[1] == "mem" and p[0].endswith(".conv2") else "maxpool" if p[0] == "maxpool3d" else p[1]
            kinds[key] = round(kinds.get(key, 0.0) + p[4], 4)
        row["ms_by_launch_kind"] = kinds
        rows[name] = row
        print(json.dumps({name: {k: (v["ms"] if isinstance(v, dict) and "ms" in v else v) for k, v in row.items()}}), flush=True)
        save(out, args.out)
        del m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", default="all", choices=["kernels", "models", "all"])
    ap.add_argument("--iters", type=int, default=0, help="calls per timed window (0: sized to ~100 ms)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_csn_bench: no GPU (there is no CPU path to time)")
    iters, rounds = (2, 2) if args.quick else (args.iters, args.rounds)
    out = {}
    if args.out and os.path.exists(args.out) and args.part != "all":       # the two parts may run as two commands into one file
        with open(args.out) as f:
            out = json.load(f)
    out.update(device=torch.cuda.get_device_name(0), binary=L.lib().ptx_version().decode(), clips=N, iters=iters, rounds=rounds,
               clock="HIP events around back-to-back launches / calls, warmed, alternating rounds, median of the rounds",
               dw_forms="ptx_dw: the library's rule (8-column strips where Wo >= 16, else 4); ptx_dw_strip4 / _strip8 / _lds: forced through "
                        "ptx_conv3d_dw_f32_force_form (the LDS-staged halo tile is the form that lost)",
               torch_modes="torch_*: MIOpen's default find mode; torch_*_benchmark: torch.backends.cudnn.benchmark = True")
    if args.part in ("kernels", "all"):
        bench_kernels(out, args, iters, rounds)
    if args.part in ("models", "all"):
        bench_models(out, args, iters, rounds)
    save(out, args.out)


if __name__ == "__main__":
    main()
