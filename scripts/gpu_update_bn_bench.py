"""update_bn on the HIP engine against torch.optim.swa_utils.update_bn on the torch.nn path it replaces, in one process.

    python scripts/gpu_update_bn_bench.py [--rounds 5] [--only kernel,models,margins] [--out logs/update_bn.json]

(a) "kernel": ptx_bn_batch_stats_f32 at layer1's shape of resnet3d50 on 8 x 3 x 16 x 224 x 224 (8*8*56*56 rows x 256 channels,
    205 MB: two activations are read in turn, so no launch finds its input in the 256 MB last-level cache), bytes read per
    second from device-event time; next to it ptx_bn_apply_f32 (plain and with a residual) and, as the HBM yardstick, the
    existing max-pool at the stem's shape (8 x 16 x 112 x 112 x 64 -> 8 x 8 x 56 x 56 x 64), bytes read + written per second.
(b) "models": resnet3d50 at 8 x 3 x 16 x 224 x 224 and r2plus1d18 at 8 x 3 x 32 x 112 x 112, a loader of four batches: wall time
    per batch (host clock around the call, ended by a device synchronise) of pretorched_x_amd.update_bn and of
    torch.optim.swa_utils.update_bn on the same model and GPU (train()-mode torch.nn children, eager.py), the two
    alternating `rounds` (>= 5) times after one warm-up call each; the median round, the range and every round are reported,
    and how far the two sets of running statistics lie apart.
(c) "margins": every case of tests/golden/update_bn.npz on the GPU: distance of the running statistics and of the eval-mode
    logits from the float64 reference, relative to the golden tensor's max-abs (the bar of tests/test_gpu_update_bn.py is 1e-3).
The output is rewritten after every part.  The committed copy of the output is profiles/update_bn.json."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pretorched_x_amd as ptx  # noqa: E402
from pretorched_x_amd import _lib as L  # noqa: E402
from pretorched_x_amd.testing import synth_state_dict  # noqa: E402

DEV = "cuda:0"


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _summary(vals, digits=5):
    return {"median": round(statistics.median(vals), digits), "min": round(min(vals), digits), "max": round(max(vals), digits),
            "rounds": [round(v, digits) for v in vals]}


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


# ------------------------------------------------------------------------------------------------ (a) kernels
def kernel(rounds):
    lib = L.lib()
    rows, C_ = 8 * 8 * 56 * 56, 256
    acts = [torch.randn(rows, C_, device=DEV) for _ in range(2)]
    res = torch.randn(rows, C_, device=DEV)
    ys = [torch.empty(rows, C_, device=DEV) for _ in range(2)]
    n = int(lib.ptx_bn_batch_stats_workspace_bytes(rows, C_))
    ws, mean, var = torch.empty(n // 4, device=DEV), torch.empty(C_, device=DEV), torch.empty(C_, device=DEV)
    scale, shift = torch.rand(C_, device=DEV) + 0.5, torch.randn(C_, device=DEV)
    turn = [0]

    def stats():
        turn[0] ^= 1
        L.check(lib.ptx_bn_batch_stats_f32(_p(acts[turn[0]]), rows, C_, C_, _p(mean), _p(var), _p(ws), n, _st()), "stats")
    d = L.BnApplyDesc()
    d.N, d.T, d.H, d.W, d.C, d.ldx, d.ldy, d.flags = 8, 8, 56, 56, C_, C_, C_, L.PTX_EPI_RELU
    dr = L.BnApplyDesc()
    dr.N, dr.T, dr.H, dr.W, dr.C, dr.ldx, dr.ldy, dr.ldr, dr.flags = 8, 8, 56, 56, C_, C_, C_, C_, L.PTX_EPI_RELU | L.PTX_EPI_RES_ADD

    def apply():
        turn[0] ^= 1
        L.check(lib.ptx_bn_apply_f32(C.byref(d), _p(acts[turn[0]]), _p(scale), _p(shift), None, _p(ys[turn[0]]), _st()), "apply")

    def apply_res():
        turn[0] ^= 1
        L.check(lib.ptx_bn_apply_f32(C.byref(dr), _p(acts[turn[0]]), _p(scale), _p(shift), _p(res), _p(ys[turn[0]]), _st()), "apply+res")
    pin = torch.randn(8, 16, 112, 112, 64, device=DEV)
    pout = torch.empty(8, 8, 56, 56, 64, device=DEV)
    pd = L.PoolDesc(8, 16, 112, 112, 64, 64, 8, 56, 56, 3, 3, 3, 2, 2, 2, 1, 1, 1, 64, 0)

    def pool():
        L.check(lib.ptx_maxpool3d_fwd(C.byref(pd), _p(pin), _p(pout), _st()), "maxpool")
    act_bytes = 4 * rows * C_
    runs = {"bn_batch_stats_f32": (stats, act_bytes), "bn_apply_f32": (apply, 2 * act_bytes), "bn_apply_f32+res": (apply_res, 3 * act_bytes),
            "maxpool3d (yardstick)": (pool, 4 * (pin.numel() + pout.numel()))}
    for fn, _ in runs.values():
        event_ms(fn, 4)
    ms = {k: [] for k in runs}
    for r in range(rounds):
        for k in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
            ms[k].append(event_ms(runs[k][0], 10))
    out = {"shape": {"rows": rows, "channels": C_, "activation_bytes": act_bytes}, "launches": {}}
    for k, v in ms.items():
        nbytes = runs[k][1]
        out["launches"][k] = {"algorithmic_bytes": nbytes, "ms": _summary(v), "TB_per_s": _summary([nbytes / (m * 1e-3) / 1e12 for m in v], 3)}
    return out


# ------------------------------------------------------------------------------------------------ (b) models
def _fresh(name):
    factory = getattr(ptx, name)
    try:
        m = factory(num_classes=339, pretrained=None)
    except TypeError:
        m = factory(num_classes=339)
    m.load_state_dict(synth_state_dict(m.state_dict(), 1234))
    return m.to(DEV).eval()


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _bn_state(model):
    layers = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    return torch.cat([b.running_mean for b in layers]).double().cpu(), torch.cat([b.running_var for b in layers]).double().cpu()


def models(rounds):
    out = {}
    for name, shape in (("resnet3d50", (8, 3, 16, 224, 224)), ("r2plus1d18", (8, 3, 32, 112, 112))):
        g = torch.Generator().manual_seed(7)
        xs = [torch.randn(shape, generator=g).to(DEV) for _ in range(4)]
        hip, ref = _fresh(name), _fresh(name)
        runs = {"hip_engine": lambda: ptx.update_bn(xs, hip), "torch_nn": lambda: torch.optim.swa_utils.update_bn(xs, ref)}
        rec = {"shape": list(shape), "batches": len(xs)}
        ok = {}
        for k, fn in runs.items():
            try:
                rec[k + "_first_call_s"] = round(_wall(fn), 4)          # plans compiled and tiles timed / MIOpen finds its kernels
                ok[k] = fn
            except Exception as e:              # one side failing is a result to report, not a reason to lose the other
                rec[k + "_error"] = "%s: %s" % (type(e).__name__, str(e)[:300])
        secs = {k: [] for k in ok}
        for r in range(rounds):
            for k in (list(ok) if r % 2 == 0 else list(ok)[::-1]):
                secs[k].append(_wall(ok[k]) / len(xs))
        for k, v in secs.items():
            rec[k + "_ms_per_batch"] = _summary([1e3 * s for s in v], 3)
        if len(ok) == 2:
            rec["torch_nn_over_hip_engine"] = round(statistics.median(secs["torch_nn"]) / statistics.median(secs["hip_engine"]), 3)
            (m0, v0), (m1, v1) = _bn_state(hip), _bn_state(ref)
            rec["hip_vs_torch_nn_fp32"] = {"running_mean": float((m0 - m1).abs().max() / m1.abs().max()),
                                           "running_var": float((v0 - v1).abs().max() / v1.abs().max())}
        assert not ref.training and not hip.training
        out[name] = rec
        del hip, ref, xs
        torch.cuda.empty_cache()
    return out


# ------------------------------------------------------------------------------------------------ (c) margins
def margins():
    spec = importlib.util.spec_from_file_location("make_update_bn_golden", os.path.join(ROOT, "tests", "golden", "make_update_bn_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    out = {"bar": 1e-3}
    for name, rec in G.load().items():
        model = G.build_model(rec["spec"]).to(DEV)
        xs = [x.to(DEV) for x in G.batches(rec["spec"])]
        ptx.update_bn(xs, model, **rec["spec"]["call"])
        layers = G.bn_layers(model)
        mean = torch.cat([b.running_mean for b in layers]).cpu().numpy().astype(np.float64)
        var = torch.cat([b.running_var for b in layers]).cpu().numpy().astype(np.float64)
        logits = model(xs[0]).cpu().numpy().astype(np.float64)
        out[name] = {"running_mean": float(np.abs(mean - rec["mean"]).max() / np.abs(rec["mean"]).max()),
                     "running_var": float(np.abs(var - rec["var"]).max() / np.abs(rec["var"]).max()),
                     "logits": float(np.abs(logits - rec["logits"]).max() / np.abs(rec["logits"]).max()),
                     "argmax_equal": bool(np.array_equal(logits.argmax(1), rec["logits"].argmax(1)))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="kernel,models,margins")
    ap.add_argument("--out", default=os.path.join(ROOT, "logs", "update_bn.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    rounds = max(5, args.rounds)
    result = {"device": torch.cuda.get_device_name(0), "library": L.lib().ptx_version().decode(), "rounds": rounds}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    parts = {"kernel": lambda: kernel(rounds), "models": lambda: models(rounds), "margins": margins}
    for part in args.only.split(","):
        result[part] = parts[part]()
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps({part: result[part]}))


if __name__ == "__main__":
    main()
