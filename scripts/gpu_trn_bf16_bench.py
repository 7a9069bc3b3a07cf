"""bf16 TRN and 2-D ResNets against their fp32 twins, in one process.

    python scripts/gpu_trn_bf16_bench.py [--iters 20] [--rounds 5] [--only w1,head,trn,resnet50] [--out logs/trn_bf16.json]

(a) "w1": the W1 launch of an MSTRN head at K = 16384, Nout = 1024 (8 frames of 2048 features -> 1024), M = 8 and M = 24 rows
    (1 and 3 frame subsets of 8 videos): ptx_relation_linear_bf16w_fwd against the fp32 ptx_relation_linear_fwd at the same
    shape.  Time per launch and weight bytes per second, twice: with ONE weight matrix (it stays in the 256 MB last-level
    cache between launches) and ROTATING over enough copies that every launch streams its weights from HBM (>= 320 MB in all).
(b) "head": the whole MultiScaleRelation(8, 2048, 1024, 1024, 3) head on 8 videos, fp32 and bf16.
(c) "trn": TRN on resnet50 (MSTRN consensus), 8 videos x 8 segments at 224 x 224, videos/s in fp32 and bf16.
(d) "resnet50": the 2-D resnet50 at 64 x 3 x 224 x 224, images/s in fp32 and bf16.
Everything is timed with device events after a warm-up of every variant, the variants alternating `rounds` (>= 5) times; the
median round, the range and every round are reported.  The output is rewritten after every part.
The committed copy of the output is profiles/trn_bf16.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pretorched_x_amd as ptx  # noqa: E402
from pretorched_x_amd import _lib as L  # noqa: E402
from pretorched_x_amd.engine import _ptr  # noqa: E402
from pretorched_x_amd.testing import synth_state_dict  # noqa: E402

DEV = "cuda:0"


def _st():
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
    reverse order on every second pass."""
    for fn in runs.values():
        timed(fn, warmup)
    ms = {k: [] for k in runs}
    for r in range(rounds):
        for k in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
            ms[k].append(timed(runs[k], iters))
    return {k: {"ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5),
                "spread_ms": round(max(v) - min(v), 5), "rounds_ms": [round(x, 5) for x in v]} for k, v in ms.items()}


# ------------------------------------------------------------------------------------------------ (a) the W1 launch
def w1(iters, rounds):
    B, T, F_, Nout = 8, 8, 2048, 1024
    K = T * F_
    lib = L.lib()
    g = torch.Generator().manual_seed(1)
    x32 = torch.randn(B, T, F_, generator=g).to(torch.bfloat16).float().to(DEV)
    x16 = x32.to(torch.bfloat16)
    n32, n16 = -(-320 * 2 ** 20 // (Nout * K * 4)), -(-320 * 2 ** 20 // (Nout * K * 2))
    w32 = [(torch.randn(Nout, K, generator=g) * K ** -0.5).to(torch.bfloat16).float().to(DEV) for _ in range(n32)]
    w16 = [w32[i % n32].to(torch.bfloat16) for i in range(n16)]
    b32 = torch.randn(Nout, generator=g).to(torch.bfloat16).float().to(DEV)
    b16 = b32.to(torch.bfloat16)
    flags = L.PTX_PRO_RELU | L.PTX_EPI_RELU
    out = {"K": K, "Nout": Nout, "weight_bytes": {"fp32": Nout * K * 4, "bf16": Nout * K * 2},
           "rotating_copies": {"fp32": n32, "bf16": n16}, "rows": {}}
    subsets_all = [tuple(range(8)), (7, 6, 5, 4, 3, 2, 1, 0), (3, 0, 7, 1, 6, 2, 5, 4)]
    for n_sets in (1, 3):
        M = n_sets * B
        d = L.RelationDesc()
        d.B, d.n_sets, d.n_frames, d.frame_len = B, n_sets, T, F_
        for r in range(n_sets):
            for f in range(T):
                d.idx[r][f] = subsets_all[r][f]
        y32 = torch.empty(M, Nout, device=DEV)
        y16 = torch.empty(M, Nout, device=DEV)
        wsn = int(lib.ptx_linear_bf16w_workspace_bytes(M, K, Nout))
        ws = torch.empty(max(wsn, 16) // 4, device=DEV)
        state = {"i32": 0, "i16": 0}

        def fp32(rot):
            def run():
                w = w32[state["i32"] % n32] if rot else w32[0]
                state["i32"] += 1
                L.check(lib.ptx_relation_linear_fwd(C.byref(d), _ptr(x32), T * F_, _ptr(w), _ptr(b32), _ptr(y32), Nout, Nout, flags, _st()), "fp32 W1")
            return run

        def bf16(rot):
            def run():
                w = w16[state["i16"] % n16] if rot else w16[0]
                state["i16"] += 1
                L.check(lib.ptx_relation_linear_bf16w_fwd(C.byref(d), _ptr(x16), T * F_, _ptr(w), _ptr(b16), _ptr(y16), Nout, Nout, flags,
                                                          _ptr(ws), wsn, _st()), "bf16 W1")
            return run
        # a launch takes tens of microseconds, less than the host needs to issue it from Python: `iters` launches are captured
        # into one graph per variant and the replay is timed (per-launch time = replay time / iters)
        runs = {"fp32_one_matrix": fp32(False), "bf16_one_matrix": bf16(False), "fp32_rotating": fp32(True), "bf16_rotating": bf16(True)}
        graphs = {}
        for k, fn in runs.items():
            fn()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                for _ in range(iters):
                    fn()
            graphs[k] = gr
        res = alternate({k: gr.replay for k, gr in graphs.items()}, 1, rounds)
        for k, v in res.items():
            for f in ("ms", "min_ms", "max_ms", "spread_ms"):
                v[f] = round(v[f] / iters, 6)
            v["rounds_ms"] = [round(t / iters, 6) for t in v["rounds_ms"]]
            v["weight_TB_per_s"] = round(out["weight_bytes"][k[:4]] / (v["ms"] * 1e-3) / 1e12, 3)
        del graphs
        # same operands (matrix 0): the bf16 launch against the fp32 one
        fp32(False)()
        state["i16"] = 0
        bf16(False)()
        torch.cuda.synchronize()
        res["max_abs_delta_bf16_vs_fp32"] = float((y16 - y32).abs().max())
        res["workspace_bytes"] = wsn
        for kind in ("one_matrix", "rotating"):
            a, b = res["fp32_" + kind], res["bf16_" + kind]
            res["bf16_faster_beyond_spread_" + kind] = bool(b["max_ms"] < a["min_ms"])
            res["speedup_" + kind] = round(a["ms"] / b["ms"], 3)
        out["rows"]["M=%d" % M] = res
    return out


# ------------------------------------------------------------------------------------------------ (b) the MSTRN head
def _pair(factory, seed=1234):
    sd = synth_state_dict(factory().state_dict(), seed)
    sd = {k: (v.to(torch.bfloat16).float() if v.is_floating_point() else v) for k, v in sd.items()}
    m32, m16 = factory(), factory()
    for m in (m32, m16):
        m.load_state_dict(sd)
    return m32.eval().to(DEV), m16.eval().to(torch.bfloat16).to(DEV)


def head(iters, rounds):
    h32, h16 = _pair(lambda: ptx.MultiScaleRelation(8, 2048, 1024, 1024, 3))
    x32 = torch.randn(8, 1, 8, 2048, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16).float().to(DEV)
    x16 = x32.to(torch.bfloat16)

    def run(m, x):
        def f():
            np.random.seed(3)
            return m(x)
        return f
    with torch.no_grad():
        res = alternate({"fp32": run(h32, x32), "bf16": run(h16, x16)}, iters, rounds)
        res["max_abs_delta_bf16_vs_fp32"] = float((run(h16, x16)().float() - run(h32, x32)()).abs().max())
        res["max_abs_fp32"] = float(run(h32, x32)().abs().max())
    n = sum(p.numel() for p in h32.parameters())
    res["parameters"] = n
    res["weights_streamed_per_call"] = "3 subsets share one read of every scale's W1"
    res["speedup"] = round(res["fp32"]["ms"] / res["bf16"]["ms"], 3)
    return res


# ------------------------------------------------------------------------------------------------ (c) TRN, (d) resnet50
def trn(iters, rounds):
    m32, m16 = _pair(lambda: ptx.TRN(339, num_segments=8, arch="resnet50", consensus="MSTRN", pretrained=None))
    for m in (m32, m16):
        m.base_model.engine().lanes = 1
    m16.base_model.engine().bf16_stem = "direct"
    x32 = torch.randn(8, 8, 3, 224, 224, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16).float().to(DEV)
    x16 = x32.to(torch.bfloat16)

    def run(m, x):
        def f():
            np.random.seed(3)
            return m(x)
        return f
    with torch.no_grad():
        ref, got = run(m32, x32)(), run(m16, x16)().float()
        res = alternate({"fp32": run(m32, x32), "bf16": run(m16, x16)}, iters, rounds)
    for k in ("fp32", "bf16"):
        res[k]["videos_per_s"] = round(8 / res[k]["ms"] * 1e3, 1)
    res["max_abs_fp32_logit"] = float(ref.abs().max())
    res["max_abs_delta_bf16_vs_fp32"] = float((got - ref).abs().max())
    res["argmax_equal"] = bool(torch.equal(got.argmax(1), ref.argmax(1)))
    res["speedup"] = round(res["fp32"]["ms"] / res["bf16"]["ms"], 3)
    return res


def resnet50(iters, rounds):
    m32, m16 = _pair(lambda: ptx.resnet50(num_classes=339, pretrained=None))
    for m in (m32, m16):
        m.engine().lanes = 1
    m16.engine().bf16_stem = "direct"
    n = 64
    x32 = torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).float().to(DEV)
    x16 = x32.to(torch.bfloat16)
    with torch.no_grad():
        ref, got = m32(x32), m16(x16).float()
        res = alternate({"fp32": lambda: m32(x32), "bf16": lambda: m16(x16)}, iters, rounds)
    for k in ("fp32", "bf16"):
        res[k]["images_per_s"] = round(n / res[k]["ms"] * 1e3, 1)
    res["batch"] = n
    res["max_abs_fp32_logit"] = float(ref.abs().max())
    res["max_abs_delta_bf16_vs_fp32"] = float((got - ref).abs().max())
    res["argmax_agreement"] = float((got.argmax(1) == ref.argmax(1)).float().mean())
    res["speedup"] = round(res["fp32"]["ms"] / res["bf16"]["ms"], 3)
    return res


PARTS = {"w1": (w1, 50), "head": (head, 20), "trn": (trn, 3), "resnet50": (resnet50, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=0, help="launches per timed window (default: per part)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=",".join(PARTS))
    ap.add_argument("--out", default=os.path.join(ROOT, "logs", "trn_bf16.json"))
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("at least 5 rounds")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = {}
    if os.path.exists(a.out):                       # parts measured by an earlier call are kept
        with open(a.out) as f:
            out = json.load(f)
    out.update({"device": torch.cuda.get_device_name(0), "library": L.lib().ptx_version().decode(), "rounds": a.rounds})
    for name in a.only.split(","):
        fn, iters = PARTS[name]
        out[name] = fn(a.iters or iters, a.rounds)
        out[name]["iters"] = a.iters or iters
        print(name, json.dumps(out[name]), flush=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
