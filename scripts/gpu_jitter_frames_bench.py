"""Per-clip resize geometry (`TransformFrames(random_short_side=.., random_resized_crop=..)`, ptx_resize_build_tables +
ptx_resize_frames_u8_tables) timed with HIP events against the fixed-window launch.

    python scripts/gpu_jitter_frames_bench.py [--iters 100] [--warmup 20] [--rounds 3] [--out profiles/jitter_frames.json]

Per shape (8 clips x 16 frames of 360x640 and 720x1280 -> 224x224 windows, uint8 out), microseconds per call, each the median
over `rounds` x `iters` calls timed one by one with device events, the arms alternating round by round:
  (a) fixed_window_us        ptx_resize_frames_u8 with the centre window's tables (short side 256): the existing launch
  (b) built_jitter_us        upload of the 8 x 40 geometry bytes + ptx_resize_build_tables + ptx_resize_frames_u8_tables, eight
      built_rrc_us           distinct drawn geometries: short-side jitter 256-320 + random crop + flips / random-resized-crop
  (c) host_tables_jitter_us  the same launch with the tables built on the host (`geometry_tables` per clip) and uploaded; the
      host_tables_rrc_us     host's wall time for building them is reported next to the device time (host_build_*_wall_us)
  (d) fresh_per_clip_us      what a user does today for the jitter: eight fresh TransformFrames(scale=.., crop=..) calls (a
                             table build, an upload and a launch each), written into one output batch
The outputs of (b), (c) and (d) must be equal bit for bit at the timed shapes; the script checks it before it times.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(360, 640), (720, 1280)]
CLIPS, FRAMES = 8, 16
OPTS = dict(input_size=[3, 224, 224], input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406],
            std=[0.229, 0.224, 0.225])


def _times(fn, iters, warmup):
    """us of each of `iters` calls, every call between its own pair of device events."""
    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) * 1000.0 for e0, e1 in ev]


def _stacked(TF, geometry, S):
    """geometry_tables per clip, stacked to [N][S] / [N][S][pitch] (the oracle's tables as the tables launch takes them)."""
    per = [TF.geometry_tables(row, S) for row in geometry]
    out = []
    for axis in ("rows", "cols"):
        taps = max(t[axis][2].shape[1] for t in per)
        k = np.zeros((len(per), S, taps), np.int32)
        for n, t in enumerate(per):
            k[n, :, :t[axis][2].shape[1]] = t[axis][2]
        out += [np.stack([t[axis][0] for t in per]), np.stack([t[axis][1] for t in per]), k]
    return out


def shape_row(a, ptx, H, W):
    from pretorched_x_amd import _lib as L
    TF = ptx.transforms
    lib, dev = L.lib(), torch.device("cuda:0")
    frames = torch.randint(0, 256, (CLIPS, FRAMES, H, W, 3), dtype=torch.uint8, device=dev)
    S = max(OPTS["input_size"])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptrs = lambda ts: [C.c_void_p(x.data_ptr()) for x in ts]
    new_out = lambda: torch.empty((CLIPS, FRAMES, S, S, 3), dtype=torch.uint8, device=dev)

    # (a) the fixed centre window
    fixed = TF.build_tables(H, W, OPTS["input_size"])
    ftabs = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in tuple(fixed["rows"]) + tuple(fixed["cols"])]
    fdesc = L.ResizeDesc(CLIPS, FRAMES, H, W, 3, S, S, fixed["rows"][2].shape[1], fixed["cols"][2].shape[1], L.PTX_RESIZE_OUT_U8)
    ya = new_out()

    def arm_a():
        L.check(lib.ptx_resize_frames_u8(C.byref(fdesc), C.c_void_p(frames.data_ptr()), *ptrs(ftabs), C.c_void_p(ya.data_ptr()),
                                         None, st), "ptx_resize_frames_u8")

    arms, row = {"a": arm_a}, {}
    draws = {"jitter": dict(random_short_side=(256, 320), random_crop=True, random_hflip=True, random_vflip=True),
             "rrc": dict(random_resized_crop=True, random_hflip=True)}
    outs = {}
    for kind, kw in draws.items():
        rt = TF.TransformFrames(OPTS, out="frames", generator=torch.Generator().manual_seed(5), **kw)
        geom = rt.draw_geometry(CLIPS, H, W)
        assert len(set(map(tuple, geom.tolist()))) == CLIPS, "the drawn geometries are not distinct: pick another seed"
        g, taps_h, taps_w = rt._checked_geometry(geom, CLIPS, H, W)
        desc = L.ResizeDesc(CLIPS, FRAMES, H, W, 3, S, S, taps_h, taps_w, L.PTX_RESIZE_OUT_U8)
        sizes = [CLIPS * S, CLIPS * S, CLIPS * S * taps_h, CLIPS * S, CLIPS * S, CLIPS * S * taps_w]
        btabs = [torch.empty(n, dtype=torch.int32, device=dev) for n in sizes]
        yb, yc = new_out(), new_out()

        # (b) upload the rows, build the tables on the device, launch
        def arm_b(g=g, desc=desc, btabs=btabs, yb=yb):
            geo = g.to(dev)
            L.check(lib.ptx_resize_build_tables(C.byref(desc), C.c_void_p(geo.data_ptr()), *ptrs(btabs), st), "ptx_resize_build_tables")
            L.check(lib.ptx_resize_frames_u8_tables(C.byref(desc), C.c_void_p(frames.data_ptr()), *ptrs(btabs),
                                                    C.c_void_p(yb.data_ptr()), None, st), "ptx_resize_frames_u8_tables")

        # (c) build the tables on the host, upload them, launch
        wall = []

        def arm_c(geom=geom, desc=desc, yc=yc, wall=wall):
            t0 = time.perf_counter()
            parts = _stacked(TF, geom.tolist(), S)
            flat = np.concatenate([p.reshape(-1) for p in parts]).astype(np.int32)
            wall.append((time.perf_counter() - t0) * 1e6)
            buf = torch.from_numpy(flat).to(dev)
            offs = np.cumsum([0] + [p.size for p in parts[:-1]])
            L.check(lib.ptx_resize_frames_u8_tables(C.byref(desc), C.c_void_p(frames.data_ptr()),
                                                    *[C.c_void_p(buf.data_ptr() + int(o) * 4) for o in offs],
                                                    C.c_void_p(yc.data_ptr()), None, st), "ptx_resize_frames_u8_tables")

        arm_b()
        arm_c()
        torch.cuda.synchronize()
        if not torch.equal(yb, yc):
            raise SystemExit("gpu_jitter_frames_bench.py: device-built and host-built tables differ at %dx%d (%s)" % (H, W, kind))
        outs[kind] = yb
        arms["b_" + kind], arms["c_" + kind] = arm_b, arm_c
        row[kind] = {"geometry": geom.tolist(), "taps_h": taps_h, "taps_w": taps_w, "host_wall": wall}

    # (d) the jitter as a user writes it today: a fresh TransformFrames per clip at the clip's scale
    jit = row["jitter"]["geometry"]
    yd = new_out()

    def per_clip_kw(g):
        R = min(g[4], g[5])
        scale = S / (R + 0.5)                                            # floor(S / scale) == R
        assert TF.resized_size(H, W, OPTS["input_size"], scale) == (g[4], g[5])
        return dict(scale=scale, crop=(g[6], g[7]), hflip=bool(g[8]), vflip=bool(g[9]))

    def arm_d():
        for n, g in enumerate(jit):
            yd[n].copy_(TF.TransformFrames(OPTS, out="frames", **per_clip_kw(g))(frames[n]))

    arm_d()
    torch.cuda.synchronize()
    if not torch.equal(yd, outs["jitter"]):
        raise SystemExit("gpu_jitter_frames_bench.py: the tables launch differs from the per-clip fixed-window calls at %dx%d" % (H, W))
    arms["d"] = arm_d

    samples = {k: [] for k in arms}
    for kind in draws:
        row[kind]["host_wall"].clear()
    for _ in range(a.rounds):                                            # alternate the arms
        for key, fn in arms.items():
            samples[key] += _times(fn, a.iters, a.warmup)
    med = {k: statistics.median(v) for k, v in samples.items()}
    p10 = {k: sorted(v)[len(v) // 10] for k, v in samples.items()}
    p90 = {k: sorted(v)[len(v) * 9 // 10] for k, v in samples.items()}
    out = {"case": "%dx%d" % (H, W), "clips": CLIPS, "frames_per_clip": FRAMES, "samples_per_arm": len(samples["a"]),
           "bit_identical_arms": True,
           "fixed_window_us": round(med["a"], 1),
           "built_jitter_us": round(med["b_jitter"], 1), "built_rrc_us": round(med["b_rrc"], 1),
           "host_tables_jitter_us": round(med["c_jitter"], 1), "host_tables_rrc_us": round(med["c_rrc"], 1),
           "host_build_jitter_wall_us": round(statistics.median(row["jitter"]["host_wall"]), 1),
           "host_build_rrc_wall_us": round(statistics.median(row["rrc"]["host_wall"]), 1),
           "fresh_per_clip_us": round(med["d"], 1),
           "p10_us": {k: round(v, 1) for k, v in p10.items()}, "p90_us": {k: round(v, 1) for k, v in p90.items()},
           "built_jitter_over_fixed": round(med["b_jitter"] / med["a"], 4), "built_rrc_over_fixed": round(med["b_rrc"] / med["a"], 4),
           "fresh_per_clip_over_built_jitter": round(med["d"] / med["b_jitter"], 3),
           "jitter": {k: v for k, v in row["jitter"].items() if k != "host_wall"},
           "rrc": {k: v for k, v in row["rrc"].items() if k != "host_wall"}}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_jitter_frames_bench.py needs a GPU: timings from anything else mean nothing")
    if a.iters * a.rounds < 100:
        raise SystemExit("gpu_jitter_frames_bench.py: a median wants at least 100 launches per arm")
    import pretorched_x_amd as ptx
    result = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds,
              "out": "uint8", "shapes": [shape_row(a, ptx, H, W) for H, W in SIZES]}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
