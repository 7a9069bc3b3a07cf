"""The resize filters of `pretorched.transforms.TransformFrames(.., interpolation=f)` timed with HIP events.

    python scripts/gpu_resample_bench.py [--iters 50] [--warmup 10] [--out profiles/resample_frames.json]
                                         [--ab-parent a1.json a2.json .. --ab-new b1.json b2.json ..]

Per case (8 clips x 16 frames of 360x640 and 720x1280 -> resize to short side 256, centre crop 224, uint8 out) one row per
filter: the tap pitches, microseconds per ptx_resize_frames_u8 launch with that filter's tables, and the time relative to
bilinear at the same shape.  Then, for bicubic, the per-clip path: ptx_resize_build_tables_filter + ptx_resize_frames_u8_tables
on one RandomResizedCrop-like geometry per clip (the builder alone, and both launches together).

--ab-parent / --ab-new: outputs of scripts/gpu_transform_bench.py (--skip-model) from the parent commit and from this one, run
alternating in one session; their per-row medians, the parent's spread (max - min) and whether the new median stays within
parent median + parent spread are recorded next to the filter rows (the bilinear path must not get slower).
"""
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

SIZES = [(360, 640), (720, 1280)]
CLIPS, FRAMES = 8, 16
FILTERS = ("bilinear", "nearest", "box", "hamming", "bicubic", "lanczos")
OPTS = dict(input_size=[3, 224, 224], input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406],
            std=[0.229, 0.224, 0.225])


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
    return e0.elapsed_time(e1) * 1000.0 / iters        # us per call


def filter_rows(a, ptx):
    from pretorched_x_amd import _lib as L
    TF = ptx.transforms
    lib, dev = L.lib(), torch.device("cuda:0")
    rows = []
    for H, W in SIZES:
        frames = torch.randint(0, 256, (CLIPS, FRAMES, H, W, 3), dtype=torch.uint8, device=dev)
        y = torch.empty((CLIPS, FRAMES, 224, 224, 3), dtype=torch.uint8, device=dev)
        base = None
        for f in FILTERS:
            t = TF.build_tables(H, W, OPTS["input_size"], interpolation=f)
            tabs = [torch.from_numpy(np.array(x)).to(dev) for x in t["rows"] + t["cols"]]
            desc = L.ResizeDesc(CLIPS, FRAMES, H, W, 3, 224, 224, t["rows"][2].shape[1], t["cols"][2].shape[1], L.PTX_RESIZE_OUT_U8)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def launch():
                L.check(lib.ptx_resize_frames_u8(C.byref(desc), C.c_void_p(frames.data_ptr()),
                                                 *[C.c_void_p(x.data_ptr()) for x in tabs], C.c_void_p(y.data_ptr()), None, st),
                        "ptx_resize_frames_u8")
            us = _time(launch, a.iters, a.warmup)
            base = us if f == "bilinear" else base
            rows.append({"case": "%dx%d" % (H, W), "filter": f, "frames": CLIPS * FRAMES, "resized": list(t["resized"]),
                         "taps_h": int(desc.taps_h), "taps_w": int(desc.taps_w), "kernel_us": round(us, 1),
                         "vs_bilinear": round(us / base, 3), "frames_per_s": round(CLIPS * FRAMES / us * 1e6)})
            print(json.dumps(rows[-1]), flush=True)
        del frames
    return rows


def per_clip_rows(a, ptx):
    """bicubic with one geometry per clip: boxes of a RandomResizedCrop draw (fixed seed), resized to 224 x 224."""
    from pretorched_x_amd import _lib as L
    TF = ptx.transforms
    lib, dev = L.lib(), torch.device("cuda:0")
    rows = []
    for H, W in SIZES:
        tf = TF.TransformFrames(OPTS, out="frames", interpolation="bicubic", random_resized_crop=True, random_hflip=True,
                                generator=torch.Generator().manual_seed(1))
        g, taps_h, taps_w = tf._checked_geometry(tf.draw_geometry(CLIPS, H, W), CLIPS, H, W)
        frames = torch.randint(0, 256, (CLIPS, FRAMES, H, W, 3), dtype=torch.uint8, device=dev)
        y = torch.empty((CLIPS, FRAMES, 224, 224, 3), dtype=torch.uint8, device=dev)
        geo = g.contiguous().to(dev)
        sizes = [CLIPS * 224, CLIPS * 224, CLIPS * 224 * taps_h, CLIPS * 224, CLIPS * 224, CLIPS * 224 * taps_w]
        buf = torch.empty(sum(sizes), device=dev, dtype=torch.int32)
        tabs = [C.c_void_p(buf.data_ptr() + int(o) * 4) for o in np.cumsum([0] + sizes[:-1])]
        desc = L.ResizeDesc(CLIPS, FRAMES, H, W, 3, 224, 224, taps_h, taps_w, L.PTX_RESIZE_OUT_U8)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def build():
            L.check(lib.ptx_resize_build_tables_filter(C.byref(desc), C.c_void_p(geo.data_ptr()), L.PTX_RESAMPLE_BICUBIC, *tabs, st),
                    "ptx_resize_build_tables_filter")

        def both():
            build()
            L.check(lib.ptx_resize_frames_u8_tables(C.byref(desc), C.c_void_p(frames.data_ptr()), *tabs, C.c_void_p(y.data_ptr()), None, st),
                    "ptx_resize_frames_u8_tables")
        rows.append({"case": "%dx%d" % (H, W), "filter": "bicubic", "path": "per-clip builder + tables launch", "clips": CLIPS,
                     "taps_h": taps_h, "taps_w": taps_w, "builder_us": round(_time(build, a.iters, a.warmup), 1),
                     "builder_plus_resize_us": round(_time(both, a.iters, a.warmup), 1), "geometry": g.tolist()})
        print(json.dumps(rows[-1]), flush=True)
        del frames
    return rows


def bilinear_ab(parent_files, new_files):
    def load(files):
        runs = [json.load(open(p))["kernel"] for p in files]
        return {(r["case"], r["out"]): [run[i]["kernel_us"] for run in runs] for i, r in enumerate(runs[0])}
    old, new = load(parent_files), load(new_files)
    rows = []
    for key in old:
        po, pn = old[key], new[key]
        spread = max(po) - min(po)
        rows.append({"case": key[0], "out": key[1], "parent_us": po, "new_us": pn, "parent_median_us": statistics.median(po),
                     "new_median_us": statistics.median(pn), "parent_spread_us": round(spread, 1),
                     "within_margin": bool(statistics.median(pn) <= statistics.median(po) + spread)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ab-parent", nargs="*", default=[])
    ap.add_argument("--ab-new", nargs="*", default=[])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_resample_bench.py needs a GPU: timings from anything else mean nothing")
    import pretorched_x_amd as ptx
    result = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "clips": CLIPS, "frames": FRAMES,
              "filters": filter_rows(a, ptx), "per_clip_bicubic": per_clip_rows(a, ptx),
              "bilinear_parent_vs_new": bilinear_ab(a.ab_parent, a.ab_new) if a.ab_parent and a.ab_new else "not recorded yet"}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
