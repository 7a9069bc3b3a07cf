"""`SampleClips` (one table-builder launch + one ptx_resize_clips_u8 launch for a batch of videos of different sizes) timed
against the loop it replaces, on the same drawn index and geometry rows.

    python scripts/gpu_sample_clips_bench.py [--iters 30] [--warmup 5] [--out profiles/sample_clips.json]

Workload: 8 videos of 90 frames (3 x 360x640, 2 x 480x640, 2 x 720x1280, 1 x 640x360), T = 16, frame_stride = 4, S = 224,
random_short_side = (256, 320) + random_crop + random_hflip; clips = 1 and 2; out = "frames" and "tensor".
  (a) sample_clips   sc(videos, indices=idx, geometry=geo): one upload, one builder launch, one resize launch
  (b) per_video_loop per video `video[idx]` (a gathered copy), one `TransformFrames(.., out=..)(gathered, geometry=rows)` call,
                     then `torch.cat`: the public API before SampleClips
(a) must equal (b) bit for bit at these sizes; the script checks it before it times.  Both arms are warmed up, then timed
alternately call by call, every call between a pair of device events AND with a host clock that ends in a synchronise.
Reported per configuration: median, minimum and spread (p90 - p10) of both clocks in microseconds, and the bytes each arm
reads and writes computed from the shapes (the referenced source rows x full row width as an upper bound on frame bytes).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(360, 640)] * 3 + [(480, 640)] * 2 + [(720, 1280)] * 2 + [(640, 360)]
TV, T, STRIDE, S = 90, 16, 4, 224
OPTS = dict(input_size=[3, S, S], input_space="RGB", input_range=[0, 1], mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])
SWITCHES = dict(random_short_side=(256, 320), random_crop=True, random_hflip=True)


def stats(xs):
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * len(xs)))]
    return {"median_us": round(statistics.median(xs), 1), "min_us": round(xs[0], 1), "spread_p10_p90_us": round(q(0.9) - q(0.1), 1)}


def timed(fn):
    """(device microseconds between two events around the call, host microseconds until a synchronise after it)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0, (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_clips.json"))
    a = ap.parse_args()
    if a.iters < 20:
        raise SystemExit("gpu_sample_clips_bench.py: at least 20 timed calls per arm")
    import pretorched_x_amd as ptx
    TF = ptx.transforms
    dev = torch.device("cuda:0")
    videos = [torch.randint(0, 256, (TV, H, W, 3), dtype=torch.uint8, device=dev) for H, W in SIZES]
    shapes = [(TV, H, W) for H, W in SIZES]
    rows = []
    for clips in (1, 2):
        idx, geo = TF.SampleClips(OPTS, T, STRIDE, clips, generator=torch.Generator().manual_seed(17), **SWITCHES).draw(shapes)
        for out in ("frames", "tensor"):
            sc = TF.SampleClips(OPTS, T, STRIDE, clips, out=out)
            tf = TF.TransformFrames(OPTS, out=out)
            idx_dev = idx.to(dev)

            def arm_a():
                return sc(videos, indices=idx, geometry=geo)

            def arm_b():
                parts = []
                for i, v in enumerate(videos):
                    gathered = v[idx_dev[i * clips:(i + 1) * clips].reshape(-1)].view(clips, T, v.shape[1], v.shape[2], 3)
                    parts.append(tf(gathered, geometry=geo[i * clips:(i + 1) * clips]))
                return torch.cat(parts)

            ya, yb = arm_a(), arm_b()
            torch.cuda.synchronize()
            if not torch.equal(ya, yb):
                raise SystemExit("gpu_sample_clips_bench.py: SampleClips differs from the per-video loop (clips=%d, out=%s)" % (clips, out))
            del ya, yb
            for _ in range(a.warmup):
                arm_a()
                arm_b()
            ta, tb = [], []
            for _ in range(a.iters):                                  # alternating, call by call
                ta.append(timed(arm_a))
                tb.append(timed(arm_b))
            NC = len(videos) * clips
            # bytes from the shapes: a clip's frames are read once (upper bound: whole frames); the loop first copies them
            frame_bytes = sum(clips * T * H * W * 3 for H, W in SIZES)
            out_bytes = NC * T * S * S * 3 * (1 if out == "frames" else 4)
            row = {"clips": clips, "out": out, "output_clips": NC,
                   "sample_clips": {"device": stats([t[0] for t in ta]), "host_sync": stats([t[1] for t in ta]),
                                    "bytes_read": frame_bytes, "bytes_written": out_bytes, "launches": 2},
                   "per_video_loop": {"device": stats([t[0] for t in tb]), "host_sync": stats([t[1] for t in tb]),
                                      "bytes_read": 2 * frame_bytes + out_bytes, "bytes_written": frame_bytes + 2 * out_bytes,
                                      "launches": "per video: gather + builder + resize; one cat"}}
            row["host_sync_ratio_a_over_b"] = round(row["sample_clips"]["host_sync"]["median_us"] /
                                                    row["per_video_loop"]["host_sync"]["median_us"], 3)
            rows.append(row)
            print(json.dumps(row))
    result = {"workload": "8 videos x %d frames (%s), T=%d, frame_stride=%d, S=%d, %s" % (
                  TV, ", ".join("%dx%d" % s for s in SIZES), T, STRIDE, S, sorted(SWITCHES)),
              "iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
              "library": ptx._lib.lib().ptx_version().decode(), "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
