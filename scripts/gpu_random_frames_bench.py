"""Per-clip crop windows and flips (`TransformFrames(random_crop=.., random_hflip=.., random_vflip=..)`,
ptx_resize_frames_u8_windows) timed with HIP events against the fixed-window launch.

    python scripts/gpu_random_frames_bench.py [--iters 100] [--warmup 20] [--rounds 3] [--out profiles/random_frames.json]

Per shape (8 clips x 16 frames of 360x640 and 720x1280 -> short side 256, 224x224 windows, uint8 out), microseconds per
call, each the median over `rounds` x `iters` calls timed one by one with device events, the three arms alternating round
by round:
  (a) fixed_window_us     ptx_resize_frames_u8 with the centre window's tables: the existing launch
  (b) windows_us          ptx_resize_frames_u8_windows with eight distinct drawn windows and flips: the new launch
  (c) per_clip_loop_us    what a user did before: one cached TransformFrames(crop=..) call per clip (eight launches), a
                          torch flip for the clips that are flipped, written into one output batch
(b) must equal the per-clip fixed-window launches bit for bit at the timed shapes; the script checks it before it times.
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


def shape_row(a, ptx, H, W):
    from pretorched_x_amd import _lib as L
    TF = ptx.transforms
    lib, dev = L.lib(), torch.device("cuda:0")
    frames = torch.randint(0, 256, (CLIPS, FRAMES, H, W, 3), dtype=torch.uint8, device=dev)
    S = max(OPTS["input_size"])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    up = lambda t: [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in tuple(t["rows"]) + tuple(t["cols"])]

    # (a) the fixed centre window
    fixed = TF.build_tables(H, W, OPTS["input_size"])
    ftabs = up(fixed)
    fdesc = L.ResizeDesc(CLIPS, FRAMES, H, W, 3, S, S, fixed["rows"][2].shape[1], fixed["cols"][2].shape[1], L.PTX_RESIZE_OUT_U8)
    ya = torch.empty((CLIPS, FRAMES, S, S, 3), dtype=torch.uint8, device=dev)

    def arm_a():
        L.check(lib.ptx_resize_frames_u8(C.byref(fdesc), C.c_void_p(frames.data_ptr()), *[C.c_void_p(x.data_ptr()) for x in ftabs],
                                         C.c_void_p(ya.data_ptr()), None, st), "ptx_resize_frames_u8")

    # (b) eight distinct drawn windows and flips, one launch
    rt = TF.TransformFrames(OPTS, out="frames", random_crop=True, random_hflip=True, random_vflip=True,
                            generator=torch.Generator().manual_seed(5))
    params = rt.draw(CLIPS, H, W)
    assert len(set(map(tuple, params[:, :2].tolist()))) == CLIPS, "the drawn windows are not distinct: pick another seed"
    assert set(params[:, 2].tolist()) == {0, 1} and set(params[:, 3].tolist()) == {0, 1}
    full = rt.frame_tables(H, W)
    h, w = full["resized"]
    wtabs = up(full)
    wdesc = L.ResizeDesc(CLIPS, FRAMES, H, W, 3, S, S, full["rows"][2].shape[1], full["cols"][2].shape[1], L.PTX_RESIZE_OUT_U8)
    wins = params.to(dev)
    yb = torch.empty((CLIPS, FRAMES, S, S, 3), dtype=torch.uint8, device=dev)

    def arm_b():
        L.check(lib.ptx_resize_frames_u8_windows(C.byref(wdesc), C.c_void_p(frames.data_ptr()),
                                                 *[C.c_void_p(x.data_ptr()) for x in wtabs], h, w, C.c_void_p(wins.data_ptr()),
                                                 C.c_void_p(yb.data_ptr()), None, st), "ptx_resize_frames_u8_windows")

    # (c) one cached TransformFrames per clip, flips in torch
    per_clip = [(TF.TransformFrames(OPTS, out="frames", crop=(top, left)), hf, vf) for top, left, hf, vf in params.tolist()]
    yc = torch.empty((CLIPS, FRAMES, S, S, 3), dtype=torch.uint8, device=dev)

    def arm_c():
        for n, (tf, hf, vf) in enumerate(per_clip):
            out = tf(frames[n])
            dims = ([-2] if hf else []) + ([-3] if vf else [])
            yc[n].copy_(out.flip(dims) if dims else out)

    arm_b()
    arm_c()
    torch.cuda.synchronize()
    equal = bool(torch.equal(yb, yc))
    for n, (top, left, hf, vf) in enumerate(params.tolist()):            # and the fixed-window launch with folded flips
        one = TF.TransformFrames(OPTS, out="frames", crop=(top, left), hflip=bool(hf), vflip=bool(vf))(frames[n])
        equal = equal and bool(torch.equal(one, yb[n]))
    if not equal:
        raise SystemExit("gpu_random_frames_bench.py: the windows launch differs from the per-clip launches at %dx%d" % (H, W))

    samples = {"a": [], "b": [], "c": []}
    for _ in range(a.rounds):                                            # alternate the arms
        for key, fn in (("a", arm_a), ("b", arm_b), ("c", arm_c)):
            samples[key] += _times(fn, a.iters, a.warmup)
    med = {k: statistics.median(v) for k, v in samples.items()}
    p10 = {k: sorted(v)[len(v) // 10] for k, v in samples.items()}
    p90 = {k: sorted(v)[len(v) * 9 // 10] for k, v in samples.items()}
    row = {"case": "%dx%d" % (H, W), "clips": CLIPS, "frames_per_clip": FRAMES, "resized": [int(h), int(w)],
           "taps_h": int(wdesc.taps_h), "taps_w": int(wdesc.taps_w), "params": params.tolist(),
           "samples_per_arm": len(samples["a"]), "bit_identical_to_per_clip_launches": equal,
           "fixed_window_us": round(med["a"], 1), "windows_us": round(med["b"], 1), "per_clip_loop_us": round(med["c"], 1),
           "p10_us": {k: round(v, 1) for k, v in p10.items()}, "p90_us": {k: round(v, 1) for k, v in p90.items()},
           "windows_over_fixed": round(med["b"] / med["a"], 4), "loop_over_windows": round(med["c"] / med["b"], 3)}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_random_frames_bench.py needs a GPU: timings from anything else mean nothing")
    if a.iters * a.rounds < 100:
        raise SystemExit("gpu_random_frames_bench.py: a median wants at least 100 launches per arm")
    import pretorched_x_amd as ptx
    result = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds,
              "out": "uint8", "shapes": [shape_row(a, ptx, H, W) for H, W in SIZES]}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
