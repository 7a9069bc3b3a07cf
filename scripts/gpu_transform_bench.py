"""ptx_resize_frames_u8 (resize + crop of uint8 frames, `pretorched.transforms.TransformFrames`) timed with HIP events.

    python scripts/gpu_transform_bench.py [--iters 50] [--warmup 10] [--out profiles/transform_frames.json]

Per case (8 clips x 16 frames of 256x340 [crop only], 360x640, 720x1280, 1080x1920 -> resize to short side 256, centre
crop 224; uint8 and fp32 outputs): microseconds per launch, the bytes the launch has to move (read: the input window the
tables reference, once; written: the output), GB/s, and that rate as a fraction of the 6.29 TB/s a float4 copy reaches on
an MI355X.  End to end on resnet3d50, 8 x 16 frames: `forward_frames` on pre-cropped 224x224 frames against
`forward_frames(360x640 frames, transform=tf)` in the same process.  For context, the host's PIL time per frame (one core).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(256, 340), (360, 640), (720, 1280), (1080, 1920)]
CLIPS, FRAMES = 8, 16
COPY_TBPS = 6.29
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


def kernel_rows(a, ptx):
    from pretorched_x_amd import _lib as L
    TF = ptx.transforms
    lib, dev = L.lib(), torch.device("cuda:0")
    norm = L.NormDesc.make(OPTS["mean"], OPTS["std"], OPTS["input_space"], OPTS["input_range"])
    rows = []
    for H, W in SIZES:
        t = TF.build_tables(H, W, OPTS["input_size"])
        S = t["S"]
        (rlo, rn, _), (clo, cn, _) = t["rows"], t["cols"]
        win_rows = int((rlo + rn).max() - rlo.min())
        win_cols = int((clo + cn).max() - clo.min())
        frames = torch.randint(0, 256, (CLIPS, FRAMES, H, W, 3), dtype=torch.uint8, device=dev)
        tabs = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in t["rows"] + t["cols"]]
        for mode, name, width in ((L.PTX_RESIZE_OUT_U8, "uint8", 1), (L.PTX_RESIZE_OUT_F32, "fp32", 4)):
            y = torch.empty(CLIPS * FRAMES * S * S * 3 * width, dtype=torch.uint8, device=dev)
            desc = L.ResizeDesc(CLIPS, FRAMES, H, W, 3, S, S, t["rows"][2].shape[1], t["cols"][2].shape[1], mode)
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def launch():
                L.check(lib.ptx_resize_frames_u8(C.byref(desc), C.c_void_p(frames.data_ptr()),
                                                 *[C.c_void_p(x.data_ptr()) for x in tabs], C.c_void_p(y.data_ptr()),
                                                 C.byref(norm), st), "ptx_resize_frames_u8")
            us = _time(launch, a.iters, a.warmup)
            rd = CLIPS * FRAMES * win_rows * win_cols * 3
            wr = CLIPS * FRAMES * S * S * 3 * width
            gbs = (rd + wr) / us / 1e3
            rows.append({"case": "%dx%d" % (H, W), "out": name, "frames": CLIPS * FRAMES, "resized": list(t["resized"]),
                         "taps_h": int(desc.taps_h), "taps_w": int(desc.taps_w), "window": [win_rows, win_cols],
                         "kernel_us": round(us, 1), "bytes_read": rd, "bytes_written": wr, "gb_per_s": round(gbs, 1),
                         "fraction_of_copy_rate": round(gbs / (COPY_TBPS * 1e3), 4),
                         "frames_per_s": round(CLIPS * FRAMES / us * 1e6)})
            print(json.dumps(rows[-1]), flush=True)
        del frames
    return rows


def end_to_end(a, ptx):
    from pretorched_x_amd.testing import synth_state_dict
    TF, dev = ptx.transforms, torch.device("cuda:0")
    model = ptx.__dict__["resnet3d50"](num_classes=339, pretrained=None)
    model.load_state_dict(synth_state_dict(model.state_dict(), 1234))
    model = model.to(dev).eval()
    tf = TF.TransformFrames(OPTS, out="frames")
    big = torch.randint(0, 256, (CLIPS, FRAMES, 360, 640, 3), dtype=torch.uint8, device=dev)
    crop = tf(big)
    with torch.no_grad():
        same = torch.equal(model.forward_frames(crop, OPTS), model.forward_frames(big, OPTS, transform=tf))
        us_crop = us_big = 0.0
        for _ in range(3):                               # alternate the two arms
            us_crop += _time(lambda: model.forward_frames(crop, OPTS), a.iters, a.warmup) / 3
            us_big += _time(lambda: model.forward_frames(big, OPTS, transform=tf), a.iters, a.warmup) / 3
    row = {"model": "resnet3d50", "clips": CLIPS, "frames": FRAMES, "precropped_224_ms": round(us_crop / 1e3, 3),
           "raw_360x640_with_transform_ms": round(us_big / 1e3, 3), "ratio": round(us_big / us_crop, 4),
           "logits_equal": bool(same)}
    print(json.dumps(row), flush=True)
    return row


def host_pil():
    try:
        from PIL import Image
    except ImportError:
        return None
    import pretorched_x_amd as ptx
    out = {}
    rs = np.random.RandomState(0)
    for H, W in SIZES:
        t = ptx.transforms.build_tables(H, W, OPTS["input_size"])
        (h, w), (top, left) = t["resized"], t["window"]
        frames = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(8)]
        t0 = time.perf_counter()
        for f in frames:
            img = Image.fromarray(f)
            if (h, w) != (H, W):
                img = img.resize((w, h), Image.BILINEAR)
            np.asarray(img.crop((left, top, left + 224, top + 224)))
        out["%dx%d" % (H, W)] = round((time.perf_counter() - t0) / len(frames) * 1e3, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_transform_bench.py needs a GPU: timings from anything else mean nothing")
    import pretorched_x_amd as ptx
    result = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "copy_rate_tb_per_s": COPY_TBPS,
              "kernel": kernel_rows(a, ptx), "end_to_end": None if a.skip_model else end_to_end(a, ptx),
              "host_pil_ms_per_frame_one_core": host_pil()}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
