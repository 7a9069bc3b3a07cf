"""Pillow as the oracle of the interpolated warps (include/ptx_amd_warp.h), shared by tests/test_warp_frames_host.py and
tests/test_gpu_warp_frames.py: Image.transform / Image.rotate per frame, the fixed coefficient sets, seeded random ones, and
RandAugment's ops with an interpolation.  Not a test module."""
import math
import os
import sys

import numpy as np
from PIL import Image

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_rand_augment_golden as MG                    # noqa: E402   (PIL's enhancement / LUT ops, inverse_affine)

RESAMPLE = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
IDENTITY, AFFINE, PERSPECTIVE = 0, 1, 2
SIZES = [(1, 1), (2, 3), (9, 11), (33, 65)]
FILL = (7, 130, 250)
ROTATIONS = (17.0, -29.5, 0.0, 90.0, 180.0, 270.0)


def pil_warp(frame, kind, a, interpolation, fill=FILL):
    """One uint8 [H,W,3] frame through Image.transform with the eight coefficients `a` of a clip of `kind`."""
    if kind == IDENTITY:
        return np.array(frame, dtype=np.uint8)
    img = Image.fromarray(np.ascontiguousarray(frame), "RGB")
    data = [float(v) for v in (a[:6] if kind == AFFINE else a)]
    out = img.transform(img.size, Image.AFFINE if kind == AFFINE else Image.PERSPECTIVE, data, RESAMPLE[interpolation], fillcolor=tuple(fill))
    return np.array(out, dtype=np.uint8)


def pil_warp_clips(frames, kinds, coeffs, interpolation, fill=FILL):
    """uint8 [N,T,H,W,3] through the per-clip kinds and coefficients, by PIL alone."""
    return np.stack([np.stack([pil_warp(f, int(kinds[n]), list(coeffs[n]), interpolation, fill) for f in clip]) for n, clip in enumerate(frames)])


def pil_rotate(frame, angle, interpolation, fill=FILL, center=None):
    img = Image.fromarray(np.ascontiguousarray(frame), "RGB")
    return np.array(img.rotate(angle, RESAMPLE[interpolation], center=center, fillcolor=tuple(fill)), dtype=np.uint8)


def fixed_affine(H, W):
    """[(name, a0 .. a5)]: identity, integer and half-pixel translations, a translation beyond the frame, scales, a shear."""
    return [("identity", [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]),
            ("translate +2 -1", [1.0, 0.0, 2.0, 0.0, 1.0, -1.0]),
            ("translate -3 +2", [1.0, 0.0, -3.0, 0.0, 1.0, 2.0]),
            ("translate half", [1.0, 0.0, 0.5, 0.0, 1.0, 0.5]),
            ("translate -half", [1.0, 0.0, -0.5, 0.0, 1.0, 1.5]),
            ("beyond", [1.0, 0.0, float(W + 5), 0.0, 1.0, 0.0]),
            ("scale 0.35", [0.35, 0.0, 0.0, 0.0, 0.35, 0.0]),
            ("scale 3.0", [3.0, 0.0, -float(W), 0.0, 3.0, -float(H)]),
            ("shear 0.3", [1.0, 0.3, 0.0, 0.0, 1.0, 0.0])]


def strong_perspective(H, W):
    """A perspective whose denominator runs from about 0.5 (bottom left) to about 1.5 (top right)."""
    return [1.1, 0.05, -0.04 * W, -0.03, 0.9, 0.06 * H, 0.5 / W, -0.5 / H]


def random_coeffs(rng, kind, H, W):
    """A seeded coefficient set: a rotation-scale-shear about anywhere near the frame, and for a perspective a denominator
    that keeps its sign on the frame."""
    ang, s = rng.uniform(-math.pi, math.pi), rng.uniform(0.3, 3.0)
    a = [s * math.cos(ang), -s * math.sin(ang) + rng.uniform(-0.3, 0.3), rng.uniform(-W, W),
         s * math.sin(ang), s * math.cos(ang), rng.uniform(-H, H), 0.0, 0.0]
    if kind == PERSPECTIVE:
        a[6], a[7] = rng.uniform(-0.45, 0.45) / W, rng.uniform(-0.45, 0.45) / H
    return a


def pil_randaug_op(frame, code, mag, interpolation, fill=FILL):
    """One frame through RandAugment op `code` as torchvision runs it on a PIL image with `interpolation`."""
    if not 1 <= code <= 5:
        return MG.pil_op(frame, code, mag, fill)
    img = Image.fromarray(np.ascontiguousarray(frame), "RGB")
    W, H = img.size
    if code == 5:
        return np.array(img.rotate(mag, RESAMPLE[interpolation], fillcolor=tuple(fill)), dtype=np.uint8)
    m = {1: lambda: MG.inverse_affine((0.0, 0.0), (0, 0), (math.degrees(math.atan(mag)), 0.0)),
         2: lambda: MG.inverse_affine((0.0, 0.0), (0, 0), (0.0, math.degrees(math.atan(mag)))),
         3: lambda: MG.inverse_affine((W * 0.5, H * 0.5), (int(mag), 0), (0.0, 0.0)),
         4: lambda: MG.inverse_affine((W * 0.5, H * 0.5), (0, int(mag)), (0.0, 0.0))}[code]()
    return np.array(img.transform(img.size, Image.AFFINE, m, RESAMPLE[interpolation], fillcolor=tuple(fill)), dtype=np.uint8)


def pil_randaug_clips(frames, codes, mags, interpolation, fill=FILL):
    out = np.empty_like(frames)
    for n, clip in enumerate(frames):
        for t, f in enumerate(clip):
            for code, mag in zip(codes[n], mags[n]):
                f = pil_randaug_op(f, int(code), float(mag), interpolation, fill)
            out[n, t] = f
    return out


# RandAugment draws of three ops on two clips that, together, hold every geometric op at both signs next to enhancement and LUT
# ops; set 0 has a position where both clips are geometric (the apply launch there only copies and is skipped), set 3 one
# whose LAST position is geometric on both clips (the apply launch writes the output from identity rows).
RANDAUG_SETS = [
    (np.array([[1, 6, 5], [2, 13, 3]], np.int32), np.array([[0.2, 0.3, -20.0], [-0.2, 0.0, 7.0]])),
    (np.array([[12, 1, 9], [8, 4, 0]], np.int32), np.array([[0.0, -0.2, 0.5], [0.4, 6.0, 0.0]])),
    (np.array([[3, 2, 10], [11, 7, 5]], np.int32), np.array([[-7.0, 0.2, 5.0], [128.0, -0.4, 20.0]])),
    (np.array([[6, 0, 4], [13, 12, 2]], np.int32), np.array([[-0.3, 0.0, -6.0], [0.0, 0.0, 0.25]])),
]


def randaug_launches(codes):
    """The launches RandAugment lists for `codes` [N, K] with an interpolated filter."""
    geo, stats, out = np.isin(codes, range(1, 6)), np.isin(codes, (8, 12, 13)), []
    K = codes.shape[1]
    for k in range(K):
        if geo[:, k].any():
            out.append("warp")
            if k < K - 1 and not (codes[:, k][~geo[:, k]] != 0).any():
                continue
        if stats[:, k].any():
            out.append("stats")
        out.append("apply")
    return tuple(out)
