"""Writes tests/golden/rand_augment.npz: inputs, draws and the expected outputs of `pretorched.transforms.RandAugment`.

    python tests/golden/make_rand_augment_golden.py

Only PIL computes the stored pixels: torchvision's RandAugment._apply_op on its PIL-image code path restated in its few lines
(`pil_op`; torchvision is not needed): Image.transform(AFFINE, NEAREST, fillcolor) with F.affine's inverse matrix for the shears
and translations, Image.rotate, ImageEnhance.Brightness / Color / Contrast / Sharpness, ImageOps.posterize / solarize /
autocontrast / equalize.  `transforms.rand_augment_numpy` must reproduce them.

Group "every": 3 clips x 2 different frames of 9 x 11; 24 one-op draws -- every op, the signed ones at both signs, at bin 15 of
31 -- case j running on clip j % 3.  Group "chain2" / "chain4": 2 clips x 2 frames of 32 x 20 with lists of 2 and 4 ops whose
codes differ between the clips at every position, statistics needed by one clip only.  Group "big": one clip x 2 frames of
224 x 224 (several tiles per frame; frame 0 is constant -- one bin holds every pixel --, frame 1 a smooth ramp inside 40..200)
through equalize, autocontrast and contrast.
"""
import math
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from pretorched_x_amd import transforms as TF          # noqa: E402
from pretorched_x_amd.testing import synth_color_frames  # noqa: E402

FILL = (7, 130, 250)
BINS = 31


def magnitude(code, bin_, H, W, negative=False, bins=BINS):
    """The magnitude torchvision takes for op `code` at `bin_` on an H x W image: float(table[bin].item()), negated on demand."""
    table = TF.rand_augment_space(bins, H, W)[code]
    mag = float(table[bin_].item()) if table is not None else 0.0
    return -mag if negative else mag


def inverse_affine(center, translate, shear):
    """torchvision.transforms.functional._get_inverse_affine_matrix with angle 0 and scale 1."""
    rot, sx, sy = 0.0, math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def pil_op(frame, code, mag, fill=FILL):
    """One uint8 [H,W,3] frame through op `code` (TF.RANDAUG_OPS) of signed magnitude `mag`, by PIL alone."""
    img = Image.fromarray(np.ascontiguousarray(frame), "RGB")
    name = TF.RANDAUG_OPS[code]
    W, H = img.size
    affine = lambda m: img.transform(img.size, Image.AFFINE, m, Image.NEAREST, fillcolor=tuple(fill))
    if name == "shear_x":
        img = affine(inverse_affine((0.0, 0.0), (0, 0), (math.degrees(math.atan(mag)), 0.0)))
    elif name == "shear_y":
        img = affine(inverse_affine((0.0, 0.0), (0, 0), (0.0, math.degrees(math.atan(mag)))))
    elif name == "translate_x":
        img = affine(inverse_affine((W * 0.5, H * 0.5), (int(mag), 0), (0.0, 0.0)))
    elif name == "translate_y":
        img = affine(inverse_affine((W * 0.5, H * 0.5), (0, int(mag)), (0.0, 0.0)))
    elif name == "rotate":
        img = img.rotate(mag, Image.NEAREST, fillcolor=tuple(fill))
    elif name == "brightness":
        img = ImageEnhance.Brightness(img).enhance(1.0 + mag)
    elif name == "color":
        img = ImageEnhance.Color(img).enhance(1.0 + mag)
    elif name == "contrast":
        img = ImageEnhance.Contrast(img).enhance(1.0 + mag)
    elif name == "sharpness":
        img = ImageEnhance.Sharpness(img).enhance(1.0 + mag)
    elif name == "posterize":
        img = ImageOps.posterize(img, int(mag))
    elif name == "solarize":
        img = ImageOps.solarize(img, mag)
    elif name == "autocontrast":
        img = ImageOps.autocontrast(img)
    elif name == "equalize":
        img = ImageOps.equalize(img)
    return np.array(img, dtype=np.uint8)


def pil_chain(frame, codes, mags, fill=FILL):
    for code, mag in zip(codes, mags):
        frame = pil_op(frame, int(code), float(mag), fill)
    return frame


def pil_clips(frames, codes, mags, fill=FILL):
    """uint8 [N,T,H,W,3] through the per-clip lists, by PIL alone."""
    return np.stack([np.stack([pil_chain(f, codes[n], mags[n], fill) for f in clip]) for n, clip in enumerate(frames)])


def every_cases(H, W, bin_=15):
    """(codes [24, 1], magnitudes [24, 1]): every op, the signed ones at both signs (identity once more to fill the last launch)."""
    cases = [(c, neg) for c in range(14) for neg in ((False, True) if TF.RANDAUG_SIGNED[c] else (False,))] + [(0, False)]
    return (np.array([[c] for c, _ in cases], np.int32), np.array([[magnitude(c, bin_, H, W, neg)] for c, neg in cases], np.float64))


def chain_params(names, H, W, bin_=12):
    """Per clip a list of (op name, negative): (codes [N, K], magnitudes [N, K])."""
    codes = np.array([[TF.RANDAUG_OPS.index(n) for n, _ in clip] for clip in names], np.int32)
    mags = np.array([[magnitude(TF.RANDAUG_OPS.index(n), bin_, H, W, neg) for n, neg in clip] for clip in names], np.float64)
    return codes, mags


CHAIN2 = [[("rotate", False), ("contrast", True)], [("autocontrast", False), ("posterize", False)]]
CHAIN4 = [[("translate_y", True), ("equalize", False), ("sharpness", False), ("solarize", False)],
          [("color", False), ("shear_y", True), ("autocontrast", False), ("rotate", True)]]


def big_frames():
    y, x = np.mgrid[0:224, 0:224]
    ramp = np.stack([40 + (x * 160) // 223, 60 + (y * 120) // 223, 200 - ((x + y) * 150) // 446], -1).astype(np.uint8)
    const = np.empty((224, 224, 3), np.uint8)
    const[...] = (90, 17, 201)
    return np.stack([const, ramp])[None]


def main():
    blob = {}
    frames = synth_color_frames(3, 2, 9, 11, 5201)
    codes, mags = every_cases(9, 11)
    out = np.concatenate([pil_clips(frames[j % 3:j % 3 + 1], codes[j:j + 1], mags[j:j + 1]) for j in range(len(codes))])
    got = np.concatenate([TF.rand_augment_numpy(frames[j % 3:j % 3 + 1], (codes[j:j + 1], mags[j:j + 1]), FILL) for j in range(len(codes))])
    assert np.array_equal(got, out)
    assert sorted(set(codes[:, 0].tolist())) == list(range(14)) and len(codes) == 24 and not np.array_equal(frames[0, 0], frames[0, 1])
    blob.update(every_in=frames, every_codes=codes, every_mags=mags, every_out=out)
    frames = synth_color_frames(2, 2, 32, 20, 5202)
    for group, names in (("chain2", CHAIN2), ("chain4", CHAIN4)):
        codes, mags = chain_params(names, 32, 20)
        out = pil_clips(frames, codes, mags)
        assert np.array_equal(TF.rand_augment_numpy(frames, (codes, mags), FILL), out), group
        assert (codes[0] != codes[1]).all()
        blob.update({group + "_in": frames, group + "_codes": codes, group + "_mags": mags, group + "_out": out})
    frames = big_frames()
    codes = np.array([[13], [12], [8]], np.int32)
    mags = np.array([[0.0], [0.0], [magnitude(8, 20, 224, 224)]], np.float64)
    out = np.concatenate([pil_clips(frames, codes[j:j + 1], mags[j:j + 1]) for j in range(3)])
    got = np.concatenate([TF.rand_augment_numpy(frames, (codes[j:j + 1], mags[j:j + 1]), FILL) for j in range(3)])
    assert np.array_equal(got, out) and not np.array_equal(out[0, 1], frames[0, 1]) and np.array_equal(out[0, 0], frames[0, 0])
    blob.update(big_in=frames, big_codes=codes, big_mags=mags, big_out=out)
    blob["fill"] = np.array(FILL, np.int32)
    path = os.path.join(HERE, "rand_augment.npz")
    np.savez_compressed(path, **blob)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
