"""Deterministic synthetic weights and inputs (there is no network for checkpoints/datasets).

The recipe is the calibrated one of SURVEY.md section 8(d): default-initialised BatchNorms are the
identity and the non-local block's output BN is all-zero (reference nonlocalnet.py:95-96), so a
parity check on default-init weights would be vacuous for BN folding and for the whole NL branch.
Every tensor is drawn from its own CPU generator seeded by (seed, crc32(key)), so the values
depend only on the state_dict key and shape -- not on module construction order -- and the same
function feeds the reference model (golden generation), the oracle and the HIP engine.
"""
import zlib
from collections import OrderedDict

import torch

# gamma of the BN that closes a residual branch is damped so that logits stay O(10) deep into
# the network (factor 0.8 -> max|logit| ~ 26 for resnet3d50).
LAST_BN_DAMP = 0.8
# the non-local branch re-injects a full-width signal after the block's ReLU; its output BN
# (`W.1`) is damped harder so NL networks stay in the same logit range (calibrated: ~10-30)
NL_BN_DAMP = 0.2


# I3D (Inception stacks, no residual paths): fan_in filters + mildly damped Unit3D BNs keep
# max|logit| ~ 16 at 16x224x224 with an fp32 noise floor of ~6e-6 (calibrated in round 1)
I3D_RECIPE = dict(unit_bn_damp=0.9, conv_fan="in")


# BigGAN-deep generator (pre-activation residual stack, no BN after the closing convs): fan_in filters,
# closing convs x0.2 -> pre-tanh std ~0.9, max ~4 at 256x256, fp32 noise floor ~4e-6
BIGGAN_RECIPE = dict(conv_fan="in", closing_conv_damp=0.2)


def _gen(seed, key):
    g = torch.Generator()
    g.manual_seed((int(seed) * 1000003 + zlib.crc32(key.encode())) & 0x7FFFFFFF)
    return g


def _is_closing_bn(prefix, keys):
    if prefix.endswith(".bn3") or prefix.endswith("downsample.1"):
        return True
    if prefix.endswith(".bn2"):
        parent = prefix.rsplit(".", 1)[0]
        return (parent + ".bn3.weight") not in keys
    return False


def synth_state_dict(template, seed=1234, last_bn_damp=LAST_BN_DAMP, nl_bn_damp=NL_BN_DAMP, inner_bn_damp=1.0,
                     unit_bn_damp=1.0, conv_fan="out", closing_conv_damp=1.0, nl_embed_damp=1.0):
    """template: mapping key -> tensor (only shape/dtype are used). Returns an OrderedDict of
    fresh CPU fp32 tensors with the same keys/shapes.

    The damping factors scale BN gammas so that logits of deep random-weight networks stay in the
    calibrated 10-30 range (SURVEY.md 8d "re-calibrate per model"): `last_bn_damp` for the BN that
    closes a residual branch, `nl_bn_damp` for the non-local block's output BN (`W.1`),
    `inner_bn_damp` for the BN inside a (2+1)D factored conv pair (`*.bn`), `unit_bn_damp` for the BN
    of an I3D Unit3D (`*.bn` next to `*.conv3d`).  `conv_fan`: 'out' = the reference's kaiming-normal
    fan_out (resnet3D.py:198); 'in' = fan_in, for Inception stacks whose 1x1x1 reductions (192 -> 16)
    would otherwise amplify 2*Cin/Cout per layer; `closing_conv_damp` scales the filters
    that close a BigGAN-deep residual branch (`conv4`, attention `o`), which has no BN after them;
    `nl_embed_damp` scales the non-local block's theta / phi embeddings (weights and biases): the softmax input
    theta^T phi grows with the SQUARE of the activation scale, and with kaiming filters it reaches 1e2 ... 1e4 in a
    random-weight network -- a hard arg-max whose winner flips under fp32 rounding (round 4: the reference's own CPU
    forward then differs from its fp64 self by 1e-2 relative).  damp^2 brings the affinities back to the O(1-30) range of
    a trained network, so the NL branch can be tested at FULL strength (`nl_bn_damp` = 1).  Fixtures record the values
    they were generated with."""
    keys = set(template.keys())
    out = OrderedDict()

    def embed_damp(key):
        # a float, or {key prefix: factor} (activations grow with depth, and the affinities with their square)
        if isinstance(nl_embed_damp, dict):
            return next((float(v) for k, v in nl_embed_damp.items() if key.startswith(k)), 1.0)
        return float(nl_embed_damp)

    for key, ref in template.items():
        shape = tuple(ref.shape)
        g = _gen(seed, key)
        prefix, _, leaf = key.rpartition(".")
        is_bn = (prefix + ".running_mean") in keys
        if leaf == "num_batches_tracked":
            out[key] = torch.zeros(shape, dtype=torch.long)
        elif is_bn and leaf == "weight":
            v = torch.rand(shape, generator=g) + 0.5
            if prefix.endswith(".W.1"):
                v = v * nl_bn_damp
            elif prefix.endswith(".bn") and (prefix[:-3] + ".spatial_conv.weight") in keys:
                v = v * inner_bn_damp
            elif prefix.endswith(".bn") and (prefix[:-3] + ".conv3d.weight") in keys:
                v = v * unit_bn_damp
            elif _is_closing_bn(prefix, keys):
                v = v * last_bn_damp
            out[key] = v
        elif is_bn and leaf == "bias":
            out[key] = torch.randn(shape, generator=g) * 0.1
        elif leaf in ("running_mean", "stored_mean"):
            out[key] = torch.randn(shape, generator=g) * 0.1
        elif leaf in ("running_var", "stored_var"):
            out[key] = torch.rand(shape, generator=g) + 0.5
        elif leaf == "gain":                                # BigGAN's plain output BN: gamma
            out[key] = torch.rand(shape, generator=g) + 0.5
        elif leaf == "gamma":                               # attention mixing scalar (init 0 upstream)
            out[key] = torch.full(shape, 0.5)
        elif leaf == "weight" and len(shape) >= 3:          # conv: kaiming-normal, fan_out
            fan = shape[0] if conv_fan == "out" else shape[1]
            for k in shape[2:]:
                fan *= k
            out[key] = torch.randn(shape, generator=g) * (2.0 / fan) ** 0.5
            if prefix.endswith(".conv4") or prefix.endswith(".o"):      # closes a BigGAN residual / attention branch
                out[key] = out[key] * closing_conv_damp
            if ".nonlocalblock." in key and (prefix.endswith(".theta") or prefix.endswith(".phi") or prefix.endswith(".phi.0")):
                out[key] = out[key] * embed_damp(key)
        elif leaf == "weight" and shape == (1, 3) and prefix.endswith(".linear") and (prefix[:-7] + ".weight") in keys:
            # MultiViewConv's view-mixing Linear(3, 1) (multiview.py:50): positive weights with sum of squares ~ 1, so the
            # three-view sum keeps the signal scale of a plain conv (default Linear init would shrink it 0.58x per layer)
            out[key] = torch.rand(shape, generator=g) * 0.6 + 0.3
        elif leaf == "weight" and len(shape) == 2:          # linear
            bound = 1.0 / shape[1] ** 0.5
            out[key] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        elif leaf == "bias":                                # conv / linear bias
            out[key] = (torch.rand(shape, generator=g) * 2 - 1) * 0.05
            if ".nonlocalblock." in key and (prefix.endswith(".theta") or prefix.endswith(".phi") or prefix.endswith(".phi.0")):
                out[key] = out[key] * embed_damp(key)
        else:
            raise KeyError("synth_state_dict: unclassified key %r" % key)
    return out


def synth_clips(batch, frames, size, seed=99, channels=3):
    """Synthetic normalised video clips, NCDHW fp32, from a seeded CPU generator."""
    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.randn(batch, channels, frames, size, size, generator=g)


def synth_yuv420(count, height, width, seed, content="noise"):
    """Synthetic decoder output: uint8 numpy planes (y [count,H,W], u, v [count,ceil(H/2),ceil(W/2)]).  "noise": seeded
    bytes from numpy's legacy generator in all three planes (independent chroma noise drives many pixels out of gamut,
    so both ends of the conversion's clamp are exercised); "extremes": constant frames cycling through (Y, Cb, Cr) =
    (255, 255, 255), (0, 0, 0), (16, 240, 16)."""
    import numpy as np
    hc, wc = (height + 1) // 2, (width + 1) // 2
    if content == "extremes":
        triples = [(255, 255, 255), (0, 0, 0), (16, 240, 16)]
        pick = [triples[i % 3] for i in range(count)]
        return tuple(np.stack([np.full(shape, t[k], np.uint8) for t in pick])
                     for k, shape in enumerate(((height, width), (hc, wc), (hc, wc))))
    if content != "noise":
        raise ValueError("synth_yuv420: content must be 'noise' or 'extremes'")
    rs = np.random.RandomState(int(seed))
    y = rs.randint(0, 256, (count, height, width)).astype(np.uint8)
    u = rs.randint(0, 256, (count, hc, wc)).astype(np.uint8)
    v = rs.randint(0, 256, (count, hc, wc)).astype(np.uint8)
    return y, u, v


def yuv420_source(planes, layout, device, matrix="bt709", color_range="limited", lead_shape=None):
    """A `transforms.YUV420` over numpy planes (y, u, v as `synth_yuv420` returns them) in one of the memory layouts a
    decoder produces: "nv12" / "i420" (packed frames, even sizes), "planes" (y, u, v tensors), "planes_uv" (y and an
    interleaved uv plane), "nv12_pitched" (y and uv are views into wider buffers: row pitch W + 14 / 2 * ceil(W/2) + 6
    bytes, base pointers 1 and 3 bytes past the allocation).  lead_shape: reshape the leading [count] to it."""
    import numpy as np
    import torch
    from .transforms import YUV420
    y, u, v = (np.ascontiguousarray(a) for a in planes)
    count, H, W = y.shape
    hc, wc = u.shape[1:]
    lead = (count,) if lead_shape is None else tuple(lead_shape)
    kw = dict(matrix=matrix, color_range=color_range)
    uv = np.stack([u, v], -1)                                       # [count, hc, wc, 2]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if layout == "nv12":
        return YUV420.from_nv12(dev(np.concatenate([y, uv.reshape(count, hc, W)], 1)).view(lead + (H * 3 // 2, W)), **kw)
    if layout == "i420":
        packed = np.concatenate([y.reshape(count, -1), u.reshape(count, -1), v.reshape(count, -1)], 1)
        return YUV420.from_i420(dev(packed).view(lead + (H * 3 // 2, W)), **kw)
    if layout == "planes":
        return YUV420(dev(y).view(lead + (H, W)), dev(u).view(lead + (hc, wc)), dev(v).view(lead + (hc, wc)), **kw)
    if layout == "planes_uv":
        return YUV420(dev(y).view(lead + (H, W)), dev(uv).view(lead + (hc, wc, 2)), **kw)
    if layout == "nv12_pitched":
        py, pc = W + 14, 2 * wc + 6
        by = torch.zeros(count * H * py + 1, dtype=torch.uint8, device=device)
        bc = torch.zeros(count * hc * pc + 3, dtype=torch.uint8, device=device)
        ty = by[1:].view(lead + (H, py))[..., :W]
        tc = bc[3:].view(lead + (hc, pc))[..., :2 * wc].unflatten(-1, (wc, 2))
        ty.copy_(dev(y).view(lead + (H, W)))
        tc.copy_(dev(uv).view(lead + (hc, wc, 2)))
        return YUV420(ty, tc, **kw)
    raise ValueError("yuv420_source: unknown layout %r" % (layout,))


def synth_yuv420p16(count, height, width, seed, bits=10, align="msb", content="noise"):
    """Synthetic 10- / 12-bit decoder output: uint16 numpy planes shaped as `synth_yuv420`'s, the sample MSB- or
    LSB-aligned in its word and seeded garbage in the bits the contract ignores (the low 16 - bits of an "msb" word, the
    high ones of an "lsb" word).  "noise": seeded samples over the whole range in all three planes; "extremes": constant
    frames cycling through (Y, Cb, Cr) = all ones, all zeros and limited-range (16, 240, 16) << (bits - 8)."""
    import numpy as np
    hc, wc = (height + 1) // 2, (width + 1) // 2
    top, d = (1 << bits) - 1, bits - 8
    shapes = ((count, height, width), (count, hc, wc), (count, hc, wc))
    rs = np.random.RandomState(int(seed))
    if content == "extremes":
        triples = [(top, top, top), (0, 0, 0), (16 << d, 240 << d, 16 << d)]
        planes = [np.stack([np.full(shape[1:], triples[i % 3][k], np.int64) for i in range(count)]) for k, shape in enumerate(shapes)]
    elif content == "noise":
        planes = [rs.randint(0, top + 1, shape).astype(np.int64) for shape in shapes]
    else:
        raise ValueError("synth_yuv420p16: content must be 'noise' or 'extremes'")
    out = []
    for p in planes:
        junk = rs.randint(0, 1 << (16 - bits), p.shape).astype(np.int64)
        out.append(((p << (16 - bits)) | junk if align == "msb" else p | (junk << bits)).astype(np.uint16))
    return tuple(out)


def yuv420p16_source(planes, layout, device, bits=10, align="msb", matrix="bt709", color_range="limited", lead_shape=None):
    """A `transforms.YUV420P16` over numpy planes (as `synth_yuv420p16` returns them) in one of the memory layouts a
    decoder produces: "p010" (packed, interleaved chroma, MSB-aligned words, even sizes), "i420p16" (packed planar,
    LSB-aligned words, even sizes), "planes" (y, u, v tensors), "planes_uv" (y and an interleaved uv plane), "p010_pitched"
    (y and uv are views into wider buffers: row pitch 2 * (W + 7) / 2 * (2 * ceil(W/2) + 3) bytes, base pointers 2 and 6
    bytes past the allocation).  align must be what the packed layouts imply; lead_shape: reshape the leading [count] to it."""
    import numpy as np
    import torch
    from .transforms import YUV420P16
    y, u, v = (np.ascontiguousarray(a).view(np.int16) for a in planes)
    count, H, W = y.shape
    hc, wc = u.shape[1:]
    lead = (count,) if lead_shape is None else tuple(lead_shape)
    kw = dict(matrix=matrix, color_range=color_range)
    uv = np.stack([u, v], -1)                                       # [count, hc, wc, 2]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    implied = {"p010": "msb", "p010_pitched": "msb", "i420p16": "lsb"}.get(layout, align)
    if implied != align:
        raise ValueError("yuv420p16_source: layout %r holds %s-aligned samples" % (layout, implied))
    if layout == "p010":
        return YUV420P16.from_p010(dev(np.concatenate([y, uv.reshape(count, hc, W)], 1)).view(lead + (H * 3 // 2, W)), bits, **kw)
    if layout == "i420p16":
        packed = np.concatenate([y.reshape(count, -1), u.reshape(count, -1), v.reshape(count, -1)], 1)
        return YUV420P16.from_i420p16(dev(packed).view(lead + (H * 3 // 2, W)), bits, **kw)
    if layout == "planes":
        return YUV420P16(dev(y).view(lead + (H, W)), dev(u).view(lead + (hc, wc)), dev(v).view(lead + (hc, wc)), bits, align, **kw)
    if layout == "planes_uv":
        return YUV420P16(dev(y).view(lead + (H, W)), dev(uv).view(lead + (hc, wc, 2)), None, bits, align, **kw)
    if layout == "p010_pitched":
        py, pc = W + 7, 2 * wc + 3                                   # words: 2 W + 14 and 4 wc + 6 bytes, no multiple of 16
        by = torch.zeros(count * H * py + 1, dtype=torch.int16, device=device)
        bc = torch.zeros(count * hc * pc + 3, dtype=torch.int16, device=device)
        ty = by[1:].view(lead + (H, py))[..., :W]
        tc = bc[3:].view(lead + (hc, pc))[..., :2 * wc].unflatten(-1, (wc, 2))
        ty.copy_(dev(y).view(lead + (H, W)))
        tc.copy_(dev(uv).view(lead + (hc, wc, 2)))
        return YUV420P16(ty, tc, None, bits, "msb", **kw)
    raise ValueError("yuv420p16_source: unknown layout %r" % (layout,))


def synth_frames(count, height, width, seed, content="noise"):
    """Synthetic decoded frames, uint8 numpy [count, height, width, 3]: seeded noise from numpy's legacy generator (its
    stream is stable across numpy versions, so fixtures store outputs only) or a smooth integer gradient."""
    import numpy as np
    if content == "gradient":
        y = np.arange(height, dtype=np.int64)[:, None]
        x = np.arange(width, dtype=np.int64)[None, :]
        one = np.stack([(x * 255) // max(width - 1, 1) + 0 * y, (y * 255) // max(height - 1, 1) + 0 * x,
                        ((x + y) * 255) // max(width + height - 2, 1)], -1).astype(np.uint8)
        return np.stack([np.roll(one, 7 * i, axis=1) for i in range(count)])
    if content != "noise":
        raise ValueError("synth_frames: content must be 'noise' or 'gradient'")
    return np.random.RandomState(int(seed)).randint(0, 256, (count, height, width, 3)).astype(np.uint8)


def synth_color_frames(clips, frames, height, width, seed):
    """Synthetic decoded clips for the colour transforms, uint8 numpy [clips, frames, height, width, 3]: colour ramps plus
    seeded noise (numpy's legacy generator), with grey, black, white and saturated pixels sprinkled in, so every branch of the
    HSV conversions and both ends of the blend's clamp are met.  Every frame differs."""
    import numpy as np
    rng = np.random.RandomState(int(seed))
    yy, xx = np.mgrid[0:height, 0:width]
    out = np.empty((clips, frames, height, width, 3), np.uint8)
    for n in range(clips):
        for t in range(frames):
            base = np.stack([(xx * 255) // max(width - 1, 1), (yy * 255) // max(height - 1, 1), ((xx + yy) * 13 + 40 * t) % 256], -1)
            img = np.clip(base + rng.randint(-60, 61, base.shape), 0, 255)
            img[rng.rand(height, width) < 0.05] = rng.randint(0, 256)        # grey pixels (max == min)
            for colour in ((255, 0, 0), (0, 0, 0), (255, 255, 255)):
                img[rng.rand(height, width) < 0.03] = colour
            out[n, t] = img
    return out
