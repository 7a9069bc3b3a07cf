"""Pre-processing edge on the device (reference pretorched/transforms/utils.py:34-81).

`TransformImage` there is a PIL half (Resize to `int(floor(max(input_size) / scale))`, CenterCrop to
`max(input_size)`; utils.py:53-64) followed by a tensor half: ToTensor (uint8 HWC -> float CHW / 255),
ToSpaceBGR, ToRange255, Normalize(mean, std).  Both halves run on the device here, for whole batches of decoded
uint8 frames:

* `FramesToTensor` is the tensor half alone (same fp32 operations in the same order: bit-identical), for frames
  that already have the model's input size.  Models go one step further with `model.forward_frames`, which
  fuses it into the stem's fold kernel so the fp32 clip never exists in HBM.
* `TransformFrames` is both halves in one HIP launch: bilinear resize + crop (+ horizontal flip) of frames of
  any size, then either the normalised clip (`out="tensor"`) or the resized uint8 frames (`out="frames"`, what
  `forward_frames(.., transform=tf)` takes).  PIL resamples uint8 images in integer arithmetic (22-bit
  fixed-point coefficients, horizontal pass, uint8 intermediate, vertical pass); the coefficient tables are
  built here on the host in float64 exactly as PIL builds them and the kernel does integer work only, so the
  result equals PIL's to the bit.  Crop and flip are folded into the tables.

Image loading and video decoding stay host work and are not on this path.
"""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import NormDesc, PtxError, ResizeDesc, check

PRECISION_BITS = 22       # PIL's fixed-point coefficient precision for 8-bit channels (32 - 8 - 2)


def _opt(opts, key):
    return opts[key] if isinstance(opts, dict) else getattr(opts, key)


class FramesToTensor:
    """opts: a model (after `pretrained=...`) or a `pretrained_settings[...]` dict -- anything with
    input_space / input_range / mean / std, as TransformImage takes (utils.py:36-45)."""

    def __init__(self, opts):
        self.input_space, self.input_range = _opt(opts, "input_space"), _opt(opts, "input_range")
        self.mean, self.std = list(_opt(opts, "mean")), list(_opt(opts, "std"))
        self.norm = NormDesc.make(self.mean, self.std, self.input_space, self.input_range)

    def __call__(self, frames):
        """uint8 CUDA frames [N,T,H,W,C] | [T,H,W,C] | [H,W,C]  ->  fp32 [N,C,T,H,W] | [C,T,H,W] | [C,H,W]."""
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8:
            raise PtxError("FramesToTensor: frames must be a uint8 CUDA tensor (no CPU fallback)")
        if frames.dim() not in (3, 4, 5):
            raise PtxError("FramesToTensor: expected [N,T,H,W,C], [T,H,W,C] or [H,W,C]")
        lead = frames.dim()
        f5 = frames.contiguous().view((1,) * (5 - lead) + tuple(frames.shape))
        N, T, H, W, Cc = f5.shape
        with torch.cuda.device(frames.device):
            out = torch.empty((N, Cc, T, H, W), device=frames.device, dtype=torch.float32)
            check(_lib.lib().ptx_frames_u8_to_ncdhw(C.c_void_p(f5.data_ptr()), C.c_void_p(out.data_ptr()), N, T, H, W,
                                                    Cc, C.byref(self.norm),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "ptx_frames_u8_to_ncdhw")
        if lead == 5:
            return out
        return out[0] if lead == 4 else out[0, :, 0]


# ---------------------------------------------------------------------------------------------
# resize + crop: size rules (torchvision's documented Resize / CenterCrop semantics) and PIL's coefficient tables
# ---------------------------------------------------------------------------------------------
def resized_size(H, W, input_size, scale=0.875, preserve_aspect_ratio=True):
    """(h, w) of the frame after TransformImage's Resize (utils.py:54-59)."""
    if preserve_aspect_ratio:
        R = int(math.floor(max(input_size) / scale))
        if (W <= H and W == R) or (H <= W and H == R):
            return H, W                                   # short side already R: not resampled
        if W < H:
            return int(R * H / W), R
        return R, int(R * W / H)
    return int(input_size[1] / scale), int(input_size[2] / scale)


def crop_window(h, w, S, crop="center"):
    """(top, left) of the S x S window in the resized h x w frame; a window that does not fit raises."""
    if isinstance(crop, str):
        if crop != "center":
            raise PtxError("TransformFrames: crop must be 'center' or (top, left), got %r" % (crop,))
        top, left = int(round((h - S) / 2.0)), int(round((w - S) / 2.0))
    else:
        try:
            top, left = (int(v) for v in crop)
        except (TypeError, ValueError):
            raise PtxError("TransformFrames: crop must be 'center' or (top, left), got %r" % (crop,))
    if top < 0 or left < 0 or top + S > h or left + S > w:
        raise PtxError("TransformFrames: the %dx%d crop at (%d, %d) does not fit the resized %dx%d frame "
                       "(padding crops are not offered)" % (S, S, top, left, h, w))
    return top, left


def resize_axis_table(n_in, n_out):
    """PIL's bilinear coefficients for one axis (precompute_coeffs + normalize_coeffs_8bpc): for every output index
    the first input index `lo`, the tap count `n` and `n` int32 coefficients (2**22 fixed point), as
    (lo[n_out], n[n_out], k[n_out][taps]) with taps = max(n).  An axis that is not resampled is one tap of 2**22."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise PtxError("TransformFrames: non-positive extent (%d -> %d)" % (n_in, n_out))
    if n_in == n_out:
        return (np.arange(n_out, dtype=np.int32), np.ones(n_out, np.int32),
                np.full((n_out, 1), 1 << PRECISION_BITS, np.int32))
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)          # C's (int) truncates; all values are >= -0.5
    hi = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = hi - lo
    j = np.arange(ksize, dtype=np.float64)[None, :]
    w = 1.0 - np.abs((j + lo[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((w > 0.0) & (j < n[:, None]), w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]                                        # sequential sum, as the C loop adds
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = (w * float(1 << PRECISION_BITS) + 0.5).astype(np.int64)             # weights are >= 0: +0.5 then truncate
    taps = int(n.max())
    return lo.astype(np.int32), n.astype(np.int32), np.ascontiguousarray(k[:, :taps].astype(np.int32))


def _select(table, start, count, reverse=False):
    lo, n, k = (a[start:start + count] for a in table)
    if reverse:
        lo, n, k = lo[::-1], n[::-1], k[::-1]
    taps = int(n.max())
    return np.ascontiguousarray(lo), np.ascontiguousarray(n), np.ascontiguousarray(k[:, :taps])


def build_tables(H, W, input_size, scale=0.875, preserve_aspect_ratio=True, crop="center", hflip=False):
    """Row and column tables of resize + crop (+ flip) for H x W frames: only the S output rows / columns of the
    window get entries.  Returns a dict with `rows`, `cols` ((lo, n, k) each), `S`, `resized`, `window`."""
    S = int(max(input_size))
    h, w = resized_size(H, W, input_size, scale, preserve_aspect_ratio)
    if h <= 0 or w <= 0:
        raise PtxError("TransformFrames: resized frame %dx%d is empty" % (h, w))
    top, left = crop_window(h, w, S, crop)
    rows = _select(resize_axis_table(H, h), top, S)
    cols = _select(resize_axis_table(W, w), left, S, reverse=bool(hflip))
    for name, t in (("rows", rows), ("columns", cols)):
        if t[2].shape[1] > _lib.PTX_RESIZE_MAX_TAPS:
            raise PtxError("TransformFrames: down-scaling the %s of a %dx%d frame to %dx%d needs %d taps, the kernel's cap is "
                           "PTX_RESIZE_MAX_TAPS = %d" % (name, H, W, h, w, t[2].shape[1], _lib.PTX_RESIZE_MAX_TAPS))
    return {"rows": rows, "cols": cols, "S": S, "resized": (h, w), "window": (top, left)}


def apply_tables_numpy(frame, tables):
    """The kernel's arithmetic in numpy (uint8 [H,W,C] -> uint8 [S,S,C]): horizontal pass, uint8 intermediate,
    vertical pass.  The host-side model the tests compare with PIL; not a fallback (TransformFrames never calls it)."""
    half = 1 << (PRECISION_BITS - 1)

    def one_pass(img, table):                       # resamples axis 0 of img
        lo, n, k = table
        out = np.empty((len(lo),) + img.shape[1:], np.uint8)
        src = img.astype(np.int64)
        for i in range(len(lo)):
            acc = np.tensordot(k[i, :n[i]].astype(np.int64), src[lo[i]:lo[i] + n[i]], axes=(0, 0)) + half
            out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
        return out

    rlo, rn, _ = tables["rows"]
    r0, r1 = int(rlo.min()), int((rlo + rn).max())                       # only the rows the window references
    mid = one_pass(np.ascontiguousarray(frame[r0:r1].transpose(1, 0, 2)), tables["cols"]).transpose(1, 0, 2)
    return one_pass(mid, (rlo - r0, rn, tables["rows"][2]))


class TransformFrames:
    """Resize + crop (+ flip) of decoded uint8 frames on the device, bit-exact with PIL's bilinear resize, then
    TransformImage's tensor half (`out="tensor"`) or nothing more (`out="frames"`).

    opts: a model or settings dict with input_size / input_space / input_range / mean / std.  scale and
    preserve_aspect_ratio as in TransformImage (utils.py:36-59); crop: "center" (CenterCrop(max(input_size))) or an
    explicit (top, left) in the resized frame; hflip: flip the cropped window horizontally; dtype: torch.float32
    or torch.bfloat16 (the fp32 value rounded once) for out="tensor"."""

    CACHE_SIZE = 8

    def __init__(self, opts, scale=0.875, preserve_aspect_ratio=True, crop="center", hflip=False, out="tensor",
                 dtype=torch.float32):
        if out not in ("tensor", "frames"):
            raise PtxError("TransformFrames: out must be 'tensor' or 'frames', got %r" % (out,))
        if dtype not in (torch.float32, torch.bfloat16):
            raise PtxError("TransformFrames: dtype must be torch.float32 or torch.bfloat16, got %s" % (dtype,))
        if out == "frames" and dtype != torch.float32:
            raise PtxError("TransformFrames: out='frames' returns uint8 frames; dtype=%s applies to out='tensor' only" % (dtype,))
        if not (isinstance(scale, (int, float)) and scale > 0):
            raise PtxError("TransformFrames: scale must be a positive number, got %r" % (scale,))
        self.input_size = [int(v) for v in _opt(opts, "input_size")]
        self.input_space, self.input_range = _opt(opts, "input_space"), _opt(opts, "input_range")
        self.mean, self.std = list(_opt(opts, "mean")), list(_opt(opts, "std"))
        self.norm = NormDesc.make(self.mean, self.std, self.input_space, self.input_range)
        self.scale, self.preserve_aspect_ratio = float(scale), bool(preserve_aspect_ratio)
        self.crop, self.hflip, self.out, self.dtype = crop, bool(hflip), out, dtype
        self.size = int(max(self.input_size))
        if not isinstance(crop, str):
            crop_window(1 << 30, 1 << 30, self.size, crop)          # a malformed or negative window fails here
        elif crop != "center":
            raise PtxError("TransformFrames: crop must be 'center' or (top, left), got %r" % (crop,))
        self._cache = collections.OrderedDict()                      # (H, W, device) -> device tables

    def tables(self, H, W):
        """Host tables for H x W frames (numpy; see build_tables)."""
        return build_tables(H, W, self.input_size, self.scale, self.preserve_aspect_ratio, self.crop, self.hflip)

    def _device_tables(self, H, W, device):
        key = (H, W, str(device))
        hit = self._cache.get(key)
        if hit is not None:
            self._cache.move_to_end(key)
            return hit
        t = self.tables(H, W)
        parts = [a.reshape(-1) for a in t["rows"] + t["cols"]]
        offs = np.cumsum([0] + [p.size for p in parts])
        buf = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(device)     # one small upload per input size
        hit = (buf, [int(o) * 4 for o in offs[:-1]], t["rows"][2].shape[1], t["cols"][2].shape[1])
        self._cache[key] = hit
        while len(self._cache) > self.CACHE_SIZE:
            self._cache.popitem(last=False)
        return hit

    def __call__(self, frames):
        """uint8 CUDA frames [N,T,H,W,3] | [T,H,W,3] | [H,W,3], any H, W  ->
        out="tensor": [N,3,T,S,S] | [3,T,S,S] | [3,S,S] (fp32 or bf16);  out="frames": uint8, same rank, H, W -> S, S."""
        if not isinstance(frames, torch.Tensor):
            raise PtxError("TransformFrames: frames must be a uint8 CUDA tensor, got %s" % type(frames).__name__)
        if frames.dim() not in (3, 4, 5):
            raise PtxError("TransformFrames: expected [N,T,H,W,3], [T,H,W,3] or [H,W,3], got shape %s" % (tuple(frames.shape),))
        if frames.shape[-1] != 3:
            raise PtxError("TransformFrames: frames must have 3 interleaved channels, got %d" % frames.shape[-1])
        if not frames.is_cuda or frames.dtype != torch.uint8:
            raise PtxError("TransformFrames: frames must be a uint8 CUDA tensor (no CPU fallback)")
        lead = frames.dim()
        f5 = frames.contiguous().view((1,) * (5 - lead) + tuple(frames.shape))
        N, T, H, W, Cc = f5.shape
        if N * T == 0:
            raise PtxError("TransformFrames: empty batch")
        S = self.size
        with torch.cuda.device(frames.device):
            buf, offs, taps_h, taps_w = self._device_tables(H, W, frames.device)
            if self.out == "frames":
                mode, y = _lib.PTX_RESIZE_OUT_U8, torch.empty((N, T, S, S, Cc), device=frames.device, dtype=torch.uint8)
            else:
                mode = _lib.PTX_RESIZE_OUT_F32 if self.dtype == torch.float32 else _lib.PTX_RESIZE_OUT_BF16
                y = torch.empty((N, Cc, T, S, S), device=frames.device, dtype=self.dtype)
            desc = ResizeDesc(N, T, H, W, Cc, S, S, taps_h, taps_w, mode)
            base = buf.data_ptr()
            check(_lib.lib().ptx_resize_frames_u8(C.byref(desc), C.c_void_p(f5.data_ptr()),
                                                  *[C.c_void_p(base + o) for o in offs],
                                                  C.c_void_p(y.data_ptr()), C.byref(self.norm),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "ptx_resize_frames_u8")
        if self.out == "frames":
            return y.view(tuple(frames.shape[:-3]) + (S, S, Cc))
        if lead == 5:
            return y
        return y[0] if lead == 4 else y[0, :, 0]


def apply_frames_transform(transform, frames, who="forward_frames"):
    """The `transform=` hook of forward_frames: a TransformFrames with out="frames", applied to the raw frames."""
    if transform is None:
        return frames
    if not isinstance(transform, TransformFrames) or transform.out != "frames":
        raise PtxError("%s: transform must be a pretorched.transforms.TransformFrames with out='frames', got %r" % (
            who, transform))
    return transform(frames)
