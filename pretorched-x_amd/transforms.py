"""Pre-processing edge on the device (reference pretorched/transforms/utils.py:34-81).

`TransformImage` there is a PIL half (Resize to `int(floor(max(input_size) / scale))`, CenterCrop to
`max(input_size)`; utils.py:53-64) followed by a tensor half: ToTensor (uint8 HWC -> float CHW / 255),
ToSpaceBGR, ToRange255, Normalize(mean, std).  Both halves run on the device here, for whole batches of decoded
uint8 frames:

* `FramesToTensor` is the tensor half alone (same fp32 operations in the same order: bit-identical), for frames
  that already have the model's input size.  Models go one step further with `model.forward_frames`, which
  fuses it into the stem's fold kernel so the fp32 clip never exists in HBM.
* `TransformFrames` is both halves in one HIP launch: resize (bilinear, or with `interpolation=` any other Pillow filter:
  nearest, box, hamming, bicubic, lanczos -- the filter lives in the tables) + crop (+ flips) of frames of any size, then either the normalised clip (`out="tensor"`) or the resized uint8 frames (`out="frames"`, what
  `forward_frames(.., transform=tf)` takes).  PIL resamples uint8 images in integer arithmetic (22-bit
  fixed-point coefficients, horizontal pass, uint8 intermediate, vertical pass); the coefficient tables are
  built here on the host in float64 exactly as PIL builds them and the kernel does integer work only, so the
  result equals PIL's to the bit.  Crop and flip are folded into the tables.  With `random_crop` / `random_hflip` /
  `random_vflip` (TransformImage's training switches, utils.py:36-70) every clip of a batch gets a window and flips of
  its own, still in one launch: the tables then cover the whole resized frame and the kernel indexes them per clip.
  With `random_short_side` (per-clip scale jitter) or `random_resized_crop` (torchvision's RandomResizedCrop) every clip
  has a resize GEOMETRY of its own: a small launch builds the clips' tables on the device from 10 integers per clip (the
  same float64 operations in the same order as the host builder: the same bits) and one resize launch applies them.

* `SampleViews` is test-time multi-view sampling of a whole decoded video: `clips` temporal clips x `crops` spatial
  crops, each resized + cropped as `TransformFrames` does (same tables, same bits), in one HIP launch per range of
  views.  Frames are read in place through an index table and the crop windows of a sampled frame share one
  horizontal pass.  `model.forward_views` feeds the views to a model chunk by chunk and averages the predictions.

* `SampleClips` is training-time sampling of a BATCH of decoded videos of any sizes and lengths: per output clip a
  random (or the test-time) frame index row and a resize geometry row drawn as `TransformFrames.draw_geometry` draws it,
  applied in place by one table-builder launch plus one resize launch whose workgroups each read their own clip's source
  row.  No gathered or same-size copy of any video is made; every clip has the bits of `TransformFrames` on its frames.

* `YUV420` describes decoder output (NV12 / I420 planes, any row pitch) and is accepted wherever RGB frames are:
  the two resize kernels convert to RGB while they stage an input row on chip (`yuv_coefficients` is the integer
  contract, `yuv420_to_rgb_numpy` its numpy statement), so the RGB frame never exists in HBM and every output bit
  is that of the RGB path on the converted frames.  `YUV420P16` is the same for 10- and 12-bit streams (P010 / P012 /
  P016 surfaces, yuv420p10le / yuv420p12le planes; `yuv_coefficients_p16`, `yuv420p16_to_rgb_numpy`).

* `ColorJitter` is torchvision's ColorJitter (+ RandomGrayscale) on uint8 frames, one draw per clip, equal to the PIL-image
  code path bit for bit (`color_jitter_numpy` is the numpy statement of the contract).  Alone it maps uint8 frames to uint8
  frames; as `TransformFrames(.., color=cj)` / `SampleClips(.., color=cj)` it runs behind the resize, which then writes uint8
  frames into scratch, and the colour launch writes the requested output (uint8 frames or the normalised fp32 / bf16 clip).

* `RandAugment` is torchvision's RandAugment on uint8 frames, one draw per clip, equal to the PIL-image code path (nearest
  interpolation) bit for bit (`rand_augment_numpy` is the numpy statement of the contract): per op position a statistics launch
  (only when an op needs a frame's histograms or mean) and an apply launch.  As `TransformFrames(.., augment=ra)` /
  `SampleClips(.., augment=ra)` it runs behind the resize and behind `color=`, its last position writing the call's output.

* `BatchMix` is the recipes' last two steps on the normalised clip: RandomErasing per clip (torchvision's draw) and MixUp /
  CutMix across the clips of the batch (torchvision v2's draw), in one launch that reads uint8 frames (or a normalised clip) and
  writes the NCDHW clip once, equal bit for bit to `batch_mix_torch`, the torch statement of the contract.  As
  `TransformFrames(.., mix=bm)` / `SampleClips(.., mix=bm)` it is the last stage; `bm.targets` gives the soft targets.

* `GaussianBlur` is torchvision's GaussianBlur (inside RandomApply with `p=`) on uint8 frames, one draw per clip: a separable
  float64 blur with reflect padding whose result is a pure function of the bytes and the fp32 weights (`gaussian_blur_numpy` is
  the numpy statement of the contract, `gaussian_kernel1d` torchvision's weights).  As `TransformFrames(.., blur=gb)` /
  `SampleClips(.., blur=gb)` it runs behind `color=` and in front of `augment=` / `mix=`, the view recipes' order.

* `CamOverlay` draws the class activation maps of `model.cam` / `model.cam_frames` over the frames they explain in one launch: the
  map resized through the resize tables, coloured through a 256-entry table and blended in, equal to Pillow's resize + `Image.blend`
  bit for bit (`cam_overlay_numpy` is the numpy statement of the contract, `cam_quantize_numpy` that of the uint8 maps).

Image loading and video decoding stay host work and are not on this path.
"""
import collections
import copy
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import ClipSrc, ClipSrcYuv420, ClipSrcYuv420P16, NormDesc, PtxError, ResizeDesc, ViewsDesc, Yuv420P16Src, Yuv420Src, check

PRECISION_BITS = 22       # PIL's fixed-point coefficient precision for 8-bit channels (32 - 8 - 2)


def _opt(opts, key):
    return opts[key] if isinstance(opts, dict) else getattr(opts, key)


# ---------------------------------------------------------------------------------------------
# The front door of every transform, in small steps that each __call__ puts in its own order; `who` names the caller
# ---------------------------------------------------------------------------------------------
def _frames_shape(frames, who):
    """(N, T, H, W) of frames [N,T,H,W,3] | [T,H,W,3] | [H,W,3] (a missing N or T is 1), or PtxError: type, rank, channels."""
    if not isinstance(frames, torch.Tensor):
        raise PtxError("%s: frames must be a uint8 CUDA tensor, got %s" % (who, type(frames).__name__))
    if frames.dim() not in (3, 4, 5) or frames.shape[-1] != 3:
        raise PtxError("%s: expected [N,T,H,W,3], [T,H,W,3] or [H,W,3], got shape %s" % (who, tuple(frames.shape)))
    return (1,) * (5 - frames.dim()) + tuple(int(n) for n in frames.shape[:-1])


def _check_not_empty(x, who):
    if x.numel() == 0:
        raise PtxError("%s: empty batch" % who)


def _u8_cuda_5d(frames, who):
    """The contiguous [N,T,H,W,C] view of uint8 CUDA frames of rank 3, 4 or 5, or PtxError."""
    if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8:
        raise PtxError("%s: frames must be a uint8 CUDA tensor (no CPU fallback)" % who)
    return frames.contiguous().view((1,) * (5 - frames.dim()) + tuple(frames.shape))


def _check_generator(generator, who, name="generator"):
    if generator is not None and not isinstance(generator, torch.Generator):
        raise PtxError("%s: %s must be a torch.Generator or None, got %r" % (who, name, generator))
    return generator


def _host_array(a, cuda_message):
    """An array or a CPU tensor as a numpy array; a CUDA tensor raises PtxError(cuda_message)."""
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise PtxError(cuda_message)
        a = a.numpy()
    return np.asarray(a)


def _out_mode(dtype, out="tensor"):
    """The PTX_RESIZE_OUT_* code of a call's output: uint8 frames, or the normalised clip of `dtype`."""
    if out == "frames":
        return _lib.PTX_RESIZE_OUT_U8
    return _lib.PTX_RESIZE_OUT_F32 if dtype == torch.float32 else _lib.PTX_RESIZE_OUT_BF16


def _alloc_out(mode, N, T, H, W, device, dtype):
    """The output of a launch by mode: uint8 [N,T,H,W,3], or [N,3,T,H,W] of `dtype`."""
    if mode == _lib.PTX_RESIZE_OUT_U8:
        return torch.empty((N, T, H, W, 3), device=device, dtype=torch.uint8)
    return torch.empty((N, 3, T, H, W), device=device, dtype=dtype)


def _restore_rank(y, lead, mode):
    """A 5-D output as the result of a call on frames of rank `lead`: the leading dimensions added for the launch go."""
    if mode == _lib.PTX_RESIZE_OUT_U8:
        return y.view(tuple(y.shape[5 - lead:]))
    if lead == 5:
        return y
    return y[0] if lead == 4 else y[0, :, 0]


class FramesToTensor:
    """opts: a model (after `pretrained=...`) or a `pretrained_settings[...]` dict -- anything with
    input_space / input_range / mean / std, as TransformImage takes (utils.py:36-45)."""

    def __init__(self, opts):
        self.input_space, self.input_range = _opt(opts, "input_space"), _opt(opts, "input_range")
        self.mean, self.std = list(_opt(opts, "mean")), list(_opt(opts, "std"))
        self.norm = NormDesc.make(self.mean, self.std, self.input_space, self.input_range)

    def __call__(self, frames):
        """uint8 CUDA frames [N,T,H,W,C] | [T,H,W,C] | [H,W,C]  ->  fp32 [N,C,T,H,W] | [C,T,H,W] | [C,H,W]."""
        f5 = _u8_cuda_5d(frames, "FramesToTensor")
        if frames.dim() not in (3, 4, 5):
            raise PtxError("FramesToTensor: expected [N,T,H,W,C], [T,H,W,C] or [H,W,C]")
        N, T, H, W, Cc = f5.shape
        with torch.cuda.device(frames.device):
            out = torch.empty((N, Cc, T, H, W), device=frames.device, dtype=torch.float32)
            check(_lib.lib().ptx_frames_u8_to_ncdhw(C.c_void_p(f5.data_ptr()), C.c_void_p(out.data_ptr()), N, T, H, W,
                                                    Cc, C.byref(self.norm),
                                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "ptx_frames_u8_to_ncdhw")
        return _restore_rank(out, frames.dim(), _lib.PTX_RESIZE_OUT_F32)


# ---------------------------------------------------------------------------------------------
# YUV 4:2:0 sources: the colour contract (integers, 16 fractional bits) and the container of a decoder's planes
# ---------------------------------------------------------------------------------------------
YUV_BITS = 16
_YUV_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}              # Kr, Kb
_YUV_RANGES = {"limited": (255.0 / 219.0, 255.0 / 224.0, 16), "full": (1.0, 1.0, 0)}   # luma scale, chroma scale, y_off


def yuv_coefficients(matrix="bt709", color_range="limited"):
    """(y_off, ky, krv, kgu, kgv, kbu): the integer coefficients (2**16 fixed point, rounded from float64) of
        R = clip8((ky*y' + krv*cr + 32768) >> 16)     G = clip8((ky*y' - kgu*cb - kgv*cr + 32768) >> 16)
        B = clip8((ky*y' + kbu*cb + 32768) >> 16)     with y' = Y - y_off, cb = Cb - 128, cr = Cr - 128."""
    if matrix not in _YUV_MATRICES:
        raise PtxError("YUV420: matrix must be 'bt601' or 'bt709', got %r" % (matrix,))
    if color_range not in _YUV_RANGES:
        raise PtxError("YUV420: color_range must be 'limited' or 'full', got %r" % (color_range,))
    kr, kb = _YUV_MATRICES[matrix]
    kg = 1.0 - kr - kb
    sy, sc, y_off = _YUV_RANGES[color_range]
    q = lambda v: int(round(v * float(1 << YUV_BITS)))
    return (y_off, q(sy), q(2.0 * (1.0 - kr) * sc), q(2.0 * kb * (1.0 - kb) / kg * sc), q(2.0 * kr * (1.0 - kr) / kg * sc),
            q(2.0 * (1.0 - kb) * sc))


def yuv420_to_rgb_numpy(y, u, v, matrix="bt709", color_range="limited"):
    """The kernels' colour conversion in numpy: uint8 planes y [..,H,W], u, v [..,ceil(H/2),ceil(W/2)] -> uint8
    [..,H,W,3].  The chroma sample of pixel (r, c) is (r >> 1, c >> 1).  The host-side model the tests compare with;
    not a fallback."""
    y_off, ky, krv, kgu, kgv, kbu = yuv_coefficients(matrix, color_range)
    y, u, v = (np.asarray(a) for a in (y, u, v))
    H, W = y.shape[-2:]
    if u.shape != v.shape or u.shape[-2:] != ((H + 1) // 2, (W + 1) // 2) or u.shape[:-2] != y.shape[:-2]:
        raise PtxError("yuv420_to_rgb_numpy: chroma planes %s / %s do not match the %dx%d luma plane" % (u.shape, v.shape, H, W))
    rows, cols = np.arange(H) >> 1, np.arange(W) >> 1
    yy = ky * (y.astype(np.int64) - y_off)
    cb = u.astype(np.int64)[..., rows, :][..., cols] - 128
    cr = v.astype(np.int64)[..., rows, :][..., cols] - 128
    half = 1 << (YUV_BITS - 1)
    rgb = np.stack([(yy + krv * cr + half) >> YUV_BITS, (yy - kgu * cb - kgv * cr + half) >> YUV_BITS,
                    (yy + kbu * cb + half) >> YUV_BITS], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


class YUV420:
    """Decoded YUV 4:2:0 frames (8 bit) as a decoder hands them back, accepted wherever RGB frames are:

        YUV420(y, uv, ...)     y [..,H,W], uv [..,ceil(H/2),ceil(W/2),2]         (NV12 surfaces, any row pitch)
        YUV420(y, u, v, ...)   u, v [..,ceil(H/2),ceil(W/2)]                      (planar)
        YUV420.from_nv12(packed, ...) / YUV420.from_i420(packed, ...)            packed [..,H*3/2,W], even H and W

    with 0, 1 or 2 leading dimensions ([H,W], [T,H,W], [N,T,H,W]: `lead` = 1, 2, 3 as an RGB tensor of rank lead + 2).
    matrix: "bt709" | "bt601"; color_range: "limited" | "full" (see `yuv_coefficients`).  Planes are read in place when
    their rows are contiguous runs (a uv plane: last strides (2, 1)) -- row pitch, frame and video strides and base
    alignment are arbitrary --, anything else costs one `.contiguous()` copy of that plane at the call."""

    # what YUV420P16 (16-bit words) replaces: the name in messages, the entry points' infix, the descriptors, bytes per sample
    _NAME = "YUV420"
    _ABI = "yuv420"
    _SRC, _CLIP_SRC = Yuv420Src, ClipSrcYuv420
    _ITEM = 1

    def __init__(self, y, u, v=None, matrix="bt709", color_range="limited"):
        coefficients = yuv_coefficients(matrix, color_range)
        for p in (y, u) if v is None else (y, u, v):
            if not isinstance(p, torch.Tensor) or p.dtype != torch.uint8:
                raise PtxError("YUV420: planes must be uint8 tensors, got %s" % (
                    p.dtype if isinstance(p, torch.Tensor) else type(p).__name__,))
        self._init_planes(y, u, v, matrix, color_range, coefficients)

    def _init_planes(self, y, u, v, matrix, color_range, coefficients):
        """The checks and attributes that do not depend on the sample type."""
        name = self._NAME
        self.coefficients = coefficients
        self.matrix, self.color_range = matrix, color_range
        planes = (y, u) if v is None else (y, u, v)
        if len({p.device for p in planes}) != 1:
            raise PtxError("%s: planes are on different devices (%s)" % (name, ", ".join(str(p.device) for p in planes)))
        if y.dim() not in (2, 3, 4):
            raise PtxError("%s: expected a luma plane [N,T,H,W], [T,H,W] or [H,W], got shape %s" % (name, tuple(y.shape)))
        H, W = int(y.shape[-2]), int(y.shape[-1])
        want = tuple(y.shape[:-2]) + ((H + 1) // 2, (W + 1) // 2)
        for pname, p in (("uv", u),) if v is None else (("u", u), ("v", v)):
            if tuple(p.shape) != want + ((2,) if v is None else ()):
                raise PtxError("%s: the %s plane has shape %s, a %dx%d luma plane of shape %s needs %s (ceil(H/2) x "
                               "ceil(W/2) samples)" % (name, pname, tuple(p.shape), H, W, tuple(y.shape),
                                                       want + ((2,) if v is None else ())))
        self.y, self.u, self.v = y, u, v                            # v is None: u holds the interleaved pairs
        self.H, self.W, self.lead, self.device = H, W, y.dim() - 1, y.device
        self.N = int(y.shape[0]) if y.dim() == 4 else 1
        self.T = int(y.shape[-3]) if y.dim() >= 3 else 1
        self.lead_shape = tuple(y.shape[:-2])

    @classmethod
    def _packed(cls, packed, who):
        name, wide = cls._NAME, cls._ITEM == 2
        if not isinstance(packed, torch.Tensor) or packed.dtype not in ((torch.int16, torch.uint16) if wide else (torch.uint8,)):
            raise PtxError("%s.%s: packed frames must be %s tensor" % (name, who, "an int16 / uint16" if wide else "a uint8"))
        if packed.dim() not in (2, 3, 4):
            raise PtxError("%s.%s: expected [N,T,H*3/2,W], [T,H*3/2,W] or [H*3/2,W], got shape %s" % (name, who, tuple(packed.shape)))
        rows, W = int(packed.shape[-2]), int(packed.shape[-1])
        H = rows * 2 // 3
        if rows % 3 or H % 2 or W % 2 or H == 0 or W == 0:
            raise PtxError("%s.%s: a packed frame is H*3/2 rows of W %s with even H and W, got %d rows of %d (pass "
                           "planes for odd sizes)" % (name, who, "words" if wide else "bytes", rows, W))
        return H, W

    @classmethod
    def from_nv12(cls, packed, matrix="bt709", color_range="limited"):
        """Packed NV12 [..,H*3/2,W]: H rows of luma, then H/2 rows of interleaved Cb Cr pairs.  Views, no copy."""
        H, W = cls._packed(packed, "from_nv12")
        return cls(packed[..., :H, :], packed[..., H:, :].unflatten(-1, (W // 2, 2)), None, matrix, color_range)

    @classmethod
    def from_i420(cls, packed, matrix="bt709", color_range="limited"):
        """Packed I420 [..,H*3/2,W]: the luma plane, then the Cb plane, then the Cr plane (H/2 x W/2 each, as flat
        runs).  Views when each packed frame is contiguous, otherwise `reshape` copies the frames once."""
        H, W = cls._packed(packed, "from_i420")
        flat = packed.reshape(tuple(packed.shape[:-2]) + (H * 3 // 2 * W,))
        q = (H // 2) * (W // 2)
        return cls(flat[..., :H * W].unflatten(-1, (H, W)), flat[..., H * W:H * W + q].unflatten(-1, (H // 2, W // 2)),
                   flat[..., H * W + q:].unflatten(-1, (H // 2, W // 2)), matrix, color_range)

    @staticmethod
    def _rows_in_place(p, inner):
        """p's trailing dimensions `inner` (a row, or a row of pairs) are a contiguous run and rows do not overlap."""
        k = len(inner)
        want, run = [], 1
        for n in reversed(inner):
            want.append(run)
            run *= n
        if any(p.shape[-1 - i] > 1 and p.stride(-1 - i) != want[i] for i in range(k)):
            return False
        return p.shape[-1 - k] == 1 or p.stride(-1 - k) >= run

    def _like(self, y, u, v):
        """A source over other planes with this one's colour parameters."""
        return YUV420(y, u, v, self.matrix, self.color_range)

    def source(self, who="YUV420"):
        """(Yuv420Src, tensors to keep alive): the kernels' descriptor of the planes, checked and copied where needed.
        Pointers, strides and pitches are in bytes (`_ITEM` per sample)."""
        if self.device.type != "cuda":
            raise PtxError("%s: the planes of a %s source must be %s CUDA tensors (no CPU fallback)" % (
                who, self._NAME, "uint8" if self._ITEM == 1 else "int16 / uint16"))
        if self.N * self.T == 0 or self.H * self.W == 0:
            raise PtxError("%s: empty batch" % who)
        Hc, Wc = (self.H + 1) // 2, (self.W + 1) // 2
        y = self.y if self._rows_in_place(self.y, (self.W,)) else self.y.contiguous()
        if self.v is None:
            u = self.u if self._rows_in_place(self.u, (Wc, 2)) else self.u.contiguous()
            c, keep = u.select(-1, 0), (y, u)
            pu, pv, step, pitch_c = u.data_ptr(), u.data_ptr() + self._ITEM, 2, (u.stride(-3) if Hc > 1 else 2 * Wc)
        else:
            u, v = self.u, self.v
            if not (self._rows_in_place(u, (Wc,)) and self._rows_in_place(v, (Wc,)) and
                    all(u.stride(i) == v.stride(i) or u.shape[i] == 1 for i in range(u.dim() - 1))):
                u, v = u.contiguous(), v.contiguous()              # one pitch and one set of strides serve both pointers
            c, keep = u, (y, u, v)
            pu, pv, step, pitch_c = u.data_ptr(), v.data_ptr(), 1, (u.stride(-2) if Hc > 1 else Wc)

        def strides(p, nd):                                         # (video, frame) strides of a plane with nd trailing dims
            lead = p.dim() - nd
            st = p.stride(lead - 1) if lead >= 1 and p.shape[lead - 1] > 1 else 0
            sn = p.stride(lead - 2) if lead >= 2 and p.shape[lead - 2] > 1 else 0
            return sn, st

        b = self._ITEM                                              # element strides -> bytes
        s = self._SRC()
        s.y, s.u, s.v = y.data_ptr(), pu, pv
        s.stride_n_y, s.stride_t_y = (b * n for n in strides(y, 2))
        s.stride_n_c, s.stride_t_c = (b * n for n in strides(c, 2))
        s.pitch_y, s.pitch_c, s.step_c = b * (y.stride(-2) if self.H > 1 else self.W), b * pitch_c, b * step
        s.y_off, s.ky, s.krv, s.kgu, s.kgv, s.kbu = self.coefficients
        return s, keep

    def to_rgb_numpy(self):
        """uint8 [..,H,W,3] through `yuv420_to_rgb_numpy` (host; tests and examples)."""
        if self.v is None:
            u, v = self.u[..., 0], self.u[..., 1]
        else:
            u, v = self.u, self.v
        return yuv420_to_rgb_numpy(self.y.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy(), self.matrix, self.color_range)


# ---------------------------------------------------------------------------------------------
# 10- and 12-bit YUV 4:2:0 sources: 16-bit words, the sample MSB-aligned (P010 / P012 / P016 surfaces of the hardware
# decoders) or LSB-aligned (yuv420p10le / yuv420p12le of the software decoders).  The contract is the 8-bit one with
# d = bits - 8 more bits in the samples and in the final shift, and the H.273 scales of the depth.
# ---------------------------------------------------------------------------------------------
_YUV_MATRICES_P16 = dict(_YUV_MATRICES, bt2020=(0.2627, 0.0593))                  # + BT.2020 non-constant luminance


def _yuv16_args(who, bits, align=None):
    if bits not in (10, 12):
        raise PtxError("%s: bits must be 10 or 12, got %r" % (who, bits))
    if align not in (None, "msb", "lsb"):
        raise PtxError("%s: align must be 'msb' (P010 / P012 / P016) or 'lsb' (yuv420p10le / yuv420p12le), got %r" % (who, align))
    return 0 if align == "lsb" else 16 - bits


def yuv_coefficients_p16(matrix="bt709", color_range="limited", bits=10):
    """(y_off, ky, krv, kgu, kgv, kbu) for `bits`-bit samples (10 or 12; d = bits - 8): 2**16 fixed point, rounded once
    from float64 as `yuv_coefficients` does, for
        R = clip8((ky*y' + krv*cr + 2**(15+d)) >> (16+d))     G = clip8((ky*y' - kgu*cb - kgv*cr + 2**(15+d)) >> (16+d))
        B = clip8((ky*y' + kbu*cb + 2**(15+d)) >> (16+d))     y' = Y - y_off, cb = Cb - (128 << d), cr = Cr - (128 << d).
    Scales of H.273: limited range luma 255/219, chroma 255/224, y_off = 16 << d (the 8-bit coefficients); full range
    both 255 * 2**d / (2**bits - 1), y_off = 0.  matrix: "bt601" | "bt709" | "bt2020" (non-constant luminance)."""
    if matrix not in _YUV_MATRICES_P16:
        raise PtxError("YUV420P16: matrix must be 'bt601', 'bt709' or 'bt2020', got %r" % (matrix,))
    if color_range not in _YUV_RANGES:
        raise PtxError("YUV420P16: color_range must be 'limited' or 'full', got %r" % (color_range,))
    _yuv16_args("YUV420P16", bits)
    d = bits - 8
    kr, kb = _YUV_MATRICES_P16[matrix]
    kg = 1.0 - kr - kb
    if color_range == "limited":
        sy, sc, y_off = 255.0 / 219.0, 255.0 / 224.0, 16 << d
    else:
        sy = sc = 255.0 * float(1 << d) / float((1 << bits) - 1)
        y_off = 0
    q = lambda v: int(round(v * float(1 << YUV_BITS)))
    return (y_off, q(sy), q(2.0 * (1.0 - kr) * sc), q(2.0 * kb * (1.0 - kb) / kg * sc), q(2.0 * kr * (1.0 - kr) / kg * sc),
            q(2.0 * (1.0 - kb) * sc))


def yuv420p16_to_rgb_numpy(y, u, v, bits=10, align="msb", matrix="bt709", color_range="limited"):
    """The kernels' colour conversion of 10- / 12-bit samples in numpy: 16-bit planes (uint16, or int16 read unsigned)
    y [..,H,W], u, v [..,ceil(H/2),ceil(W/2)] -> uint8 [..,H,W,3].  A sample is (word >> shift) & (2**bits - 1) with
    shift = 16 - bits for align="msb" and 0 for "lsb"; the chroma sample of pixel (r, c) is (r >> 1, c >> 1).  The
    host-side model the tests compare with; not a fallback."""
    shift = _yuv16_args("yuv420p16_to_rgb_numpy", bits, align)
    y_off, ky, krv, kgu, kgv, kbu = yuv_coefficients_p16(matrix, color_range, bits)
    y, u, v = (np.asarray(a) for a in (y, u, v))
    for a in (y, u, v):
        if a.dtype not in (np.uint16, np.int16):
            raise PtxError("yuv420p16_to_rgb_numpy: planes must be uint16 (or int16) arrays, got %s" % a.dtype)
    H, W = y.shape[-2:]
    if u.shape != v.shape or u.shape[-2:] != ((H + 1) // 2, (W + 1) // 2) or u.shape[:-2] != y.shape[:-2]:
        raise PtxError("yuv420p16_to_rgb_numpy: chroma planes %s / %s do not match the %dx%d luma plane" % (u.shape, v.shape, H, W))
    d, mask = bits - 8, (1 << bits) - 1
    sample = lambda a: (a.view(np.uint16).astype(np.int64) >> shift) & mask
    rows, cols = np.arange(H) >> 1, np.arange(W) >> 1
    yy = ky * (sample(y) - y_off)
    cb = sample(u)[..., rows, :][..., cols] - (128 << d)
    cr = sample(v)[..., rows, :][..., cols] - (128 << d)
    half, sh = 1 << (YUV_BITS - 1 + d), YUV_BITS + d
    rgb = np.stack([(yy + krv * cr + half) >> sh, (yy - kgu * cb - kgv * cr + half) >> sh, (yy + kbu * cb + half) >> sh], -1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


class YUV420P16(YUV420):
    """Decoded 10- or 12-bit YUV 4:2:0 frames in 16-bit words, accepted wherever `YUV420` is:

        YUV420P16(y, uv, ...)     y [..,H,W], uv [..,ceil(H/2),ceil(W/2),2]       (P010 / P016 surfaces, any row pitch)
        YUV420P16(y, u, v, ...)   u, v [..,ceil(H/2),ceil(W/2)]                    (planar)
        YUV420P16.from_p010(packed, bits=10, ...)       packed [..,H*3/2,W] words, MSB-aligned (bits=12: P012 / P016)
        YUV420P16.from_i420p16(packed, bits, ...)       packed [..,H*3/2,W] words, planar, LSB-aligned (yuv420p10le / p12le)

    Planes are `torch.int16` or `torch.uint16` tensors (the same bits, read unsigned) with 0, 1 or 2 leading dimensions.
    bits: 10 | 12; align: "msb" (the sample in the high bits, the low 16 - bits ignored whatever they hold) | "lsb" (the
    sample in the low bits, the high bits masked); matrix: "bt709" | "bt601" | "bt2020"; color_range: "limited" | "full"
    (see `yuv_coefficients_p16`).  The output is 8-bit RGB; transfer functions are not touched, so PQ / HLG content
    comes out as PQ / HLG-coded RGB.  Planes are read in place when their rows are contiguous runs, as `YUV420`'s."""

    _NAME = "YUV420P16"
    _ABI = "yuv420p16"
    _SRC, _CLIP_SRC = Yuv420P16Src, ClipSrcYuv420P16
    _ITEM = 2

    def __init__(self, y, u, v=None, bits=10, align="msb", matrix="bt709", color_range="limited"):
        coefficients = yuv_coefficients_p16(matrix, color_range, bits)
        self.bits, self.align, self.shift = bits, align, _yuv16_args("YUV420P16", bits, align)
        planes = (y, u) if v is None else (y, u, v)
        for p in planes:
            if isinstance(p, torch.Tensor) and p.dtype == torch.uint8:
                raise PtxError("YUV420P16: planes must be int16 / uint16 tensors of 10- or 12-bit samples, got torch.uint8 "
                               "(8-bit planes are a YUV420 source)")
            if not isinstance(p, torch.Tensor) or p.dtype not in (torch.int16, torch.uint16):
                raise PtxError("YUV420P16: planes must be int16 / uint16 tensors, got %s" % (
                    p.dtype if isinstance(p, torch.Tensor) else type(p).__name__,))
        y, u, v = (p if p is None or p.dtype == torch.int16 else p.view(torch.int16) for p in (y, u, v))   # the same bits
        self._init_planes(y, u, v, matrix, color_range, coefficients)

    @classmethod
    def from_p010(cls, packed, bits=10, matrix="bt709", color_range="limited"):
        """Packed P010 (bits=12: P012 / P016) [..,H*3/2,W] words: H rows of luma, then H/2 rows of interleaved Cb Cr
        pairs, samples MSB-aligned.  Views, no copy."""
        H, W = cls._packed(packed, "from_p010")
        return cls(packed[..., :H, :], packed[..., H:, :].unflatten(-1, (W // 2, 2)), None, bits, "msb", matrix, color_range)

    @classmethod
    def from_i420p16(cls, packed, bits, matrix="bt709", color_range="limited"):
        """Packed yuv420p10le / yuv420p12le [..,H*3/2,W] words: the luma plane, then the Cb plane, then the Cr plane (H/2 x
        W/2 each, as flat runs), samples LSB-aligned.  Views when each packed frame is contiguous."""
        H, W = cls._packed(packed, "from_i420p16")
        flat = packed.reshape(tuple(packed.shape[:-2]) + (H * 3 // 2 * W,))
        q = (H // 2) * (W // 2)
        return cls(flat[..., :H * W].unflatten(-1, (H, W)), flat[..., H * W:H * W + q].unflatten(-1, (H // 2, W // 2)),
                   flat[..., H * W + q:].unflatten(-1, (H // 2, W // 2)), bits, "lsb", matrix, color_range)

    def _like(self, y, u, v):
        return YUV420P16(y, u, v, self.bits, self.align, self.matrix, self.color_range)

    def source(self, who="YUV420P16"):
        """(Yuv420P16Src, tensors to keep alive): the kernels' descriptor of the planes, checked and copied where needed."""
        s, keep = super().source(who)
        s.bits, s.shift = self.bits, self.shift
        return s, keep

    def to_rgb_numpy(self):
        """uint8 [..,H,W,3] through `yuv420p16_to_rgb_numpy` (host; tests and examples)."""
        if self.v is None:
            u, v = self.u[..., 0], self.u[..., 1]
        else:
            u, v = self.u, self.v
        return yuv420p16_to_rgb_numpy(self.y.cpu().numpy(), u.cpu().numpy(), v.cpu().numpy(), self.bits, self.align,
                                      self.matrix, self.color_range)


# ---------------------------------------------------------------------------------------------
# resize + crop: size rules (torchvision's documented Resize / CenterCrop semantics) and PIL's coefficient tables
# ---------------------------------------------------------------------------------------------
def resized_size_for(H, W, R):
    """(h, w) of an H x W frame after Resize(R): the short side becomes R, the long side follows the aspect ratio
    (truncated, as torchvision does)."""
    H, W, R = int(H), int(W), int(R)
    if (W <= H and W == R) or (H <= W and H == R):
        return H, W                                       # short side already R: not resampled
    if W < H:
        return int(R * H / W), R
    return R, int(R * W / H)


def resized_size(H, W, input_size, scale=0.875, preserve_aspect_ratio=True):
    """(h, w) of the frame after TransformImage's Resize (utils.py:54-59)."""
    if preserve_aspect_ratio:
        return resized_size_for(H, W, int(math.floor(max(input_size) / scale)))
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


INTERPOLATIONS = ("nearest", "lanczos", "bilinear", "bicubic", "box", "hamming")     # by Pillow's code (the PTX_RESAMPLE_* codes)
DEVICE_INTERPOLATIONS = ("nearest", "box", "bilinear", "bicubic")                   # what the device table builder takes
_SUPPORT = {"box": 0.5, "bilinear": 1.0, "hamming": 1.0, "bicubic": 2.0, "lanczos": 3.0}   # Resample.c's filter supports


def check_interpolation(interpolation, who="TransformFrames"):
    """The canonical name of a resize filter: one of INTERPOLATIONS as a string, Pillow's integer code, or any enum whose
    `.value` is one of those (PIL.Image.Resampling, torchvision's InterpolationMode); anything else raises."""
    v = interpolation
    if not isinstance(v, (str, int)) and isinstance(getattr(v, "value", None), (str, int)):
        v = v.value
    if isinstance(v, str) and v in INTERPOLATIONS:
        return v
    if isinstance(v, int) and not isinstance(v, bool) and 0 <= v < len(INTERPOLATIONS):
        return INTERPOLATIONS[int(v)]
    raise PtxError("%s: interpolation must be one of %s, Pillow's code 0..5 or an enum of those, got %r" % (
        who, ", ".join(repr(n) for n in ("nearest", "box", "bilinear", "hamming", "bicubic", "lanczos")), interpolation))


def _filter_weight(name):
    """Resample.c's filter functions, operation for operation (Python floats are C doubles; math.sin / math.cos are the C
    library's, as Pillow calls them -- numpy's vector routines may differ in the last bit)."""
    if name == "box":
        return lambda x: 1.0 if -0.5 < x <= 0.5 else 0.0
    if name == "bilinear":
        def bilinear(x):
            x = -x if x < 0.0 else x
            return 1.0 - x if x < 1.0 else 0.0
        return bilinear
    if name == "hamming":
        c54, c46 = float(np.float32(0.54)), float(np.float32(0.46))    # 0.54f, 0.46f in the C source
        def hamming(x):
            x = -x if x < 0.0 else x
            if x == 0.0:
                return 1.0
            if x >= 1.0:
                return 0.0
            x = x * math.pi
            return math.sin(x) / x * (c54 + c46 * math.cos(x))
        return hamming
    if name == "bicubic":
        a = -0.5
        def bicubic(x):
            x = -x if x < 0.0 else x
            if x < 1.0:
                return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
            if x < 2.0:
                return (((x - 5) * x + 8) * x - 4) * a
            return 0.0
        return bicubic

    def sinc(x):
        if x == 0.0:
            return 1.0
        x = x * math.pi
        return math.sin(x) / x
    return lambda x: sinc(x) * sinc(x / 3) if -3.0 <= x < 3.0 else 0.0          # lanczos: a truncated sinc


_FILTER_TABLES = collections.OrderedDict()                # (n_in, n_out, filter) -> read-only (lo, n, k)
_FILTER_TABLES_MAX = 256


def _filter_axis_table(n_in, n_out, name):
    """resize_axis_table for the filters other than bilinear: a scalar restatement of precompute_coeffs +
    normalize_coeffs_8bpc (and of ImagingScaleAffine's index walk for nearest), paid once per (n_in, n_out, filter)."""
    key = (n_in, n_out, name)
    hit = _FILTER_TABLES.get(key)
    if hit is not None:
        _FILTER_TABLES.move_to_end(key)
        return hit
    if name == "nearest":                                  # xo = a * 0.5; idx[x] = (int)xo; xo += a -- sequential in fp64
        a = n_in / n_out
        xo, lo = a * 0.5, np.empty(n_out, np.int32)
        for x in range(n_out):
            lo[x] = min(int(xo), n_in - 1)
            xo += a
        hit = (lo, np.ones(n_out, np.int32), np.full((n_out, 1), 1 << PRECISION_BITS, np.int32))
    else:
        weight = _filter_weight(name)
        scale = n_in / n_out
        fs = max(scale, 1.0)
        support = _SUPPORT[name] * fs
        ksize = int(math.ceil(support)) * 2 + 1
        ss = 1.0 / fs
        one = float(1 << PRECISION_BITS)
        lo, n, k = np.empty(n_out, np.int32), np.empty(n_out, np.int32), np.zeros((n_out, ksize), np.int32)
        for xx in range(n_out):
            center = (xx + 0.5) * scale
            xmin = max(int(center - support + 0.5), 0)     # int() truncates, as C's (int)
            xmax = min(int(center + support + 0.5), n_in) - xmin
            w = [weight((x + xmin - center + 0.5) * ss) for x in range(xmax)]
            ww = 0.0
            for v in w:
                ww += v
            if ww != 0.0:
                w = [v / ww for v in w]
            k[xx, :xmax] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
            lo[xx], n[xx] = xmin, xmax
        hit = (lo, n, np.ascontiguousarray(k[:, :int(n.max())]))
    for a_ in hit:
        a_.flags.writeable = False
    _FILTER_TABLES[key] = hit
    while len(_FILTER_TABLES) > _FILTER_TABLES_MAX:
        _FILTER_TABLES.popitem(last=False)
    return hit


def check_coefficients(k, who="TransformFrames"):
    """What the kernels need of a coefficient table k[entries][taps] (ptx_amd_resample.h): every |k| < 2**23 (the 24-bit
    multiply) and per entry 255 * sum|k| + 2**21 < 2**31 (the 32-bit accumulator), else PtxError.  Pillow's own tables of every
    filter keep far inside both (the largest sum|k| is about 1.55 * 2**22)."""
    k = np.abs(np.asarray(k).astype(np.int64))
    if k.size and int(k.max()) >= 1 << 23:
        raise PtxError("%s: a resize coefficient of magnitude %d is not below 2**23 (the kernels multiply 24-bit integers)" % (
            who, int(k.max())))
    total = k.reshape(k.shape[0], -1).sum(axis=1) if k.ndim > 1 else k
    if total.size and 255 * int(total.max()) + (1 << (PRECISION_BITS - 1)) >= 1 << 31:
        raise PtxError("%s: a resize table entry with sum|k| = %d overflows the 32-bit accumulator (255 * sum|k| + 2**21 must "
                       "stay below 2**31)" % (who, int(total.max())))


def resize_axis_table(n_in, n_out, interpolation="bilinear"):
    """PIL's coefficients of a resize filter for one axis (precompute_coeffs + normalize_coeffs_8bpc): for every output
    index the first input index `lo`, the tap count `n` and `n` int32 coefficients (2**22 fixed point; negative ones where
    the filter has negative lobes), as (lo[n_out], n[n_out], k[n_out][taps]) with taps = max(n).  An axis that is not
    resampled is one tap of 2**22 for every filter (PIL skips that pass).  "nearest" is PIL's affine index walk as one-tap
    entries.  Tables of the filters other than bilinear are cached and read-only."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in <= 0 or n_out <= 0:
        raise PtxError("TransformFrames: non-positive extent (%d -> %d)" % (n_in, n_out))
    if n_in == n_out:
        return (np.arange(n_out, dtype=np.int32), np.ones(n_out, np.int32),
                np.full((n_out, 1), 1 << PRECISION_BITS, np.int32))
    name = interpolation if interpolation == "bilinear" else check_interpolation(interpolation)
    if name != "bilinear":
        return _filter_axis_table(n_in, n_out, name)
    scale = n_in / n_out                                   # the bilinear branch: vectorised, its bits pinned by the tests
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


def _check_taps(rows, cols, H, W, h, w, interpolation="bilinear", who="TransformFrames"):
    """The tap cap and the coefficient bounds of a pair of tables (see check_coefficients)."""
    for name, t in (("rows", rows), ("columns", cols)):
        if t[2].shape[1] > _lib.PTX_RESIZE_MAX_TAPS:
            raise PtxError("%s: down-scaling the %s of a %dx%d frame to %dx%d%s needs %d taps, the kernel's cap is "
                           "PTX_RESIZE_MAX_TAPS = %d" % (who, name, H, W, h, w, "" if interpolation == "bilinear" else
                                                         " with the %s filter" % interpolation, t[2].shape[1],
                                                         _lib.PTX_RESIZE_MAX_TAPS))
        check_coefficients(t[2], who)


def build_tables(H, W, input_size, scale=0.875, preserve_aspect_ratio=True, crop="center", hflip=False, vflip=False,
                 interpolation="bilinear"):
    """Row and column tables of resize + crop (+ flips) for H x W frames: only the S output rows / columns of the
    window get entries (reversed where a flip asks for it).  Returns a dict with `rows`, `cols` ((lo, n, k) each), `S`,
    `resized`, `window`.  interpolation: the resize filter (see `check_interpolation`)."""
    S = int(max(input_size))
    h, w = resized_size(H, W, input_size, scale, preserve_aspect_ratio)
    if h <= 0 or w <= 0:
        raise PtxError("TransformFrames: resized frame %dx%d is empty" % (h, w))
    top, left = crop_window(h, w, S, crop)
    rows = _select(resize_axis_table(H, h, interpolation), top, S, reverse=bool(vflip))
    cols = _select(resize_axis_table(W, w, interpolation), left, S, reverse=bool(hflip))
    _check_taps(rows, cols, H, W, h, w, interpolation)
    return {"rows": rows, "cols": cols, "S": S, "resized": (h, w), "window": (top, left)}


def build_frame_tables(H, W, input_size, scale=0.875, preserve_aspect_ratio=True, interpolation="bilinear"):
    """Row and column tables of the WHOLE resized frame (h rows, w columns): what the per-clip windows launch indexes.
    `build_tables(.., crop=(top, left), hflip=.., vflip=..)` is the slice [top, top + S) x [left, left + S) of these,
    reversed where a flip asks for it.  Returns a dict with `rows`, `cols`, `S`, `resized`."""
    S = int(max(input_size))
    h, w = resized_size(H, W, input_size, scale, preserve_aspect_ratio)
    if h <= 0 or w <= 0:
        raise PtxError("TransformFrames: resized frame %dx%d is empty" % (h, w))
    if h < S or w < S:
        raise PtxError("TransformFrames: a %dx%d crop does not fit the resized %dx%d frame (padding crops are not "
                       "offered)" % (S, S, h, w))
    rows, cols = resize_axis_table(H, h, interpolation), resize_axis_table(W, w, interpolation)
    _check_taps(rows, cols, H, W, h, w, interpolation)
    return {"rows": rows, "cols": cols, "S": S, "resized": (h, w)}


# ---------------------------------------------------------------------------------------------
# per-clip resize geometry: (box_top, box_left, box_h, box_w, h, w, top, left, hflip, vflip)
# ---------------------------------------------------------------------------------------------
GEOMETRY_FIELDS = ("box_top", "box_left", "box_h", "box_w", "h", "w", "top", "left", "hflip", "vflip")


def geometry_tables(row, S, interpolation="bilinear"):
    """Row and column tables of ONE clip's geometry, in build_tables' form.  The row means, in PIL terms: crop the box
    [box_top, +box_h) x [box_left, +box_w) out of the frame, resize it to h x w (`interpolation`; an axis whose extent
    does not change is not resampled), crop the S x S window at (top, left), mirror if hflip, flip if vflip.  Resizing
    a crop references only the crop's pixels, at positions relative to its origin, so its table is
    `resize_axis_table(box_len, out_len)` with `lo` shifted by the origin; window and flips select and order the
    entries as in build_tables.  The numpy statement of the per-clip tables the device builds (the tests' oracle; the
    product path does not call it)."""
    bt, bl, bh, bw, h, w, top, left, hf, vf = (int(v) for v in row)
    S = int(S)

    def axis(origin, n_in, n_out, start, flip):
        if start < 0 or start + S > n_out:
            raise PtxError("TransformFrames: geometry: the %d-entry window at %d does not fit the resized extent %d" % (S, start, n_out))
        lo, n, k = resize_axis_table(n_in, n_out, interpolation)
        return _select((lo + np.int32(origin), n, k), start, S, reverse=bool(flip))

    t = {"rows": axis(bt, bh, h, top, vf), "cols": axis(bl, bw, w, left, hf), "S": S, "resized": (h, w),
         "window": (top, left)}
    for name in ("rows", "cols"):
        check_coefficients(t[name][2])
    return t


def _axis_taps(n_in, n_out, start, S, interpolation="bilinear"):
    """Largest tap count of the entries [start, start + S) of resize_axis_table(n_in, n_out, interpolation), per clip
    (int64 arrays [N]): lo / hi of the table alone (the same float64 operations, the filter's support), no weight is
    computed.  Nearest is one tap."""
    if interpolation == "nearest":
        return np.ones(len(n_in), np.int64)
    scale = n_in / n_out                                             # int64 / int64: the float64 quotient, as Python's
    fs = np.maximum(scale, 1.0)[:, None]
    if interpolation != "bilinear":
        fs = _SUPPORT[interpolation] * fs                            # the support (bilinear: 1.0 * fs, fs itself)
    center = ((start[:, None] + np.arange(S, dtype=np.int64)[None, :]).astype(np.float64) + 0.5) * scale[:, None]
    lo = np.maximum((center - fs + 0.5).astype(np.int64), 0)
    hi = np.minimum((center + fs + 0.5).astype(np.int64), n_in[:, None])
    return np.where(n_in == n_out, 1, (hi - lo).max(axis=1))


def _axis_bicubic_bound(n_in, n_out, start, S):
    """Per clip (int64 [N]) the largest |k| and the largest sum|k| of the bicubic entries [start, start + S) of every clip's
    axis, vectorised: the per-clip tables are built on the device, so the host bounds what it will not see.  The weights are
    PIL's polynomial in numpy (only + - * /: IEEE, no contraction), summed along the taps."""
    scale = n_in / n_out
    fs = np.maximum(scale, 1.0)[:, None]
    support = 2.0 * fs
    center = ((start[:, None] + np.arange(S, dtype=np.int64)[None, :]).astype(np.float64) + 0.5) * scale[:, None]
    lo = np.maximum((center - support + 0.5).astype(np.int64), 0)
    hi = np.minimum((center + support + 0.5).astype(np.int64), n_in[:, None])
    ksize = int(max((hi - lo).max(), 1))
    j = np.arange(ksize, dtype=np.float64)[None, None, :]
    x = np.abs((j + lo[..., None] - center[..., None] + 0.5) * (1.0 / fs)[..., None])
    a = -0.5
    w = np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1, np.where(x < 2.0, (((x - 5) * x + 8) * x - 4) * a, 0.0))
    w = np.where(j < (hi - lo)[..., None], w, 0.0)
    ww = np.cumsum(w, axis=2)[..., -1:]
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    k = np.where(j < (hi - lo)[..., None], np.abs(w) * float(1 << PRECISION_BITS) + 0.5, 0.0)   # >= |k| of the table, by less than 1 per tap
    same, one = n_in == n_out, float(1 << PRECISION_BITS)           # not resampled: one tap of 2**22
    return np.where(same, one, k.max(axis=(1, 2))), np.where(same, one, k.sum(axis=2).max(axis=1))


def random_resized_crop_box(H, W, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """torchvision's RandomResizedCrop.get_params on an H x W frame: (i, j, h, w), the box's top, left, height, width.
    Up to 10 attempts, each drawing `area = H * W * uniform_(scale[0], scale[1])` and then
    `r = exp(uniform_(log(ratio[0]), log(ratio[1])))` (the logs taken in float32, as torch.log(torch.tensor(ratio)) gives
    them), with w = int(round(sqrt(area * r))), h = int(round(sqrt(area / r))); the first attempt with 0 < w <= W and
    0 < h <= H is accepted and then draws i = randint(0, H - h + 1), j = randint(0, W - w + 1).  After 10 rejections the
    central fallback: the whole frame, cut to ratio[0] (full width) when W / H is below it or to ratio[1] (full height)
    when above, centred; it draws nothing more."""
    g = generator
    area = H * W
    log_ratio = torch.log(torch.tensor([float(ratio[0]), float(ratio[1])]))
    for _ in range(10):
        target = area * torch.empty(1).uniform_(float(scale[0]), float(scale[1]), generator=g).item()
        r = torch.exp(torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]), generator=g)).item()
        w = int(round(math.sqrt(target * r)))
        h = int(round(math.sqrt(target / r)))
        if 0 < w <= W and 0 < h <= H:
            i = int(torch.randint(0, H - h + 1, (1,), generator=g))
            j = int(torch.randint(0, W - w + 1, (1,), generator=g))
            return i, j, h, w
    in_ratio = float(W) / float(H)
    if in_ratio < min(ratio):
        w = W
        h = max(int(round(w / min(ratio))), 1)
    elif in_ratio > max(ratio):
        h = H
        w = max(int(round(h * max(ratio))), 1)
    else:
        w, h = W, H
    return (H - h) // 2, (W - w) // 2, h, w


def apply_tables_numpy(frame, tables):
    """The kernel's arithmetic in numpy (uint8 [H,W,C] -> uint8 [S,S,C]): horizontal pass, uint8 intermediate,
    vertical pass, each `clip((2**21 + sum) >> 22, 0, 255)` with an arithmetic shift (coefficients, and so sums, may be
    negative).  The host-side model the tests compare with PIL; not a fallback (TransformFrames never calls it)."""
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


# ---------------------------------------------------------------------------------------------
# ColorJitter / RandomGrayscale per clip (include/ptx_amd_color.h): the arithmetic contract in numpy, the draw, the launches
# ---------------------------------------------------------------------------------------------
COLOR_OPS = ("none", "brightness", "contrast", "saturation", "hue", "grayscale")          # the PTX_COLOR_* codes, by index
COLOR_MAX_OPS = _lib.PTX_COLOR_MAX_OPS


def color_luma_numpy(rgb):
    """PIL's convert("L") of uint8 [..., 3]: (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16, as int32 [...]."""
    c = np.asarray(rgb).astype(np.int32)
    return (c[..., 0] * 19595 + c[..., 1] * 38470 + c[..., 2] * 7471 + 0x8000) >> 16


def color_blend_numpy(d, x, f):
    """PIL's Image.blend(degenerate, image, f) on integer arrays (ImageEnhance's one operation): t = fp32(d) + fp32(f *
    fp32(x - d)), every operation rounded to fp32; 0 if t <= 0, 255 if t >= 255, else trunc(t).  int32 result."""
    d, x = np.asarray(d).astype(np.int32), np.asarray(x).astype(np.int32)
    t = d.astype(np.float32) + np.float32(f) * (x - d).astype(np.float32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.int32)


def color_rgb_to_hsv_numpy(rgb):
    """PIL's convert("HSV") of uint8 [..., 3] (the contract in include/ptx_amd_color.h): fp32 divisions, the hue assembled in
    fp64 from the widened floats and rounded back to fp32.  uint8 [..., 3]."""
    c = np.asarray(rgb).astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(np.float32)
    s = cr / np.where(grey, 1, maxc).astype(np.float32)
    rc, gc, bc = ((maxc - v).astype(np.float32) / cr for v in (r, g, b))
    rc, gc, bc = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
    hd = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc))
    hf = hd.astype(np.float32)
    h2 = np.fmod(hf.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = np.clip((h2.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    S = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(grey, 0, H), np.where(grey, 0, S), maxc], axis=-1)
    return out.astype(np.uint8)


def color_hsv_to_rgb_numpy(hsv):
    """PIL's HSV -> RGB of uint8 [..., 3], all in fp64; round is floor(a + 0.5) clipped to 0..255.  uint8 [..., 3]."""
    c = np.asarray(hsv).astype(np.int64)
    H, S, V = c[..., 0], c[..., 1], c[..., 2]
    x = H * 6.0 / 255.0
    i = np.floor(x)
    f = x - i
    fs = S / 255.0
    v = V.astype(np.float64)

    def rnd(a):
        return np.clip(np.floor(a + 0.5), 0, 255).astype(np.int64)

    p, q, t = rnd(v * (1.0 - fs)), rnd(v * (1.0 - fs * f)), rnd(v * (1.0 - fs * (1.0 - f)))
    k = i.astype(np.int64) % 6
    pick = lambda a: np.choose(k, a)
    out = np.stack([pick([V, q, p, p, t, V]), pick([t, V, V, q, p, p]), pick([p, p, t, V, V, q])], axis=-1)
    return np.where((S == 0)[..., None], V[..., None], out).astype(np.uint8)


def hue_shift(hue_factor):
    """torchvision's uint8 wrap of adjust_hue: trunc(hue_factor * 255) mod 256, from the factor as a Python float."""
    return int(float(hue_factor) * 255.0) % 256


def _color_rows(ops, N=None, who="ColorJitter"):
    """`ops` = (codes [N, 5] integers, factors [N, 5] floats) -- arrays or CPU tensors -- as contiguous (int32, float32) numpy
    arrays, or PtxError.  Shapes only; the values are checked by ptx_color_jitter_supported."""
    try:
        codes, factors = ops
    except (TypeError, ValueError):
        raise PtxError("%s: params must be a pair (codes [N, %d], factors [N, %d]), got %r" % (who, COLOR_MAX_OPS, COLOR_MAX_OPS, type(ops).__name__))
    arrs = []
    for name, a, kinds in (("codes", codes, "iu"), ("factors", factors, "fiu")):
        a = _host_array(a, "%s: params %s must be an array or a CPU tensor, got a CUDA tensor" % (who, name))
        if a.dtype.kind not in kinds:
            raise PtxError("%s: params %s must hold %s, got dtype %s" % (who, name, "integers" if kinds == "iu" else "numbers", a.dtype))
        if a.ndim != 2 or a.shape[1] != COLOR_MAX_OPS:
            raise PtxError("%s: params %s must be [N, %d], got shape %s" % (who, name, COLOR_MAX_OPS, a.shape))
        if N is not None and a.shape[0] != N:
            raise PtxError("%s: params %s hold %d clips, the frames hold N = %d" % (who, name, a.shape[0], N))
        arrs.append(a)
    if arrs[0].shape != arrs[1].shape:
        raise PtxError("%s: params codes and factors differ in shape: %s and %s" % (who, arrs[0].shape, arrs[1].shape))
    if arrs[0].shape[0] == 0:
        raise PtxError("%s: empty batch" % who)
    return np.ascontiguousarray(arrs[0].astype(np.int32)), np.ascontiguousarray(arrs[1].astype(np.float32))


def check_color_params(ops, N=None, who="ColorJitter"):
    """`ops` as (CPU int32 [N, 5], CPU float32 [N, 5]) tensors, or PtxError with the library's reason: a code out of range, a
    repeated code, a hue shift that is not an integer 0..255, a factor that is negative or not finite.  No device is touched."""
    codes, factors = _color_rows(ops, N, who)
    desc = _lib.ColorDesc(codes.shape[0], 1, 1, 1, _lib.PTX_RESIZE_OUT_U8, int((codes == _lib.PTX_COLOR_CONTRAST).any()))
    if not _lib.lib().ptx_color_jitter_supported(C.byref(desc), C.c_void_p(codes.ctypes.data), C.c_void_p(factors.ctypes.data)):
        raise PtxError("%s: %s" % (who, _lib.lib().ptx_last_error().decode(errors="replace")))
    return torch.from_numpy(codes), torch.from_numpy(factors)


def color_jitter_numpy(frames, ops):
    """The kernels' arithmetic in numpy: uint8 frames [N,T,H,W,3] and `ops` = (codes [N, 5], factors [N, 5]) -> uint8
    [N,T,H,W,3].  Every clip's list runs in order on every frame; contrast takes the mean luma of the FRAME as it stands when
    contrast is applied.  The host-side model the tests compare with PIL; not a fallback (ColorJitter never calls it)."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 5 or frames.shape[-1] != 3:
        raise PtxError("color_jitter_numpy: frames must be uint8 [N,T,H,W,3], got %s %s" % (frames.dtype, frames.shape))
    codes, factors = (t.numpy() for t in check_color_params(ops, frames.shape[0], "color_jitter_numpy"))
    out = np.empty_like(frames)
    for n in range(frames.shape[0]):
        for t in range(frames.shape[1]):
            img = frames[n, t].astype(np.int32)
            for code, f in zip(codes[n].tolist(), factors[n]):
                name = COLOR_OPS[code]
                if name == "brightness":
                    img = color_blend_numpy(0, img, f)
                elif name == "contrast":
                    lum = color_luma_numpy(img)
                    m = int(int(lum.sum()) / lum.size + 0.5)
                    img = color_blend_numpy(m, img, f)
                elif name == "saturation":
                    img = color_blend_numpy(color_luma_numpy(img)[..., None], img, f)
                elif name == "hue":
                    hsv = color_rgb_to_hsv_numpy(img)
                    hsv[..., 0] += np.uint8(int(f) & 255)                    # uint8 wrap
                    img = color_hsv_to_rgb_numpy(hsv).astype(np.int32)
                elif name == "grayscale":
                    img = np.repeat(color_luma_numpy(img)[..., None], 3, axis=-1)
            out[n, t] = img.astype(np.uint8)
    return out


class ColorJitter:
    """torchvision's ColorJitter (+ RandomGrayscale) on decoded uint8 frames on the device, one draw per CLIP, equal to the
    PIL-image code path (ImageEnhance.Brightness / Contrast / Color, the HSV round trip of adjust_hue, convert("L")) bit for
    bit.  include/ptx_amd_color.h states the arithmetic, `color_jitter_numpy` restates it.

    brightness / contrast / saturation: a number v gives the range [max(0, 1 - v), 1 + v], a pair (lo, hi) with 0 <= lo <= hi
    is taken as it is; hue: v in [0, 0.5] gives [-v, v], a pair lies inside [-0.5, 0.5].  A range that is the identity alone
    (0, or (1, 1); (0, 0) for hue) switches the op off: nothing is drawn for it and it does not run.  grayscale: the
    probability of RandomGrayscale, applied after the jitter.  generator: a CPU torch.Generator (None: torch's default one).

    `cj(frames)` jitters uint8 CUDA frames [N,T,H,W,3] | [T,H,W,3] | [H,W,3] (one draw per clip: N, or one) and keeps the draw
    as `last_params` = (codes CPU int32 [N, 5], factors CPU float32 [N, 5]): per clip the ordered op list, codes indexing
    `COLOR_OPS`, the factor of hue being the integer shift `hue_shift(h)`.  `cj(frames, params=p)` applies given lists.
    A call is one small upload and one launch, plus a statistics launch when a list holds contrast (`last_launches`)."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, grayscale=0.0, generator=None):
        self.brightness = self._range(brightness, "brightness")
        self.contrast = self._range(contrast, "contrast")
        self.saturation = self._range(saturation, "saturation")
        self.hue = self._range(hue, "hue", center=0.0, bound=(-0.5, 0.5), clip=False)
        if isinstance(grayscale, bool) or not isinstance(grayscale, (int, float)) or not 0.0 <= grayscale <= 1.0:
            raise PtxError("ColorJitter: grayscale must be a probability in [0, 1], got %r" % (grayscale,))
        self.grayscale = float(grayscale)
        self.generator, self.last_params, self.last_launches = _check_generator(generator, "ColorJitter"), None, ()

    @staticmethod
    def _range(value, name, center=1.0, bound=(0.0, float("inf")), clip=True):
        """torchvision's ColorJitter._check_input: the (lo, hi) range of a factor, or None when the op is off."""
        if isinstance(value, bool):
            raise PtxError("ColorJitter: %s must be a number or a pair (lo, hi), got %r" % (name, value))
        if isinstance(value, (int, float)):
            if not value >= 0 or not math.isfinite(value):
                raise PtxError("ColorJitter: %s=%r: a single number must be non-negative and finite" % (name, value))
            lo, hi = center - float(value), center + float(value)
            if clip:
                lo = max(lo, 0.0)
        else:
            try:
                lo, hi = (float(v) for v in value)
            except (TypeError, ValueError):
                raise PtxError("ColorJitter: %s must be a number or a pair (lo, hi), got %r" % (name, value))
        if not (bound[0] <= lo <= hi <= bound[1]) or not math.isfinite(hi):
            raise PtxError("ColorJitter: %s: the range (%r, %r) must be ordered and lie inside [%g, %g]" % (name, lo, hi, bound[0], bound[1]))
        return None if lo == hi == center else (lo, hi)

    def draw(self, n):
        """Lists of n clips: (codes CPU int32 [n, 5], factors CPU float32 [n, 5]).  Per clip, in torchvision's order, from
        `generator`: torch.randperm(4); torch.empty(1).uniform_(lo, hi) for each enabled one of brightness, contrast,
        saturation, hue, in that order; if grayscale > 0, torch.rand(1) < grayscale.  The enabled ops run in the permutation's
        order (0 brightness, 1 contrast, 2 saturation, 3 hue), grayscale last; factors stay the fp32 values drawn."""
        g = self.generator
        codes = torch.zeros((int(n), COLOR_MAX_OPS), dtype=torch.int32)
        factors = torch.zeros((int(n), COLOR_MAX_OPS), dtype=torch.float32)
        ranges = (self.brightness, self.contrast, self.saturation, self.hue)
        for i in range(int(n)):
            order = torch.randperm(4, generator=g).tolist()
            drawn = [None if r is None else torch.empty(1).uniform_(r[0], r[1], generator=g)[0] for r in ranges]
            gray = self.grayscale > 0 and bool(torch.rand(1, generator=g) < self.grayscale)
            k = 0
            for fn in order:
                if drawn[fn] is None:
                    continue
                codes[i, k] = fn + 1
                factors[i, k] = float(hue_shift(float(drawn[fn]))) if fn == 3 else drawn[fn]
                k += 1
            if gray:
                codes[i, k] = _lib.PTX_COLOR_GRAYSCALE
        return codes, factors

    def check_params(self, params, N=None):
        """See `check_color_params`."""
        return check_color_params(params, N)

    def _launch(self, f5, params, mode, norm, dtype):
        """The launches on contiguous uint8 CUDA frames f5 [N,T,H,W,3] with checked params: uint8 [N,T,H,W,3] or the
        normalised [N,3,T,H,W] of `dtype`."""
        codes, factors = params
        N, T, H, W, _ = f5.shape
        contrast = bool((codes == _lib.PTX_COLOR_CONTRAST).any())
        lib = _lib.lib()
        with torch.cuda.device(f5.device):
            rows = torch.cat([codes.reshape(-1).view(torch.uint8), factors.reshape(-1).view(torch.uint8)]).to(f5.device)   # one upload
            ops_p, fac_p = C.c_void_p(rows.data_ptr()), C.c_void_p(rows.data_ptr() + N * COLOR_MAX_OPS * 4)
            desc = _lib.ColorDesc(N, T, H, W, mode, int(contrast))
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            sums = None
            if contrast:
                sums = torch.empty(N * T, device=f5.device, dtype=torch.int64)
                check(lib.ptx_color_jitter_stats(C.byref(desc), C.c_void_p(f5.data_ptr()), ops_p, fac_p, C.c_void_p(sums.data_ptr()),
                                                 stream), "ptx_color_jitter_stats")
            y = _alloc_out(mode, N, T, H, W, f5.device, dtype)
            check(lib.ptx_color_jitter_apply(C.byref(desc), C.c_void_p(f5.data_ptr()), ops_p, fac_p,
                                             C.c_void_p(sums.data_ptr()) if contrast else None, C.c_void_p(y.data_ptr()),
                                             C.byref(norm) if norm is not None else None, stream), "ptx_color_jitter_apply")
        self.last_launches = ("stats", "apply") if contrast else ("apply",)
        return y

    def _run(self, f5, params, mode=_lib.PTX_RESIZE_OUT_U8, norm=None, dtype=torch.uint8):
        """The stage on contiguous uint8 frames f5 [N,T,H,W,3]: `params`, or a draw that is kept as `last_params`; see `_launch`."""
        if params is None:
            params = self.last_params = self.draw(f5.shape[0])
        return self._launch(f5, self.check_params(params, f5.shape[0]), mode, norm, dtype)

    def __call__(self, frames, params=None):
        N = _frames_shape(frames, "ColorJitter")[0]
        if params is not None:                                       # validated before a device is touched
            params = self.check_params(params, N)
        f5 = _u8_cuda_5d(frames, "ColorJitter")
        _check_not_empty(frames, "ColorJitter")
        return self._run(f5, params).view(frames.shape)


# ---------------------------------------------------------------------------------------------
# GaussianBlur per clip (include/ptx_amd_blur.h): torchvision's weights, the arithmetic contract in numpy, the draw, the launch
# ---------------------------------------------------------------------------------------------
BLUR_MAX_TAPS = _lib.PTX_BLUR_MAX_TAPS


def _blur_kernel_size(kernel_size, who="GaussianBlur"):
    """(kx, ky) of `kernel_size` (an int or a pair (kx, ky), torchvision's order): odd, 1 .. PTX_BLUR_MAX_TAPS."""
    ks = (kernel_size, kernel_size) if isinstance(kernel_size, int) and not isinstance(kernel_size, bool) else kernel_size
    try:
        ks = tuple(ks)
        ok = len(ks) == 2 and all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) for k in ks)
    except TypeError:
        ok = False
    if not ok:
        raise PtxError("%s: kernel_size must be an int or a pair (kx, ky) of ints, got %r" % (who, kernel_size))
    for k in ks:
        if k < 1 or k % 2 == 0 or k > BLUR_MAX_TAPS:
            raise PtxError("%s: kernel_size=%r: every size must be odd and 1 .. %d (PTX_BLUR_MAX_TAPS)" % (who, kernel_size, BLUR_MAX_TAPS))
    return int(ks[0]), int(ks[1])


def gaussian_kernel1d(k, sigma):
    """torchvision's `_get_gaussian_kernel1d(k, sigma)` in float32, with the same torch CPU ops and therefore the same bits: a
    CPU float32 tensor [k].  k: odd, >= 1; sigma > 0."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k % 2 == 0:
        raise PtxError("gaussian_kernel1d: k must be an odd integer >= 1, got %r" % (k,))
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.floating)) or not (sigma > 0) or not math.isfinite(sigma):
        raise PtxError("gaussian_kernel1d: sigma must be a finite number > 0, got %r" % (sigma,))
    sigma = float(sigma)
    half = (int(k) - 1) * 0.5
    x = torch.linspace(-half, half, steps=int(k), dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def _blur_reflect(i, n):
    """torch's "reflect" padding index for i in (-n, 2 n - 1)."""
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def _blur_rows(apply, wx, wy, N, who):
    """(apply int32 [N], wx float32 [N, kx], wy float32 [N, ky]) as contiguous numpy arrays; a 1-D weight row serves every clip."""
    arrs = []
    for name, a in (("apply", apply), ("wx", wx), ("wy", wy)):
        arrs.append(_host_array(a, "%s: %s must be an array or a CPU tensor, got a CUDA tensor" % (who, name)))
    ap, wx, wy = arrs
    if ap.dtype.kind not in "iub" or ap.ndim != 1 or ap.shape[0] != N:
        raise PtxError("%s: apply must hold N = %d integer flags, got dtype %s shape %s" % (who, N, ap.dtype, ap.shape))
    out = [np.ascontiguousarray(ap.astype(np.int32))]
    for name, w in (("wx", wx), ("wy", wy)):
        if w.dtype.kind != "f":
            raise PtxError("%s: %s must hold floats, got dtype %s" % (who, name, w.dtype))
        if w.ndim == 1:
            w = np.broadcast_to(w, (N, w.shape[0]))
        if w.ndim != 2 or w.shape[0] != N or w.shape[1] < 1:
            raise PtxError("%s: %s must be [N, k] or [k] with N = %d, got shape %s" % (who, name, N, w.shape))
        w32 = np.ascontiguousarray(w.astype(np.float32))
        if not np.array_equal(w32.astype(w.dtype), w, equal_nan=True):
            raise PtxError("%s: %s must hold float32 values (the device reads fp32 weights)" % (who, name))
        out.append(w32)
    return tuple(out)


def _blur_supported(apply, wx, wy, H, W, who, mode=_lib.PTX_RESIZE_OUT_U8, T=1):
    """The library's host-side check of a launch (no device is touched), with its reason as a PtxError; the reflect condition is
    named in the caller's terms first."""
    kx, ky = wx.shape[1], wy.shape[1]
    if kx // 2 >= W or ky // 2 >= H:
        raise PtxError("%s: kernel_size=(%d, %d) does not fit frames of H=%d, W=%d: reflect padding needs kx // 2 < W and "
                       "ky // 2 < H (torch raises there too)" % (who, kx, ky, H, W))
    desc = _lib.BlurDesc(apply.shape[0], T, H, W, kx, ky, mode)
    if not _lib.lib().ptx_gaussian_blur_supported(C.byref(desc), C.c_void_p(apply.ctypes.data), C.c_void_p(wx.ctypes.data),
                                                  C.c_void_p(wy.ctypes.data)):
        raise PtxError("%s: %s" % (who, _lib.lib().ptx_last_error().decode(errors="replace")))


def gaussian_blur_numpy(frames, apply, wx, wy, return_real=False):
    """The kernel's arithmetic in numpy: uint8 frames [N,T,H,W,3], flags [N], float32 weights wx [N, kx] and wy [N, ky] (a 1-D row
    serves every clip) -> uint8 [N,T,H,W,3].  Per frame and channel, in float64, the taps in ascending order from 0.0, every
    product and every add rounded on its own: the horizontal pass h = sum_j wx[j] * p[y][refl(x + j - kx // 2)], the vertical
    pass v = sum_i wy[i] * h[refl(y + i - ky // 2)][x], out = clip(round_half_to_even(v), 0, 255); a clip whose flag is 0 is
    copied.  return_real=True returns (out, v) with v float64 (the bytes themselves for a copied clip).  The host-side model
    the tests compare the device with; not a fallback (GaussianBlur never calls it)."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 5 or frames.shape[-1] != 3:
        raise PtxError("gaussian_blur_numpy: frames must be uint8 [N,T,H,W,3], got %s %s" % (frames.dtype, frames.shape))
    N, T, H, W, _ = frames.shape
    if frames.size == 0:
        raise PtxError("gaussian_blur_numpy: empty batch")
    apply, wx, wy = _blur_rows(apply, wx, wy, N, "gaussian_blur_numpy")
    _blur_supported(apply, wx, wy, H, W, "gaussian_blur_numpy")
    kx, ky = wx.shape[1], wy.shape[1]
    xi = _blur_reflect(np.arange(W)[None, :] + np.arange(kx)[:, None] - kx // 2, W)           # [kx, W]
    yi = _blur_reflect(np.arange(H)[None, :] + np.arange(ky)[:, None] - ky // 2, H)           # [ky, H]
    out = np.empty_like(frames)
    real = np.empty(frames.shape, np.float64) if return_real else None
    for n in range(N):
        p = frames[n].astype(np.float64)
        if apply[n]:
            h = np.zeros_like(p)
            for j in range(kx):
                h = h + np.float64(wx[n, j]) * p[:, :, xi[j], :]
            v = np.zeros_like(p)
            for i in range(ky):
                v = v + np.float64(wy[n, i]) * h[:, yi[i], :, :]
            out[n] = np.clip(np.rint(v), 0.0, 255.0).astype(np.uint8)
        else:
            v = p
            out[n] = frames[n]
        if return_real:
            real[n] = v
    return (out, real) if return_real else out


class GaussianBlur:
    """torchvision's GaussianBlur (inside RandomApply when `p` is given) on decoded uint8 frames on the device, one draw per CLIP:
    the blur of the SimCLR / MoCo / BYOL view recipes and their video forms.  include/ptx_amd_blur.h states the arithmetic (a
    separable float64 blur with reflect padding, rounded half to even), `gaussian_blur_numpy` restates it; it is torchvision's
    result up to one level where the real value lies within fp32 summation error of a tie.

    kernel_size: an odd int or a pair (kx, ky), each 1 .. 33; sigma: a number > 0 or a range (lo, hi) with 0 < lo <= hi, one
    value per clip for both axes; p: None (every clip is blurred) or the probability of RandomApply; generator: a CPU
    torch.Generator (None: torch's default one).

    `gb(frames)` blurs uint8 CUDA frames [N,T,H,W,3] | [T,H,W,3] | [H,W,3] (one draw per clip: N, or one) and keeps the draw as
    `last_params` = (apply CPU int32 [N], sigma CPU float64 [N]; 0.0 where a clip is not blurred).  `gb(frames, params=p)`
    applies a given draw.  A call is one small upload (flags and weights) and one launch."""

    def __init__(self, kernel_size, sigma=(0.1, 2.0), p=None, generator=None):
        self.kernel_size = _blur_kernel_size(kernel_size)
        if isinstance(sigma, bool):
            raise PtxError("GaussianBlur: sigma must be a number > 0 or a range (lo, hi), got %r" % (sigma,))
        if isinstance(sigma, (int, float)):
            lo = hi = float(sigma)
            self.sigma_range = None
        else:
            try:
                lo, hi = (float(v) for v in sigma)
            except (TypeError, ValueError):
                raise PtxError("GaussianBlur: sigma must be a number > 0 or a range (lo, hi), got %r" % (sigma,))
            self.sigma_range = (lo, hi)
        if not (0.0 < lo <= hi) or not math.isfinite(hi):
            raise PtxError("GaussianBlur: sigma=%r: values must be finite, > 0 and ordered" % (sigma,))
        self.sigma = (lo, hi)
        if p is not None and (isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0):
            raise PtxError("GaussianBlur: p must be None or a probability in [0, 1], got %r" % (p,))
        self.p = None if p is None else float(p)
        self.generator, self.last_params = _check_generator(generator, "GaussianBlur"), None

    def draw(self, n):
        """The draw of n clips: (apply CPU int32 [n], sigma CPU float64 [n]).  Per clip, in clip order, from `generator`: with p
        given, u = torch.rand(1) and the clip is blurred iff u <= p (torchvision's RandomApply skips when p < u); only a blurred
        clip draws a sigma, torch.empty(1).uniform_(lo, hi).item() (torchvision's GaussianBlur.get_params), when sigma is a
        range.  p=None and a scalar sigma consume nothing.  A clip that is not blurred has sigma 0.0."""
        g = self.generator
        apply = torch.ones(int(n), dtype=torch.int32)
        sigma = torch.zeros(int(n), dtype=torch.float64)
        for i in range(int(n)):
            if self.p is not None and not bool(torch.rand(1, generator=g) <= self.p):
                apply[i] = 0
                continue
            if self.sigma_range is None:
                sigma[i] = self.sigma[0]
            else:
                sigma[i] = torch.empty(1).uniform_(self.sigma[0], self.sigma[1], generator=g).item()
        return apply, sigma

    def weights(self, params):
        """(wx CPU float32 [N, kx], wy CPU float32 [N, ky]) of a checked draw: `gaussian_kernel1d` per blurred clip, the one-hot
        centre row for a clip that is not blurred (the launch does not read it)."""
        apply, sigma = params
        kx, ky = self.kernel_size
        wx, wy = torch.zeros((len(apply), kx), dtype=torch.float32), torch.zeros((len(apply), ky), dtype=torch.float32)
        wx[:, kx // 2], wy[:, ky // 2] = 1.0, 1.0
        for i in range(len(apply)):
            if int(apply[i]):
                wx[i], wy[i] = gaussian_kernel1d(kx, float(sigma[i])), gaussian_kernel1d(ky, float(sigma[i]))
        return wx, wy

    def check_params(self, params, N=None, H=None, W=None):
        """`params` = (apply [N] integers, sigma [N] numbers) -- arrays or CPU tensors -- as (CPU int32, CPU float64) tensors, or
        PtxError: N does not match, a flag is not 0 or 1, the sigma of a blurred clip is not finite and > 0, and, with H and W
        given, a kernel_size that reflect padding cannot serve on H x W frames.  No device is touched."""
        try:
            apply, sigma = params
        except (TypeError, ValueError):
            raise PtxError("GaussianBlur: params must be a pair (apply [N], sigma [N]), got %r" % (params,))
        arrs = []
        for name, a in (("apply", apply), ("sigma", sigma)):
            arrs.append(_host_array(a, "GaussianBlur: params: %s must be an array or a CPU tensor, got a CUDA tensor" % name))
        ap, sg = arrs
        if ap.dtype.kind not in "iu" or ap.ndim != 1:
            raise PtxError("GaussianBlur: params: apply must be [N] integers, got dtype %s shape %s" % (ap.dtype, ap.shape))
        if sg.dtype.kind not in "fiu" or sg.shape != ap.shape:
            raise PtxError("GaussianBlur: params: sigma must be [N] numbers like apply, got dtype %s shape %s" % (sg.dtype, sg.shape))
        if N is not None and ap.shape[0] != N:
            raise PtxError("GaussianBlur: params hold %d clips, the frames hold N = %d" % (ap.shape[0], N))
        if ap.shape[0] == 0:
            raise PtxError("GaussianBlur: params: empty batch")
        sg = sg.astype(np.float64)
        for i, (a, s) in enumerate(zip(ap.tolist(), sg.tolist())):
            if a not in (0, 1):
                raise PtxError("GaussianBlur: params[%d]: the apply flag must be 0 or 1, got %d" % (i, a))
            if a and not (s > 0.0 and math.isfinite(s)):
                raise PtxError("GaussianBlur: params[%d]: sigma must be finite and > 0, got %r" % (i, s))
        out = torch.from_numpy(ap.astype(np.int32)), torch.from_numpy(np.where(ap != 0, sg, 0.0))
        kx, ky = self.kernel_size
        wx, wy = self.weights(out)
        _blur_supported(out[0].numpy(), wx.numpy(), wy.numpy(), ky // 2 + 1 if H is None else int(H), kx // 2 + 1 if W is None else int(W),
                        "GaussianBlur")
        return out

    def _params_for(self, N, H, W, params):
        if params is None:
            self.last_params = self.draw(N)
            return self.check_params(self.last_params, N, H, W)
        return self.check_params(params, N, H, W)

    def _run(self, f5, params, mode=_lib.PTX_RESIZE_OUT_U8, norm=None, dtype=torch.uint8):
        """The stage on contiguous uint8 frames f5 [N,T,H,W,3]: `params`, or a draw that is kept as `last_params`; see `_launch`."""
        return self._launch(f5, self._params_for(f5.shape[0], f5.shape[2], f5.shape[3], params), mode, norm, dtype)

    def _launch(self, f5, params, mode, norm, dtype):
        """The launch on contiguous uint8 CUDA frames f5 [N,T,H,W,3] with checked params: uint8 [N,T,H,W,3] or the normalised
        [N,3,T,H,W] of `dtype`."""
        N, T, H, W, _ = f5.shape
        kx, ky = self.kernel_size
        wx, wy = self.weights(params)
        with torch.cuda.device(f5.device):
            rows = torch.cat([params[0].reshape(-1).view(torch.uint8), wx.reshape(-1).view(torch.uint8),
                              wy.reshape(-1).view(torch.uint8)]).to(f5.device)                       # one upload
            base = rows.data_ptr()
            y = _alloc_out(mode, N, T, H, W, f5.device, dtype)
            desc = _lib.BlurDesc(N, T, H, W, kx, ky, mode)
            check(_lib.lib().ptx_gaussian_blur_frames(C.byref(desc), C.c_void_p(f5.data_ptr()), C.c_void_p(base),
                                                      C.c_void_p(base + 4 * N), C.c_void_p(base + 4 * N * (1 + kx)),
                                                      C.c_void_p(y.data_ptr()), C.byref(norm) if norm is not None else None,
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ptx_gaussian_blur_frames")
        return y

    def __call__(self, frames, params=None):
        N, _, H, W = _frames_shape(frames, "GaussianBlur")
        _check_not_empty(frames, "GaussianBlur")
        kx, ky = self.kernel_size
        if kx // 2 >= W or ky // 2 >= H:                             # before a draw and before a device is touched
            raise PtxError("GaussianBlur: kernel_size=(%d, %d) does not fit frames of H=%d, W=%d: reflect padding needs "
                           "kx // 2 < W and ky // 2 < H (torch raises there too)" % (kx, ky, H, W))
        if params is not None:                                       # validated before a device is touched
            params = self.check_params(params, N, H, W)
        return self._run(_u8_cuda_5d(frames, "GaussianBlur"), params).view(frames.shape)


# ---------------------------------------------------------------------------------------------
# RandAugment per clip (include/ptx_amd_randaug.h): the op table and the draw, PIL's affine coefficients, the arithmetic contract
# in numpy, the launches
# ---------------------------------------------------------------------------------------------
RANDAUG_OPS = ("identity", "shear_x", "shear_y", "translate_x", "translate_y", "rotate", "brightness", "color", "contrast",
               "sharpness", "posterize", "solarize", "autocontrast", "equalize")             # the PTX_RANDAUG_* codes, by index
RANDAUG_SIGNED = (False,) + (True,) * 9 + (False,) * 4
RANDAUG_MAX_OPS = _lib.PTX_RANDAUG_MAX_OPS
_RANDAUG_GEOMETRIC = range(_lib.PTX_RANDAUG_SHEAR_X, _lib.PTX_RANDAUG_ROTATE + 1)
_RANDAUG_ENHANCE = range(_lib.PTX_RANDAUG_BRIGHTNESS, _lib.PTX_RANDAUG_SHARPNESS + 1)
_RANDAUG_STATS = (_lib.PTX_RANDAUG_CONTRAST, _lib.PTX_RANDAUG_AUTOCONTRAST, _lib.PTX_RANDAUG_EQUALIZE)


def rand_augment_space(num_bins, H, W):
    """torchvision's RandAugment._augmentation_space(num_bins, (H, W)): per op code the float32 magnitude table (None: the op
    takes no magnitude), in RANDAUG_OPS order."""
    lin = lambda a, b: torch.linspace(a, b, num_bins)
    return [None, lin(0.0, 0.3), lin(0.0, 0.3), lin(0.0, 150.0 / 331.0 * W), lin(0.0, 150.0 / 331.0 * H), lin(0.0, 30.0),
            lin(0.0, 0.9), lin(0.0, 0.9), lin(0.0, 0.9), lin(0.0, 0.9),
            8 - (torch.arange(num_bins) / ((num_bins - 1) / 4)).round().int(), lin(255.0, 0.0), None, None]


def _inverse_affine_matrix(center, angle, translate, shear, scale=1.0):
    """torchvision's _get_inverse_affine_matrix: PIL's six coefficients, output pixel -> input position.  `scale` divides the
    six entries before the translation and the centre go in, as torchvision does."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [v / scale for v in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def rand_augment_matrix(code, magnitude, H, W):
    """The six coefficients that torchvision's RandAugment hands to Image.transform(AFFINE) for a geometric op (codes 1..5) of
    `magnitude` on an H x W image: F.affine's inverse matrix for the shears (centre (0, 0)) and translations (centre (W * 0.5,
    H * 0.5), the offset truncated to an integer), PIL.Image.Image.rotate's own matrix for the rotation."""
    mag = float(magnitude)
    if code == _lib.PTX_RANDAUG_SHEAR_X:
        return _inverse_affine_matrix((0.0, 0.0), 0.0, (0, 0), (math.degrees(math.atan(mag)), 0.0))
    if code == _lib.PTX_RANDAUG_SHEAR_Y:
        return _inverse_affine_matrix((0.0, 0.0), 0.0, (0, 0), (0.0, math.degrees(math.atan(mag))))
    if code == _lib.PTX_RANDAUG_TRANSLATE_X:
        return _inverse_affine_matrix((W * 0.5, H * 0.5), 0.0, (int(mag), 0), (0.0, 0.0))
    if code == _lib.PTX_RANDAUG_TRANSLATE_Y:
        return _inverse_affine_matrix((W * 0.5, H * 0.5), 0.0, (0, int(mag)), (0.0, 0.0))
    if code != _lib.PTX_RANDAUG_ROTATE:
        raise PtxError("rand_augment_matrix: op code %r is not geometric (1..5)" % (code,))
    return rotation_matrix(mag, H, W)


def rotation_matrix(angle, H, W, center=None):
    """PIL.Image.Image.rotate's own matrix (expand=False, no translate) for `angle` degrees counter-clockwise on an H x W image:
    the sine and cosine rounded to 15 decimals, about `center` = (cx, cy) (None: (W / 2, H / 2))."""
    angle = -math.radians(float(angle) % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = (W / 2, H / 2) if center is None else center
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def affine_fixed(m, H, W, who="RandAugment"):
    """PIL's 16.16 fixed-point form (a0 .. a5) of the affine coefficients m for an H x W image (Geometry.c, affine_fixed), or
    PtxError when PIL itself would leave the fixed-point walk: a source coordinate of a frame corner at or beyond +-32768."""
    for x, y in ((0, 0), (W, 0), (0, H), (W, H)):
        if not (abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0):
            raise PtxError("%s: the affine coefficients leave PIL's fixed-point range on a %dx%d frame (a source coordinate beyond "
                           "+-32768); such frames are not offered" % (who, H, W))
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))
    a = [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    if any(not -2 ** 31 <= v < 2 ** 31 for v in a):
        raise PtxError("%s: the affine coefficients leave PIL's fixed-point range on a %dx%d frame (a source coordinate beyond "
                       "+-32768); such frames are not offered" % (who, H, W))
    return a


def _randaug_params(params, N=None, who="RandAugment"):
    """`params` = (codes [N, K] integers, magnitudes [N, K] numbers) -- arrays or CPU tensors -- as contiguous (int32, float64)
    numpy arrays, or PtxError: shapes, K outside 1..PTX_RANDAUG_MAX_OPS, a code out of range, a magnitude that an op cannot take."""
    try:
        codes, mags = params
    except (TypeError, ValueError):
        raise PtxError("%s: params must be a pair (codes [N, num_ops], magnitudes [N, num_ops]), got %r" % (who, type(params).__name__))
    arrs = []
    for name, a, kinds in (("codes", codes, "iu"), ("magnitudes", mags, "fiu")):
        a = _host_array(a, "%s: params %s must be an array or a CPU tensor, got a CUDA tensor" % (who, name))
        if a.dtype.kind not in kinds:
            raise PtxError("%s: params %s must hold %s, got dtype %s" % (who, name, "integers" if kinds == "iu" else "numbers", a.dtype))
        if a.ndim != 2 or not 1 <= a.shape[1] <= RANDAUG_MAX_OPS:
            raise PtxError("%s: params %s must be [N, num_ops] with num_ops 1..%d, got shape %s" % (who, name, RANDAUG_MAX_OPS, a.shape))
        if N is not None and a.shape[0] != N:
            raise PtxError("%s: params %s hold %d clips, the frames hold N = %d" % (who, name, a.shape[0], N))
        arrs.append(a)
    if arrs[0].shape != arrs[1].shape:
        raise PtxError("%s: params codes and magnitudes differ in shape: %s and %s" % (who, arrs[0].shape, arrs[1].shape))
    if arrs[0].shape[0] == 0:
        raise PtxError("%s: empty batch" % who)
    codes, mags = np.ascontiguousarray(arrs[0].astype(np.int64)), np.ascontiguousarray(arrs[1].astype(np.float64))
    for (n, k), code in np.ndenumerate(codes):
        mag = float(mags[n, k])
        if not 0 <= code < len(RANDAUG_OPS):
            raise PtxError("%s: clip %d position %d: op code %d out of range 0..%d" % (who, n, k, code, len(RANDAUG_OPS) - 1))
        if not math.isfinite(mag):
            raise PtxError("%s: clip %d position %d: magnitude %r is not finite" % (who, n, k, mag))
        if code in _RANDAUG_ENHANCE and mag < -1.0:
            raise PtxError("%s: clip %d position %d: %s magnitude %r gives a negative factor (1 + magnitude)" % (who, n, k, RANDAUG_OPS[code], mag))
        if code == _lib.PTX_RANDAUG_POSTERIZE and not 0 <= int(mag) <= 8:
            raise PtxError("%s: clip %d position %d: posterize keeps int(magnitude) = %d bits, not 0..8" % (who, n, k, int(mag)))
    return codes.astype(np.int32), mags


def rand_augment_rows(params, H, W, N=None, who="RandAugment"):
    """The kernels' rows of `params` = (codes [N, K], magnitudes [N, K]) for H x W frames: int32 [N, K, PTX_RANDAUG_ROW] -- the
    code, then a0 .. a5 (geometric ops, `affine_fixed(rand_augment_matrix(..))`), the bits of the fp32 factor 1 + magnitude
    (brightness, color, contrast, sharpness), the posterize mask ~(2**(8 - int(magnitude)) - 1) & 255, or the bits of the solarize
    threshold (its ceiling clamped to 0..256: for a byte c, c < thr is c < ceil(thr)).  PtxError when a row is refused."""
    codes, mags = _randaug_params(params, N, who)
    rows = np.zeros(codes.shape + (_lib.PTX_RANDAUG_ROW,), np.int32)
    rows[..., 0] = codes
    for (n, k), code in np.ndenumerate(codes):
        mag = float(mags[n, k])
        if code in _RANDAUG_GEOMETRIC:
            rows[n, k, 1:7] = affine_fixed(rand_augment_matrix(int(code), mag, H, W), H, W, who)
        elif code in _RANDAUG_ENHANCE:
            rows[n, k, 1] = np.float32(1.0 + mag).view(np.int32)
        elif code == _lib.PTX_RANDAUG_POSTERIZE:
            rows[n, k, 1] = ~(2 ** (8 - int(mag)) - 1) & 255
        elif code == _lib.PTX_RANDAUG_SOLARIZE:
            rows[n, k, 1] = np.float32(math.ceil(min(max(mag, 0.0), 256.0))).view(np.int32)
    return rows


def _randaug_fill(fill, who="RandAugment"):
    if isinstance(fill, int) and not isinstance(fill, bool):
        fill = (fill,) * 3
    try:
        fill = tuple(fill)
        ok = len(fill) == 3 and all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= 255 for v in fill)
    except TypeError:
        ok = False
    if not ok:
        raise PtxError("%s: fill must be an integer or an RGB triple of integers in 0..255, got %r" % (who, fill))
    return fill


def _randaug_supported(rows, H, W, fill, who="RandAugment"):
    """ptx_rand_augment_supported on host rows [N, K, 8], position by position; PtxError with the library's reason."""
    N, K = rows.shape[:2]
    rows = np.ascontiguousarray(rows, np.int32)
    for k in range(K):
        stats = int(np.isin(rows[:, k, 0], _RANDAUG_STATS).any())
        desc = _lib.RandAugDesc(N, 1, H, W, _lib.PTX_RESIZE_OUT_U8, K, k, stats, fill[0], fill[1], fill[2], 0)
        if not _lib.lib().ptx_rand_augment_supported(C.byref(desc), C.c_void_p(rows.ctypes.data)):
            raise PtxError("%s: %s" % (who, _lib.lib().ptx_last_error().decode(errors="replace")))
    return rows


def randaug_smooth_numpy(img):
    """PIL's ImageFilter.SMOOTH of uint8 / integer [H, W, 3] (3 x 3 kernel 1 1 1 / 1 5 1 / 1 1 1 over 13): interior pixels are
    (2 * S + 13) // 26 with S the neighbourhood's sum plus 4 times the centre; border pixels -- all, when H < 3 or W < 3 -- are
    copied.  int32 [H, W, 3]."""
    c = np.asarray(img).astype(np.int32)
    out = c.copy()
    H, W = c.shape[:2]
    if H >= 3 and W >= 3:
        S = 4 * c[1:-1, 1:-1]
        for dy in range(3):
            for dx in range(3):
                S = S + c[dy:H - 2 + dy, dx:W - 2 + dx]
        out[1:-1, 1:-1] = (2 * S + 13) // 26
    return out


def randaug_autocontrast_lut(h):
    """ImageOps.autocontrast's LUT (256 ints) of one channel with histogram h (256 counts)."""
    nz = [i for i in range(256) if h[i]]
    lo, hi = (nz[0], nz[-1]) if nz else (255, 0)
    if hi <= lo:
        return list(range(256))
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return [min(max(int(i * scale + offset), 0), 255) for i in range(256)]


def randaug_equalize_lut(h):
    """ImageOps.equalize's LUT (256 ints) of one channel with histogram h (256 counts); an entry above 255 is stored as 255, as
    Image.point stores it."""
    histo = [int(v) for v in h if v]
    if len(histo) <= 1:
        return list(range(256))
    step = (sum(histo) - histo[-1]) // 255
    if not step:
        return list(range(256))
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))
        n += int(h[i])
    return lut


def rand_augment_op_numpy(img, row, fill=(0, 0, 0)):
    """One position on one frame: uint8 [H, W, 3] and one row (PTX_RANDAUG_ROW int32 words, see `rand_augment_rows`) -> uint8
    [H, W, 3], as include/ptx_amd_randaug.h states it."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    row = np.asarray(row, np.int32)
    code = int(row[0])
    f = row[1:2].view(np.float32)[0]
    if code in _RANDAUG_GEOMETRIC:
        a0, a1, a2, a3, a4, a5 = (int(v) for v in row[1:7])
        y, x = np.mgrid[0:H, 0:W].astype(np.int64)
        xin, yin = (a2 + a1 * y + a0 * x) >> 16, (a5 + a4 * y + a3 * x) >> 16
        inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
        out = np.empty_like(img)
        out[...] = np.asarray(fill, np.uint8)
        out[inside] = img[yin[inside], xin[inside]]
        return out
    c = img.astype(np.int32)
    if code == _lib.PTX_RANDAUG_BRIGHTNESS:
        c = color_blend_numpy(0, c, f)
    elif code == _lib.PTX_RANDAUG_COLOR:
        c = color_blend_numpy(color_luma_numpy(c)[..., None], c, f)
    elif code == _lib.PTX_RANDAUG_CONTRAST:
        lum = color_luma_numpy(c)
        c = color_blend_numpy(int(int(lum.sum()) / lum.size + 0.5), c, f)
    elif code == _lib.PTX_RANDAUG_SHARPNESS:
        c = color_blend_numpy(randaug_smooth_numpy(c), c, f)
    elif code == _lib.PTX_RANDAUG_POSTERIZE:
        c = c & int(row[1])
    elif code == _lib.PTX_RANDAUG_SOLARIZE:
        c = np.where(c.astype(np.float32) < f, c, 255 - c)
    elif code in (_lib.PTX_RANDAUG_AUTOCONTRAST, _lib.PTX_RANDAUG_EQUALIZE):
        make = randaug_autocontrast_lut if code == _lib.PTX_RANDAUG_AUTOCONTRAST else randaug_equalize_lut
        c = np.stack([np.asarray(make(np.bincount(c[..., ch].ravel(), minlength=256)), np.int32)[c[..., ch]] for ch in range(3)], -1)
    return c.astype(np.uint8)


def _randaug_plan(params, H, W, N, fill, interpolation, who="RandAugment"):
    """The checked launches of `params` on N clips of H x W frames under `interpolation`: (rows, warps).  "nearest": the rows
    of `rand_augment_rows`, warps None.  "bilinear" / "bicubic": per position k, warps[k] is None or the (kinds int32 [N],
    coeffs float64 [N, 8]) of a warp launch -- AFFINE with `rand_augment_matrix` for the clips whose op there is geometric,
    IDENTITY for the others --, and those clips' rows are PTX_RANDAUG_IDENTITY."""
    if interpolation == "nearest":
        return _randaug_supported(rand_augment_rows(params, H, W, N, who), H, W, fill, who), None
    codes, mags = _randaug_params(params, N, who)
    geometric = np.isin(codes, _RANDAUG_GEOMETRIC)
    rows = _randaug_supported(rand_augment_rows((np.where(geometric, _lib.PTX_RANDAUG_IDENTITY, codes), mags), H, W, N, who), H, W, fill, who)
    warps = []
    for k in range(codes.shape[1]):
        if not geometric[:, k].any():
            warps.append(None)
            continue
        kinds = np.where(geometric[:, k], _lib.PTX_WARP_AFFINE, _lib.PTX_WARP_IDENTITY).astype(np.int32)
        coeffs = np.zeros((codes.shape[0], _lib.PTX_WARP_COEFFS), np.float64)
        for n in np.nonzero(geometric[:, k])[0]:
            coeffs[n, :6] = rand_augment_matrix(int(codes[n, k]), float(mags[n, k]), H, W)
        warps.append(_warp_supported(kinds, coeffs, H, W, fill, interpolation, who))
    return rows, warps


def rand_augment_numpy(frames, params, fill=0, interpolation="nearest"):
    """The kernels' arithmetic in numpy: uint8 frames [N,T,H,W,3] and `params` = (codes [N, K], magnitudes [N, K]) -> uint8
    [N,T,H,W,3].  Every clip's positions run in order on every frame; contrast, autocontrast and equalize take the statistics of
    the FRAME as it stands at their position.  With `interpolation` "bilinear" or "bicubic" the geometric ops are `warp_numpy`
    of `rand_augment_matrix`'s coefficients.  The host-side model the tests compare with PIL; not a fallback (RandAugment never
    calls it)."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 5 or frames.shape[-1] != 3:
        raise PtxError("rand_augment_numpy: frames must be uint8 [N,T,H,W,3], got %s %s" % (frames.dtype, frames.shape))
    fill = _randaug_fill(fill, "rand_augment_numpy")
    interpolation = check_warp_interpolation(interpolation, "rand_augment_numpy")
    N, T, H, W, _ = frames.shape
    rows, warps = _randaug_plan(params, H, W, N, fill, interpolation, "rand_augment_numpy")
    out = frames.copy()
    for k in range(rows.shape[1]):
        if warps is not None and warps[k] is not None:
            out = warp_numpy(out, warps[k][0], warps[k][1], interpolation, fill)
        for n in range(N):
            for t in range(T):
                out[n, t] = rand_augment_op_numpy(out[n, t], rows[n, k], fill)
    return out


class RandAugment:
    """torchvision's RandAugment on decoded uint8 frames on the device, one draw per CLIP, equal to its PIL-image code path
    (nearest interpolation: Image.transform / rotate, ImageEnhance, ImageOps) bit for bit.  include/ptx_amd_randaug.h states the
    arithmetic, `rand_augment_numpy` restates it.

    num_ops: ops per clip, 1..PTX_RANDAUG_MAX_OPS; magnitude: the bin, 0 <= magnitude < num_magnitude_bins; fill: what the
    geometric ops write where they have no source pixel, an integer or an RGB triple in 0..255; generator: a CPU torch.Generator
    (None: torch's default one); interpolation: how shear, translate and rotate resample -- "nearest" (the default, PIL's
    fixed-point walk inside the apply launch), "bilinear" or "bicubic" (a name, Pillow's code or an enum of those; the draws do
    not depend on it).  With bilinear or bicubic a position where some clip's op is geometric runs a "warp" launch first
    (include/ptx_amd_warp.h: those clips AFFINE with `rand_augment_matrix`'s coefficients in fp64, the others copied), then the
    apply launch with those clips' rows rewritten to identity; the apply launch is skipped where every row of the position is
    identity and the position does not write the call's output.

    `ra(frames)` augments uint8 CUDA frames [N,T,H,W,3] | [T,H,W,3] | [H,W,3] (one draw per clip: N, or one; statistics are per
    frame) and keeps the draw as `last_params` = (codes CPU int32 [N, num_ops], magnitudes CPU float64 [N, num_ops]): per clip
    the op codes in running order, indexing `RANDAUG_OPS`, and the signed magnitudes.  `ra(frames, params=p)` applies a given
    draw (on any RandAugment, any num_ops in range).  Per position a call is one apply launch, plus a statistics launch when some
    clip's op there is contrast, autocontrast or equalize (`last_launches`: "stats", "apply" and "warp" in running order)."""

    def __init__(self, num_ops=2, magnitude=9, num_magnitude_bins=31, fill=0, generator=None, interpolation="nearest"):
        for name, v in (("num_ops", num_ops), ("magnitude", magnitude), ("num_magnitude_bins", num_magnitude_bins)):
            if not isinstance(v, int) or isinstance(v, bool):
                raise PtxError("RandAugment: %s must be an integer, got %r" % (name, v))
        if not 1 <= num_ops <= RANDAUG_MAX_OPS:
            raise PtxError("RandAugment: num_ops must be 1..%d (PTX_RANDAUG_MAX_OPS), got %d" % (RANDAUG_MAX_OPS, num_ops))
        if num_magnitude_bins < 2:
            raise PtxError("RandAugment: num_magnitude_bins must be at least 2, got %d" % num_magnitude_bins)
        if not 0 <= magnitude < num_magnitude_bins:
            raise PtxError("RandAugment: magnitude must be a bin 0..%d, got %d" % (num_magnitude_bins - 1, magnitude))
        _check_generator(generator, "RandAugment")
        self.num_ops, self.magnitude, self.num_magnitude_bins = num_ops, magnitude, num_magnitude_bins
        self.fill = _randaug_fill(fill)
        self.interpolation = check_warp_interpolation(interpolation, "RandAugment")
        self.generator, self.last_params, self.last_launches = generator, None, ()

    def draw(self, n, H, W):
        """The draw of n clips of H x W frames: (codes CPU int32 [n, num_ops], magnitudes CPU float64 [n, num_ops]).  Per clip and
        position, in torchvision's order, from `generator`: op = int(torch.randint(14, (1,))); the magnitude is
        float(table[magnitude].item()) of `rand_augment_space(num_magnitude_bins, H, W)` (0.0 for an op without a table); only
        for a signed op, torch.randint(2, (1,)), a non-zero value negating the magnitude."""
        g = self.generator
        space = rand_augment_space(self.num_magnitude_bins, int(H), int(W))
        codes = torch.zeros((int(n), self.num_ops), dtype=torch.int32)
        mags = torch.zeros((int(n), self.num_ops), dtype=torch.float64)
        for i in range(int(n)):
            for k in range(self.num_ops):
                op = int(torch.randint(len(RANDAUG_OPS), (1,), generator=g))
                mag = float(space[op][self.magnitude].item()) if space[op] is not None else 0.0
                if RANDAUG_SIGNED[op] and torch.randint(2, (1,), generator=g):
                    mag *= -1.0
                codes[i, k], mags[i, k] = op, mag
        return codes, mags

    def check_params(self, params, N=None, H=None, W=None):
        """`params` as (CPU int32 [N, K], CPU float64 [N, K]) tensors, or PtxError: shapes, N, K outside 1..PTX_RANDAUG_MAX_OPS, a
        code out of range, a magnitude that is not finite or that its op cannot take; with H and W also the library's own check
        of the rows (`rand_augment_rows`) for frames of that size.  No device is touched."""
        codes, mags = _randaug_params(params, N)
        if H is not None and W is not None:
            _randaug_plan((codes, mags), int(H), int(W), N, self.fill, self.interpolation)
        return torch.from_numpy(codes), torch.from_numpy(mags)

    def _rows_for(self, N, H, W, params):
        """The checked host rows of a call on N clips of H x W frames: of a new draw (kept as last_params) or of `params`.  With an
        interpolated filter a `_RandAugPlan`: the rows and the warp launches of `_randaug_plan`."""
        if params is None:
            params = self.last_params = self.draw(N, H, W)
        rows, warps = _randaug_plan(params, H, W, N, self.fill, self.interpolation)
        return rows if warps is None else _RandAugPlan(rows, warps)

    def _run(self, f5, params, mode=_lib.PTX_RESIZE_OUT_U8, norm=None, dtype=torch.uint8):
        """The stage on contiguous uint8 frames f5 [N,T,H,W,3]: `params`, or a draw that is kept as `last_params`; see `_launch`."""
        return self._launch(f5, self._rows_for(f5.shape[0], f5.shape[2], f5.shape[3], params), mode, norm, dtype)

    def _launch(self, f5, rows, mode, norm, dtype):
        """The launches on contiguous uint8 CUDA frames f5 [N,T,H,W,3] with checked host rows [N, K, 8]: uint8 [N,T,H,W,3] or the
        normalised [N,3,T,H,W] of `dtype`.  Positions ping-pong between two uint8 scratch buffers; the last one writes y.  `rows`
        may be a `_RandAugPlan`, whose warp launches run in front of their positions."""
        if isinstance(rows, _RandAugPlan):
            return self._launch_warped(f5, rows, mode, norm, dtype)
        N, T, H, W, _ = f5.shape
        K = rows.shape[1]
        lib = _lib.lib()
        launches = []
        with torch.cuda.device(f5.device):
            dev_rows = torch.from_numpy(rows.reshape(-1)).to(f5.device)                  # one upload
            rows_p = C.c_void_p(dev_rows.data_ptr())
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            scratch = [torch.empty_like(f5) for _ in range(min(K - 1, 2))]
            y = _alloc_out(mode, N, T, H, W, f5.device, dtype)
            stats = None
            cur = f5
            for k in range(K):
                last = k == K - 1
                need = bool(np.isin(rows[:, k, 0], _RANDAUG_STATS).any())
                desc = _lib.RandAugDesc(N, T, H, W, mode if last else _lib.PTX_RESIZE_OUT_U8, K, k, int(need), self.fill[0],
                                        self.fill[1], self.fill[2], 0)
                if need:
                    if stats is None:
                        stats = torch.empty(N * T * _lib.PTX_RANDAUG_STATS_WORDS, device=f5.device, dtype=torch.int32)
                    check(lib.ptx_rand_augment_stats(C.byref(desc), C.c_void_p(cur.data_ptr()), rows_p, C.c_void_p(stats.data_ptr()),
                                                     stream), "ptx_rand_augment_stats")
                    launches.append("stats")
                dst = y if last else scratch[k % 2]
                check(lib.ptx_rand_augment_apply(C.byref(desc), C.c_void_p(cur.data_ptr()), rows_p,
                                                 C.c_void_p(stats.data_ptr()) if need else None, C.c_void_p(dst.data_ptr()),
                                                 C.byref(norm) if (last and norm is not None) else None, stream), "ptx_rand_augment_apply")
                launches.append("apply")
                cur = dst
        self.last_launches = tuple(launches)
        return y

    def _launch_warped(self, f5, plan, mode, norm, dtype):
        """`_launch` with an interpolated filter: per position the warp launch (when some clip's op there is geometric), the
        statistics launch (when needed) and the apply launch, which is skipped where it would only copy into a scratch buffer."""
        N, T, H, W, _ = f5.shape
        rows, warps = plan.rows, plan.warps
        K = rows.shape[1]
        lib = _lib.lib()
        launches = []
        with torch.cuda.device(f5.device):
            dev_rows = torch.from_numpy(rows.reshape(-1)).to(f5.device)                  # one upload
            rows_p = C.c_void_p(dev_rows.data_ptr())
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            pool = []

            def scratch(cur):                                                            # a uint8 buffer that is not `cur`
                for b in pool:
                    if b is not cur:
                        return b
                pool.append(torch.empty_like(f5))
                return pool[-1]

            y = _alloc_out(mode, N, T, H, W, f5.device, dtype)
            stats = None
            cur = f5
            for k in range(K):
                last = k == K - 1
                if warps[k] is not None:
                    dst = scratch(cur)
                    _warp_launch(cur, dst, warps[k][0], warps[k][1], self.interpolation, self.fill, stream)
                    launches.append("warp")
                    cur = dst
                    if not last and not rows[:, k, 0].any():                             # every row identity: nothing left to do
                        continue
                need = bool(np.isin(rows[:, k, 0], _RANDAUG_STATS).any())
                desc = _lib.RandAugDesc(N, T, H, W, mode if last else _lib.PTX_RESIZE_OUT_U8, K, k, int(need), self.fill[0],
                                        self.fill[1], self.fill[2], 0)
                if need:
                    if stats is None:
                        stats = torch.empty(N * T * _lib.PTX_RANDAUG_STATS_WORDS, device=f5.device, dtype=torch.int32)
                    check(lib.ptx_rand_augment_stats(C.byref(desc), C.c_void_p(cur.data_ptr()), rows_p, C.c_void_p(stats.data_ptr()),
                                                     stream), "ptx_rand_augment_stats")
                    launches.append("stats")
                dst = y if last else scratch(cur)
                check(lib.ptx_rand_augment_apply(C.byref(desc), C.c_void_p(cur.data_ptr()), rows_p,
                                                 C.c_void_p(stats.data_ptr()) if need else None, C.c_void_p(dst.data_ptr()),
                                                 C.byref(norm) if (last and norm is not None) else None, stream), "ptx_rand_augment_apply")
                launches.append("apply")
                cur = dst
        self.last_launches = tuple(launches)
        return y

    def __call__(self, frames, params=None):
        N, _, H, W = _frames_shape(frames, "RandAugment")
        _check_not_empty(frames, "RandAugment")
        if params is not None:                                       # validated before a device is touched
            params = self.check_params(params, N, H, W)
        return self._run(_u8_cuda_5d(frames, "RandAugment"), params).view(frames.shape)


class _RandAugPlan:
    """The launches of a RandAugment call with an interpolated filter: `rows` [N, K, 8] and, per position, None or the (kinds,
    coeffs) of its warp launch (`_randaug_plan`)."""

    def __init__(self, rows, warps):
        self.rows, self.warps = rows, warps


# ---------------------------------------------------------------------------------------------
# Interpolated per-clip warps (include/ptx_amd_warp.h): the arithmetic contract in numpy, the launch, RandomAffine /
# RandomRotation / RandomPerspective
# ---------------------------------------------------------------------------------------------
WARP_KINDS = ("identity", "affine", "perspective")                                  # the PTX_WARP_* codes, by index
WARP_INTERPOLATIONS = ("nearest", "bilinear", "bicubic")                            # what Image.transform takes


def check_warp_interpolation(interpolation, who="warp"):
    """`check_interpolation`, then the three filters a warp can take (Image.transform's); PtxError for the other three."""
    name = check_interpolation(interpolation, who)
    if name not in WARP_INTERPOLATIONS:
        raise PtxError("%s: a warp takes interpolation 'nearest', 'bilinear' or 'bicubic' (what PIL's Image.transform takes), got %r"
                       % (who, interpolation))
    return name


def _warp_params(kinds, coeffs, N=None, who="warp"):
    """(kinds [N] integers, coeffs [N, 8] numbers) -- arrays or CPU tensors -- as contiguous (int32, float64) numpy arrays, or
    PtxError (shapes and dtypes only; the values are ptx_warp_frames_supported's to check)."""
    arrs = []
    for name, a, ok, shape in (("kinds", kinds, "iu", "[N]"), ("coeffs", coeffs, "fiu", "[N, %d]" % _lib.PTX_WARP_COEFFS)):
        a = _host_array(a, "%s: params %s must be an array or a CPU tensor, got a CUDA tensor" % (who, name))
        if a.dtype.kind not in ok:
            raise PtxError("%s: params %s must hold %s, got dtype %s" % (who, name, "integers" if ok == "iu" else "numbers", a.dtype))
        if a.ndim != (1 if name == "kinds" else 2) or (name == "coeffs" and a.shape[1] != _lib.PTX_WARP_COEFFS):
            raise PtxError("%s: params %s must be %s, got shape %s" % (who, name, shape, a.shape))
        if N is not None and a.shape[0] != N:
            raise PtxError("%s: params %s hold %d clips, the frames hold N = %d" % (who, name, a.shape[0], N))
        arrs.append(a)
    if arrs[0].shape[0] != arrs[1].shape[0]:
        raise PtxError("%s: params kinds and coeffs differ in length: %d and %d" % (who, arrs[0].shape[0], arrs[1].shape[0]))
    if arrs[0].shape[0] == 0:
        raise PtxError("%s: empty batch" % who)
    k64 = arrs[0].astype(np.int64)
    if (np.abs(k64) >= 2 ** 31).any():
        raise PtxError("%s: params kinds must be PTX_WARP_* codes 0..2" % who)
    return np.ascontiguousarray(k64.astype(np.int32)), np.ascontiguousarray(arrs[1].astype(np.float64))


def _warp_supported(kinds, coeffs, H, W, fill, interpolation, who="warp"):
    """ptx_warp_frames_supported on host kinds [N] and coeffs [N, 8]: the contiguous (int32, float64) arrays, or PtxError with
    the library's reason."""
    kinds, coeffs = _warp_params(kinds, coeffs, None, who)
    desc = _lib.WarpDesc(kinds.shape[0], 1, int(H), int(W), INTERPOLATIONS.index(interpolation), fill[0], fill[1], fill[2], 0)
    if not _lib.lib().ptx_warp_frames_supported(C.byref(desc), C.c_void_p(kinds.ctypes.data), C.c_void_p(coeffs.ctypes.data)):
        raise PtxError("%s: %s" % (who, _lib.lib().ptx_last_error().decode(errors="replace")))
    return kinds, coeffs


def _warp_clip_numpy(clip, kind, a, interpolation, fill):
    """One clip, uint8 [T, H, W, 3]: include/ptx_amd_warp.h's arithmetic, operation for operation (numpy's float64 is IEEE and
    numpy does not contract)."""
    T, H, W, _ = clip.shape
    if kind == _lib.PTX_WARP_IDENTITY:
        return clip.copy()
    X, Y = np.arange(W, dtype=np.float64)[None, :] + 0.5, np.arange(H, dtype=np.float64)[:, None] + 0.5
    with np.errstate(all="ignore"):
        xin, yin = a[0] * X + a[1] * Y + a[2], a[3] * X + a[4] * Y + a[5]
        if kind == _lib.PTX_WARP_PERSPECTIVE:
            den = a[6] * X + a[7] * Y + 1.0
            xin, yin = xin / den, yin / den
        inside = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)
    xin, yin = np.where(inside, xin, 0.0), np.where(inside, yin, 0.0)
    out = np.empty_like(clip)
    out[...] = np.asarray(fill, np.uint8)
    if interpolation == "nearest":                       # xin >= 0 here, so PIL's COORD is the truncation
        out[:, inside] = clip[:, yin.astype(np.int64)[inside], xin.astype(np.int64)[inside]]
        return out
    xin, yin = xin - 0.5, yin - 0.5
    xi, yi = np.floor(xin), np.floor(yin)
    dx, dy = (xin - xi)[None, :, :, None], (yin - yi)[None, :, :, None]
    xi, yi = xi.astype(np.int64), yi.astype(np.int64)
    src = clip.astype(np.float64)                        # bytes and their small integer sums are exact in float64
    cx = lambda i: np.clip(i, 0, W - 1)
    if interpolation == "bilinear":
        x0, x1 = cx(xi), cx(xi + 1)

        def row(r):
            return src[:, r, x0] + (src[:, r, x1] - src[:, r, x0]) * dx

        v1 = row(np.clip(yi, 0, H - 1))
        ok = ((yi + 1 >= 0) & (yi + 1 < H))[None, :, :, None]
        v2 = np.where(ok, row(np.clip(yi + 1, 0, H - 1)), v1)
        val = np.trunc(v1 + (v2 - v1) * dy)
    else:
        xi, yi = xi - 1, yi - 1
        xs = [cx(xi + j) for j in range(4)]

        def cub(v1, v2, v3, v4, d):
            p1, p2, p3, p4 = v2, -v1 + v3, 2 * (v1 - v2) + v3 - v4, -v1 + v2 - v3 + v4
            return p1 + d * (p2 + d * (p3 + d * p4))

        def row(r):
            return cub(src[:, r, xs[0]], src[:, r, xs[1]], src[:, r, xs[2]], src[:, r, xs[3]], dx)

        r = [row(np.clip(yi, 0, H - 1))]
        for k in (1, 2, 3):
            ok = ((yi + k >= 0) & (yi + k < H))[None, :, :, None]
            r.append(np.where(ok, row(np.clip(yi + k, 0, H - 1)), r[-1]))
        v = cub(r[0], r[1], r[2], r[3], dy)
        val = np.where(v <= 0.0, 0.0, np.where(v >= 255.0, 255.0, np.trunc(v)))
    out[:, inside] = val.astype(np.uint8)[:, inside]
    return out


def warp_numpy(frames, kinds, coeffs, interpolation="bilinear", fill=0):
    """The warp kernel's arithmetic in numpy: uint8 frames [N,T,H,W,3], kinds [N] (PTX_WARP_* codes, `WARP_KINDS` by index) and
    coeffs float64 [N, 8] (a0 .. a7 of Image.transform's AFFINE -- a6, a7 unused -- or PERSPECTIVE data) -> uint8 [N,T,H,W,3],
    as include/ptx_amd_warp.h states it.  A nearest affine clip is refused, as the kernel refuses it (PIL walks it in fixed
    point: `affine_fixed`).  The host-side model the tests compare with Pillow; not a fallback (nothing on the device path calls
    it)."""
    frames = np.asarray(frames)
    if frames.dtype != np.uint8 or frames.ndim != 5 or frames.shape[-1] != 3:
        raise PtxError("warp_numpy: frames must be uint8 [N,T,H,W,3], got %s %s" % (frames.dtype, frames.shape))
    fill = _randaug_fill(fill, "warp_numpy")
    interpolation = check_warp_interpolation(interpolation, "warp_numpy")
    N, T, H, W, _ = frames.shape
    kinds, coeffs = _warp_params(kinds, coeffs, N, "warp_numpy")
    kinds, coeffs = _warp_supported(kinds, coeffs, H, W, fill, interpolation, "warp_numpy")
    return np.stack([_warp_clip_numpy(frames[n], int(kinds[n]), [float(v) for v in coeffs[n]], interpolation, fill) for n in range(N)])


def _warp_launch(src, dst, kinds, coeffs, interpolation, fill, stream):
    """ptx_warp_frames on contiguous uint8 CUDA frames src -> dst [N,T,H,W,3] with checked host kinds and coeffs."""
    N, T, H, W, _ = src.shape
    dev_kinds = torch.from_numpy(kinds).to(src.device)
    dev_coeffs = torch.from_numpy(coeffs.reshape(-1)).to(src.device)
    desc = _lib.WarpDesc(N, T, H, W, INTERPOLATIONS.index(interpolation), fill[0], fill[1], fill[2], 0)
    check(_lib.lib().ptx_warp_frames(C.byref(desc), C.c_void_p(src.data_ptr()), C.c_void_p(dev_kinds.data_ptr()),
                                     C.c_void_p(dev_coeffs.data_ptr()), C.c_void_p(dst.data_ptr()), stream), "ptx_warp_frames")


def _uniform(lo, hi, generator):
    return float(torch.empty(1).uniform_(float(lo), float(hi), generator=generator).item())


def _warp_range(value, name, who, lengths=(2,), nonneg=False, number=True):
    """A number d (the range -d .. d; only with `number`) or a sequence of one of `lengths` numbers, as a tuple of floats."""
    if number and isinstance(value, (int, float)) and not isinstance(value, bool):
        if value < 0:
            raise PtxError("%s: a single %s must not be negative, got %r" % (who, name, value))
        return (-float(value), float(value))
    try:
        vals = tuple(float(v) for v in value)
    except (TypeError, ValueError):
        vals = ()
    if len(vals) not in lengths or not all(math.isfinite(v) for v in vals):
        raise PtxError("%s: %s must be %sa sequence of %s finite numbers, got %r" % (who, name, "a number or " if number else "",
                                                                                 " or ".join(map(str, lengths)), value))
    if nonneg and any(v <= 0 for v in vals):
        raise PtxError("%s: %s values must be positive, got %r" % (who, name, value))
    return vals


class _ClipWarp:
    """What RandomAffine, RandomRotation and RandomPerspective share: one draw per CLIP as (kinds CPU int32 [N], coeffs CPU
    float64 [N, 8]) -- `WARP_KINDS` codes and the a0 .. a7 that Image.transform takes --, kept as `last_params` and replayed
    with `params=`; the call on uint8 CUDA frames [N,T,H,W,3] | [T,H,W,3] | [H,W,3], which returns uint8 frames of the same
    shape in one launch (`last_launches`): ptx_warp_frames ("warp"), or, for nearest affine clips, one position of
    ptx_rand_augment_apply ("apply") with `affine_fixed`'s rotate-coded row, PIL's own fixed-point walk."""

    def _init_warp(self, interpolation, fill, generator):
        who = type(self).__name__
        self.interpolation = check_warp_interpolation(interpolation, who)
        self.fill = _randaug_fill(fill, who)
        self.generator, self.last_params, self.last_launches = _check_generator(generator, who), None, ()

    def check_params(self, params, N=None, H=None, W=None):
        """`params` as (CPU int32 [N], CPU float64 [N, 8]) tensors, or PtxError: shapes, N; with H and W also the library's own
        check of the kinds and coefficients for frames of that size.  No device is touched."""
        who = type(self).__name__
        try:
            kinds, coeffs = params
        except (TypeError, ValueError):
            raise PtxError("%s: params must be a pair (kinds [N], coeffs [N, 8]), got %r" % (who, type(params).__name__))
        kinds, coeffs = _warp_params(kinds, coeffs, N, who)
        if H is not None and W is not None:
            self._plan(kinds, coeffs, int(H), int(W))
        return torch.from_numpy(kinds), torch.from_numpy(coeffs)

    def _plan(self, kinds, coeffs, H, W):
        """("apply", rows [N, 1, 8]) for nearest affine clips, else ("warp", kinds, coeffs); checked by the library."""
        who = type(self).__name__
        if self.interpolation == "nearest" and (kinds == _lib.PTX_WARP_AFFINE).any():
            if not np.isin(kinds, (_lib.PTX_WARP_IDENTITY, _lib.PTX_WARP_AFFINE)).all():
                raise PtxError("%s: nearest affine clips run PIL's fixed-point walk and cannot share a launch with another kind" % who)
            rows = np.zeros((kinds.shape[0], 1, _lib.PTX_RANDAUG_ROW), np.int32)
            for n in np.nonzero(kinds == _lib.PTX_WARP_AFFINE)[0]:
                if not np.isfinite(coeffs[n, :6]).all():
                    raise PtxError("%s: clip %d: a coefficient is not finite" % (who, n))
                rows[n, 0, 0] = _lib.PTX_RANDAUG_ROTATE
                rows[n, 0, 1:7] = affine_fixed([float(v) for v in coeffs[n, :6]], H, W, who)
            return ("apply", _randaug_supported(rows, H, W, self.fill, who))
        return ("warp",) + _warp_supported(kinds, coeffs, H, W, self.fill, self.interpolation, who)

    def __call__(self, frames, params=None):
        who = type(self).__name__
        N, _, H, W = _frames_shape(frames, who)
        _check_not_empty(frames, who)
        if params is not None:                                       # validated before a device is touched
            params = self.check_params(params, N, H, W)
        f5 = _u8_cuda_5d(frames, who)
        if params is None:
            params = self.last_params = self.draw(N, H, W)
        plan = self._plan(params[0].numpy(), params[1].numpy(), H, W)
        with torch.cuda.device(f5.device):
            y = torch.empty_like(f5)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if plan[0] == "warp":
                _warp_launch(f5, y, plan[1], plan[2], self.interpolation, self.fill, stream)
            else:
                dev_rows = torch.from_numpy(plan[1].reshape(-1)).to(f5.device)
                desc = _lib.RandAugDesc(N, f5.shape[1], H, W, _lib.PTX_RESIZE_OUT_U8, 1, 0, 0, self.fill[0], self.fill[1], self.fill[2], 0)
                check(_lib.lib().ptx_rand_augment_apply(C.byref(desc), C.c_void_p(f5.data_ptr()), C.c_void_p(dev_rows.data_ptr()), None,
                                                        C.c_void_p(y.data_ptr()), None, stream), "ptx_rand_augment_apply")
        self.last_launches = (plan[0],)
        return y.view(frames.shape)

    @staticmethod
    def _pack(rows):
        """[(kind, coefficients)] per clip -> (kinds CPU int32 [N], coeffs CPU float64 [N, 8])."""
        kinds = torch.tensor([k for k, _ in rows], dtype=torch.int32)
        coeffs = torch.zeros((len(rows), _lib.PTX_WARP_COEFFS), dtype=torch.float64)
        for n, (_, a) in enumerate(rows):
            coeffs[n, :len(a)] = torch.tensor([float(v) for v in a], dtype=torch.float64)
        return kinds, coeffs


class RandomAffine(_ClipWarp):
    """torchvision's RandomAffine on decoded uint8 frames on the device, one draw per CLIP, equal to its PIL-image code path
    (Image.transform(AFFINE) with the interpolation) bit for bit on the drawn coefficients.  degrees: a number d (-d .. d) or a
    pair; translate: None or a pair of fractions in 0..1 of the width and the height; scale: None or a (lo, hi) pair of positive
    numbers; shear: None, a number s (x shear -s .. s), a pair (x) or four numbers (x, then y); center: None (the image centre,
    (W * 0.5, H * 0.5)) or (cx, cy); fill and generator as RandAugment's.

    THE DRAW (the contract: torchvision's RandomAffine.get_params order), per clip from `generator`, each a
    torch.empty(1).uniform_(lo, hi): the angle; if translate, tx then ty, each int(round(.)) of a draw in -max .. max with max_dx
    = translate[0] * W, max_dy = translate[1] * H; if scale, the scale; if shear, the x shear, then (four numbers only) the y
    shear.  The coefficients are `_inverse_affine_matrix(center, angle, (tx, ty), (shear_x, shear_y), scale)`."""

    def __init__(self, degrees, translate=None, scale=None, shear=None, interpolation="nearest", fill=0, center=None, generator=None):
        who = "RandomAffine"
        self._init_warp(interpolation, fill, generator)
        self.degrees = _warp_range(degrees, "degrees", who)
        self.translate = None if translate is None else _warp_range(translate, "translate", who, number=False)
        if self.translate is not None and not all(0.0 <= v <= 1.0 for v in self.translate):
            raise PtxError("%s: translate values must be between 0 and 1, got %r" % (who, translate))
        self.scale = None if scale is None else _warp_range(scale, "scale", who, nonneg=True, number=False)
        self.shear = None if shear is None else _warp_range(shear, "shear", who, lengths=(2, 4))
        self.center = None if center is None else _warp_range(center, "center", who, number=False)

    def draw(self, n, H, W):
        g, rows = self.generator, []
        for _ in range(int(n)):
            angle = _uniform(self.degrees[0], self.degrees[1], g)
            tx = ty = 0
            if self.translate is not None:
                max_dx, max_dy = float(self.translate[0] * W), float(self.translate[1] * H)
                tx = int(round(_uniform(-max_dx, max_dx, g)))
                ty = int(round(_uniform(-max_dy, max_dy, g)))
            scale = _uniform(self.scale[0], self.scale[1], g) if self.scale is not None else 1.0
            sx = sy = 0.0
            if self.shear is not None:
                sx = _uniform(self.shear[0], self.shear[1], g)
                if len(self.shear) == 4:
                    sy = _uniform(self.shear[2], self.shear[3], g)
            center = (W * 0.5, H * 0.5) if self.center is None else self.center
            rows.append((_lib.PTX_WARP_AFFINE, _inverse_affine_matrix(center, angle, (tx, ty), (sx, sy), scale)))
        return self._pack(rows)


class RandomRotation(_ClipWarp):
    """torchvision's RandomRotation on decoded uint8 frames on the device, one draw per CLIP, equal to its PIL-image code path
    (Image.rotate(angle, interpolation, center=.., fillcolor=..)) bit for bit on the drawn coefficients.  degrees: a number d
    (-d .. d) or a pair; center: None (PIL's (W / 2, H / 2)) or (cx, cy); expand=True is not offered: the clips of a batch would
    differ in size.

    THE DRAW (the contract), per clip from `generator`: the angle, one torch.empty(1).uniform_(lo, hi).  The coefficients are
    `rotation_matrix(angle, H, W, center)`: Image.rotate's own matrix, its sine and cosine rounded to 15 decimals."""

    def __init__(self, degrees, interpolation="nearest", center=None, fill=0, generator=None, expand=False):
        who = "RandomRotation"
        if expand:
            raise PtxError("%s: expand=True is not offered: the clips of a batch would differ in size" % who)
        self._init_warp(interpolation, fill, generator)
        self.degrees = _warp_range(degrees, "degrees", who)
        self.center = None if center is None else _warp_range(center, "center", who, number=False)

    def draw(self, n, H, W):
        return self._pack([(_lib.PTX_WARP_AFFINE, rotation_matrix(_uniform(self.degrees[0], self.degrees[1], self.generator), H, W, self.center))
                           for _ in range(int(n))])


def perspective_coefficients(startpoints, endpoints):
    """torchvision's _get_perspective_coeffs (0.15 and later): the eight coefficients that map the four `endpoints` to the four
    `startpoints`, from the 8 x 8 least-squares system in float64 (torch.linalg.lstsq, driver gels), rounded to float32 and
    widened to Python floats."""
    a = torch.zeros(8, 8, dtype=torch.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i, :] = torch.tensor([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]], dtype=torch.float64)
        a[2 * i + 1, :] = torch.tensor([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]], dtype=torch.float64)
    b = torch.tensor(startpoints, dtype=torch.float64).view(8)
    return torch.linalg.lstsq(a, b, driver="gels").solution.to(torch.float32).tolist()


class RandomPerspective(_ClipWarp):
    """torchvision's RandomPerspective on decoded uint8 frames on the device, one draw per CLIP, equal to its PIL-image code path
    (Image.transform(PERSPECTIVE) with the interpolation) bit for bit on the drawn coefficients.  distortion_scale: 0..1; p: the
    probability that a clip is warped (the others are copied).

    THE DRAW (the contract: torchvision's forward and get_params order), per clip from `generator`: torch.rand(1) < p; only
    then eight torch.randint(lo, hi, (1,)) -- top-left x, y, top-right x, y, bottom-right x, y, bottom-left x, y -- with hw =
    int(distortion_scale * (W // 2)), hh = int(distortion_scale * (H // 2)): a left x in 0 .. hw, a right x in W - hw - 1 .. W -
    1, a top y in 0 .. hh, a bottom y in H - hh - 1 .. H - 1.  The coefficients are `perspective_coefficients` of the frame's
    corners [0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1] and the drawn ones.  A degenerate quadrilateral, whose denominator
    vanishes inside the frame, raises PtxError."""

    def __init__(self, distortion_scale=0.5, p=0.5, interpolation="bilinear", fill=0, generator=None):
        who = "RandomPerspective"
        self._init_warp(interpolation, fill, generator)
        for name, v in (("distortion_scale", distortion_scale), ("p", p)):
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not 0.0 <= v <= 1.0:
                raise PtxError("%s: %s must be a number in 0..1, got %r" % (who, name, v))
        self.distortion_scale, self.p = float(distortion_scale), float(p)

    def draw(self, n, H, W):
        g, rows = self.generator, []
        ri = lambda lo, hi: int(torch.randint(lo, hi, (1,), generator=g).item())
        hw, hh = int(self.distortion_scale * (W // 2)), int(self.distortion_scale * (H // 2))
        for _ in range(int(n)):
            if not bool(torch.rand(1, generator=g) < self.p):
                rows.append((_lib.PTX_WARP_IDENTITY, []))
                continue
            topleft = [ri(0, hw + 1), ri(0, hh + 1)]
            topright = [ri(W - hw - 1, W), ri(0, hh + 1)]
            botright = [ri(W - hw - 1, W), ri(H - hh - 1, H)]
            botleft = [ri(0, hw + 1), ri(H - hh - 1, H)]
            start = [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]]
            rows.append((_lib.PTX_WARP_PERSPECTIVE, perspective_coefficients(start, [topleft, topright, botright, botleft])))
        return self._pack(rows)


# ---------------------------------------------------------------------------------------------
# BatchMix: RandomErasing per clip and MixUp / CutMix across the clips of a batch, on the normalised clip (include/ptx_amd_mix.h)
# ---------------------------------------------------------------------------------------------
MIX_MODES = ("none", "mixup", "cutmix")
MIX_FIELDS = ("partner", "mode", "box_y0", "box_x0", "box_y1", "box_x1", "erase", "erase_top", "erase_left", "erase_h", "erase_w")


def _mix_params(params, N=None, who="BatchMix"):
    """A draw as (int64 numpy [N, 11] of MIX_FIELDS, float64 numpy [N] of lam), or PtxError (shapes and dtypes only)."""
    try:
        rows, lam = params
    except (TypeError, ValueError):
        raise PtxError("%s: params must be a pair (rows [N, %d], lam [N]), got %r" % (who, len(MIX_FIELDS), params))
    out = []
    for name, a, kinds in (("rows", rows, "iu"), ("lam", lam, "f")):
        a = _host_array(a, "%s: params %s must be an array or a CPU tensor, got a CUDA tensor" % (who, name))
        if a.dtype.kind not in kinds:
            raise PtxError("%s: params %s must hold %s, got dtype %s" % (who, name, "integers" if kinds == "iu" else "floats", a.dtype))
        out.append(a)
    rows, lam = out[0].astype(np.int64), out[1].astype(np.float64)
    if rows.ndim != 2 or rows.shape[1] != len(MIX_FIELDS):
        raise PtxError("%s: params rows must be [N, %d] (%s), got shape %s" % (who, len(MIX_FIELDS), ", ".join(MIX_FIELDS), rows.shape))
    if lam.shape != (rows.shape[0],):
        raise PtxError("%s: params lam must be [N] = [%d], got shape %s" % (who, rows.shape[0], lam.shape))
    if N is not None and rows.shape[0] != N:
        raise PtxError("%s: params hold %d clips, the batch holds N = %d" % (who, rows.shape[0], N))
    if rows.shape[0] == 0:
        raise PtxError("%s: empty batch" % who)
    if np.abs(rows).max() >= 2 ** 31:
        raise PtxError("%s: params rows must fit int32" % who)
    return rows, lam


def _mix_erase_value(value, who="BatchMix"):
    """erase_value as "random" or a tuple of three floats (one per output channel, in the normalised domain)."""
    if isinstance(value, str):
        if value != "random":
            raise PtxError("%s: erase_value must be a number, an RGB triple or 'random', got %r" % (who, value))
        return value
    try:
        v = [float(value)] * 3 if isinstance(value, (int, float)) and not isinstance(value, bool) else [float(c) for c in value]
    except (TypeError, ValueError):
        v = None
    if v is None or len(v) != 3 or not all(math.isfinite(c) for c in v):
        raise PtxError("%s: erase_value must be a finite number, an RGB triple or 'random', got %r" % (who, value))
    return tuple(v)


def batch_mix_rows(params, T, erase_value=0, N=None, who="BatchMix"):
    """The int32 rows [N, PTX_MIX_ROW] of a draw for clips of T frames (include/ptx_amd_mix.h) and the number of noise
    elements they address: a = fp32(lam), b = fp32(1.0 - lam); an erased clip's kind is CONST with the three constants, or NOISE
    with the offset of its [3, T, h, w] block, the blocks packed in clip order."""
    rows, lam = _mix_params(params, N, who)
    value = _mix_erase_value(erase_value, who)
    out = np.zeros((rows.shape[0], _lib.PTX_MIX_ROW), np.int32)
    out[:, _lib.PTX_MIX_W_PARTNER], out[:, _lib.PTX_MIX_W_MODE] = rows[:, 0], rows[:, 1]
    out[:, _lib.PTX_MIX_W_A] = lam.astype(np.float32).view(np.int32)
    out[:, _lib.PTX_MIX_W_B] = (1.0 - lam).astype(np.float32).view(np.int32)
    out[:, _lib.PTX_MIX_W_BOX:_lib.PTX_MIX_W_BOX + 4] = rows[:, 2:6]
    out[:, _lib.PTX_MIX_W_ERASE:_lib.PTX_MIX_W_ERASE + 4] = rows[:, 7:11]
    noise = 0
    for n in np.flatnonzero(rows[:, 6]):
        if value == "random":
            out[n, _lib.PTX_MIX_W_ERASE_KIND] = _lib.PTX_MIX_ERASE_NOISE
            out[n, _lib.PTX_MIX_W_NOISE:_lib.PTX_MIX_W_NOISE + 2] = np.array([noise], np.int64).view(np.int32)
            noise += 3 * int(T) * max(int(rows[n, 9]), 0) * max(int(rows[n, 10]), 0)
        else:
            out[n, _lib.PTX_MIX_W_ERASE_KIND] = _lib.PTX_MIX_ERASE_CONST
            out[n, _lib.PTX_MIX_W_CONST:_lib.PTX_MIX_W_CONST + 3] = np.array(value, np.float32).view(np.int32)
    return out, noise


def _mix_supported(rows, noise_elems, T, H, W, src_mode=_lib.PTX_MIX_SRC_U8, out_mode=_lib.PTX_RESIZE_OUT_F32, who="BatchMix"):
    """The library's host-side check of the rows (ptx_batch_mix_supported: no device), or PtxError with its message."""
    desc = _lib.MixDesc(rows.shape[0], int(T), int(H), int(W), src_mode, out_mode, int(noise_elems))
    rows = np.ascontiguousarray(rows, np.int32)
    if not _lib.lib().ptx_batch_mix_supported(C.byref(desc), C.c_void_p(rows.ctypes.data)):
        raise PtxError("%s: %s" % (who, _lib.lib().ptx_last_error().decode(errors="replace")))
    return rows


def batch_mix_torch(clips, params, erase_value=0, noise=None):
    """torch-on-CPU statement of the contract (the tests' reference).  clips: a CPU tensor [N,3,T,H,W], fp32 or bf16; params: a
    draw (rows [N, 11] of MIX_FIELDS, lam [N]); noise: for erase_value="random" the list of [3,T,h,w] tensors of the erased
    clips in clip order.  E_i is clip i with its rectangle replaced on every frame (constants and noise cast to the clips'
    dtype); then MixUp is  E_p.mul(1.0 - lam).add_(E_i.mul(lam)),  CutMix E_p inside the box and E_i outside it, no mix E_i."""
    rows, lam = _mix_params(params, clips.shape[0], "batch_mix_torch")
    value = _mix_erase_value(erase_value, "batch_mix_torch")
    if clips.dim() != 5 or clips.shape[1] != 3 or clips.is_cuda:
        raise PtxError("batch_mix_torch: clips must be a CPU tensor [N,3,T,H,W], got %s" % (tuple(clips.shape),))
    erased, k = [], 0
    for i, r in enumerate(rows.tolist()):
        e = clips[i].clone()
        if r[6]:
            top, left, h, w = r[7:11]
            if value == "random":
                fill = noise[k].to("cpu").to(clips.dtype)
                k += 1
            else:
                fill = torch.tensor(value, dtype=torch.float32).to(clips.dtype).view(3, 1, 1, 1)
            if h > 0 and w > 0:
                e[:, :, top:top + h, left:left + w] = fill
        erased.append(e)
    out = torch.empty_like(clips)
    for i, r in enumerate(rows.tolist()):
        p, mode, (y0, x0, y1, x1) = r[0], r[1], r[2:6]
        if mode == _lib.PTX_MIX_MIXUP:
            out[i] = erased[p].mul(1.0 - float(lam[i])).add_(erased[i].mul(float(lam[i])))
        elif mode == _lib.PTX_MIX_CUTMIX:
            out[i] = erased[i]
            out[i][:, :, y0:y1, x0:x1] = erased[p][:, :, y0:y1, x0:x1]
        else:
            out[i] = erased[i]
    return out


def batch_mix_targets_torch(labels, num_classes, params, smoothing=0.0):
    """torch-on-CPU statement of `BatchMix.targets`: fp32 [N, num_classes].  One-hot rows with off = smoothing / K and
    on = 1 - smoothing + off; a mixed clip's row is  row_p.mul(1.0 - lam).add_(row_i.mul(lam)),  an unmixed clip keeps its own."""
    rows, lam = _mix_params(params, len(labels), "batch_mix_targets_torch")
    off = float(smoothing) / int(num_classes)
    on = 1.0 - float(smoothing) + off
    onehot = torch.full((len(labels), int(num_classes)), off, dtype=torch.float32)
    onehot.scatter_(1, torch.as_tensor(labels, dtype=torch.int64).cpu().view(-1, 1), on)
    out = onehot.clone()
    for i, r in enumerate(rows.tolist()):
        if r[1] != _lib.PTX_MIX_NONE:
            out[i] = onehot[r[0]].mul(1.0 - float(lam[i])).add_(onehot[i].mul(float(lam[i])))
    return out


class BatchMix:
    """RandomErasing per clip, then MixUp / CutMix across the clips of a batch, on the NORMALISED clip, in one launch that writes
    the NCDHW clip once (include/ptx_amd_mix.h states the arithmetic, `batch_mix_torch` restates it: every output equals it bit
    for bit).  The last two steps of the video fine-tuning recipes (timm's Mixup + RandomErasing, torchvision's v2.MixUp /
    v2.CutMix / RandomErasing).

    mixup_alpha / cutmix_alpha: the Beta(alpha, alpha) of lam, 0 switches the kind off; prob: the chance that a call (mode="batch")
    or a clip (mode="clip") is mixed; switch_prob: with both alphas positive, the chance of CutMix.  erase_prob / erase_scale /
    erase_ratio: torchvision's RandomErasing p / scale / ratio; erase_value: a number or an RGB triple in the normalised domain (one
    per output channel), or "random".  generator: a CPU torch.Generator (None: torch's default one) for the draws;
    noise_generator: a CUDA torch.Generator (None: the device's default one) for erase_value="random".

    `bm(x)`: x a normalised CUDA clip [N,3,T,H,W], fp32 or bf16 -> the same shape and dtype; or uint8 CUDA frames [N,T,H,W,3] with
    `opts=` (a model or settings dict, as FramesToTensor takes) -> the normalised fp32 clip, `dtype=torch.bfloat16` the bf16 one:
    exactly FramesToTensor's value of every byte (bf16: rounded once) erased and mixed.  The draw is kept as `last_params` =
    (rows CPU int32 [N, 11] of MIX_FIELDS, lam CPU float64 [N]) and `bm(x, params=p)` replays a given one; a row names its partner,
    so a replayed draw may use any permutation.  `bm.targets(labels, num_classes, smoothing)` gives the soft targets of the last
    (or a given) draw.

    The draw, on the host from `generator` (`draw`): first the erase of every clip in clip order, which is torchvision's
    RandomErasing.get_params on an H x W image (torch.rand(1) < erase_prob; then up to 10 attempts of area * uniform_(scale),
    exp(uniform_(log ratio)), h = int(round(sqrt(area * ratio))), w = int(round(sqrt(area / ratio))), accepted when h < H and
    w < W with i = randint(0, H - h + 1), j = randint(0, W - w + 1); no accepted attempt: no box); the box covers every frame and
    channel of the clip.  Then the mix, torchvision v2's, once per call (mode="batch") or per clip in clip order (mode="clip"):
    torch.rand(1) < prob; with both alphas positive torch.rand(1) < switch_prob chooses CutMix; lam =
    float(torch._sample_dirichlet(torch.tensor([[a, a]]), generator)[0, 0]); CutMix draws r_x = randint(W), r_y = randint(H), takes
    r = 0.5 * sqrt(1 - lam), the half extents int(r * W), int(r * H), the box clamped to the frame, and replaces lam by
    1 - box_area / (W * H).  The partner of clip i is clip (i - 1) mod N (`roll(1, 0)`).

    The one departure from torchvision: the noise of erase_value="random" is not drawn from the host stream but on the device, per
    erased clip in clip order, as torch.randn((3, T, h, w), device=.., generator=noise_generator) (fp32; rounded once to bf16 for
    bf16 output), packed into one buffer that the kernel copies from (`last_noise`; `bm(x, params=p, noise=buf)` replays it)."""

    def __init__(self, mixup_alpha=0.8, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, mode="batch", erase_prob=0.25,
                 erase_scale=(0.02, 0.33), erase_ratio=(0.3, 3.3), erase_value=0, generator=None, noise_generator=None):
        for name, v in (("mixup_alpha", mixup_alpha), ("cutmix_alpha", cutmix_alpha)):
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v) or v < 0:
                raise PtxError("BatchMix: %s must be a finite number >= 0, got %r" % (name, v))
        for name, v in (("prob", prob), ("switch_prob", switch_prob), ("erase_prob", erase_prob)):
            if not isinstance(v, (int, float)) or isinstance(v, bool) or not 0.0 <= v <= 1.0:
                raise PtxError("BatchMix: %s must be a probability in [0, 1], got %r" % (name, v))
        if mode not in ("batch", "clip"):
            raise PtxError("BatchMix: mode must be 'batch' or 'clip', got %r (timm's 'pair' mode is not offered)" % (mode,))
        pairs = []
        for name, v, hi in (("erase_scale", erase_scale, 1.0), ("erase_ratio", erase_ratio, float("inf"))):
            try:
                lo_, hi_ = (float(c) for c in v)
                ok = (0.0 <= lo_ <= hi_ <= hi) if name == "erase_scale" else (0.0 < lo_ <= hi_ and math.isfinite(hi_))
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise PtxError("BatchMix: %s must be a pair lo <= hi (scale in [0, 1], ratio positive), got %r" % (name, v))
            pairs.append((lo_, hi_))
        for name, g in (("generator", generator), ("noise_generator", noise_generator)):
            _check_generator(g, "BatchMix", name)
        if generator is not None and generator.device.type != "cpu":
            raise PtxError("BatchMix: generator must be a CPU torch.Generator (the draws are made on the host)")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob, self.mode, self.erase_prob = float(prob), float(switch_prob), mode, float(erase_prob)
        self.erase_scale, self.erase_ratio = pairs
        self.erase_value = _mix_erase_value(erase_value)
        self._log_ratio = [float(v) for v in torch.log(torch.tensor(self.erase_ratio))]     # float32 logarithms, as torchvision's
        self.generator, self.noise_generator = generator, noise_generator
        self.last_params, self.last_noise = None, None

    # ---- host only: no device is touched -------------------------------------------------------
    def _draw_erase(self, H, W):
        g = self.generator
        if not bool(torch.rand(1, generator=g) < self.erase_prob):
            return 0, 0, 0, 0, 0
        area = H * W
        for _ in range(10):
            erase_area = area * torch.empty(1).uniform_(self.erase_scale[0], self.erase_scale[1], generator=g).item()
            aspect = torch.exp(torch.empty(1).uniform_(self._log_ratio[0], self._log_ratio[1], generator=g)).item()
            h, w = int(round(math.sqrt(erase_area * aspect))), int(round(math.sqrt(erase_area / aspect)))
            if not (h < H and w < W):
                continue
            i = int(torch.randint(0, H - h + 1, size=(1,), generator=g))
            j = int(torch.randint(0, W - w + 1, size=(1,), generator=g))
            return 1, i, j, h, w
        return 0, 0, 0, 0, 0

    def _draw_mix(self, H, W):
        g = self.generator
        if self.mixup_alpha <= 0 and self.cutmix_alpha <= 0:
            return _lib.PTX_MIX_NONE, 1.0, (0, 0, 0, 0)
        if not bool(torch.rand(1, generator=g) < self.prob):
            return _lib.PTX_MIX_NONE, 1.0, (0, 0, 0, 0)
        cutmix = self.cutmix_alpha > 0
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cutmix = bool(torch.rand(1, generator=g) < self.switch_prob)
        a = self.cutmix_alpha if cutmix else self.mixup_alpha
        lam = float(torch._sample_dirichlet(torch.tensor([[a, a]]), g)[0, 0])
        if not cutmix:
            return _lib.PTX_MIX_MIXUP, lam, (0, 0, 0, 0)
        r_x = int(torch.randint(W, size=(1,), generator=g))
        r_y = int(torch.randint(H, size=(1,), generator=g))
        r = 0.5 * math.sqrt(1.0 - lam)
        r_w_half, r_h_half = int(r * W), int(r * H)
        x1, y1 = max(r_x - r_w_half, 0), max(r_y - r_h_half, 0)
        x2, y2 = min(r_x + r_w_half, W), min(r_y + r_h_half, H)
        return _lib.PTX_MIX_CUTMIX, float(1.0 - (x2 - x1) * (y2 - y1) / (W * H)), (y1, x1, y2, x2)

    def draw(self, N, H, W):
        """The draw of N clips of H x W frames: (rows CPU int32 [N, 11] of MIX_FIELDS, lam CPU float64 [N]); see the class for the
        order.  An unmixed clip has mode 0, lam 1 and is its own partner."""
        N, H, W = int(N), int(H), int(W)
        erase = [self._draw_erase(H, W) for _ in range(N)]
        shared = self._draw_mix(H, W) if self.mode == "batch" else None
        rows, lam = [], []
        for i in range(N):
            mode, l, box = shared if shared is not None else self._draw_mix(H, W)
            rows.append(((i - 1) % N if mode != _lib.PTX_MIX_NONE else i, mode) + tuple(box) + tuple(erase[i]))
            lam.append(l)
        return torch.tensor(rows, dtype=torch.int32).view(N, len(MIX_FIELDS)), torch.tensor(lam, dtype=torch.float64)

    def check_params(self, params, N=None, H=None, W=None):
        """`params` as (CPU int32 [N, 11], CPU float64 [N]) tensors, or PtxError: shapes, N, and with H and W the library's own
        check of the rows (`batch_mix_rows`, ptx_batch_mix_supported): a partner or a mode out of range, a box or an erase
        rectangle outside the H x W frame or with a negative extent, a lam that is not finite or outside [0, 1].  No device is
        touched."""
        rows, lam = _mix_params(params, N)
        bad = np.flatnonzero((rows[:, 6] != 0) & (rows[:, 6] != 1))
        if len(bad):
            raise PtxError("BatchMix: params[%d]: the erase flag must be 0 or 1, got %d" % (bad[0], rows[bad[0], 6]))
        bad = np.flatnonzero(~np.isfinite(lam) | (lam < 0.0) | (lam > 1.0))
        if len(bad):
            raise PtxError("BatchMix: params[%d]: lam = %r must be finite and in [0, 1]" % (bad[0], float(lam[bad[0]])))
        if H is not None and W is not None:
            r, noise = batch_mix_rows((rows, lam), 1, self.erase_value)
            _mix_supported(r, noise, 1, H, W)
        return torch.from_numpy(rows.astype(np.int32)), torch.from_numpy(lam)

    def _rows_for(self, N, T, H, W, params, src_mode, out_mode):
        """The checked host rows and the noise size of a call on N clips of T frames of H x W: of a new draw (kept as
        last_params) or of `params`."""
        if params is None:
            params = self.last_params = self.draw(N, H, W)
        else:
            params = self.check_params(params, N)
        rows, noise = batch_mix_rows(params, T, self.erase_value, N)
        return _mix_supported(rows, noise, T, H, W, src_mode, out_mode), noise

    # ---- the launch ----------------------------------------------------------------------------
    def _noise(self, rows, noise_elems, T, device, dtype, noise):
        """The packed noise buffer of a call: given, or drawn per erased clip in clip order."""
        if noise_elems == 0:
            return None
        if noise is not None:
            if not isinstance(noise, torch.Tensor) or noise.device != device or noise.dtype != dtype or noise.numel() != noise_elems:
                raise PtxError("BatchMix: noise= must be a %s tensor of %d elements on %s (last_noise of the same draw)" % (
                    dtype, noise_elems, device))
            return noise.contiguous().view(-1)
        parts = []
        for r in rows[rows[:, _lib.PTX_MIX_W_ERASE_KIND] == _lib.PTX_MIX_ERASE_NOISE]:
            h, w = int(r[_lib.PTX_MIX_W_ERASE + 2]), int(r[_lib.PTX_MIX_W_ERASE + 3])
            parts.append(torch.randn((3, T, h, w), device=device, generator=self.noise_generator).to(dtype).view(-1))
        return torch.cat(parts)

    def _run(self, f5, params, mode, norm, dtype):
        """The stage on contiguous uint8 frames f5 [N,T,H,W,3]: `params`, or a draw that is kept as `last_params`; see `_launch`.
        The library refuses PTX_RESIZE_OUT_U8: erasing and mixing are defined on normalised values."""
        N, T, H, W, _ = f5.shape
        rows, noise_elems = self._rows_for(N, T, H, W, params, _lib.PTX_MIX_SRC_U8, mode)
        return self._launch(f5, _lib.PTX_MIX_SRC_U8, mode, N, T, H, W, dtype, norm, rows, noise_elems)

    def _launch(self, src, src_mode, out_mode, N, T, H, W, dtype, norm, rows, noise_elems, noise=None):
        """The launch on a contiguous CUDA source (uint8 [N,T,H,W,3] or a normalised [N,3,T,H,W]) with the checked host rows of
        `_rows_for`: the normalised [N,3,T,H,W] of `dtype`."""
        with torch.cuda.device(src.device):
            buf = self._noise(rows, noise_elems, T, src.device, dtype, noise)
            self.last_noise = buf
            dev_rows = torch.from_numpy(rows.reshape(-1)).to(src.device)                 # one upload
            y = torch.empty((N, 3, T, H, W), device=src.device, dtype=dtype)
            desc = _lib.MixDesc(N, T, H, W, src_mode, out_mode, noise_elems)
            check(_lib.lib().ptx_batch_mix_apply(C.byref(desc), C.c_void_p(src.data_ptr()), C.c_void_p(dev_rows.data_ptr()),
                                                 C.c_void_p(buf.data_ptr()) if buf is not None else None, C.c_void_p(y.data_ptr()),
                                                 C.byref(norm) if norm is not None else None,
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ptx_batch_mix_apply")
        return y

    def __call__(self, x, params=None, opts=None, dtype=None, noise=None):
        if not isinstance(x, torch.Tensor):
            raise PtxError("BatchMix: expected a CUDA tensor, got %s" % type(x).__name__)
        if x.dtype == torch.uint8:
            if x.dim() != 5 or x.shape[-1] != 3:
                raise PtxError("BatchMix: uint8 frames must be [N,T,H,W,3], got shape %s" % (tuple(x.shape),))
            if opts is None:
                raise PtxError("BatchMix: uint8 frames need opts= (a model or settings dict with input_space / input_range / mean / "
                               "std): the arithmetic is defined on normalised values")
            dtype = torch.float32 if dtype is None else dtype
            if dtype not in (torch.float32, torch.bfloat16):
                raise PtxError("BatchMix: dtype must be torch.float32 or torch.bfloat16, got %s" % (dtype,))
            N, T, H, W, _ = x.shape
            src_mode, norm = _lib.PTX_MIX_SRC_U8, FramesToTensor(opts).norm
        elif x.dtype in (torch.float32, torch.bfloat16):
            if x.dim() != 5 or x.shape[1] != 3:
                raise PtxError("BatchMix: a normalised clip must be [N,3,T,H,W], got shape %s" % (tuple(x.shape),))
            if dtype is not None and dtype != x.dtype:
                raise PtxError("BatchMix: a normalised clip keeps its dtype (%s), got dtype=%s" % (x.dtype, dtype))
            N, _, T, H, W = x.shape
            src_mode = _lib.PTX_MIX_SRC_F32 if x.dtype == torch.float32 else _lib.PTX_MIX_SRC_BF16
            dtype, norm = x.dtype, None
        else:
            raise PtxError("BatchMix: expected uint8 frames or an fp32 / bf16 clip, got dtype %s" % (x.dtype,))
        _check_not_empty(x, "BatchMix")
        out_mode = _out_mode(dtype)
        if params is not None or x.is_cuda:                          # given params are validated before a device is touched
            rows, noise_elems = self._rows_for(N, T, H, W, params, src_mode, out_mode)
        if not x.is_cuda:
            raise PtxError("BatchMix: expected a CUDA tensor (no CPU fallback; batch_mix_torch states the arithmetic)")
        return self._launch(x.contiguous(), src_mode, out_mode, N, T, H, W, dtype, norm, rows, noise_elems, noise)

    def targets(self, labels, num_classes, smoothing=0.0, params=None):
        """Soft targets fp32 [N, num_classes] of CUDA int64 labels [N] for the LAST call's draw (or `params`): one-hot rows with
        off = smoothing / K and on = 1 - smoothing + off, mixed exactly as MixUp mixes pixels, in fp32, with the draw's lam (CutMix:
        its adjusted lam) and partner; clips that were not mixed keep their own row (`batch_mix_targets_torch` restates it)."""
        if not isinstance(num_classes, int) or isinstance(num_classes, bool) or num_classes < 1:
            raise PtxError("BatchMix: num_classes must be a positive integer, got %r" % (num_classes,))
        if not isinstance(smoothing, (int, float)) or isinstance(smoothing, bool) or not 0.0 <= smoothing <= 1.0:
            raise PtxError("BatchMix: smoothing must be in [0, 1], got %r" % (smoothing,))
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.dim() != 1:
            raise PtxError("BatchMix: labels must be an int64 tensor [N]")
        N = labels.shape[0]
        if params is None:
            if self.last_params is None:
                raise PtxError("BatchMix: targets() needs a draw: call the transform first or pass params=")
            params = self.last_params
        params = self.check_params(params, N)
        rows, _ = batch_mix_rows(params, 1, 0, N)
        rows[:, _lib.PTX_MIX_W_BOX:_lib.PTX_MIX_W_ERASE_KIND + 1] = 0    # the boxes and the erase play no part here
        _mix_supported(rows, 0, 1, 1, 1)                             # partners, modes, lam
        if not labels.is_cuda:
            raise PtxError("BatchMix: labels must be a CUDA tensor (no CPU fallback; batch_mix_targets_torch states the arithmetic)")
        off = float(smoothing) / num_classes
        on = 1.0 - float(smoothing) + off
        with torch.cuda.device(labels.device):
            lab = labels.contiguous()
            dev_rows = torch.from_numpy(rows.reshape(-1)).to(labels.device)
            y = torch.empty((N, num_classes), device=labels.device, dtype=torch.float32)
            check(_lib.lib().ptx_batch_mix_targets(C.c_void_p(lab.data_ptr()), C.c_void_p(dev_rows.data_ptr()), C.c_void_p(y.data_ptr()),
                                                   N, num_classes, off, on, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "ptx_batch_mix_targets")
        return y


# ---------------------------------------------------------------------------------------------
# The clip stages behind the resize of TransformFrames / SampleClips
# ---------------------------------------------------------------------------------------------
_STAGES = ("color", "blur", "augment", "mix")            # the recipes' order: the stages run, and so draw, in it
_STAGE_TYPES = {"color": ColorJitter, "blur": GaussianBlur, "augment": RandAugment, "mix": BatchMix}


def _apply_stages(stages, frames_u8, out, dtype, norm, params):
    """The stages behind a resize, in the order of `_STAGES`.  stages: name -> stage (None or missing: off), at least one on;
    frames_u8: the resize's uint8 output [N,T,S,S,3] or of a lower rank (one clip); params: name -> checked params (None or
    missing: the stage draws when it runs and keeps the draw as `last_params`).  The last stage writes the output of `out` /
    `dtype` with `norm`, every stage in front of it uint8 frames."""
    present = [name for name in _STAGES if stages.get(name) is not None]
    lead = frames_u8.dim()
    f5 = frames_u8.view((1,) * (5 - lead) + tuple(frames_u8.shape))
    for name in present[:-1]:
        f5 = stages[name]._run(f5, params.get(name), _lib.PTX_RESIZE_OUT_U8, None, torch.uint8)
    mode = _out_mode(dtype, out)
    if out == "frames":
        norm, dtype = None, torch.uint8
    return _restore_rank(stages[present[-1]]._run(f5, params.get(present[-1]), mode, norm, dtype), lead, mode)


class _ClipStages:
    """What TransformFrames and SampleClips share: the stages `color`, `blur`, `augment` and `mix` behind their resize, the
    checks of those arguments (`who` names the class in messages, `_NOUN` what it calls itself), the checks of a call's
    `*_params`, and `_resize`, the resize half of a call with stages."""

    def _init_stages(self, who, out, color, augment, mix):
        for name, stage in (("color", color), ("augment", augment), ("mix", mix)):
            if stage is not None and not isinstance(stage, _STAGE_TYPES[name]):
                raise PtxError("%s: %s must be a pretorched.transforms.%s or None, got %r" % (who, name, _STAGE_TYPES[name].__name__, stage))
        if mix is not None and out != "tensor":
            raise PtxError("%s: mix= needs out='tensor': erasing and mixing are defined on normalised values, out='frames' returns "
                           "uint8 frames (forward_frames(.., transform=) takes those alone)" % who)
        self.color, self.augment, self.mix = color, augment, mix

    def _init_blur(self, who, blur):
        """After `size` is known: the kernel must fit the S x S output."""
        if blur is not None and not isinstance(blur, GaussianBlur):
            raise PtxError("%s: blur must be a pretorched.transforms.GaussianBlur or None, got %r" % (who, blur))
        if blur is not None and max(blur.kernel_size) // 2 >= self.size:
            raise PtxError("%s: blur: kernel_size=%r does not fit the %dx%d output (H=%d, W=%d): reflect padding needs "
                           "kernel_size // 2 < H, W" % (who, blur.kernel_size, self.size, self.size, self.size, self.size))
        self.blur = blur

    def _init_resize_half(self):
        """Last in a constructor.  `_resize` is this object without its stages, writing uint8 frames (the generator and the
        tables cache are shared with it), or None when no stage is given."""
        self._resize = None
        if any(getattr(self, name) is not None for name in _STAGES):
            rs = self._resize = copy.copy(self)
            rs.color = rs.blur = rs.augment = rs.mix = None
            rs.out, rs.dtype = "frames", torch.float32

    def _checked_params(self, who, given, order, validate=True):
        """`given` maps a stage's name to a call's `<name>_params`.  In `order`, a given one whose stage is missing is refused and,
        with `validate`, every other given one is replaced by its checked form.  No device is touched."""
        for name in order:
            if given[name] is None:
                continue
            stage = getattr(self, name)
            if stage is None:
                raise PtxError("%s: %s_params= needs a %s built with %s=%s(..)" % (who, name, self._NOUN, name, _STAGE_TYPES[name].__name__))
            if validate:
                given[name] = stage.check_params(given[name], *(() if name == "color" else (None, self.size, self.size)))
        return given

    def _run_stages(self, frames_u8, given):
        """The stages on `_resize`'s output with the checked `given` params: the output of `out` / `dtype`."""
        return _apply_stages({name: getattr(self, name) for name in _STAGES}, frames_u8, self.out, self.dtype, self.norm, given)


class TransformFrames(_ClipStages):
    """Resize + crop (+ flip) of decoded uint8 frames on the device, bit-exact with PIL's bilinear resize, then
    TransformImage's tensor half (`out="tensor"`) or nothing more (`out="frames"`).

    opts: a model or settings dict with input_size / input_space / input_range / mean / std.  scale and
    preserve_aspect_ratio as in TransformImage (utils.py:36-59); crop: "center" (CenterCrop(max(input_size))) or an
    explicit (top, left) in the resized frame; hflip / vflip: flip the cropped window horizontally / vertically; dtype:
    torch.float32 or torch.bfloat16 (the fp32 value rounded once) for out="tensor".

    random_crop / random_hflip / random_vflip (TransformImage's switches of the same names, utils.py:36-70): every CLIP of a
    call gets a window / flips of its own, drawn by `draw` from `generator` (None: torch's default CPU generator, so
    `torch.manual_seed` governs) and shared by all frames of the clip; the whole batch is still one launch and the draw is
    kept as `last_params`.  `tf(frames, params=p)` applies given parameters instead (on any TransformFrames).

    random_short_side=(a, b) / random_resized_crop=True | dict(scale=(0.08, 1.0), ratio=(3/4, 4/3)): every clip gets a
    resize GEOMETRY of its own (see `draw_geometry`), still in one resize launch: a small launch builds the clips'
    coefficient tables on the device from the [N, 10] geometry rows, which are kept as `last_geometry`.
    random_short_side is the video recipes' scale jitter (the short side resized to R = randint(a, b + 1), then the
    centre window or, with random_crop, a drawn one); it needs a >= max(input_size), preserve_aspect_ratio=True and
    crop="center", and does not use `scale`.  random_resized_crop is torchvision's RandomResizedCrop
    (`random_resized_crop_box` states the algorithm; torchvision is not needed): the drawn box is resized to S x S; it
    excludes random_crop, random_short_side and an explicit crop and ignores scale / preserve_aspect_ratio.  Flips
    apply as above.  `tf(frames, geometry=g)` applies given rows instead (on any TransformFrames).

    color: a `ColorJitter` (None: off, the code path without it).  The resize then writes uint8 frames into scratch and the
    colour launch writes the output of `out` / `dtype`; the lists are drawn per clip after every other draw of the call and
    kept as `color.last_params`; `tf(frames, color_params=p)` applies given lists instead.

    augment: a `RandAugment` (None: off, the code path without it), run behind the resize and behind `color`: the stage in front
    writes uint8 scratch and the augment's last position writes the output of `out` / `dtype`.  Its draw comes after every other
    draw of the call (a seed gives the same geometry and colour with and without it) and is kept as `augment.last_params`;
    `tf(frames, augment_params=p)` applies a given draw instead.

    mix: a `BatchMix` (None: off, the code path without it), run last: RandomErasing per clip and MixUp / CutMix across the clips
    of the call on the normalised values, in one launch that reads the uint8 frames of the stage in front and writes the output.
    It needs out="tensor".  Its draw comes after every other draw of the call (when it shares their generator, a seed gives the
    same geometry, colour and augment draws with and without it) and is kept as `mix.last_params`; `tf(frames, mix_params=p)`
    applies a given draw instead.

    blur: a `GaussianBlur` (None: off, the code path without it), run behind `color` and in front of `augment` and `mix`, the view
    recipes' order (RandomResizedCrop, flip, ColorJitter, RandomGrayscale, GaussianBlur).  The stage in front writes uint8 scratch
    and the blur launch writes the output of `out` / `dtype` when it is the last stage.  Its draw comes in execution order: after
    the colour draw (a seed gives the same geometry and colour lists with and without it), before the augment's and the mix's;
    it is kept as `blur.last_params`; `tf(frames, blur_params=p)` applies a given draw instead.

    interpolation: the resize filter, Pillow's `Image.resize(size, filter)` bit for bit: "nearest" | "box" | "bilinear" (the
    default) | "hamming" | "bicubic" | "lanczos", Pillow's integer code, or an enum of either (PIL.Image.Resampling,
    torchvision's InterpolationMode); kept as the canonical string `interpolation`.  The contract stays crop-then-resize
    (torchvision's resized_crop), not `resize(box=)`.  A per-clip geometry (random_short_side, random_resized_crop,
    geometry=) supports nearest, box, bilinear and bicubic: its tables are built on the device.  No draw depends on it."""

    CACHE_SIZE = 8
    _NOUN = "transform"

    def __init__(self, opts, scale=0.875, preserve_aspect_ratio=True, crop="center", hflip=False, out="tensor",
                 dtype=torch.float32, *, random_crop=False, random_hflip=False, random_vflip=False, vflip=False,
                 generator=None, random_short_side=None, random_resized_crop=False, color=None, augment=None,
                 interpolation="bilinear", mix=None, blur=None):
        self.interpolation = check_interpolation(interpolation, "TransformFrames")
        self._init_stages("TransformFrames", out, color, augment, mix)
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
        self.crop, self.hflip, self.vflip, self.out, self.dtype = crop, bool(hflip), bool(vflip), out, dtype
        self.random_crop, self.random_hflip, self.random_vflip = bool(random_crop), bool(random_hflip), bool(random_vflip)
        if self.random_crop and not isinstance(crop, str):
            raise PtxError("TransformFrames: random_crop=True draws the window; it cannot be combined with crop=%r" % (crop,))
        if self.random_hflip and self.hflip:
            raise PtxError("TransformFrames: random_hflip=True draws the flip; it cannot be combined with hflip=True")
        if self.random_vflip and self.vflip:
            raise PtxError("TransformFrames: random_vflip=True draws the flip; it cannot be combined with vflip=True")
        self.random = self.random_crop or self.random_hflip or self.random_vflip
        self.generator, self.last_params = _check_generator(generator, "TransformFrames"), None
        self.size = int(max(self.input_size))
        self._init_blur("TransformFrames", blur)
        if not isinstance(crop, str):
            crop_window(1 << 30, 1 << 30, self.size, crop)          # a malformed or negative window fails here
        elif crop != "center":
            raise PtxError("TransformFrames: crop must be 'center' or (top, left), got %r" % (crop,))
        self._cache = collections.OrderedDict()                      # (H, W, device) -> device tables
        self.random_short_side, self.random_resized_crop, self.last_geometry = None, None, None
        if random_short_side is not None:
            try:
                a, b = random_short_side
                ok = all(isinstance(v, int) and not isinstance(v, bool) for v in (a, b)) and a <= b
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise PtxError("TransformFrames: random_short_side must be a pair of integers (a, b) with a <= b, got %r" % (
                    random_short_side,))
            if a < self.size:
                raise PtxError("TransformFrames: random_short_side=(%d, %d): the short side must hold the %dx%d window (a >= %d; "
                               "padding crops are not offered)" % (a, b, self.size, self.size, self.size))
            if not self.preserve_aspect_ratio:
                raise PtxError("TransformFrames: random_short_side resizes the short side; it needs preserve_aspect_ratio=True")
            if not isinstance(crop, str):
                raise PtxError("TransformFrames: random_short_side draws the resized size; it cannot be combined with crop=%r "
                               "(use random_crop=True or the centre window)" % (crop,))
            self.random_short_side = (a, b)
        if random_resized_crop is not False and random_resized_crop is not None:
            rrc = {"scale": (0.08, 1.0), "ratio": (3.0 / 4.0, 4.0 / 3.0)}
            if isinstance(random_resized_crop, dict):
                extra = set(random_resized_crop) - set(rrc)
                if extra:
                    raise PtxError("TransformFrames: random_resized_crop takes scale and ratio, got %s" % sorted(extra))
                rrc.update(random_resized_crop)
            elif random_resized_crop is not True:
                raise PtxError("TransformFrames: random_resized_crop must be True or dict(scale=.., ratio=..), got %r" % (
                    random_resized_crop,))
            for key in ("scale", "ratio"):
                try:
                    lo_, hi_ = (float(v) for v in rrc[key])
                    ok = 0.0 < lo_ <= hi_ and math.isfinite(hi_)
                except (TypeError, ValueError):
                    ok = False
                if not ok:
                    raise PtxError("TransformFrames: random_resized_crop: %s must be a pair 0 < lo <= hi, got %r" % (key, rrc[key]))
                rrc[key] = (lo_, hi_)
            if self.random_crop:
                raise PtxError("TransformFrames: random_resized_crop draws the box; it cannot be combined with random_crop=True")
            if self.random_short_side is not None:
                raise PtxError("TransformFrames: random_resized_crop cannot be combined with random_short_side")
            if not isinstance(crop, str):
                raise PtxError("TransformFrames: random_resized_crop draws the box; it cannot be combined with crop=%r" % (crop,))
            self.random_resized_crop = rrc
        self.per_clip_geometry = self.random_short_side is not None or self.random_resized_crop is not None
        if self.per_clip_geometry:
            self._device_filter("random_short_side / random_resized_crop")
        self._init_resize_half()

    def _device_filter(self, what):
        """The PTX_RESAMPLE_* code of this transform's filter for the device table builder, or PtxError: a per-clip
        geometry's tables are built on the device, which takes the filters whose weights are polynomials."""
        if self.interpolation not in DEVICE_INTERPOLATIONS:
            raise PtxError("TransformFrames: interpolation=%r cannot be combined with a per-clip geometry (%s): its "
                           "trigonometric weights are built on the host only; a per-clip geometry supports %s (the %s filter "
                           "serves every fixed-geometry route: a fixed window, random_crop / flips, SampleViews)" % (
                               self.interpolation, what, ", ".join(DEVICE_INTERPOLATIONS), self.interpolation))
        return INTERPOLATIONS.index(self.interpolation)

    def tables(self, H, W):
        """Host tables for H x W frames (numpy; see build_tables)."""
        return build_tables(H, W, self.input_size, self.scale, self.preserve_aspect_ratio, self.crop, self.hflip, self.vflip,
                            interpolation=self.interpolation)

    def frame_tables(self, H, W):
        """Host tables of the whole resized frame of H x W frames (numpy; see build_frame_tables)."""
        return build_frame_tables(H, W, self.input_size, self.scale, self.preserve_aspect_ratio, interpolation=self.interpolation)

    def draw(self, N, H, W):
        """Parameters of N clips of H x W frames: a CPU int32 tensor [N, 4] of (top, left, hflip, vflip) in the resized
        frame.  Per clip, in order (torchvision's consumption order for RandomCrop, RandomHorizontalFlip,
        RandomVerticalFlip): random_crop draws top = randint(0, h - S + 1), then left = randint(0, w - S + 1); random_hflip
        draws rand(1) < 0.5; random_vflip draws rand(1) < 0.5.  A switch that is off consumes nothing and gives the
        constructor's crop / hflip / vflip."""
        S, g = self.size, self.generator
        h, w = resized_size(H, W, self.input_size, self.scale, self.preserve_aspect_ratio)
        if self.random_crop:
            crop_window(h, w, S, (0, 0))                            # the frame must hold a window
        else:
            top, left = crop_window(h, w, S, self.crop)
        hf, vf = int(self.hflip), int(self.vflip)
        out = torch.empty((int(N), 4), dtype=torch.int32)
        for n in range(int(N)):
            if self.random_crop:
                top = int(torch.randint(0, h - S + 1, (1,), generator=g))
                left = int(torch.randint(0, w - S + 1, (1,), generator=g))
            if self.random_hflip:
                hf = int(torch.rand(1, generator=g) < 0.5)
            if self.random_vflip:
                vf = int(torch.rand(1, generator=g) < 0.5)
            out[n, 0], out[n, 1], out[n, 2], out[n, 3] = top, left, hf, vf
        return out

    def check_params(self, params, N, H, W):
        """`params` ([N, 4] integers: an array or a CPU tensor) as a CPU int32 tensor, or PtxError: N does not match, a
        window does not fit the resized frame of H x W frames, a flip is not 0 / 1."""
        p = _host_array(params, "TransformFrames: params must be an integer array or a CPU tensor [N, 4], got a CUDA tensor")
        if p.dtype.kind not in "iu":
            raise PtxError("TransformFrames: params must hold integers, got dtype %s" % (p.dtype,))
        if p.ndim != 2 or p.shape[1] != 4:
            raise PtxError("TransformFrames: params must be [N, 4] (top, left, hflip, vflip), got shape %s" % (p.shape,))
        if p.shape[0] != N:
            raise PtxError("TransformFrames: params hold %d clips, the frames hold N = %d" % (p.shape[0], N))
        p = p.astype(np.int64)
        S = self.size
        h, w = resized_size(H, W, self.input_size, self.scale, self.preserve_aspect_ratio)
        for n, (top, left, hf, vf) in enumerate(p.tolist()):
            if top < 0 or left < 0 or top + S > h or left + S > w:
                raise PtxError("TransformFrames: params[%d]: the %dx%d crop at (%d, %d) does not fit the resized %dx%d frame "
                               "(padding crops are not offered)" % (n, S, S, top, left, h, w))
            if hf not in (0, 1) or vf not in (0, 1):
                raise PtxError("TransformFrames: params[%d]: a flip must be 0 or 1, got hflip=%d vflip=%d" % (n, hf, vf))
        return torch.from_numpy(p.astype(np.int32))

    def draw_geometry(self, N, H, W):
        """Geometries of N clips of H x W frames: a CPU int32 tensor [N, 10] of (box_top, box_left, box_h, box_w, h, w, top,
        left, hflip, vflip) -- see `geometry_tables` for the meaning.  Per clip, in order, from `generator`:
          1. random_short_side: R = randint(a, b + 1), (h, w) = resized_size_for(H, W, R), the box is the frame;  or
             random_resized_crop: the `random_resized_crop_box` sequence, the box is resized to S x S;
             neither: the box is the frame and (h, w) = resized_size(..) as for every clip of a plain call;
          2. random_crop: top = randint(0, h - S + 1), then left = randint(0, w - S + 1) (else the centre window of h x w,
             or the constructor's crop; (0, 0) for random_resized_crop);
          3. random_hflip: rand(1) < 0.5;   4. random_vflip: rand(1) < 0.5.
        A switch that is off consumes nothing."""
        S, g = self.size, self.generator
        N, H, W = int(N), int(H), int(W)
        hf, vf = int(self.hflip), int(self.vflip)
        out = torch.empty((N, 10), dtype=torch.int32)
        for n in range(N):
            box = (0, 0, H, W)
            if self.random_short_side is not None:
                a, b = self.random_short_side
                h, w = resized_size_for(H, W, int(torch.randint(a, b + 1, (1,), generator=g)))
            elif self.random_resized_crop is not None:
                box = random_resized_crop_box(H, W, self.random_resized_crop["scale"], self.random_resized_crop["ratio"], g)
                h, w = S, S
            else:
                h, w = resized_size(H, W, self.input_size, self.scale, self.preserve_aspect_ratio)
            if self.random_crop:
                crop_window(h, w, S, (0, 0))                        # the resized frame must hold a window
                top = int(torch.randint(0, h - S + 1, (1,), generator=g))
                left = int(torch.randint(0, w - S + 1, (1,), generator=g))
            else:
                top, left = crop_window(h, w, S, self.crop)
            if self.random_hflip:
                hf = int(torch.rand(1, generator=g) < 0.5)
            if self.random_vflip:
                vf = int(torch.rand(1, generator=g) < 0.5)
            out[n] = torch.tensor(box + (h, w, top, left, hf, vf), dtype=torch.int32)
        return out

    def _checked_geometry(self, geometry, N, H, W):
        self._device_filter("geometry=")
        p = _host_array(geometry, "TransformFrames: geometry must be an integer array or a CPU tensor [N, 10], got a CUDA tensor")
        if p.dtype.kind not in "iu":
            raise PtxError("TransformFrames: geometry must hold integers, got dtype %s" % (p.dtype,))
        if p.ndim != 2 or p.shape[1] != 10:
            raise PtxError("TransformFrames: geometry must be [N, 10] (%s), got shape %s" % (", ".join(GEOMETRY_FIELDS), p.shape))
        if p.shape[0] != N:
            raise PtxError("TransformFrames: geometry holds %d clips, the frames hold N = %d" % (p.shape[0], N))
        p = p.astype(np.int64)
        S = self.size
        for n, (bt, bl, bh, bw, h, w, top, left, hf, vf) in enumerate(p.tolist()):
            if bh < 1 or bw < 1 or bt < 0 or bl < 0 or bt + bh > H or bl + bw > W:
                raise PtxError("TransformFrames: geometry[%d]: the %dx%d box at (%d, %d) is empty or does not lie inside the %dx%d "
                               "frame" % (n, bh, bw, bt, bl, H, W))
            if h < S or w < S:
                raise PtxError("TransformFrames: geometry[%d]: a %dx%d crop does not fit the resized %dx%d box (padding crops are "
                               "not offered)" % (n, S, S, h, w))
            if top < 0 or left < 0 or top + S > h or left + S > w:
                raise PtxError("TransformFrames: geometry[%d]: the %dx%d crop at (%d, %d) does not fit the resized %dx%d box "
                               "(padding crops are not offered)" % (n, S, S, top, left, h, w))
            if hf not in (0, 1) or vf not in (0, 1):
                raise PtxError("TransformFrames: geometry[%d]: a flip must be 0 or 1, got hflip=%d vflip=%d" % (n, hf, vf))
        if N == 0:
            raise PtxError("TransformFrames: empty batch")
        f = self.interpolation
        taps = (_axis_taps(p[:, 2], p[:, 4], p[:, 6], S, f), _axis_taps(p[:, 3], p[:, 5], p[:, 7], S, f))
        for name, t, src, dst in (("rows", taps[0], 2, 4), ("columns", taps[1], 3, 5)):
            n = int(np.argmax(t))
            if t[n] > _lib.PTX_RESIZE_MAX_TAPS:
                raise PtxError("TransformFrames: geometry[%d]: down-scaling %d %s to %d%s needs %d taps, the kernel's cap is "
                               "PTX_RESIZE_MAX_TAPS = %d" % (n, p[n, src], name, p[n, dst], "" if f == "bilinear" else
                                                             " with the %s filter" % f, t[n], _lib.PTX_RESIZE_MAX_TAPS))
        if f == "nearest" and int(p[:, 4:6].max()) > _lib.PTX_RESAMPLE_NEAREST_MAX_EXTENT:
            raise PtxError("TransformFrames: geometry: a resized extent of %d exceeds the nearest filter's device walk (%d)" % (
                int(p[:, 4:6].max()), _lib.PTX_RESAMPLE_NEAREST_MAX_EXTENT))
        if f == "bicubic":             # the coefficient bounds of tables the host does not build (box / nearest / bilinear: k >= 0, sum 2**22)
            for n_in, n_out, start in ((p[:, 2], p[:, 4], p[:, 6]), (p[:, 3], p[:, 5], p[:, 7])):
                kmax, ksum = _axis_bicubic_bound(n_in, n_out, start, S)
                check_coefficients(np.array([kmax.max()]), "TransformFrames: geometry")
                check_coefficients(np.array([ksum.max()]), "TransformFrames: geometry")
        return torch.from_numpy(p.astype(np.int32)), int(taps[0].max()), int(taps[1].max())

    def check_geometry(self, geometry, N, H, W):
        """`geometry` ([N, 10] integers: an array or a CPU tensor, see `draw_geometry`) as a CPU int32 tensor, or PtxError: N
        does not match, a box is empty or leaves the H x W frame, h or w is below S, a window does not fit h x w, a flip is
        not 0 / 1, an axis needs more than PTX_RESIZE_MAX_TAPS taps.  No device is touched."""
        return self._checked_geometry(geometry, N, H, W)[0]

    def _device_tables(self, H, W, device, whole=False):
        key = (H, W, str(device)) + (("frame",) if whole else ())
        hit = self._cache.get(key)
        if hit is not None:
            self._cache.move_to_end(key)
            return hit
        t = self.frame_tables(H, W) if whole else self.tables(H, W)
        parts = [a.reshape(-1) for a in t["rows"] + t["cols"]]
        offs = np.cumsum([0] + [p.size for p in parts])
        buf = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(device)     # one small upload per input size
        hit = (buf, [int(o) * 4 for o in offs[:-1]], t["rows"][2].shape[1], t["cols"][2].shape[1])
        self._cache[key] = hit
        while len(self._cache) > self.CACHE_SIZE:
            self._cache.popitem(last=False)
        return hit

    def __call__(self, frames, params=None, geometry=None, color_params=None, augment_params=None, mix_params=None, blur_params=None):
        """uint8 CUDA frames [N,T,H,W,3] | [T,H,W,3] | [H,W,3], any H, W  ->
        out="tensor": [N,3,T,S,S] | [3,T,S,S] | [3,S,S] (fp32 or bf16);  out="frames": uint8, same rank, H, W -> S, S.
        A `YUV420` source is taken in place of the frames (converted while the kernel stages its rows: the same bits as
        the call on the converted frames); the result's rank follows `src.lead` as it follows the tensor's rank.
        A random transform draws one (top, left, hflip, vflip) per clip (N draws for [N,T,..], one for the lower ranks;
        per-image augmentation of an image batch is [N,1,H,W,3]) and keeps the draw as `last_params`; params ([N, 4]
        integers, see `check_params`) applies given parameters instead.  Both are one launch.
        With random_short_side / random_resized_crop one geometry row is drawn per clip in the same way and kept as
        `last_geometry`; geometry ([N, 10] integers, see `check_geometry`) applies given rows instead, on any transform.
        Both are a table-builder launch plus one resize launch.
        With color= (a `ColorJitter`) the resize writes uint8 frames into scratch and the colour launch writes the output;
        the colour lists are drawn after every other draw of the call, clip by clip (a seed gives the same geometry with and
        without colour), and kept as `color.last_params`; color_params applies given lists instead.
        With augment= (a `RandAugment`) its positions run behind the resize and behind the colour launch, the last one writing
        the output; its draw comes after every other draw of the call and is kept as `augment.last_params`; augment_params
        applies a given draw instead.
        With mix= (a `BatchMix`) its launch runs last, behind the resize, the colour launch and the augment, reads their uint8
        frames and writes the erased and mixed normalised clip; its draw comes after every other draw of the call and is kept as
        `mix.last_params` (`mix.targets(labels, K)` gives the matching soft targets); mix_params applies a given draw instead.
        With blur= (a `GaussianBlur`) its launch runs behind the colour launch and in front of the augment and the mix; its draw
        comes in that order too (after the colour draw) and is kept as `blur.last_params`; blur_params applies a given draw."""
        given = self._checked_params("TransformFrames", {"blur": blur_params, "mix": mix_params, "color": color_params,
                                                         "augment": augment_params}, ("blur", "mix", "color", "augment"))
        if self._resize is not None:                                 # the resize (every draw of the plain call), then the stages
            u8 = self._resize(frames, params=params, geometry=geometry)
            self.last_params, self.last_geometry = self._resize.last_params, self._resize.last_geometry
            return self._run_stages(u8, given)
        if params is not None and geometry is not None:
            raise PtxError("TransformFrames: params= and geometry= cannot be combined (a geometry row holds the window and flips)")
        if params is not None and self.per_clip_geometry:
            raise PtxError("TransformFrames: params= are windows in ONE resized frame; with random_short_side / "
                           "random_resized_crop every clip has its own: pass geometry=")
        if isinstance(frames, YUV420):
            return self._call_yuv(frames, params, geometry)
        if not isinstance(frames, torch.Tensor):
            raise PtxError("TransformFrames: frames must be a uint8 CUDA tensor, got %s" % type(frames).__name__)
        if frames.dim() not in (3, 4, 5):
            raise PtxError("TransformFrames: expected [N,T,H,W,3], [T,H,W,3] or [H,W,3], got shape %s" % (tuple(frames.shape),))
        if frames.shape[-1] != 3:
            raise PtxError("TransformFrames: frames must have 3 interleaved channels, got %d" % frames.shape[-1])
        if geometry is not None:                                     # validated before a device is touched
            geometry = self.check_geometry(geometry, frames.shape[0] if frames.dim() == 5 else 1, frames.shape[-3], frames.shape[-2])
        f5 = _u8_cuda_5d(frames, "TransformFrames")
        N, T, H, W, Cc = f5.shape
        if N * T == 0:
            raise PtxError("TransformFrames: empty batch")
        S, lead, mode = self.size, frames.dim(), _out_mode(self.dtype, self.out)
        if params is not None or geometry is not None or self.random or self.per_clip_geometry:
            if geometry is not None or self.per_clip_geometry:
                y = self._call_geometry(f5, None, N, T, H, W, frames.device, geometry)
            else:
                y = self._call_windows(f5, None, N, T, H, W, frames.device, params)
            return _restore_rank(y, lead, mode)
        with torch.cuda.device(frames.device):
            buf, offs, taps_h, taps_w = self._device_tables(H, W, frames.device)
            y = _alloc_out(mode, N, T, S, S, frames.device, self.dtype)
            desc = ResizeDesc(N, T, H, W, Cc, S, S, taps_h, taps_w, mode)
            base = buf.data_ptr()
            check(_lib.lib().ptx_resize_frames_u8(C.byref(desc), C.c_void_p(f5.data_ptr()),
                                                  *[C.c_void_p(base + o) for o in offs],
                                                  C.c_void_p(y.data_ptr()), C.byref(self.norm),
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "ptx_resize_frames_u8")
        return _restore_rank(y, lead, mode)

    def _call_windows(self, f5, ysrc, N, T, H, W, device, params):
        """The per-clip windows launch on frames f5 [N,T,H,W,3] or, when ysrc is given, on a YUV source: the drawn or the
        given parameters, the tables of the whole resized frame (cached per input size), one small upload of the
        parameters."""
        S = self.size
        if params is None:
            p = self.last_params = self.draw(N, H, W)
        else:
            p = self.check_params(params, N, H, W)
        with torch.cuda.device(device):
            buf, offs, taps_h, taps_w = self._device_tables(H, W, device, whole=True)
            h, w = resized_size(H, W, self.input_size, self.scale, self.preserve_aspect_ratio)
            wins = p.contiguous().to(device)
            mode = _out_mode(self.dtype, self.out)
            y = _alloc_out(mode, N, T, S, S, device, self.dtype)
            desc = ResizeDesc(N, T, H, W, 3, S, S, taps_h, taps_w, mode)
            base = buf.data_ptr()
            name = "ptx_resize_frames_%s_windows" % ("u8" if ysrc is None else _abi_of(ysrc))
            source = C.c_void_p(f5.data_ptr()) if ysrc is None else C.byref(ysrc)
            check(getattr(_lib.lib(), name)(C.byref(desc), source, *[C.c_void_p(base + o) for o in offs], h, w,
                                            C.c_void_p(wins.data_ptr()), C.c_void_p(y.data_ptr()), C.byref(self.norm),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)
        return y

    def _call_geometry(self, f5, ysrc, N, T, H, W, device, geometry):
        """The per-clip tables path on frames f5 [N,T,H,W,3] or, when ysrc is given, on a YUV source: the drawn or the given
        geometry rows (one upload of N x 40 bytes), ptx_resize_build_tables into a scratch buffer, the tables launch.  The
        host only derives the tap pitch of each axis (from lo / hi of the entries; no weights)."""
        S = self.size
        code = self._device_filter("geometry=")
        if geometry is None:
            self.last_geometry = self.draw_geometry(N, H, W)
        g, taps_h, taps_w = self._checked_geometry(self.last_geometry if geometry is None else geometry, N, H, W)
        with torch.cuda.device(device):
            geo = g.contiguous().to(device)
            sizes = [N * S, N * S, N * S * taps_h, N * S, N * S, N * S * taps_w]
            buf = torch.empty(sum(sizes), device=device, dtype=torch.int32)
            offs = np.cumsum([0] + sizes[:-1])
            tabs = [C.c_void_p(buf.data_ptr() + int(o) * 4) for o in offs]
            mode = _out_mode(self.dtype, self.out)
            y = _alloc_out(mode, N, T, S, S, device, self.dtype)
            desc = ResizeDesc(N, T, H, W, 3, S, S, taps_h, taps_w, mode)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if code == _lib.PTX_RESAMPLE_BILINEAR:                   # the default: the launch it always was
                check(_lib.lib().ptx_resize_build_tables(C.byref(desc), C.c_void_p(geo.data_ptr()), *tabs, stream),
                      "ptx_resize_build_tables")
            else:
                check(_lib.lib().ptx_resize_build_tables_filter(C.byref(desc), C.c_void_p(geo.data_ptr()), code, *tabs, stream),
                      "ptx_resize_build_tables_filter")
            name = "ptx_resize_frames_%s_tables" % ("u8" if ysrc is None else _abi_of(ysrc))
            source = C.c_void_p(f5.data_ptr()) if ysrc is None else C.byref(ysrc)
            check(getattr(_lib.lib(), name)(C.byref(desc), source, *tabs, C.c_void_p(y.data_ptr()), C.byref(self.norm), stream),
                  name)
        return y

    def _call_yuv(self, src, params=None, geometry=None):
        if geometry is not None:                                     # validated before a device is touched
            geometry = self.check_geometry(geometry, src.N, src.H, src.W)
        ysrc, keep = src.source("TransformFrames")
        N, T, H, W, S = src.N, src.T, src.H, src.W, self.size
        mode = _out_mode(self.dtype, self.out)
        if params is not None or geometry is not None or self.random or self.per_clip_geometry:
            if geometry is not None or self.per_clip_geometry:
                y = self._call_geometry(None, ysrc, N, T, H, W, src.device, geometry)
            else:
                y = self._call_windows(None, ysrc, N, T, H, W, src.device, params)
            del keep
            return _restore_rank(y, src.lead + 2, mode)
        with torch.cuda.device(src.device):
            buf, offs, taps_h, taps_w = self._device_tables(H, W, src.device)
            y = _alloc_out(mode, N, T, S, S, src.device, self.dtype)
            desc = ResizeDesc(N, T, H, W, 3, S, S, taps_h, taps_w, mode)
            base = buf.data_ptr()
            name = "ptx_resize_frames_" + src._ABI
            check(getattr(_lib.lib(), name)(C.byref(desc), C.byref(ysrc), *[C.c_void_p(base + o) for o in offs],
                                            C.c_void_p(y.data_ptr()), C.byref(self.norm),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)
            del keep                                                 # planes (copies included) stayed alive up to the launch
        return _restore_rank(y, src.lead + 2, mode)


def _abi_of(ysrc):
    """The entry points' infix for a source descriptor: "yuv420" or "yuv420p16"."""
    return YUV420P16._ABI if isinstance(ysrc, Yuv420P16Src) else YUV420._ABI


def apply_frames_transform(transform, frames, who="forward_frames"):
    """The `transform=` hook of forward_frames: a TransformFrames with out="frames", applied to the raw frames, or a
    SampleClips with out="frames", applied to the raw videos (a list of any sizes and lengths).  A `YUV420` source has no
    RGB frames to pass on, so it needs one (a crop-only transform serves frames of the input size)."""
    if transform is None:
        if isinstance(frames, YUV420):
            raise PtxError("%s: a %s source needs transform=TransformFrames(.., out='frames') (the colour conversion "
                           "runs in its row staging; a crop-only transform serves frames that have the input size)" % (
                               who, frames._NAME))
        return frames
    if not isinstance(transform, (TransformFrames, SampleClips)) or transform.out != "frames":
        raise PtxError("%s: transform must be a pretorched.transforms.TransformFrames with out='frames', got %r" % (
            who, transform))
    return transform(frames)


# ---------------------------------------------------------------------------------------------
# multi-view sampling: clips x crops of a decoded video (deterministic test-time rules, no RNG)
# ---------------------------------------------------------------------------------------------
def clip_frame_indices(Tv, num_frames, frame_stride=1, clips=1, sampling="dense"):
    """Source frame of every (clip, frame): int64 [clips][num_frames], all in [0, Tv).
    dense: clips of `num_frames` frames `frame_stride` apart, their starts spread evenly over the video (the centre for
    one clip); a video shorter than one clip's span starts every clip at 0 and repeats its last frame.
    segments (TSN / TRN): the video is cut into `num_frames` segments, clip c takes the frame at (c + 0.5) / clips of
    each segment; `frame_stride` is not used."""
    Tv, T, clips = int(Tv), int(num_frames), int(clips)
    if Tv < 1:
        raise PtxError("SampleViews: the video has no frames")
    out = np.empty((clips, T), np.int64)
    if sampling == "dense":
        span = (T - 1) * int(frame_stride) + 1
        for c in range(clips):
            if Tv >= span:
                start = ((Tv - span) * c) // (clips - 1) if clips > 1 else (Tv - span) // 2
            else:
                start = 0
            for i in range(T):
                out[c, i] = min(start + i * int(frame_stride), Tv - 1)
    elif sampling == "segments":
        for c in range(clips):
            for i in range(T):
                out[c, i] = min(int((i + (c + 0.5) / clips) * Tv / T), Tv - 1)
    else:
        raise PtxError("SampleViews: sampling must be 'dense' or 'segments', got %r" % (sampling,))
    return out


def crop_windows(h, w, S, crops=1):
    """(top, left) of the `crops` S x S windows in the resized h x w frame: the centre crop, or three windows along the
    longer side (the width when w >= h) at offsets 0, round((L - S) / 2), L - S with the other axis centred."""
    if crops == 1:
        return [crop_window(h, w, S, "center")]
    if crops != 3:
        raise PtxError("SampleViews: crops must be 1 or 3, got %r" % (crops,))
    ctop, cleft = int(round((h - S) / 2.0)), int(round((w - S) / 2.0))
    if w >= h:
        return [crop_window(h, w, S, (ctop, off)) for off in (0, cleft, w - S)]
    return [crop_window(h, w, S, (off, cleft)) for off in (0, ctop, h - S)]


def _union(table, starts, S):
    """Entries of the sorted distinct indices that the windows [start, start + S) contain, and each window's first entry."""
    idx = np.unique(np.concatenate([np.arange(st, st + S) for st in starts]))
    lo, n, k = (a[idx] for a in table)
    taps = int(n.max())
    offs = [int(np.searchsorted(idx, st)) for st in starts]
    return (np.ascontiguousarray(lo), np.ascontiguousarray(n), np.ascontiguousarray(k[:, :taps])), offs


class SampleViews:
    """Multi-view sampling of decoded uint8 video on the device: `clips` temporal clips x `crops` spatial crops, every
    view resized + cropped exactly as `TransformFrames(opts, crop=window)` does on the clip's frames (bit-identical).

    opts, scale, preserve_aspect_ratio, out, dtype: as for TransformFrames.  num_frames / frame_stride / clips /
    sampling: see `clip_frame_indices`; crops: 1 or 3, see `crop_windows`.  View v = clip * crops + crop.
    share: "auto" (the library picks the workgroup shape), "always" / "never" force the shared horizontal pass on or
    off (measurements; the results are the same bits).  interpolation: the resize filter, as for TransformFrames (all six:
    the tables are built on the host, one per frame size)."""

    CACHE_SIZE = 8
    _SHARE = {"auto": _lib.PTX_VIEWS_SHARE_AUTO, "always": _lib.PTX_VIEWS_SHARE_ALWAYS, "never": _lib.PTX_VIEWS_SHARE_NEVER}

    def __init__(self, opts, num_frames=16, frame_stride=4, clips=10, crops=3, sampling="dense", scale=0.875,
                 preserve_aspect_ratio=True, out="frames", dtype=torch.float32, share="auto", interpolation="bilinear"):
        self.interpolation = check_interpolation(interpolation, "SampleViews")
        if out not in ("tensor", "frames"):
            raise PtxError("SampleViews: out must be 'tensor' or 'frames', got %r" % (out,))
        if dtype not in (torch.float32, torch.bfloat16):
            raise PtxError("SampleViews: dtype must be torch.float32 or torch.bfloat16, got %s" % (dtype,))
        if out == "frames" and dtype != torch.float32:
            raise PtxError("SampleViews: out='frames' returns uint8 frames; dtype=%s applies to out='tensor' only" % (dtype,))
        if not (isinstance(scale, (int, float)) and scale > 0):
            raise PtxError("SampleViews: scale must be a positive number, got %r" % (scale,))
        for name, v in (("num_frames", num_frames), ("frame_stride", frame_stride), ("clips", clips)):
            if not isinstance(v, int) or isinstance(v, bool) or v < 1:
                raise PtxError("SampleViews: %s must be a positive integer, got %r" % (name, v))
        if crops not in (1, 3) or isinstance(crops, bool):
            raise PtxError("SampleViews: crops must be 1 or 3, got %r" % (crops,))
        if sampling not in ("dense", "segments"):
            raise PtxError("SampleViews: sampling must be 'dense' or 'segments', got %r" % (sampling,))
        if share not in self._SHARE:
            raise PtxError("SampleViews: share must be 'auto', 'always' or 'never', got %r" % (share,))
        self.input_size = [int(v) for v in _opt(opts, "input_size")]
        self.input_space, self.input_range = _opt(opts, "input_space"), _opt(opts, "input_range")
        self.mean, self.std = list(_opt(opts, "mean")), list(_opt(opts, "std"))
        self.norm = NormDesc.make(self.mean, self.std, self.input_space, self.input_range)
        self.num_frames, self.frame_stride, self.clips, self.crops = num_frames, frame_stride, clips, crops
        self.sampling, self.scale, self.preserve_aspect_ratio = sampling, float(scale), bool(preserve_aspect_ratio)
        self.out, self.dtype, self.share = out, dtype, share
        self.size = int(max(self.input_size))
        self.num_views = clips * crops
        self._cache = collections.OrderedDict()                      # (H, W, device) -> device tables
        self._idx_cache = collections.OrderedDict()                  # (Tv, device) -> device frame index table

    def frame_indices(self, Tv):
        """Host: int64 [clips][num_frames], the source frame of every (clip, frame) of a video of Tv frames."""
        return clip_frame_indices(Tv, self.num_frames, self.frame_stride, self.clips, self.sampling)

    def windows(self, H, W):
        """Host: [(top, left)] * crops, the crop windows in the resized frame of H x W input frames."""
        h, w = resized_size(H, W, self.input_size, self.scale, self.preserve_aspect_ratio)
        if h <= 0 or w <= 0:
            raise PtxError("SampleViews: resized frame %dx%d is empty" % (h, w))
        return crop_windows(h, w, self.size, self.crops)

    def tables(self, H, W):
        """Host tables for H x W frames: `rows` / `cols` ((lo, n, k) over the union of the windows' rows / columns),
        `row_off` / `col_off` (each window's first entry), `S`, `resized`, `windows`."""
        S = self.size
        h, w = resized_size(H, W, self.input_size, self.scale, self.preserve_aspect_ratio)
        wins = self.windows(H, W)
        rows, row_off = _union(resize_axis_table(H, h, self.interpolation), [t for t, _ in wins], S)
        cols, col_off = _union(resize_axis_table(W, w, self.interpolation), [l for _, l in wins], S)
        _check_taps(rows, cols, H, W, h, w, self.interpolation, "SampleViews")
        return {"rows": rows, "cols": cols, "row_off": row_off, "col_off": col_off, "S": S, "resized": (h, w), "windows": wins}

    def view_tables(self, H, W, crop):
        """The tables of ONE crop window cut out of the union tables, in build_tables' form (apply_tables_numpy takes it)."""
        t = self.tables(H, W)
        return {"rows": _select(t["rows"], t["row_off"][crop], t["S"]), "cols": _select(t["cols"], t["col_off"][crop], t["S"]),
                "S": t["S"], "resized": t["resized"], "window": t["windows"][crop]}

    def _cached(self, cache, key, make):
        hit = cache.get(key)
        if hit is not None:
            cache.move_to_end(key)
            return hit
        hit = cache[key] = make()
        while len(cache) > self.CACHE_SIZE:
            cache.popitem(last=False)
        return hit

    def _device_tables(self, H, W, device):
        def make():
            t = self.tables(H, W)
            parts = [a.reshape(-1) for a in t["rows"] + t["cols"]]
            offs = np.cumsum([0] + [p.size for p in parts])
            buf = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(device)  # one small upload per input size
            return buf, [int(o) * 4 for o in offs[:-1]], t
        return self._cached(self._cache, (H, W, str(device)), make)

    def _device_indices(self, Tv, device):
        return self._cached(self._idx_cache, (Tv, str(device)),
                            lambda: torch.from_numpy(self.frame_indices(Tv).astype(np.int32)).to(device))

    def describe(self, H, W):
        """Which workgroup shape the library runs for H x W frames: "shared" (one horizontal pass over the union of
        the windows per sampled frame) or "per-window"; raises PtxError when neither fits."""
        d = self._desc(1, 1, H, W, 3, H * W * 3, H * W * 3, self.tables(H, W), 0, self.num_views)
        r = _lib.lib().ptx_resize_views_u8_supported(C.byref(d))
        if r == 0:
            raise PtxError("SampleViews: %s" % _lib.lib().ptx_last_error().decode(errors="replace"))
        return "shared" if r == 2 else "per-window"

    def _desc(self, N, Tv, H, W, Cc, stride_n, stride_t, t, v0, nv):
        d = ViewsDesc()
        d.N, d.Tv, d.H, d.W, d.C = N, Tv, H, W, Cc
        d.clips, d.T, d.crops = self.clips, self.num_frames, self.crops
        d.stride_n, d.stride_t = stride_n, stride_t
        d.S, d.Ur, d.Uc = self.size, len(t["rows"][0]), len(t["cols"][0])
        d.taps_h, d.taps_w = t["rows"][2].shape[1], t["cols"][2].shape[1]
        for k in range(self.crops):
            d.row_off[k], d.col_off[k] = t["row_off"][k], t["col_off"][k]
        d.v0, d.nv = v0, nv
        d.out_mode = _out_mode(self.dtype, self.out)
        d.share = self._SHARE[self.share]
        return d

    def __call__(self, video):
        """uint8 CUDA video [N,Tv,H,W,3] | [Tv,H,W,3], any Tv, H, W  ->  every view:
        out="frames": uint8 [N,V,T,S,S,3] | [V,T,S,S,3];  out="tensor": fp32 | bf16 [N,V,3,T,S,S] | [V,3,T,S,S]."""
        return self.sample(video)

    def sample(self, video, v0=0, nv=None):
        """Views v0 .. v0 + nv - 1 only (default: all from v0 on), shaped as __call__'s result with V -> nv.  The
        video is read in place: any view whose frames are contiguous [H,W,3] blocks (slices and steps over N and Tv
        included) is taken without a copy.  A `YUV420` source ([N,Tv,..] or [Tv,..] planes) is read in place of the video."""
        if isinstance(video, YUV420):
            return self._sample_yuv(video, v0, nv)
        if not isinstance(video, torch.Tensor):
            raise PtxError("SampleViews: video must be a uint8 CUDA tensor, got %s" % type(video).__name__)
        if video.dim() not in (4, 5):
            raise PtxError("SampleViews: expected [N,Tv,H,W,3] or [Tv,H,W,3], got shape %s" % (tuple(video.shape),))
        if video.shape[-1] != 3:
            raise PtxError("SampleViews: frames must have 3 interleaved channels, got %d" % video.shape[-1])
        if not video.is_cuda or video.dtype != torch.uint8:
            raise PtxError("SampleViews: video must be a uint8 CUDA tensor (no CPU fallback)")
        lead = video.dim()
        v5 = video if lead == 5 else video.unsqueeze(0)
        N, Tv, H, W, Cc = v5.shape
        if N * Tv * H * W == 0:
            raise PtxError("SampleViews: empty video")
        V = self.num_views
        nv = V - v0 if nv is None else nv
        if not (isinstance(v0, int) and isinstance(nv, int) and 0 <= v0 and 1 <= nv and v0 + nv <= V):
            raise PtxError("SampleViews: view range [%r, %r + %r) is outside the %d views" % (v0, v0, nv, V))
        frame = H * W * Cc
        sn, st = v5.stride(0), v5.stride(1)
        if (tuple(v5.stride()[2:]) != (W * Cc, Cc, 1) or (Tv > 1 and st < frame) or (N > 1 and sn < frame)):
            v5 = v5.contiguous()                                     # frames that are not [H,W,3] blocks: one copy
            sn, st = v5.stride(0), v5.stride(1)
        st = st if Tv > 1 else frame
        sn = sn if N > 1 else max(frame, st * Tv)
        S, T = self.size, self.num_frames
        with torch.cuda.device(video.device):
            buf, offs, t = self._device_tables(H, W, video.device)
            idx = self._device_indices(Tv, video.device)
            if self.out == "frames":
                y = torch.empty((N, nv, T, S, S, Cc), device=video.device, dtype=torch.uint8)
            else:
                y = torch.empty((N, nv, Cc, T, S, S), device=video.device, dtype=self.dtype)
            desc = self._desc(N, Tv, H, W, Cc, sn, st, t, v0, nv)
            base = buf.data_ptr()
            check(_lib.lib().ptx_resize_views_u8(C.byref(desc), C.c_void_p(v5.data_ptr()), C.c_void_p(idx.data_ptr()),
                                                 *[C.c_void_p(base + o) for o in offs],
                                                 C.c_void_p(y.data_ptr()), C.byref(self.norm),
                                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                  "ptx_resize_views_u8")
        return y if lead == 5 else y[0]

    def _sample_yuv(self, src, v0, nv):
        if src.lead not in (2, 3):
            raise PtxError("SampleViews: expected a %s video with planes [N,Tv,H,W] or [Tv,H,W], got one frame" % src._NAME)
        ysrc, keep = src.source("SampleViews")
        N, Tv, H, W = src.N, src.T, src.H, src.W
        V = self.num_views
        nv = V - v0 if nv is None else nv
        if not (isinstance(v0, int) and isinstance(nv, int) and 0 <= v0 and 1 <= nv and v0 + nv <= V):
            raise PtxError("SampleViews: view range [%r, %r + %r) is outside the %d views" % (v0, v0, nv, V))
        S, T = self.size, self.num_frames
        with torch.cuda.device(src.device):
            buf, offs, t = self._device_tables(H, W, src.device)
            idx = self._device_indices(Tv, src.device)
            if self.out == "frames":
                y = torch.empty((N, nv, T, S, S, 3), device=src.device, dtype=torch.uint8)
            else:
                y = torch.empty((N, nv, 3, T, S, S), device=src.device, dtype=self.dtype)
            desc = self._desc(N, Tv, H, W, 3, 0, 0, t, v0, nv)         # the source carries the frame strides
            base = buf.data_ptr()
            name = "ptx_resize_views_" + src._ABI
            check(getattr(_lib.lib(), name)(C.byref(desc), C.byref(ysrc), C.c_void_p(idx.data_ptr()),
                                            *[C.c_void_p(base + o) for o in offs],
                                            C.c_void_p(y.data_ptr()), C.byref(self.norm),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), name)
            del keep
        return y if src.lead == 3 else y[0]


# ---------------------------------------------------------------------------------------------
# training clips from a batch of videos of any sizes and lengths: a source row, an index row and a geometry row per clip
# ---------------------------------------------------------------------------------------------
_CLIP_SRC = np.dtype([("base", "<u8"), ("stride_t", "<i8"), ("H", "<i4"), ("W", "<i4"), ("Tv", "<i4"), ("reserved", "<i4")])


class SampleClips(_ClipStages):
    """Training clips from decoded videos of ANY sizes and lengths in one resize launch: `clips` clips of `num_frames`
    frames per video, every clip resized + cropped (+ flipped) exactly as `TransformFrames` with the same spatial switches
    does on the clip's gathered frames (bit-identical), read in place through a frame index row per clip.

    opts, scale, preserve_aspect_ratio, crop, hflip, vflip, random_crop, random_hflip, random_vflip, random_short_side,
    random_resized_crop, out, dtype, generator: exactly TransformFrames' (same meaning, same checks; the transform is kept
    as `spatial`).  num_frames / frame_stride / clips / sampling: as for SampleViews.  random_start=True draws the
    temporal position per clip (see `draw`); False takes SampleViews' deterministic rows (`clip_frame_indices`).

    A call draws one index row and one geometry row per output clip (kept as `last_indices`, CPU int64 [N*clips, T], and
    `last_geometry`, CPU int32 [N*clips, 10]); `sc(videos, indices=.., geometry=..)` applies given rows instead, on any
    SampleClips.  Output clip j comes from video j // clips.

    color: a `ColorJitter` applied behind the resize, one list per output clip, as for `TransformFrames(.., color=)`.
    augment: a `RandAugment` applied behind the resize and the colour, one draw per output clip, as for `TransformFrames(.., augment=)`.
    mix: a `BatchMix` applied last, across the output clips of the call, as for `TransformFrames(.., mix=)` (out="tensor" only).
    blur: a `GaussianBlur` applied behind the colour and in front of the augment, one draw per output clip, as for `TransformFrames(.., blur=)`.
    interpolation: the resize filter, passed to `spatial`; every clip's tables are built on the device, so nearest, box,
    bilinear and bicubic (see TransformFrames)."""

    _NOUN = "sampler"

    def __init__(self, opts, num_frames=16, frame_stride=4, clips=1, sampling="dense", random_start=True, scale=0.875,
                 preserve_aspect_ratio=True, crop="center", hflip=False, vflip=False, random_crop=False, random_hflip=False,
                 random_vflip=False, random_short_side=None, random_resized_crop=False, out="tensor", dtype=torch.float32,
                 generator=None, color=None, augment=None, interpolation="bilinear", mix=None, blur=None):
        self._init_stages("SampleClips", out, color, augment, mix)
        for name, v in (("num_frames", num_frames), ("frame_stride", frame_stride), ("clips", clips)):
            if not isinstance(v, int) or isinstance(v, bool) or v < 1:
                raise PtxError("SampleClips: %s must be a positive integer, got %r" % (name, v))
        if sampling not in ("dense", "segments"):
            raise PtxError("SampleClips: sampling must be 'dense' or 'segments', got %r" % (sampling,))
        self.spatial = TransformFrames(opts, scale, preserve_aspect_ratio, crop, hflip, out, dtype, random_crop=random_crop,
                                       random_hflip=random_hflip, random_vflip=random_vflip, vflip=vflip, generator=generator,
                                       random_short_side=random_short_side, random_resized_crop=random_resized_crop,
                                       interpolation=interpolation)
        self.interpolation = self.spatial.interpolation
        self._filter = self.spatial._device_filter("SampleClips builds every clip's tables on the device")
        self.num_frames, self.frame_stride, self.clips, self.sampling = num_frames, frame_stride, clips, sampling
        self.random_start, self.generator = bool(random_start), generator
        self.out, self.dtype, self.size, self.norm = out, dtype, self.spatial.size, self.spatial.norm
        self._init_blur("SampleClips", blur)
        self.last_indices, self.last_geometry = None, None
        self._init_resize_half()

    # ---- host only: no device is touched -------------------------------------------------------
    @staticmethod
    def _shapes(shapes):
        try:
            out = [tuple(int(v) for v in s) for s in shapes]
        except (TypeError, ValueError):
            out = None
        if not out or any(len(s) != 3 for s in out):
            raise PtxError("SampleClips: shapes must be a non-empty list of (Tv, H, W), got %r" % (shapes,))
        for i, s in enumerate(out):
            if min(s) < 1:
                raise PtxError("SampleClips: videos[%d] is empty (Tv, H, W = %d, %d, %d)" % ((i,) + s))
        return out

    def draw_indices(self, Tv):
        """One clip's frame index row (a list of T ints in [0, Tv)) from `generator`.
        dense: span = (T - 1) * frame_stride + 1; Tv >= span draws start = randint(0, Tv - span + 1) (one draw), a shorter
        video starts at 0 and consumes nothing; frame i is min(start + i * frame_stride, Tv - 1).
        segments (TSN training): lo_i = (i * Tv) // T, hi_i = max(((i + 1) * Tv) // T, lo_i + 1); one call
        r = randint(0, 2**30, (T,)); frame i is lo_i + r_i % (hi_i - lo_i)."""
        T, g, Tv = self.num_frames, self.generator, int(Tv)
        if self.sampling == "dense":
            span = (T - 1) * self.frame_stride + 1
            start = int(torch.randint(0, Tv - span + 1, (1,), generator=g)) if Tv >= span else 0
            return [min(start + i * self.frame_stride, Tv - 1) for i in range(T)]
        r = torch.randint(0, 2 ** 30, (T,), generator=g).tolist()
        out = []
        for i in range(T):
            lo = (i * Tv) // T
            hi = max(((i + 1) * Tv) // T, lo + 1)
            out.append(lo + r[i] % (hi - lo))
        return out

    def draw(self, shapes):
        """(indices, geometry) for videos of `shapes` = [(Tv, H, W), ...]: CPU int64 [N*clips, T] and CPU int32 [N*clips, 10].
        Video by video, clip by clip: first the temporal draw (`draw_indices`; with random_start=False nothing is drawn and
        clip c takes row c of `clip_frame_indices(Tv, T, frame_stride, clips, sampling)`), then the spatial one, which is
        `spatial.draw_geometry(1, H, W)` -- a fixed transform draws nothing and gives every clip of a video the same row."""
        shapes = self._shapes(shapes)
        K, T = self.clips, self.num_frames
        idx = torch.empty((len(shapes) * K, T), dtype=torch.int64)
        geo = torch.empty((len(shapes) * K, 10), dtype=torch.int32)
        for i, (Tv, H, W) in enumerate(shapes):
            fixed = None if self.random_start else clip_frame_indices(Tv, T, self.frame_stride, K, self.sampling)
            for c in range(K):
                j = i * K + c
                idx[j] = torch.tensor(self.draw_indices(Tv) if fixed is None else fixed[c], dtype=torch.int64)
                try:
                    geo[j] = self.spatial.draw_geometry(1, H, W)[0]
                except PtxError as e:
                    raise PtxError("SampleClips: clip %d (videos[%d], %dx%d): %s" % (j, i, H, W, e))
        return idx, geo

    def _checked(self, indices, geometry, shapes):
        shapes = self._shapes(shapes)
        K, T = self.clips, self.num_frames
        NC = len(shapes) * K
        arrs = []
        for name, a, cols in (("indices", indices, T), ("geometry", geometry, 10)):
            a = _host_array(a, "SampleClips: %s must be an integer array or a CPU tensor [N*clips, %d], got a CUDA tensor" % (name, cols))
            if a.dtype.kind not in "iu":
                raise PtxError("SampleClips: %s must hold integers, got dtype %s" % (name, a.dtype))
            if a.ndim != 2 or a.shape[1] != cols:
                raise PtxError("SampleClips: %s must be [N*clips, %d], got shape %s" % (name, cols, a.shape))
            if a.shape[0] != NC:
                raise PtxError("SampleClips: %s holds %d clips, %d videos x %d clips need %d" % (name, a.shape[0], len(shapes), K, NC))
            arrs.append(a.astype(np.int64))
        idx, geo = arrs
        taps_h = taps_w = 1
        rows = []
        for i, (Tv, H, W) in enumerate(shapes):
            mine = idx[i * K:(i + 1) * K]
            bad = np.argwhere((mine < 0) | (mine >= Tv))
            if len(bad):
                c, t = (int(v) for v in bad[0])
                raise PtxError("SampleClips: clip %d (videos[%d]): frame index %d (position %d) is outside [0, %d)" % (
                    i * K + c, i, mine[c, t], t, Tv))
            try:
                g, th, tw = self.spatial._checked_geometry(geo[i * K:(i + 1) * K], K, H, W)
            except PtxError:
                for c in range(K):                                   # name the clip: its row alone fails the same way
                    try:
                        self.spatial._checked_geometry(geo[i * K + c:i * K + c + 1], 1, H, W)
                    except PtxError as e:
                        raise PtxError("SampleClips: clip %d (videos[%d], %dx%d): %s" % (i * K + c, i, H, W, e))
                raise
            rows.append(g)
            taps_h, taps_w = max(taps_h, th), max(taps_w, tw)
        return torch.from_numpy(idx), torch.cat(rows), taps_h, taps_w

    def check(self, indices, geometry, shapes):
        """`indices` ([N*clips, T]) and `geometry` ([N*clips, 10]) -- integer arrays or CPU tensors -- for videos of `shapes`
        as (CPU int64, CPU int32) tensors, or PtxError naming the clip: a wrong row count, an index outside [0, Tv_i), a row
        that `check_geometry` refuses for video i's own H x W."""
        return self._checked(indices, geometry, shapes)[:2]

    # ---- the call ------------------------------------------------------------------------------
    @staticmethod
    def _videos(videos):
        """The batch as a list of per-video sources (uint8 tensors [Tv,H,W,3] or YUV420 with planes [Tv,H,W]), checked on
        the host."""
        if isinstance(videos, YUV420):
            if videos.lead == 3:
                return [videos._like(videos.y[n], videos.u[n], None if videos.v is None else videos.v[n]) for n in range(videos.N)]
            if videos.lead != 2:
                raise PtxError("SampleClips: expected a %s source with planes [N,Tv,H,W] or [Tv,H,W], got %d leading "
                               "dimension(s)" % (videos._NAME, videos.lead - 1))
            return [videos]
        if isinstance(videos, torch.Tensor):
            if videos.dim() not in (4, 5):
                raise PtxError("SampleClips: expected [N,Tv,H,W,3], [Tv,H,W,3] or a list of videos, got shape %s" % (
                    tuple(videos.shape),))
            videos = list(videos) if videos.dim() == 5 else [videos]
        elif isinstance(videos, (list, tuple)):
            videos = list(videos)
        else:
            raise PtxError("SampleClips: videos must be a list of uint8 CUDA tensors [Tv,H,W,3] or YUV420 sources, one tensor "
                           "or one YUV420, got %s" % type(videos).__name__)
        if not videos:
            raise PtxError("SampleClips: empty batch (no videos)")
        yuv = isinstance(videos[0], YUV420)
        for i, v in enumerate(videos):
            if yuv != isinstance(v, YUV420):
                raise PtxError("SampleClips: videos[%d]: a batch is all tensors or all YUV420 sources" % i)
            if yuv:
                if type(v) is not type(videos[0]):
                    raise PtxError("SampleClips: videos[%d] is a %s source, videos[0] a %s: a batch is all of one source kind" % (
                        i, v._NAME, videos[0]._NAME))
                if v.lead != 2:
                    raise PtxError("SampleClips: videos[%d]: expected a %s source with planes [Tv,H,W], got %d leading "
                                   "dimension(s)" % (i, v._NAME, v.lead - 1))
                continue
            if not isinstance(v, torch.Tensor):
                raise PtxError("SampleClips: videos[%d] must be a uint8 CUDA tensor [Tv,H,W,3], got %s" % (i, type(v).__name__))
            if v.dtype != torch.uint8:
                raise PtxError("SampleClips: videos[%d] must be a uint8 tensor, got %s" % (i, v.dtype))
            if v.dim() != 4 or v.shape[-1] != 3:
                raise PtxError("SampleClips: videos[%d]: expected [Tv,H,W,3], got shape %s" % (i, tuple(v.shape)))
        devs = [v.device for v in videos]
        if len(set(devs)) != 1:
            i = next(i for i, d in enumerate(devs) if d != devs[0])
            raise PtxError("SampleClips: videos[%d] is on %s, videos[0] on %s: a batch lives on one device" % (i, devs[i], devs[0]))
        return videos

    def __call__(self, videos, indices=None, geometry=None, color_params=None, augment_params=None, mix_params=None, blur_params=None):
        """videos: a list / tuple of uint8 CUDA tensors [Tv_i,H_i,W_i,3] of any sizes and lengths on one device | one
        [N,Tv,H,W,3] tensor (N videos) | one [Tv,H,W,3] tensor | a list of `YUV420` sources with planes [Tv,H,W] | one
        `YUV420` with planes [N,Tv,H,W] or [Tv,H,W]  ->  out="tensor": [N*clips,3,T,S,S] (fp32 or bf16); out="frames": uint8
        [N*clips,T,S,S,3].  A video is read in place when its frames are contiguous [H,W,3] blocks (slices and steps over
        Tv included); any other video costs one `.contiguous()` copy of that video only.  One call is one upload (source,
        index and geometry rows in one buffer), one table-builder launch and one resize launch, whatever the batch holds;
        the tap pitches are the maxima over the batch.
        With color= (a `ColorJitter`) the resize writes uint8 clips into scratch and the colour launch writes the output: one
        list per output clip, drawn after every other draw of the call and kept as `color.last_params`; color_params applies
        given lists instead.  With augment= (a `RandAugment`) its positions run behind the resize and the colour launch, one draw
        per output clip after every other draw of the call (`augment.last_params`); augment_params applies a given draw instead.
        With mix= (a `BatchMix`) its launch runs last across the output clips (`mix.last_params`); mix_params applies a given draw.
        With blur= (a `GaussianBlur`) its launch runs behind the colour launch, one draw per output clip after the colour draw
        (`blur.last_params`); blur_params applies a given draw."""
        given = {"blur": blur_params, "mix": mix_params, "color": color_params, "augment": augment_params}
        self._checked_params("SampleClips", given, ("blur", "mix", "color", "augment"), validate=False)   # every refusal first
        if self._resize is not None:
            given = self._checked_params("SampleClips", given, ("blur", "color", "augment", "mix"))
            u8 = self._resize(videos, indices=indices, geometry=geometry)
            self.last_indices, self.last_geometry = self._resize.last_indices, self._resize.last_geometry
            return self._run_stages(u8, given)
        if (indices is None) != (geometry is None):
            raise PtxError("SampleClips: indices= and geometry= are given together (a replay) or not at all (a draw)")
        vids = self._videos(videos)
        yuv = isinstance(vids[0], YUV420)
        shapes = [(v.T, v.H, v.W) if yuv else tuple(int(n) for n in v.shape[:3]) for v in vids]
        if indices is None:                                          # validated before a device is touched
            drawn = self.draw(shapes)
            idx, geo, taps_h, taps_w = self._checked(drawn[0], drawn[1], shapes)
        else:
            idx, geo, taps_h, taps_w = self._checked(indices, geometry, shapes)
        device = vids[0].device
        if device.type != "cuda":
            raise PtxError("SampleClips: videos must be uint8 CUDA tensors (no CPU fallback)")
        K, T, S = self.clips, self.num_frames, self.size
        NC = len(vids) * K
        keep = []
        src = np.zeros(len(vids), _CLIP_SRC)
        ysrc = (vids[0]._CLIP_SRC * len(vids))() if yuv else None
        for i, (v, (Tv, H, W)) in enumerate(zip(vids, shapes)):
            src[i]["H"], src[i]["W"], src[i]["Tv"] = H, W, Tv
            if yuv:
                ysrc[i].planes, planes = v.source("SampleClips")
                ysrc[i].H, ysrc[i].W, ysrc[i].Tv = H, W, Tv
                keep.append(planes)
                continue
            frame = H * W * 3
            if tuple(v.stride()[1:]) != (W * 3, 3, 1) or (Tv > 1 and v.stride(0) < frame):
                v = v.contiguous()                                   # frames that are not [H,W,3] blocks: one copy of this video
            keep.append(v)
            src[i]["base"], src[i]["stride_t"] = v.data_ptr(), (v.stride(0) if Tv > 1 else frame)
        parts = [np.repeat(src, K).view(np.uint8)]
        if yuv:
            parts.append(np.repeat(np.frombuffer(ysrc, dtype=np.uint8).reshape(len(vids), -1), K, axis=0).reshape(-1))
        parts += [idx.numpy().astype(np.int32).reshape(-1).view(np.uint8), geo.numpy().astype(np.int32).reshape(-1).view(np.uint8)]
        offs, total = [], 0
        for p in parts:                                              # every part starts on a 16-byte boundary
            offs.append(total)
            total += (p.size + 15) & ~15
        host = np.zeros(total, np.uint8)
        for o, p in zip(offs, parts):
            host[o:o + p.size] = p
        Hm, Wm = max(s[1] for s in shapes), max(s[2] for s in shapes)
        with torch.cuda.device(device):
            rows = torch.from_numpy(host).to(device)                 # the one upload of the call
            at = [C.c_void_p(rows.data_ptr() + o) for o in offs]
            sizes = [NC * S, NC * S, NC * S * taps_h, NC * S, NC * S, NC * S * taps_w]
            buf = torch.empty(sum(sizes), device=device, dtype=torch.int32)
            tabs = [C.c_void_p(buf.data_ptr() + int(o) * 4) for o in np.cumsum([0] + sizes[:-1])]
            mode = _out_mode(self.dtype, self.out)
            y = _alloc_out(mode, NC, T, S, S, device, self.dtype)
            desc = ResizeDesc(NC, T, Hm, Wm, 3, S, S, taps_h, taps_w, mode)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if self._filter == _lib.PTX_RESAMPLE_BILINEAR:           # the default: the launch it always was
                check(_lib.lib().ptx_resize_build_tables_clips(C.byref(desc), at[0], at[-1], *tabs, stream),
                      "ptx_resize_build_tables_clips")
            else:
                check(_lib.lib().ptx_resize_build_tables_clips_filter(C.byref(desc), at[0], at[-1], self._filter, *tabs, stream),
                      "ptx_resize_build_tables_clips_filter")
            name = "ptx_resize_clips_" + (vids[0]._ABI if yuv else "u8")
            check(getattr(_lib.lib(), name)(C.byref(desc), at[1] if yuv else at[0], at[-2], *tabs, C.c_void_p(y.data_ptr()),
                                            C.byref(self.norm), stream), name)
            del keep                                                 # videos (copies included) stayed alive up to the launch
        if indices is None:
            self.last_indices, self.last_geometry = idx, geo
        return y


# ---------------------------------------------------------------------------------------------
# Class activation maps (include/ptx_amd_cam.h): the uint8 map of a score field, its overlay on uint8 frames
# ---------------------------------------------------------------------------------------------
CAM_OUT = ("overlay", "heat", "map")                   # the PTX_CAM_OUT_* codes, by index


def cam_quantize_numpy(scores):
    """ptx_cam_quantize in numpy: float32 scores [N, k, *positions] -> uint8 of the same shape, one map per (n, j).  With mn / mx
    the smallest / largest score of the map that is not a NaN: v = 255 * ((s - mn) / (mx - mn)), every operation rounded to
    float32; 255 if v >= 255, trunc(v) if v > 0, else 0 (a NaN gives 0).  A flat map (mx == mn, or NaN throughout) is all zeros."""
    s = np.ascontiguousarray(np.asarray(scores), dtype=np.float32)
    if s.ndim < 2:
        raise PtxError("cam_quantize_numpy: scores must be [N, k, *positions] (got shape %s)" % (s.shape,))
    flat = s.reshape(s.shape[0] * s.shape[1], -1)
    out = np.zeros(flat.shape, np.uint8)
    with np.errstate(all="ignore"):
        for i, row in enumerate(flat):
            mn, mx = np.fmin.reduce(row), np.fmax.reduce(row)        # NaN only when every score is one
            if not mx > mn:
                continue
            v = np.float32(255.0) * ((row - mn) / (mx - mn))
            out[i] = np.where(v >= 255, 255, np.where(v > 0, np.trunc(v), 0)).astype(np.uint8)
    return out.reshape(s.shape)


def jet_colormap():
    """The default colour table, uint8 [256, 3]: level i at x = i / 255 is round(255 * clip(1.5 - |4 x - p|, 0, 1)) with p = 3, 2, 1
    for red, green, blue -- the piecewise-linear "jet" (blue, cyan, yellow, red).  Data, not a contract: any uint8 [256, 3] serves."""
    x = np.arange(256, dtype=np.float64)[:, None] / 255.0
    return np.floor(255.0 * np.clip(1.5 - np.abs(4.0 * x - np.array([3.0, 2.0, 1.0])[None, :]), 0.0, 1.0) + 0.5).astype(np.uint8)


CAM_COLORMAPS = {"jet": jet_colormap}


def _cam_colormap(colormap, who="CamOverlay"):
    if isinstance(colormap, str):
        if colormap not in CAM_COLORMAPS:
            raise PtxError("%s: colormap %r is not one of %s (or pass a uint8 [256, 3] array)" % (who, colormap, sorted(CAM_COLORMAPS)))
        return CAM_COLORMAPS[colormap]()
    lut = colormap.detach().cpu().numpy() if isinstance(colormap, torch.Tensor) else np.asarray(colormap)
    if lut.dtype != np.uint8 or lut.shape != (256, 3):
        raise PtxError("%s: a colour table must be uint8 [256, 3] (got %s %s)" % (who, lut.dtype, lut.shape))
    return np.ascontiguousarray(lut)


def cam_default_steps(T, Tm):
    """The map step every frame shows: floor(t * Tm / T), int32 [T]."""
    return (np.arange(T, dtype=np.int64) * int(Tm) // int(T)).astype(np.int32)


def _cam_steps(steps, T, Tm, who="CamOverlay"):
    if steps is None:
        return cam_default_steps(T, Tm)
    st = np.asarray(steps.cpu() if isinstance(steps, torch.Tensor) else steps)
    if st.shape != (T,) or st.dtype.kind not in "iu" or st.min() < 0 or st.max() >= Tm:
        raise PtxError("%s: steps must be %d integers in [0, %d) (got %r)" % (who, T, Tm, steps))
    return st.astype(np.int32)


def _cam_mode(out, who="CamOverlay"):
    if out not in CAM_OUT:
        raise PtxError("%s: out=%r is not one of %s" % (who, out, CAM_OUT))
    return CAM_OUT.index(out)


def _cam_alpha(alpha, who="CamOverlay"):
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0.0 <= float(alpha) <= 1.0:
        raise PtxError("%s: alpha must be a number in [0, 1] (got %r)" % (who, alpha))
    return float(alpha)


def cam_overlay_numpy(maps, frames, lut=None, alpha=0.4, steps=None, out="overlay"):
    """ptx_cam_overlay in numpy: maps uint8 [N, k, Tm, h, w], frames uint8 [N, T, H, W, 3] (out="heat" / "map": only their shape is
    read; a tuple (T, H, W) serves) -> uint8 [N, k, T, H, W, 3] ([N, k, T, H, W] for out="map").  Per frame t the map of step
    steps[t] (default `cam_default_steps`) is resized as Pillow resizes an "L" image with BILINEAR (`resize_axis_table` +
    `apply_tables_numpy`: horizontal pass, uint8 intermediate, vertical pass), coloured through `lut` (default `jet_colormap()`) and
    blended as `Image.blend(frame, heat, alpha)` blends (`color_blend_numpy(frame, heat, alpha)`)."""
    maps = np.asarray(maps)
    mode = _cam_mode(out, "cam_overlay_numpy")
    alpha = _cam_alpha(alpha, "cam_overlay_numpy")
    lut = _cam_colormap("jet" if lut is None else lut, "cam_overlay_numpy")
    if maps.dtype != np.uint8 or maps.ndim != 5:
        raise PtxError("cam_overlay_numpy: maps must be uint8 [N, k, Tm, h, w] (got %s %s)" % (maps.dtype, maps.shape))
    N, k, Tm, h, w = maps.shape
    if isinstance(frames, tuple):
        T, H, W = frames
        frames = None
    else:
        frames = np.asarray(frames)
        if frames.dtype != np.uint8 or frames.ndim != 5 or frames.shape[0] != N or frames.shape[4] != 3:
            raise PtxError("cam_overlay_numpy: frames must be uint8 [%d, T, H, W, 3] (got %s %s)" % (N, frames.dtype, frames.shape))
        T, H, W = frames.shape[1:4]
    if mode == _lib.PTX_CAM_OUT_OVERLAY and frames is None:
        raise PtxError("cam_overlay_numpy: out=\"overlay\" needs the frames")
    steps = _cam_steps(steps, T, Tm, "cam_overlay_numpy")
    tables = {"rows": resize_axis_table(h, H), "cols": resize_axis_table(w, W)}
    y = np.empty((N, k, T, H, W) + (() if mode == _lib.PTX_CAM_OUT_MAP else (3,)), np.uint8)
    for n in range(N):
        for j in range(k):
            big = {}
            for t in range(T):
                s = int(steps[t])
                if s not in big:
                    big[s] = apply_tables_numpy(maps[n, j, s][:, :, None], tables)[:, :, 0]
                if mode == _lib.PTX_CAM_OUT_MAP:
                    y[n, j, t] = big[s]
                elif mode == _lib.PTX_CAM_OUT_HEAT:
                    y[n, j, t] = lut[big[s]]
                else:
                    y[n, j, t] = color_blend_numpy(frames[n, t], lut[big[s]], alpha).astype(np.uint8)
    return y


def _cam_overlay_desc(N, k, Tm, h, w, T, H, W, taps_h, taps_w, mode, alpha):
    return _lib.CamOverlayDesc(N, k, Tm, h, w, T, H, W, taps_h, taps_w, mode, alpha)


def _cam_overlay_supported(desc, rows=None, cols=None, who="CamOverlay"):
    """The library's host-side check of an overlay launch (no device is touched), with its reason as a PtxError.  rows / cols: the
    host tables, whose coefficients are then checked too."""
    rk = None if rows is None else np.ascontiguousarray(rows[2], dtype=np.int32)
    ck = None if cols is None else np.ascontiguousarray(cols[2], dtype=np.int32)
    if not _lib.lib().ptx_cam_overlay_supported(C.byref(desc), C.c_void_p(None if rk is None else rk.ctypes.data),
                                                C.c_void_p(None if ck is None else ck.ctypes.data)):
        raise PtxError("%s: %s" % (who, _lib.lib().ptx_last_error().decode(errors="replace")))


class CamOverlay:
    """Draws class activation maps over the frames they explain, on the device, equal to Pillow bit for bit:
    `Image.blend(frame, Image.fromarray(lut[np.asarray(Image.fromarray(map, "L").resize((W, H), BILINEAR))]), alpha)` per frame,
    in one launch per batch (`ptx_cam_overlay`; `cam_overlay_numpy` is its numpy statement).
    alpha: the weight of the heat image, 0 .. 1.  colormap: "jet" (`jet_colormap`) or any uint8 [256, 3] table.
    out: "overlay" (the blend), "heat" (the coloured map alone; the frames give the size only) or "map" (the resized map, one byte
    per pixel).  Called as `(frames_u8, maps_u8, steps=None)`:
      frames uint8 CUDA [N, T, H, W, 3], maps uint8 CUDA [N, k, T', h, w]  ->  uint8 [N, k, T, H, W, 3]  ("map": [N, k, T, H, W]);
      frames [N, H, W, 3],               maps [N, k, h, w] (the 2-D nets)  ->  uint8 [N, k, H, W, 3]     ("map": [N, k, H, W]).
    steps: which map step every frame shows, T integers (default floor(t * T' / T)).  The tables are built once per
    (h, w, H, W) and kept on the device.  `model.cam_frames(..)` returns both arguments: `ov(r.frames, r.maps)`."""
    CACHE_SIZE = 8
    LIMIT_BYTES = (1 << 31) - 1

    def __init__(self, alpha=0.4, colormap="jet", out="overlay"):
        self.alpha = _cam_alpha(alpha)
        self.out = out
        self.mode = _cam_mode(out)
        self.lut = _cam_colormap(colormap)
        self._cache = collections.OrderedDict()
        self._luts = {}

    def tables(self, h, w, H, W):
        """Host tables of the map's resize, in build_tables' form: `rows` for h -> H and `cols` for w -> W."""
        return {"rows": resize_axis_table(h, H), "cols": resize_axis_table(w, W)}

    def _device_tables(self, h, w, H, W, device):
        key = (h, w, H, W, str(device))
        hit = self._cache.get(key)
        if hit is not None:
            self._cache.move_to_end(key)
            return hit
        t = self.tables(h, w, H, W)
        _cam_overlay_supported(_cam_overlay_desc(1, 1, 1, h, w, 1, H, W, t["rows"][2].shape[1], t["cols"][2].shape[1], self.mode,
                                                 self.alpha), t["rows"], t["cols"])
        parts = [a.reshape(-1) for a in t["rows"] + t["cols"]]
        offs = np.cumsum([0] + [p.size for p in parts])
        buf = torch.from_numpy(np.concatenate(parts).astype(np.int32)).to(device)         # one small upload per geometry
        hit = (buf, [int(o) * 4 for o in offs[:-1]], t["rows"][2].shape[1], t["cols"][2].shape[1])
        self._cache[key] = hit
        while len(self._cache) > self.CACHE_SIZE:
            self._cache.popitem(last=False)
        return hit

    def _device_lut(self, device):
        hit = self._luts.get(str(device))
        if hit is None:
            hit = self._luts[str(device)] = torch.from_numpy(self.lut).to(device)
        return hit

    def __call__(self, frames, maps, steps=None):
        for name, t in (("frames", frames), ("maps", maps)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
                raise PtxError("CamOverlay: %s must be a uint8 CUDA tensor (no CPU fallback; cam_overlay_numpy states the result)" % name)
        if frames.device != maps.device:
            raise PtxError("CamOverlay: frames on %s but maps on %s" % (frames.device, maps.device))
        flat = maps.dim() == 4 and frames.dim() == 4                                     # the 2-D nets: one frame, one step
        if flat:
            frames, maps = frames.unsqueeze(1), maps.unsqueeze(2)
        if maps.dim() != 5 or frames.dim() != 5 or frames.shape[4] != 3 or frames.shape[0] != maps.shape[0]:
            raise PtxError("CamOverlay: expected frames [N,T,H,W,3] with maps [N,k,T',h,w], or frames [N,H,W,3] with maps [N,k,h,w] "
                           "(got %s and %s)" % (tuple(frames.shape), tuple(maps.shape)))
        frames, maps = frames.contiguous(), maps.contiguous()
        N, k, Tm, h, w = maps.shape
        T, H, W = frames.shape[1:4]
        st = _cam_steps(steps, T, Tm)
        dev = frames.device
        bpp = 1 if self.mode == _lib.PTX_CAM_OUT_MAP else 3
        with torch.cuda.device(dev):
            buf, offs, taps_h, taps_w = self._device_tables(h, w, H, W, dev)
            lut = self._device_lut(dev)
            step = torch.from_numpy(st).to(dev)
            y = torch.empty((N, k, T, H, W) + ((3,) if bpp == 3 else ()), device=dev, dtype=torch.uint8)
            per_map = T * H * W * bpp
            fit = self.LIMIT_BYTES // per_map                                             # maps of one launch
            if fit < 1:
                raise PtxError("CamOverlay: one map over %d frames of %dx%d exceeds the 2 GiB per-launch limit" % (T, H, W))
            base = buf.data_ptr()
            tabs = [C.c_void_p(base + o) for o in offs]
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            # ranges of (n, j): whole clips while k maps fit a launch, else runs of one clip's classes
            if fit >= k:
                ranges = [(n0, min(n0 + fit // k, N), 0, k) for n0 in range(0, N, fit // k)]
            else:
                ranges = [(n, n + 1, j0, min(j0 + fit, k)) for n in range(N) for j0 in range(0, k, fit)]
            for n0, n1, j0, j1 in ranges:
                desc = _cam_overlay_desc(n1 - n0, j1 - j0, Tm, h, w, T, H, W, taps_h, taps_w, self.mode, self.alpha)
                _cam_overlay_supported(desc)
                check(_lib.lib().ptx_cam_overlay(C.byref(desc), C.c_void_p(maps[n0, j0].data_ptr()), C.c_void_p(frames[n0].data_ptr()),
                                                 C.c_void_p(lut.data_ptr()), *tabs, C.c_void_p(step.data_ptr()),
                                                 C.c_void_p(y[n0, j0].data_ptr()), stream), "ptx_cam_overlay")
        return y[:, :, 0] if flat else y
