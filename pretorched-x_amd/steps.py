"""What a plan is made of: activations, packed filters and the launch records ("steps") a plan runs in order.

A step is a callable taking the HIP stream; everything else of its launch -- descriptor, device pointers, tile
configuration, split-K factor -- was frozen when the plan was compiled (plan.py).  Every step class sets all of its slots
in __init__, so the code that reads them (the tuner, the profiler, bench.py's per-launch rows) uses plain attribute reads.
"""
import contextlib
import ctypes as C
import os
import re
import warnings

import torch
import torch.nn as nn

from . import _lib
from ._lib import (PackDesc, PTX_BF16_OPERANDS, PTX_PACK_BF16, PtxError, check)


def _r4(v):
    return (v + 3) // 4 * 4


def _stem_ld():
    """Row length (floats) of the kW-folded stem operand: 24 = 96-byte rows for the register-staged BK = 24 tiles,
    32 = 128-byte rows, which the conflict-free LDS-DMA K22 tile can stage (the fold writes 33 % more)."""
    return 32 if os.environ.get("PTX_STEM_LD", "24") == "32" else 24


def _r8(v):
    return (v + 7) // 8 * 8


def _r128(v):
    return (v + 127) // 128 * 128


def _device_ctx(dev):
    """torch.cuda.device(dev) for real devices; a no-op for the 'meta' device used by dry-run
    plan compilation (host-logic tests without a GPU)."""
    return torch.cuda.device(dev) if torch.device(dev).type == "cuda" else contextlib.nullcontext()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, offset_elems=0):
    return C.c_void_p(t.data_ptr() + 4 * offset_elems)


def _dense16(x):
    """Contiguous and 16-byte aligned: the kernels read the caller's tensor in 16-byte pieces (a contiguous view whose storage
    offset is not a multiple of 4 floats gets one aligned copy)."""
    x = x.contiguous()
    return x.clone() if x.data_ptr() % 16 else x


def _geom(conv):
    """(kernel, stride, padding) as (T,H,W) triples for Conv3d, or Conv2d seen as T == 1."""
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    if isinstance(conv, nn.Conv2d):
        return (1,) + tuple(k), (1,) + tuple(s), (0,) + tuple(p)
    if isinstance(conv, nn.Conv1d):
        return (1, 1) + tuple(k), (1, 1) + tuple(s), (0, 0) + tuple(p)
    return tuple(k), tuple(s), tuple(p)


def _tag(step, label, nbytes=0, macs=0):
    """Measurement metadata of a non-conv plan step: the ALGORITHMIC HBM bytes (compulsory reads + writes) or MACs of
    one launch -- what Engine.profile_steps / bench.py's `roofline_hbm` divide the HIP-event time into."""
    step.label, step.hbm_bytes, step.macs = label, int(nbytes), int(macs)
    return step


class RawInput:
    """Shape of the user's NCDHW (or NCHW, T == 1) input; its pointer is bound at run time."""
    __slots__ = ("N", "C", "T", "H", "W", "t_step", "T_full", "norm")

    def __init__(self, N, C_, T, H, W, t_step=1, T_full=None, norm=None):
        self.N, self.C, self.T, self.H, self.W = N, C_, T, H, W
        self.t_step = int(t_step)                       # every t_step-th frame of a T_full-frame clip
        self.T_full = T if T_full is None else T_full
        self.norm = norm                                # NormDesc: the input is uint8 [N,T,H,W,C] frames


class Act:
    """A channels-last activation: tensor [N,T,H,W,ld], C valid channels."""
    __slots__ = ("t", "N", "T", "H", "W", "C", "ld", "f16", "bf16")

    def __init__(self, dev, N, T, H, W, C_, ld=None, f16=False, bf16=False):
        self.N, self.T, self.H, self.W, self.C = N, T, H, W, C_
        self.f16 = bool(f16 or bf16)   # 16-bit: the operand of an fp16-MFMA conv (row stride a multiple of 8 elements)
        self.bf16 = bool(bf16)         # ... and its bfloat16 flavour (bf16 plans)
        self.ld = ((C_ + 7) // 8 * 8 if self.f16 else _r4(C_)) if ld is None else ld
        dt = torch.bfloat16 if bf16 else torch.float16 if f16 else torch.float32
        self.t = torch.empty((N, T, H, W, self.ld), device=dev, dtype=dt)
        if self.ld != C_ and self.t.device.type != "meta":
            self.t.zero_()

    @property
    def S(self):
        return self.T * self.H * self.W

    def slice(self, c0, C_):
        """Channels [c0, c0 + C_) of this activation as an output target: same row stride, so a conv /
        pool writing it fills its part of a channel concatenation (torch.cat(dim=1)) in place."""
        assert c0 % 4 == 0 and c0 + C_ <= self.ld
        # bf16 slices start on an 8-channel (16-byte) boundary; fp16 activations are never sliced
        assert not self.f16 or (self.bf16 and c0 % 8 == 0), "channel slices are fp32 / 16-byte aligned bf16 only"
        v = Act.__new__(Act)
        v.f16 = v.bf16 = self.bf16
        v.N, v.T, v.H, v.W, v.C, v.ld = self.N, self.T, self.H, self.W, C_, self.ld
        v.t = self.t[..., c0:c0 + C_]
        return v


def _t3(v):
    return (int(v),) * 3 if isinstance(v, int) else tuple(int(i) for i in v)


def _same_geometry(dims, k, s):
    """TF-"SAME" output extents and FRONT pads (the back pad is total - front; zeros either way)."""
    out = tuple(-(-i // st) for i, st in zip(dims, s))
    front = tuple(max((o - 1) * st + kk - i, 0) // 2 for o, st, kk, i in zip(out, s, k, dims))
    return out, front



class _Ref:
    """A module of the model tree by qualified name.  Plans outlive the module OBJECTS they were compiled
    from: torch.nn.DataParallel builds fresh replicas (new module objects, new broadcast copies of the
    parameters) on every forward (reference examples/imagenet_eval.py:136), so everything a plan needs from
    the model later -- weights to re-pack, the classifier head -- is re-resolved by name on the model that is
    executing.  Modules outside the tree (never the case for zoo models) are held directly."""
    __slots__ = ("name", "obj")

    def __init__(self, name, obj=None):
        self.name, self.obj = name, obj


class Packed:
    """BN-folded, K-major filter + bias living on one device; refreshable in place."""

    def __init__(self, plan, convs, bn, fold_kw=False, scale=None, f16=False, x3=None, stem4=False, fold_hw=False, pad8=False):
        dev = plan.dev
        # pad8: each of several Co-concatenated filters starts on an 8-row boundary, zero filter rows / bias in between
        # (the bf16 non-local theta|phi|g projection: every slice of its output is 16-byte aligned, its pad channels zero)
        self.pad8 = bool(pad8)
        self.stem4 = bool(stem4)     # direct split-operand stem (ptx_conv_stem_x3_fwd): Cin zero-padded to 4, kW folded
        self.plan = plan
        # bf16 plans: every filter is stored as bf16 (ptx_pack_desc.f16 == 3) for a bf16-operand conv
        self.bf16 = bool(plan.bf16)
        self.f16 = bool(f16) or self.bf16   # filter stored as 16-bit values for a 16-bit-operand conv
        # bf16 stem: the (kh, kw) taps folded into the channel axis (ptx_im2col_hw_bf16), a (kT, 1, 1) conv over kH*kW*Cin
        self.fold_hw = bool(fold_hw)
        # split operands (Engine.precision == "x3"): every dense fp32 filter is packed as (hi8 | lo8) half blocks
        convs = list(convs)          # >1: concatenated along Co (non-local g/theta/phi)
        self.convs = [plan.ref(c) for c in convs]
        self.bn = plan.ref(bn) if bn is not None else None
        # scalar Parameter multiplying the filter (self-attention gamma): (owning module, attribute name)
        self.scale = (plan.ref(scale[0]), scale[1]) if scale is not None else None
        c0 = convs[0]
        (kT, kH, kW), _, _ = _geom(c0)
        self.Co = sum(_r8(c.out_channels) if self.pad8 else c.out_channels for c in convs)
        self.groups = int(getattr(c0, "groups", 1))
        if self.groups > 1 and (len(convs) > 1 or fold_kw):
            raise PtxError("grouped convolutions are packed one at a time, unfolded")
        self.Ci = c0.in_channels // self.groups      # K extent of one filter row (per group)
        if self.fold_hw:
            self.Ci = c0.in_channels * kH * kW
            kH = kW = 1
        self.real_ci = self.Ci
        if self.stem4:
            self.Ci = 4
        self.sub_groups = 0
        cog = c0.out_channels // self.groups
        SUPER = 32      # narrow groups (width 4/8/16, resnext3D.py:85-92) are packed as block-diagonal 32-wide
        if (self.groups > 1 and self.Ci == cog and self.Ci < SUPER and SUPER % self.Ci == 0
                and c0.in_channels % SUPER == 0 and os.environ.get("PTX_SUPERGROUP", "1") != "0"):
            # super-groups: the MFMA tiles then run them (8x / 4x / 2x padded work, but coalesced operands)
            self.sub_groups = SUPER // self.Ci
            self.groups //= self.sub_groups
            self.Ci = SUPER
        self.fold_kw = bool(fold_kw)
        # narrow outputs (Co <= 32: SlowFast's fast pathway, lateral convs) keep the fp32 narrow / direct tiles -- there is no
        # 16-wide split-operand tile, and a 64-wide one would spend 4-8x padded work on them
        self.x3 = (bool(plan.x3 if x3 is None else x3) and not self.f16 and self.groups == 1
                   and (self.Co > 32 or stem4))
        keff = kW * self.Ci if fold_kw else self.Ci
        self.Kc = (keff + 7) // 8 * 8 if (self.f16 or self.x3) else _r4(keff)
        if self.f16 and (fold_kw or self.groups > 1 or (self.Ci % 2 and not self.bf16)):
            raise PtxError("fp16 filters: dense, unfolded convs with an even channel count only")
        if self.fold_hw:
            self.Kc = (self.Ci + 31) // 32 * 32      # whole 32-channel (16-word) chunks of the BK = 16 stem tiles
        if fold_kw:
            self.Kc = max(self.Kc, 32 if self.x3 else _stem_ld()) if keff <= 24 else self.Kc
        if self.stem4:
            self.Kc = 32
        self.Co_pad = _r128(self.Co)
        self.k_eff = (kT, kH, 1) if fold_kw else (kT, kH, kW)
        self.d = PackDesc(self.Co, self.Ci, kT, kH, kW, self.Kc, self.Co_pad, int(fold_kw), 0, 0, 0,
                          self.sub_groups, self.Ci if self.sub_groups else 0,
                          PTX_PACK_BF16 if self.bf16 else 2 if self.x3 else int(self.f16))
        n = _lib.lib().ptx_packed_weight_elems(C.byref(self.d))
        self.w = torch.empty(n, device=dev, dtype=torch.bfloat16 if self.bf16 else torch.float16 if self.f16 else torch.float32)
        self.b = torch.empty(self.Co_pad, device=dev, dtype=torch.float32)

    def refresh(self):
        get = self.plan.get
        convs, bn = [get(c) for c in self.convs], (get(self.bn) if self.bn is not None else None)
        if len(convs) == 1 and hasattr(convs[0], "effective_weight_bias"):
            w, cb = convs[0].effective_weight_bias()      # MultiViewConv: three views of one 2-D bank as a dense filter
        elif len(convs) == 1:
            w = convs[0].weight.detach()
            cb = convs[0].bias.detach() if convs[0].bias is not None else None
        elif self.pad8:
            def rows8(t):
                return torch.cat([t, t.new_zeros((_r8(t.shape[0]) - t.shape[0],) + tuple(t.shape[1:]))], 0)
            w = torch.cat([rows8(c.weight.detach()) for c in convs], 0)
            cb = torch.cat([rows8(c.bias.detach()) for c in convs], 0) if convs[0].bias is not None else None
        else:
            w = torch.cat([c.weight.detach() for c in convs], 0)
            cb = torch.cat([c.bias.detach() for c in convs], 0) if convs[0].bias is not None else None
        if self.stem4 and w.shape[1] < 4:             # zero channel(s) up to the 16-byte position the stem kernel reads
            w = torch.cat([w, w.new_zeros((w.shape[0], 4 - w.shape[1]) + tuple(w.shape[2:]))], 1)
        if self.bf16:
            # bf16 plans: the BN fold runs in fp32 on the exactly upcast bf16 parameters and buffers; the folded filter
            # is rounded to bf16 once, by the pack kernel
            if w.dtype != torch.bfloat16 or not w.is_cuda:
                raise PtxError("weights of a bf16 model must be bf16 CUDA tensors on the plan's device (got %s)" % w.dtype)
            if self.fold_hw:          # [Co][Cin][kT][kH][kW] -> [Co][(kh*kW + kw)*Cin + c][kT][1][1] (ptx_im2col_hw_bf16's order)
                if w.dim() == 4:      # a 2-D ResNet's Conv2d stem: kT = 1
                    w = w.unsqueeze(2)
                co, ci, kt, kh, kw = w.shape
                w = w.permute(0, 3, 4, 1, 2).reshape(co, kh * kw * ci, kt, 1, 1)
            w = w.float()
            cb = cb.float() if cb is not None else None
        w = w.contiguous()
        if w.dtype != torch.float32 or not w.is_cuda:
            raise PtxError("weights must be fp32 CUDA tensors on the plan's device")
        null = C.c_void_p(0)
        args = [null] * 4
        eps = 0.0
        keep = [w, cb]
        if bn is not None:
            ts = [bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var]
            ts = [t.float().contiguous() if self.bf16 else t.contiguous() for t in ts]
            keep += ts
            args = [_ptr(t) for t in ts]
            eps = float(bn.eps)
        elif self.scale is not None:     # w * gamma through the BN-fold path: gamma / sqrt(1 + 0), beta = mean = 0
            one = torch.ones(self.Co, device=w.device, dtype=torch.float32)
            gamma = getattr(get(self.scale[0]), self.scale[1])
            ts = [one * gamma.detach().reshape(()), torch.zeros_like(one), torch.zeros_like(one), one]
            keep += ts
            args = [_ptr(t) for t in ts]
        check(_lib.lib().ptx_pack_conv_weight(C.byref(self.d), _ptr(w), _ptr(cb) if cb is not None else null,
                                              args[0], args[1], args[2], args[3], C.c_float(eps),
                                              _ptr(self.w), _ptr(self.b), _stream()), "ptx_pack_conv_weight")
        return keep


class _ConcatRowsPack(Packed):
    """bf16 'concatenation' mode: the filter of one 1x1x1 conv producing the affinity rows (a_i, 1, 0, ..) ("a", from
    theta: row 0 = concat_project's theta half, bias (proj bias, 1, 0, ..)) or (1, b_j, 0, ..) ("b", from phi: row 1 = its
    phi half, bias (1, 0, ..)), Co = 8 with explicit zero rows; rebuilt from concat_project on every refresh, as the fp32
    path rebuilds its GEMV weights."""

    def __init__(self, plan, nl, ci, side):
        shape = nn.Conv3d(ci, 8, 1, bias=True, device="meta")       # geometry only: the rows come from concat_project
        super().__init__(plan, [shape], None)
        self.proj, self.side, self.ci = plan.ref(nl.concat_project[0]), side, ci

    def refresh(self):
        proj = self.plan.get(self.proj)
        w = proj.weight.detach().reshape(-1)                         # [2 ci]: theta half | phi half
        if w.dtype != torch.bfloat16 or not w.is_cuda:
            raise PtxError("weights of a bf16 model must be bf16 CUDA tensors on the plan's device (got %s)" % w.dtype)
        ci = self.ci
        wf = torch.zeros((8, ci, 1, 1, 1), device=w.device, dtype=torch.float32)
        bf = torch.zeros(8, device=w.device, dtype=torch.float32)
        if self.side == "a":
            wf[0].view(-1).copy_(w[:ci])
            bf[1] = 1.0
            if proj.bias is not None:
                bf[0:1].copy_(proj.bias.detach().reshape(1))
        else:
            wf[1].view(-1).copy_(w[ci:])
            bf[0] = 1.0
        null = C.c_void_p(0)
        check(_lib.lib().ptx_pack_conv_weight(C.byref(self.d), _ptr(wf), _ptr(bf), null, null, null, null, C.c_float(0.0),
                                              _ptr(self.w), _ptr(self.b), _stream()), "ptx_pack_conv_weight (concat rows)")
        return [wf, bf]


class PackedDual:
    """K-concatenated filter of a bottleneck's last 1x1x1 conv (+BN) and its shortcut-B conv (+BN):
    rows [Kc | Kc2], summed biases -- the operand of ptx_conv3d_dual_fwd."""

    def __init__(self, plan, conv, bn, conv2, bn2):
        dev = plan.dev
        self.plan = plan
        self.parts = [(plan.ref(conv), plan.ref(bn)), (plan.ref(conv2), plan.ref(bn2))]
        self.Co, self.Ci, self.Ci2 = conv.out_channels, conv.in_channels, conv2.in_channels
        assert conv2.out_channels == self.Co
        self.x3 = bool(plan.x3)
        rk = _r8 if self.x3 else _r4
        self.f16 = self.bf16 = self.fold_kw = False      # (what Plan.conv reads on any filter: fp32 / x3, dense, unfolded)
        self.groups, self.real_ci = 1, self.Ci
        self.Kc, self.Kc2 = rk(self.Ci), rk(self.Ci2)
        self.Co_pad = _r128(self.Co)
        self.k_eff = (1, 1, 1)
        ld = self.Kc + self.Kc2
        sp = 2 if self.x3 else 0
        self.descs = [PackDesc(self.Co, self.Ci, 1, 1, 1, self.Kc, self.Co_pad, 0, ld, 0, 0, 0, 0, sp),
                      PackDesc(self.Co, self.Ci2, 1, 1, 1, self.Kc2, self.Co_pad, 0, ld, self.Kc, 1, 0, 0, sp)]
        self.d = self.descs[0]
        self.w = torch.zeros(self.Co_pad * ld, device=dev, dtype=torch.float32)
        self.b = torch.empty(self.Co_pad, device=dev, dtype=torch.float32)

    def refresh(self):
        null = C.c_void_p(0)
        for d, (conv, bn) in zip(self.descs, self.parts):
            conv, bn = self.plan.get(conv), self.plan.get(bn)
            w = conv.weight.detach().contiguous()
            cb = conv.bias.detach().contiguous() if conv.bias is not None else None
            ts = [t.contiguous() for t in (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var)]
            check(_lib.lib().ptx_pack_conv_weight(C.byref(d), _ptr(w), _ptr(cb) if cb is not None else null,
                                                  _ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), _ptr(ts[3]),
                                                  C.c_float(float(bn.eps)), _ptr(self.w), _ptr(self.b), _stream()),
                  "ptx_pack_conv_weight (dual)")


class PackedDw:
    """BN-folded filter of a depthwise conv (groups == in_channels == out_channels), tap-major [kT*kH*kW][C], + fp32 bias: the
    operands of ptx_conv3d_dw_f32_fwd (include/ptx_amd_dw.h); refreshable in place like `Packed`.  Always fp32 -- the launch has
    nothing for the matrix cores, so a split-operand ("x3") plan packs it the same way."""

    def __init__(self, plan, conv, bn):
        self.plan = plan
        self.convs, self.bn = [plan.ref(conv)], (plan.ref(bn) if bn is not None else None)
        self.x3 = False                    # (what readers of plan.packs ask of every pack)
        self.C = conv.out_channels
        self.k_eff = _geom(conv)[0]
        if self.C % 4:
            raise PtxError("depthwise conv: %d channels -- the kernel takes multiples of 4" % self.C)
        taps = self.k_eff[0] * self.k_eff[1] * self.k_eff[2]
        self.w = torch.empty(taps * self.C, device=plan.dev, dtype=torch.float32)
        self.b = torch.empty(self.C, device=plan.dev, dtype=torch.float32)

    def refresh(self):
        get = self.plan.get
        conv, bn = get(self.convs[0]), (get(self.bn) if self.bn is not None else None)
        w = conv.weight.detach().contiguous()
        cb = conv.bias.detach().contiguous() if conv.bias is not None else None
        if w.dtype != torch.float32 or not w.is_cuda:
            raise PtxError("weights must be fp32 CUDA tensors on the plan's device")
        null = C.c_void_p(0)
        args, eps, keep = [null] * 4, 0.0, [w, cb]
        if bn is not None:
            ts = [t.contiguous() for t in (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var)]
            keep += ts
            args, eps = [_ptr(t) for t in ts], float(bn.eps)
        kT, kH, kW = self.k_eff
        check(_lib.lib().ptx_pack_dw_weight_f32(self.C, kT, kH, kW, _ptr(w), _ptr(cb) if cb is not None else null, args[0], args[1],
                                                args[2], args[3], C.c_float(eps), _ptr(self.w), _ptr(self.b), _stream()),
              "ptx_pack_dw_weight_f32")
        return keep


def _tile_dims(name):
    """(BM, BN, BK) of an MFMA tile configuration name ("32x64x64/2x2/m16/dma/re"), or None for the direct (VALU) tiles."""
    m = re.match(r"^(\d+)x(\d+)x(\d+)/", name)
    return None if (m is None or "direct" in name) else tuple(int(v) for v in m.groups())


def issued_conv_flop(d, tile, words=1):
    """FLOP of the MFMA instructions one implicit-GEMM launch ISSUES (what SQ_INSTS_MFMA counts), as opposed to the
    algorithmic 2 x MACs that price every padding tap as work: per M tile the kernel walks the (kt, kh)
    planes that are inside the image for AT LEAST ONE of its rows (conv_igemm_kernel.h "block-uniform tap pruning": the
    contiguous span kt_lo..kt_hi x kh_lo..kh_hi), every kw, every BK-wide channel chunk, on full BM x BN x BK tiles
    (row / column / K padding of edge tiles included).  Host-side twin of the kernel's own loop bounds."""
    import numpy as np
    BM, BN, BK = tile
    M = d.N * d.To * d.Ho * d.Wo
    ncol = _r4(d.Co)
    n_tiles = -(-ncol // BN)
    # a grouped conv walks its own group's input columns only (Kc per tap), not the whole row
    kch = -(-(d.Kc if d.groups > 1 else max(d.ldx, d.Kc)) // BK)
    if d.x2_C > 0 and d.x2_ld > 0:
        kch = -(-d.ldx // BK) + -(-d.x2_ld // BK)
    m = np.arange(M, dtype=np.int64)
    t = m // d.Wo
    ho = t % d.Ho
    to = (t // d.Ho) % d.To

    def span(c, pad, k, extent):
        lo = np.maximum(0, pad - c)
        hi = np.minimum(k - 1, extent - 1 + pad - c)
        return lo, hi
    edges = np.arange(0, M, BM)
    steps = np.ones(len(edges), dtype=np.int64)
    for (c, pad, k, ext) in ((to * d.sT, d.pT, d.kT, d.Ti), (ho * d.sH, d.pH, d.kH, d.Hi)):
        lo, hi = span(c, pad, k, ext)
        ok = hi >= lo
        lo_t = np.minimum.reduceat(np.where(ok, lo, k), edges)
        hi_t = np.maximum.reduceat(np.where(ok, hi, -1), edges)
        steps *= np.maximum(hi_t - lo_t + 1, 0)
    return float(steps.sum()) * d.kW * kch * n_tiles * 2.0 * BM * BN * BK * words


class _Step:
    """Base of the launch records: a new step has every slot set -- to the class's `_defaults` entry, else None -- and the
    plan compiler fills in the rest, so readers never probe for a missing attribute."""
    __slots__ = ()
    _defaults = {}

    def __init__(self):
        for name in self.__slots__:
            setattr(self, name, self._defaults.get(name))


class ConvStep(_Step):
    """One ptx_conv3d_fwd (or, with a second source, ptx_conv3d_dual_fwd) launch with everything but
    the stream frozen."""
    __slots__ = ("d", "x", "x2", "w", "b", "res", "y", "cfg", "split", "plan", "label", "macs", "ext", "fused", "from_table",
                 "body", "body_w", "body_ok")
    _defaults = {"split": 1, "fused": False, "from_table": False, "body_ok": ()}

    @property
    def kernel(self):
        """Name the launch goes by in the per-launch rows: the tile configuration, or the body kernel."""
        if self.body is not None:
            return "conv_tstack_f32" if self.d.kH == 1 else "conv_body_f32"
        return _lib.lib().ptx_conv3d_config_name(self.cfg).decode()

    def issued_flop(self):
        if self.body is not None:
            # the body kernel walks only the temporal taps inside the clip, on full 32-row x 64-column x 16-channel blocks
            d = self.d
            frames = sum(max(0, min(d.kT - 1, d.Ti - 1 - (t - d.pT)) - max(0, d.pT - t) + 1) for t in range(d.To))
            rows = -(-(d.Ho * d.Wo) // 32) * 32
            if d.kH == 1:        # the T-stacked tile: 16-channel chunks, (frame, tap) pairs outside the clip are skipped
                return 2.0 * d.N * frames * rows * (-(-d.Ci // 16) * 16) * (-(-_r4(d.Co) // 64) * 64)
            return 2.0 * d.N * frames * rows * 9 * d.Ci * (-(-_r4(d.Co) // 64) * 64)
        tile = _tile_dims(_lib.lib().ptx_conv3d_config_name(self.cfg).decode())
        # bf16 descriptors count 32-bit words (two channels) along K
        words = 2 if self.d.flags & PTX_BF16_OPERANDS else 1
        return 2.0 * self.macs if tile is None else issued_conv_flop(self.d, tile, words)

    def __call__(self, st):
        try:
            self._launch(st)
        except PtxError as e:
            # a tile taken from the tuned table that this build / this problem cannot run (a stale or hand-edited
            # entry): fall back to the library's own default once, loudly, instead of failing the forward.  Only a
            # REFUSAL qualifies (PTX_ERR_INVALID / PTX_ERR_UNSUPPORTED / PTX_ERR_WORKSPACE: nothing was launched); HIP
            # launch or asynchronous device errors are genuine faults and propagate.
            if not self.from_table or e.status not in (1, 2, 4):
                raise
            sk = C.c_int(1)
            self.cfg = self.plan.lib.ptx_conv3d_pick_config(C.byref(self.d), C.byref(sk))
            self.split, self.from_table = sk.value, False
            p = self.plan
            need = int(p.lib.ptx_conv3d_workspace_bytes(C.byref(self.d), self.split))
            if need > p.ws_bytes:           # the workspace was sized for the tuned split: grow it for the default one
                p.ws = torch.zeros(need // 4, device=p.dev, dtype=torch.float32)
                p.ws_bytes, p.ws_ptr = need, _ptr(p.ws)
            warnings.warn("pretorched-x_amd: tuned tile for %s rejected by the library (%s); using the default tile" % (self.label, e))
            self._launch(st)

    def _launch(self, st):
        p = self.plan
        if self.body is not None:      # 3x3x3 body conv on its own patch-resident kernel (conv_body_f32.hip)
            check(_lib.lib().ptx_conv_body_f32_fwd(C.byref(self.d), self.x, self.body_w, self.b, self.res, self.y, self.body, st), self.label)
            return
        if self.fused:        # fp16 generator stage: per-sample affine / halfs out / dual output / upsampling loader
            check(_lib.lib().ptx_conv3d_fused_fwd(C.byref(self.d), self.x, self.w, self.b, self.res, self.y,
                                                  C.byref(self.ext) if self.ext is not None else None,
                                                  p.ws_ptr, p.ws_bytes, self.cfg, self.split, st), self.label)
        elif self.x2 is not None:
            check(_lib.lib().ptx_conv3d_dual_fwd(C.byref(self.d), self.x, self.x2, self.w, self.b, self.y,
                                                 p.ws_ptr, p.ws_bytes, self.cfg, self.split, st), self.label)
        else:
            check(_lib.lib().ptx_conv3d_fwd(C.byref(self.d), self.x, self.w, self.b, self.res, self.y,
                                            p.ws_ptr, p.ws_bytes, self.cfg, self.split, st), self.label)


class DwConvStep(_Step):
    """One ptx_conv3d_dw_f32_fwd launch (include/ptx_amd_dw.h): a depthwise conv + folded BN (+ ReLU).  A plain streaming launch:
    no tile, no split, no workspace -- it is not part of Plan.conv_steps, so the tuner, the Winograd forms and the body-kernel
    selection never see it; `macs` / `hbm_bytes` (compulsory reads + writes) feed the per-launch rows like a tagged closure's."""
    __slots__ = ("d", "x", "w", "b", "y", "label", "macs", "hbm_bytes")
    kernel = "conv_dw_f32"

    def __call__(self, st):
        check(_lib.lib().ptx_conv3d_dw_f32_fwd(C.byref(self.d), self.x, self.w, self.b, self.y, st), self.label)


class ChainStep(_Step):
    """One ptx_conv3d_chain_fwd launch: conv -> BN -> ReLU -> 1x1x1 conv -> BN (-> + residual) -> ReLU, the intermediate
    tile kept in LDS (conv_chain.hip)."""
    __slots__ = ("d", "d2", "x", "w", "b", "w2", "b2", "res", "y", "cfg", "plan", "label", "macs", "hbm_bytes", "key",
                 "body", "body_ok", "body_w", "body_w2")
    _defaults = {"hbm_bytes": 0, "body_ok": ()}

    @property
    def kernel(self):
        if self.body is not None:
            return "conv_body_chain_f32"
        return _lib.lib().ptx_conv3d_chain_config_name(self.cfg).decode()

    def issued_flop(self):
        if self.body is not None:
            d = self.d
            frames = sum(max(0, min(d.kT - 1, d.Ti - 1 - (t - d.pT)) - max(0, d.pT - t) + 1) for t in range(d.To))
            rows = -(-(d.Ho * d.Wo) // 32) * 32
            return 2.0 * d.N * rows * 64.0 * (frames * 9 * d.Ci + d.To * (-(-_r4(self.d2.Co) // 64) * 64))
        tile = _tile_dims(self.kernel)
        if tile is None:
            return 2.0 * self.macs
        BM, BN, BK = tile
        m_tiles = -(-(self.d.N * self.d.To * self.d.Ho * self.d.Wo) // BM)
        tail = m_tiles * -(-_r4(self.d2.Co) // BN) * -(-min(_r4(self.d.Co), BN) // BK) * 2.0 * BM * BN * BK
        return issued_conv_flop(self.d, tile) + tail

    def __call__(self, st):
        if self.body is not None:       # the patch-resident body kernel with its chained tail
            check(_lib.lib().ptx_conv_body_chain_f32_fwd(C.byref(self.d), C.byref(self.d2), self.x, self.body_w, self.b, self.body_w2,
                                                         self.b2, self.res, self.y, self.body, st), self.label)
            return
        check(_lib.lib().ptx_conv3d_chain_fwd(C.byref(self.d), C.byref(self.d2), self.x, self.w, self.b, self.w2, self.b2,
                                              self.res, self.y, self.cfg, st), self.label)


class AltStep(_Step):
    """A conv -> 1x1x1 conv pair with two compiled executions: ONE chained launch (ChainStep) or the two launches it
    replaces (ConvSteps through an intermediate tensor).  Which one runs is a tuning decision like the tile choice --
    measured per problem pair by Engine.autotune, remembered in the tuned table ("alt:" keys), and defaulted by the
    measured rule of thumb: chained up to 64 intermediate channels (round 3, MI355X: 64-plane bottleneck tails and the
    (2+1)D pairs through <= 64 mid channels gain 10-30 %, 128-wide intermediate tiles lose a few per cent)."""
    __slots__ = ("chain", "pair", "use_chain", "label", "key")

    def __call__(self, st):
        if self.use_chain:
            self.chain(st)
        else:
            for s in self.pair:
                s(st)

    def active(self):
        if self.use_chain:
            return [self.chain]
        return [t for s in self.pair for t in (s.active() if isinstance(s, _WinoExec) else [s])]


_WINO_SLOTS = ("direct", "wino", "gemm", "use_wino", "wino4", "gemm4", "use_wino4", "need_u4", "alt", "label", "key", "v_ptr", "m_ptr",
               "m4_ptr", "v_bytes", "v4_bytes", "arena_bytes")


class _WinoExec(_Step):
    """A stride-1 (kT,3,3) fp32 conv with up to three compiled executions, one of which runs (`active()`):
    `direct`  its ConvStep, on a tile or the body kernel -- the default;
    `wino`    Winograd F(2x2,3x3) as three launches: the input transform, the 16-group (kT,1,1) ConvStep `gemm` on the ordinary
              tiles, the output transform with the conv's bias / residual / ReLU (csrc/conv_wino_f32.hip); `use_wino`;
    `wino4`   Winograd F(4x4,3x3), the same three launches on 6x6 patches around the 36-group ConvStep `gemm4`; `use_wino4`,
              exclusive with `use_wino`.  Its filter U4 is allocated and packed only where the step can run (`need_u4`:
              Plan.wino4_weights -- a stored verdict, the forced mode, or the tuner about to time it).
    Which one runs is measured per problem by the tuner ("wino:" / "wino4:" keys); PTX_CONV_WINO=0 compiles no such step, =1
    runs F(2x2) wherever it exists, =4 F(4x4) wherever it exists.  `alt`: the AltStep whose pair this conv is the first launch
    of (a bottleneck's conv2 + conv3), or None: the Winograd forms then compete with the chained launch too, and winning it
    switches the AltStep to its pair.  V and M live in the plan's Winograd arena (bound once it is allocated)."""
    __slots__ = ()
    _defaults = {"use_wino": False, "use_wino4": False}

    def _steps(self):
        return self.wino4 if self.use_wino4 else self.wino if self.use_wino else self.direct

    def __call__(self, st):
        for s in self._steps():
            s(st)

    def active(self):
        return list(self._steps())


class WinoStep(_WinoExec):
    """A conv with the F(2x2) form (even H and W) -- and, by the wider rule, the F(4x4) form next to it."""
    __slots__ = _WINO_SLOTS


class Wino4Step(_WinoExec):
    """A conv only F(4x4) takes (odd H or W: partial tiles): `wino` and `gemm` are None, `use_wino` stays False."""
    __slots__ = _WINO_SLOTS



class ProgramStep(_Step):
    """A run of consecutive small-M ConvSteps as ONE persistent launch (ptx_conv_program_fwd, csrc/conv_program.hip): the
    tiles of all its convs on one queue, per-row-tile dependencies instead of kernel boundaries.  `convs` are the launches it
    stands for -- still complete ConvSteps, run instead when `use_program` is off (PTX_PROGRAM=0, or the tuner measured the
    launches faster).
    Numerical caveat: "bit-identical to the launches" holds for the SAME tile and split.  Under PTX_PROGRAM=auto
    the program runs the library's own tile / split picks while the fallback ConvSteps run the tuned table's, so which bits
    a forward produces depends on which side the tuner's 3 % timing rule picked on that machine (same 1e-5 class either
    way); and Engine._autotune retunes the member ConvSteps AFTER the image was built, so with PTX_PROGRAM_TILES=tuned the
    image keeps the pre-tune tiles until the plan is recompiled.  Experimental, off by default."""
    __slots__ = ("convs", "use_program", "label", "macs", "hbm_bytes", "info", "image", "ws", "wgs", "plan", "stages", "kernel", "key")

    def __call__(self, st):
        if self.use_program:
            check(_lib.lib().ptx_conv_program_fwd(C.byref(self.info), _ptr(self.image), _ptr(self.ws), self.wgs, st), self.label)
        else:
            for s in self.convs:
                s(st)

    def active(self):
        return [self] if self.use_program else list(self.convs)

    def issued_flop(self):
        # every stage runs a conv_igemm tile body: its own plan line names the tile
        buf = C.create_string_buffer(1 << 16)
        check(_lib.lib().ptx_conv_program_describe(self.stages, len(self.convs), buf, len(buf)), "conv program describe")
        tot = 0.0
        for c, line in zip(self.convs, buf.value.decode().splitlines()[1:]):
            tot += issued_conv_flop(c.d, _tile_dims(line.split()[3]))
        return tot

    def error(self):
        """Synchronise and read the program's error word: None, or (code, waiting stage, queue index, producer stage)."""
        code = (C.c_int32 * 4)()
        check(_lib.lib().ptx_conv_program_error(_ptr(self.ws), code, _stream()), self.label)
        return None if code[0] == 0 else tuple(code)


class StemStep(_Step):
    """One ptx_conv_stem_x3_fwd launch (split-operand stem read from 4-channel positions) -- or, `planar`, one
    ptx_conv_stem_x3p_fwd launch (the same stem read from six half planes per frame: 21 % fewer matrix instructions)."""
    __slots__ = ("d", "x", "w", "b", "y", "label", "macs", "hbm_bytes", "planar")
    _defaults = {"hbm_bytes": 0}
    kernel = "conv_stem_x3"

    def __call__(self, st):
        fn = _lib.lib().ptx_conv_stem_x3p_fwd if self.planar else _lib.lib().ptx_conv_stem_x3_fwd
        check(fn(C.byref(self.d), self.x, self.w, self.b, self.y, st), self.label)


class PatchConvStep(_Step):
    """One launch of a generator-stage kernel designed for the fp16 matrix cores (gen_stage_f16.hip) instead of the
    implicit-GEMM tiles: ptx_conv3x3_f16_fwd (a GBlock's 3x3 convs, one staged input patch per tile) or, with `res` set /
    kernel == "conv1x1_skip_f16", ptx_conv1x1_skip_f16_fwd (its closing 1x1 conv + skip + both outputs); the "_bf16"
    kernels are their bf16 builds (bf16 generator plans)."""
    __slots__ = ("d", "x", "w", "b", "y", "ext", "res", "kernel", "label", "macs", "hbm_bytes", "ext_in")
    _defaults = {"hbm_bytes": 0}
    ENTRY = {"conv1x1_pro_f16": "ptx_conv1x1_pro_f16_fwd", "conv3x3_f16": "ptx_conv3x3_f16_fwd",
             "conv3x3_bf16": "ptx_conv3x3_bf16_fwd", "conv1x1_skip_f16": "ptx_conv1x1_skip_f16_fwd",
             "conv1x1_skip_bf16": "ptx_conv1x1_skip_bf16_fwd"}

    def __call__(self, st):
        fn = getattr(_lib.lib(), self.ENTRY[self.kernel])
        ext = C.byref(self.ext) if self.ext is not None else None
        if self.kernel == "conv1x1_pro_f16":      # the affine applied to the input fragments precedes the filter
            check(fn(C.byref(self.d), self.x, C.byref(self.ext_in), self.w, self.b, self.y, ext, st), self.label)
        elif self.kernel.startswith("conv1x1_skip"):
            check(fn(C.byref(self.d), self.x, self.w, self.b, self.res, self.y, ext, st), self.label)
        else:
            check(fn(C.byref(self.d), self.x, self.w, self.b, self.y, ext, st), self.label)


# temporal fast-FIR schemes of the fp32 stem the tuner times under PTX_STEM_TFIR=auto (include/ptx_amd_tfir.h).  Scheme 3,
# F(4,7), is the fastest and the least accurate (1.8e-5 of the output scale against 1.9e-6): it runs only when forced.
TFIR_SCHEMES = (1, 2)


class StemF32Step(_Step):
    """The RGB stem on the fp32 matrix cores, read straight from the caller's NCDHW tensor (bound per run: plan.in_ptr) -- no
    fold, no layout pass.  One ptx_conv_stem_f32_fwd launch, the default -- or, where the stem is a 7-tap stride-1 FIR along
    time, `tfir[scheme]` = [temporal input transform, StemTfirStep]: fewer frame-convolutions on the same step loop
    (csrc/conv_stem_tfir_f32.hip).  `use_tfir`: 0 = direct, else the scheme that runs -- PTX_STEM_TFIR=1|2|3 forces one, else
    the tuner's "tfir:" verdict; without one the step is the direct launch.  `active()`: the launches that run."""
    __slots__ = ("d", "plan", "strides", "w", "b", "y", "label", "macs", "hbm_bytes", "src", "tfir", "use_tfir", "key")
    _defaults = {"hbm_bytes": 0, "use_tfir": 0}
    kernel = "conv_stem_f32"

    def issued_flop(self):
        """FLOP of the MFMAs one launch ISSUES (what SQ_INSTS_MFMA x 4096 counts): `macs` prices padding taps as work
        (SURVEY.md 8d), the kernel skips the temporal taps outside the clip; per workgroup and (kt, kh) step 4 waves x 44
        v_mfma_f32_32x32x2_f32 (K = 21 padded to 22, 64 channels per tile)."""
        d = self.d
        tiles = -(-(d.Ho * d.Wo) // 256) * -(-_r4(d.Co) // 64)
        steps = 0
        for to in range(d.To):
            t0 = to * d.sT - d.pT
            steps += max(0, min(d.kT - 1, d.Ti - 1 - t0) - max(0, -t0) + 1) * d.kH
        return float(d.N * tiles * steps * 4 * 44 * 4096)

    def active(self):
        return list(self.tfir[self.use_tfir]) if self.use_tfir else [self]

    def __call__(self, st):
        if self.use_tfir:
            for s in self.tfir[self.use_tfir]:
                s(st)
            return
        sn, sc, stt = self.strides
        # src: a plan-owned fp32 NCDHW buffer (normalised uint8 frames / pitch-padded rows) or None = the caller's tensor
        x = self.src if self.src is not None else self.plan.in_ptr
        check(_lib.lib().ptx_conv_stem_f32_fwd(C.byref(self.d), x, sn, sc, stt, self.w, self.b, self.y, st), self.label)


class StemTfirStep(_Step):
    """One ptx_conv_stem_tfir_f32_fwd launch: the stem's P frame-convolutions per group of m output frames, read from the
    transformed input V (the plan's Winograd arena, free while the stem runs) and folded into the m frames."""
    __slots__ = ("d", "scheme", "m", "P", "v", "w", "b", "y", "label", "macs", "hbm_bytes")
    _defaults = {"hbm_bytes": 0}
    kernel = "conv_stem_tfir_f32"

    def issued_flop(self):
        """FLOP of the MFMAs one launch issues: every group runs all P products (no pruning); per 128-output workgroup and
        (product, kh) step 4 waves x 22 v_mfma_f32_32x32x2_f32."""
        d = self.d
        tiles = -(-(d.Ho * d.Wo) // 128) * -(-_r4(d.Co) // 64)
        return float(d.N * tiles * -(-d.To // self.m) * self.P * d.kH * 4 * 22 * 4096)

    def __call__(self, st):
        check(_lib.lib().ptx_conv_stem_tfir_f32_fwd(C.byref(self.d), self.scheme, self.v, self.w, self.b, self.y, st), self.label)


def stem_bf16_tiles(d):
    """Tiles per output frame of ptx_conv_stem_bf16_fwd (host-side twin of stem_bf16_geom, csrc/conv_stem_bf16.hip): raster
    runs of 256 outputs while the full-width input patch fits 40 KiB of LDS, else segments of <= 256 outputs of one row."""
    nrows = min(d.Ho, (255 + d.Wo - 1) // d.Wo + 1)
    if ((nrows - 1) * d.sH + d.kH) * ((d.Wo - 1) * d.sW + 8) * 8 <= 40960:
        return -(-(d.Ho * d.Wo) // 256)
    return d.Ho * -(-d.Wo // 256)


class StemBf16Step(_Step):
    """One ptx_conv_stem_bf16_fwd launch (Engine.bf16_stem = "direct"): the RGB stem of a bf16 plan on the bf16 matrix
    cores, read straight from the caller's bf16 NCDHW clip or from decoded uint8 frames (bound per run: plan.in_ptr;
    `norm` set = uint8 frames, normalised while the patch is staged) -- no im2col pass, no folded copy.
    `frame_step` set (SlowFast's pathways, any sub-sampled stem): ptx_conv_stem_bf16_strided_fwd -- d.Ti frames are used,
    conv frame t is frame t * frame_step of the T_full the source holds."""
    __slots__ = ("d", "plan", "src", "norm", "w", "b", "y", "label", "macs", "hbm_bytes", "frame_step", "T_full")
    _defaults = {"hbm_bytes": 0, "norm": None}
    kernel = "conv_stem_bf16"

    def issued_flop(self):
        """FLOP of the MFMAs one launch ISSUES: per 256-output tile and (kt, kh) step inside the clip, 4 waves x 4 position
        tiles x one v_mfma_f32_16x16x32_bf16 (K = 8 pixels x 4 channels = 32 for the 21 live entries of a kW = 7 row; 16384
        FLOP) per 16-channel tile that holds channels below ldy."""
        d = self.d
        tiles = stem_bf16_tiles(d)
        per_step = 4 * 4 * -(-d.ldy // 16) * 16384
        steps = 0
        for to in range(d.To):
            t0 = to * d.sT - d.pT
            steps += max(0, min(d.kT - 1, d.Ti - 1 - t0) - max(0, -t0) + 1) * d.kH
        return float(d.N * tiles * steps * per_step)

    def __call__(self, st):
        norm = C.byref(self.norm) if self.norm is not None else None
        if self.frame_step is not None:
            check(_lib.lib().ptx_conv_stem_bf16_strided_fwd(C.byref(self.d), self.plan.in_ptr, self.src, norm, self.frame_step,
                                                            self.T_full, self.w, self.b, self.y, st), self.label)
            return
        check(_lib.lib().ptx_conv_stem_bf16_fwd(C.byref(self.d), self.plan.in_ptr, self.src, norm, self.w, self.b, self.y, st),
              self.label)


class BnStatsStep(_Step):
    """One ptx_bn_batch_stats_f32 call (two launches) of a batch-statistics plan: mean and biased variance of activation `x`
    over its rows, into the plan-owned `mean` / `var` of BatchNorm number `index`.  The partials go through the plan's
    `bn_ws` (bound after the plan is built: one workspace, the largest need)."""
    __slots__ = ("plan", "index", "x", "rows", "C", "ld", "mean", "var", "label", "macs", "hbm_bytes")
    _defaults = {"macs": 0, "hbm_bytes": 0}
    kernel = "bn_batch_stats_f32"

    def __call__(self, st):
        p = self.plan
        check(_lib.lib().ptx_bn_batch_stats_f32(self.x, self.rows, self.C, self.ld, self.mean, self.var, p.bn_ws_ptr, p.bn_ws_bytes, st),
              self.label)


class BnUpdateStep(_Step):
    """One ptx_bn_batch_update_f32 launch: this batch's scale / shift, and the running statistics of BatchNorm `index` -- its
    slice of the plan's `bn_run` pair, which Engine.update_bn points at the buffers of the pass -- moved by the factor
    `plan.bn_f[index]` the pass sets per batch."""
    __slots__ = ("plan", "index", "off", "n", "C", "eps", "mean", "var", "gamma", "beta", "scale", "shift", "bn", "label", "macs", "hbm_bytes")
    _defaults = {"macs": 0, "hbm_bytes": 0}
    kernel = "bn_batch_update_f32"

    def __call__(self, st):
        p = self.plan
        bn = p.get(self.bn)
        gamma = _ptr(bn.weight.detach()) if bn.weight is not None else None
        beta = _ptr(bn.bias.detach()) if bn.bias is not None else None
        rm, rv = p.bn_run
        check(_lib.lib().ptx_bn_batch_update_f32(self.mean, self.var, self.n, C.c_float(p.bn_f[self.index]), C.c_float(self.eps),
                                                 gamma, beta, _ptr(rm, self.off), _ptr(rv, self.off), self.scale, self.shift,
                                                 self.C, st), self.label)


class BnApplyStep(_Step):
    """One ptx_bn_apply_f32 launch: y = act(raw * scale + shift [+ residual]) with the scale / shift of this batch."""
    __slots__ = ("d", "raw", "scale", "shift", "res", "y", "label", "macs", "hbm_bytes")
    _defaults = {"macs": 0, "hbm_bytes": 0}
    kernel = "bn_apply_f32"

    def __call__(self, st):
        check(_lib.lib().ptx_bn_apply_f32(C.byref(self.d), self.raw, self.scale, self.shift, self.res, self.y, st), self.label)
