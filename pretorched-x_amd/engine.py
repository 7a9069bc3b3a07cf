"""Forward-pass engine: compiles a zoo model + input shape into a list of libptx_amd launches.

Design (MI355X-first, not a translation of the reference's nn.Module graphs):
  * one *plan* per (input shape, device): every activation buffer is allocated once
    (channels-last NDHWC fp32, sized for 288 GB of HBM -- no reuse games), every conv descriptor,
    tile configuration and split-K factor is fixed at compile time, weights are BN-folded and
    re-laid-out K-major once (`ptx_pack_conv_weight`) and only re-packed when a parameter changes;
  * running a plan is a straight sequence of asynchronous C-ABI calls on torch's current HIP
    stream -- no synchronisation, no allocation except the returned tensor -- so it can be
    captured into a hipGraph (`Engine.capture`) and replayed;
  * there is no eager / CPU fallback: CPU tensors, training mode or a missing library raise.

torch is used for device memory (torch.empty), streams and parameter storage only.
"""
import collections
import contextlib
import ctypes as C
import json
import os
import threading
import time
import weakref

import torch
import torch.nn as nn

from . import _lib
from ._lib import (ConvDesc, ConvStage, ConvProgramInfo, NormDesc, PackDesc, PoolDesc, PTX_EPI_RELU, PTX_EPI_RES_ADD, PTX_EPI_RES_PADA,
                   PTX_EPI_RES_UP, PTX_F16_OPERANDS, PTX_F16X3_OPERANDS, PTX_SPLITK_FUSED, PTX_PRO_RELU, PTX_EPI_ACCUM, PTX_POOL_SAME, PTX_POOL_PAD_ZERO, PtxError, check,
                   PTX_BF16_OPERANDS, PTX_PACK_BF16, PTX_POOL_BF16)

# PTX_TUNED_TABLE: another table file (tuning sessions: A/B a freshly dumped table against the shipped one on the same box)
_TUNED_PATH = os.environ.get("PTX_TUNED_TABLE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_gfx950.json")
_tuned = None                    # conv problem key -> (tile configuration NAME, split-K)
_tuned_lock = threading.Lock()
_cfg_index = None                # configuration name -> index into this build's kConfigs table


# Structure epoch: bumped whenever ANY nn.Module in the process registers a parameter, buffer or sub-module (torch's
# global registration hooks fire from `register_parameter`, i.e. also from `blk.conv2.weight = nn.Parameter(w)`,
# `model.bn1 = FrozenBN(...)`, weight_norm / parametrize re-parametrisation).  An Engine's cached flat tensor list
# (`_owner_tensors`) is only valid for the epoch it was built in, so a replaced Parameter / module is noticed by the
# next forward's (data_ptr, _version) comparison instead of being served from stale packed filters.
_struct_epoch = [0]


def _bump_struct_epoch(*_a, **_k):
    _struct_epoch[0] += 1
    return None


def _install_struct_hooks():
    mod = torch.nn.modules.module
    for name in ("register_module_parameter_registration_hook", "register_module_buffer_registration_hook",
                 "register_module_module_registration_hook"):
        reg = getattr(mod, name, None)
        if reg is None:
            return False
        reg(_bump_struct_epoch)
    return True


_STRUCT_HOOKS = _install_struct_hooks()


def _config_index(name):
    """Index of a tile configuration by NAME in the loaded library (None when this build has no such tile).
    The tuned table stores names, so inserting / reordering kConfigs entries cannot remap it silently."""
    global _cfg_index
    if _cfg_index is None:
        lib = _lib.lib()
        n = lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16()      # the bf16 tiles close the table
        _cfg_index = {lib.ptx_conv3d_config_name(i).decode(): i for i in range(n)}
    return _cfg_index.get(name)


_chain_index = None              # chained-tile configuration name -> index (ptx_conv3d_chain_config_name)


def _chain_config_index(name):
    global _chain_index
    if _chain_index is None:
        lib = _lib.lib()
        _chain_index = {lib.ptx_conv3d_chain_config_name(i).decode(): i for i in range(lib.ptx_conv3d_chain_num_configs())}
    return _chain_index.get(name)


def chain_key(d, d2):
    return "chain:" + json.dumps(d.key() + d2.key())


def chain_lookup(key):
    """Tuned chained-tile index of a (conv, tail) problem pair, or None."""
    ent = _tuned_table().get(key)
    return None if ent is None else _chain_config_index(ent[0])


def chain_store(key, cfg_index):
    name = _lib.lib().ptx_conv3d_chain_config_name(int(cfg_index)).decode()
    table = _tuned_table()
    with _tuned_lock:
        table[key] = (name, 1)


def _tuned_table():
    global _tuned
    with _tuned_lock:
        if _tuned is None:
            _tuned = {}
            if os.path.exists(_TUNED_PATH):
                try:
                    _tuned = {k: (str(v[0]), int(v[1])) for k, v in json.load(open(_TUNED_PATH)).items()
                              if isinstance(v[0], str)}
                except Exception:
                    _tuned = {}
        return _tuned


def _tile_kind(name):
    """Operand flavour of a tile configuration by name: "f16" (halfs), "bf16", "x3" (split fp32 on f16 MFMA) or "" (fp32)."""
    return "f16" if name.endswith("/f16") else "bf16" if name.endswith("/bf16") else "x3" if name.endswith("/x3") else ""


def _flags_kind(flags):
    if flags & PTX_BF16_OPERANDS:
        return "bf16"
    return "f16" if flags & PTX_F16_OPERANDS else "x3" if flags & PTX_F16X3_OPERANDS else ""


# bf16 inference (a model whose floating-point parameters are torch.bfloat16): the families whose plans run end to end on the
# bf16 kernels.  Everything else raises at plan build time.
BF16_FAMILIES = ("resnet3d10", "resnet3d18", "resnet3d34", "resnet3d50", "resnet3d101", "resnet3d152", "resnet3d200",
                 "r2plus1d10", "r2plus1d18", "r2plus1d34", "r2plus1d50")
# ... and the plan kinds built from non-local blocks alone: NonLocalBlock1D / 2D / 3D and MNISTNonLocalNet (the networks that
# embed blocks in a ResNet, nonlocalresnet3d50 / nonlocal_r2plus1d50, keep raising)
BF16_NL_KINDS = ("nlblock", "mnist_nl")
# ... and the BigGAN-deep generator (every resolution and width; plans.build_biggan's bf16 flow)
BF16_GEN_KINDS = ("biggan",)


def model_precision(model):
    """"bf16" when the model's floating-point parameters are torch.bfloat16, "fp16" for torch.float16, else "fp32" -- read
    from the first weight (a generator step, not a walk of the tree: this runs on every forward)."""
    w = next(iter(model.parameters()), None)
    if w is None:
        w = next((getattr(m, "weight", None) for m in model.modules() if isinstance(getattr(m, "weight", None), torch.Tensor)), None)
    return {torch.bfloat16: "bf16", torch.float16: "fp16"}.get(getattr(w, "dtype", None), "fp32")


def tuned_lookup(key, kind=""):
    """(config index, split-K) of a tuned conv problem, or None: unknown keys, tiles this build does not
    have and entries of the wrong operand flavour all fall back to ptx_conv3d_pick_config."""
    kind = "f16" if kind is True else "" if kind is False else kind
    ent = _tuned_table().get(key)
    if ent is None or _tile_kind(ent[0]) != kind:
        return None
    idx = _config_index(ent[0])
    return None if idx is None else (idx, ent[1])


def tuned_store(key, cfg_index, split):
    name = _lib.lib().ptx_conv3d_config_name(int(cfg_index)).decode()
    table = _tuned_table()
    with _tuned_lock:
        table[key] = (name, int(split))


def tuned_snapshot():
    table = _tuned_table()
    with _tuned_lock:
        return dict(table)


def tuned_merge(entries):
    """Adopt another process's tuned entries (rank 0 tunes, every rank runs the same tiles)."""
    table = _tuned_table()
    with _tuned_lock:
        for k, v in entries.items():
            table[k] = (str(v[0]), int(v[1]))


def save_tuned_table(path=_TUNED_PATH):
    snap = tuned_snapshot()
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join('%s: ["%s", %d]' % (json.dumps(k), v[0], v[1]) for k, v in sorted(snap.items())) + "\n}\n")


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


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _device_ctx(dev):
    """torch.cuda.device(dev) for real devices; a no-op for the 'meta' device used by dry-run
    plan compilation (host-logic tests without a GPU)."""
    return torch.cuda.device(dev) if torch.device(dev).type == "cuda" else _NullCtx()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, offset_elems=0):
    return C.c_void_p(t.data_ptr() + 4 * offset_elems)


def _geom(conv):
    """(kernel, stride, padding) as (T,H,W) triples for Conv3d, or Conv2d seen as T == 1."""
    k, s, p = conv.kernel_size, conv.stride, conv.padding
    if isinstance(conv, nn.Conv2d):
        return (1,) + tuple(k), (1,) + tuple(s), (0,) + tuple(p)
    if isinstance(conv, nn.Conv1d):
        return (1, 1) + tuple(k), (1, 1) + tuple(s), (0, 0) + tuple(p)
    return tuple(k), tuple(s), tuple(p)


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
        self.bf16 = bool(getattr(plan, "bf16", False))
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
        self.x3 = (bool(getattr(plan, "x3", False) if x3 is None else x3) and not self.f16 and self.groups == 1
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
        self.x3 = bool(getattr(plan, "x3", False))
        rk = _r8 if self.x3 else _r4
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


def _tile_dims(name):
    """(BM, BN, BK) of an MFMA tile configuration name ("32x64x64/2x2/m16/dma/re"), or None for the direct (VALU) tiles."""
    import re
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
    kch = -(-max(d.ldx, d.Kc) // BK)
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


class ConvStep:
    """One ptx_conv3d_fwd (or, with a second source, ptx_conv3d_dual_fwd) launch with everything but
    the stream frozen."""
    __slots__ = ("d", "x", "x2", "w", "b", "res", "y", "cfg", "split", "plan", "label", "macs", "ext", "fused", "from_table",
                 "body", "body_w", "body_ok")

    @property
    def kernel(self):
        """Name the launch goes by in the per-launch rows: the tile configuration, or the body kernel."""
        if getattr(self, "body", None) is not None:
            return "conv_tstack_f32" if self.d.kH == 1 else "conv_body_f32"
        return _lib.lib().ptx_conv3d_config_name(self.cfg).decode()

    def issued_flop(self):
        if getattr(self, "body", None) is not None:
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
            if not getattr(self, "from_table", False) or getattr(e, "status", None) not in (1, 2, 4):
                raise
            sk = C.c_int(1)
            self.cfg = self.plan.lib.ptx_conv3d_pick_config(C.byref(self.d), C.byref(sk))
            self.split, self.from_table = sk.value, False
            p = self.plan
            need = int(p.lib.ptx_conv3d_workspace_bytes(C.byref(self.d), self.split))
            if need > p.ws_bytes:           # the workspace was sized for the tuned split: grow it for the default one
                p.ws = torch.zeros(need // 4, device=p.dev, dtype=torch.float32)
                p.ws_bytes, p.ws_ptr = need, _ptr(p.ws)
            import warnings
            warnings.warn("pretorched-x_amd: tuned tile for %s rejected by the library (%s); using the default tile" % (self.label, e))
            self._launch(st)

    def _launch(self, st):
        p = self.plan
        if getattr(self, "body", None) is not None:      # 3x3x3 body conv on its own patch-resident kernel (conv_body_f32.hip)
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


class ChainStep:
    """One ptx_conv3d_chain_fwd launch: conv -> BN -> ReLU -> 1x1x1 conv -> BN (-> + residual) -> ReLU, the intermediate
    tile kept in LDS (conv_chain.hip)."""
    __slots__ = ("d", "d2", "x", "w", "b", "w2", "b2", "res", "y", "cfg", "plan", "label", "macs", "hbm_bytes", "key",
                 "body", "body_ok", "body_w", "body_w2")

    @property
    def kernel(self):
        if getattr(self, "body", None) is not None:
            return "conv_body_chain_f32"
        return _lib.lib().ptx_conv3d_chain_config_name(self.cfg).decode()

    def issued_flop(self):
        if getattr(self, "body", None) is not None:
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
        if getattr(self, "body", None) is not None:       # the patch-resident body kernel with its chained tail
            check(_lib.lib().ptx_conv_body_chain_f32_fwd(C.byref(self.d), C.byref(self.d2), self.x, self.body_w, self.b, self.body_w2,
                                                         self.b2, self.res, self.y, self.body, st), self.label)
            return
        check(_lib.lib().ptx_conv3d_chain_fwd(C.byref(self.d), C.byref(self.d2), self.x, self.w, self.b, self.w2, self.b2,
                                              self.res, self.y, self.cfg, st), self.label)


class AltStep:
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
        return [self.chain] if self.use_chain else list(self.pair)


def prog_lookup(key):
    ent = _tuned_table().get("prog:" + key)
    return None if ent is None else ent[0] == "program"


def prog_store(key, use_program):
    table = _tuned_table()
    with _tuned_lock:
        table["prog:" + key] = ("program" if use_program else "launches", 1)


def lanes_key(model, shape, precision="fp32"):
    """Tuned-table key of the clip-lanes decision: one per (architecture, input shape, arithmetic)."""
    name = getattr(model, "arch_name", None) or type(model).__name__
    return "lanes:" + json.dumps([str(name), [int(v) for v in shape], precision])


def lanes_lookup(key):
    """Lanes the tuner measured best for this (architecture, shape), or None when it was never measured."""
    ent = _tuned_table().get(key)
    return None if ent is None or ent[0] != "lanes" else int(ent[1])


def lanes_store(key, n):
    table = _tuned_table()
    with _tuned_lock:
        table[key] = ("lanes", int(n))


BODY_SHAPES = ("tall", "square")      # ptx_conv_body_f32_fwd shapes 0 / 1
# filters the body kernels take: (1|3)x3x3 on the patch-resident tile; (3|5|7)x1x1 on the T-stacked tile (shape 0 only)
BODY_FILTERS = ((3, 3, 3), (1, 3, 3), (3, 1, 1), (5, 1, 1), (7, 1, 1))


def body_lookup(key):
    """Tuned verdict of a 3x3x3 problem on the patch-resident body kernel: shape index (0 tall, 1 square), -1 = the
    implicit-GEMM tile stays, None = never measured."""
    ent = _tuned_table().get("body:" + key)
    if ent is None:
        return None
    return BODY_SHAPES.index(ent[0]) if ent[0] in BODY_SHAPES else -1


def body_store(key, shape):
    table = _tuned_table()
    with _tuned_lock:
        table["body:" + key] = (BODY_SHAPES[shape] if shape is not None and shape >= 0 else "igemm", 1)


def alt_lookup(key):
    ent = _tuned_table().get("alt:" + key)
    return None if ent is None else ent[0] == "chain"


def alt_store(key, use_chain):
    table = _tuned_table()
    with _tuned_lock:
        table["alt:" + key] = ("chain" if use_chain else "pair", 1)


class ProgramStep:
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


class StemStep:
    """One ptx_conv_stem_x3_fwd launch (split-operand stem read from 4-channel positions) -- or, `planar`, one
    ptx_conv_stem_x3p_fwd launch (the same stem read from six half planes per frame: 21 % fewer matrix instructions)."""
    __slots__ = ("d", "x", "w", "b", "y", "label", "macs", "hbm_bytes", "planar")
    kernel = "conv_stem_x3"

    def __call__(self, st):
        fn = _lib.lib().ptx_conv_stem_x3p_fwd if self.planar else _lib.lib().ptx_conv_stem_x3_fwd
        check(fn(C.byref(self.d), self.x, self.w, self.b, self.y, st), self.label)


class PatchConvStep:
    """One launch of a generator-stage kernel designed for the fp16 matrix cores (gen_stage_f16.hip) instead of the
    implicit-GEMM tiles: ptx_conv3x3_f16_fwd (a GBlock's 3x3 convs, one staged input patch per tile) or, with `res` set /
    kernel == "conv1x1_skip_f16", ptx_conv1x1_skip_f16_fwd (its closing 1x1 conv + skip + both outputs); the "_bf16"
    kernels are their bf16 builds (bf16 generator plans)."""
    __slots__ = ("d", "x", "w", "b", "y", "ext", "res", "kernel", "label", "macs", "hbm_bytes", "ext_in")

    def __call__(self, st):
        ext = C.byref(self.ext) if self.ext is not None else None
        if self.kernel == "conv1x1_pro_f16":
            check(_lib.lib().ptx_conv1x1_pro_f16_fwd(C.byref(self.d), self.x, C.byref(self.ext_in), self.w, self.b, self.y, ext, st), self.label)
        elif self.kernel == "conv3x3_f16":
            check(_lib.lib().ptx_conv3x3_f16_fwd(C.byref(self.d), self.x, self.w, self.b, self.y, ext, st), self.label)
        elif self.kernel == "conv3x3_bf16":
            check(_lib.lib().ptx_conv3x3_bf16_fwd(C.byref(self.d), self.x, self.w, self.b, self.y, ext, st), self.label)
        elif self.kernel == "conv1x1_skip_bf16":
            check(_lib.lib().ptx_conv1x1_skip_bf16_fwd(C.byref(self.d), self.x, self.w, self.b, self.res, self.y, ext, st), self.label)
        else:
            check(_lib.lib().ptx_conv1x1_skip_f16_fwd(C.byref(self.d), self.x, self.w, self.b, self.res, self.y, ext, st), self.label)


class StemF32Step:
    """One ptx_conv_stem_f32_fwd launch: the RGB stem on the fp32 matrix cores, read straight from the caller's NCDHW
    tensor (bound per run: plan.in_ptr) -- no fold, no layout pass."""
    __slots__ = ("d", "plan", "strides", "w", "b", "y", "label", "macs", "hbm_bytes", "src")
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

    def __call__(self, st):
        sn, sc, stt = self.strides
        # src: a plan-owned fp32 NCDHW buffer (normalised uint8 frames / pitch-padded rows) or None = the caller's tensor
        x = self.src if self.src is not None else self.plan.in_ptr
        check(_lib.lib().ptx_conv_stem_f32_fwd(C.byref(self.d), x, sn, sc, stt, self.w, self.b, self.y, st), self.label)


class Plan:
    def __init__(self, engine, model, shape, dev, norm=None):
        self.dev = dev
        self.shape = tuple(shape)        # always the NCDHW / NCHW view of the input
        self.norm = norm                 # NormDesc when the input is uint8 frames (Engine.forward_frames)
        self.head = None                 # custom classifier tail (two-pathway / per-frame heads)
        self.refreshers = []             # extra weight-derived tables rebuilt with the packed filters
        self._run_lock = threading.Lock()
        self._last_done, self._last_stream = None, None
        self.in_ptr2 = C.c_void_p(0)     # second input (BigGAN: class embedding)
        self.lib = _lib.lib()
        self.steps = []          # callables(stream)
        self.conv_steps = []
        self.chain_steps = []    # ChainStep launches (two convs each; tuned over their own tile table)
        self.alt_steps = []      # AltStep: chained launch | the two launches, chosen by measurement
        # chained convs (conv -> 1x1x1 conv in one launch): fp32 and split-operand plans; PTX_CHAIN=0 keeps every conv its
        # own launch
        self.chain = os.environ.get("PTX_CHAIN", "1") != "0"
        self.packs = []
        self.acts = []
        self._pack_cache = {}
        self.ws_bytes = 0
        self.ws = None
        self.ws_ptr = C.c_void_p(0)
        self.nl_ws_bytes, self.nl_ws, self.nl_ws_ptr = 0, None, C.c_void_p(0)      # stream-K attention partials
        self.in_ptr = C.c_void_p(0)      # set per run
        self.keepalive = []
        self.tuned = False
        self.graph = None
        self.fuse_shortcut = os.environ.get("PTX_FUSE_SHORTCUT", "1") != "0"
        # arithmetic: the model's parameter dtype decides bf16 (every conv on the bf16 tiles, bf16 activations); for fp32
        # models Engine.precision picks fp32 / x3
        prec = model_precision(model)
        if prec == "fp16":
            raise PtxError("fp16 models (model.half()) are not supported: use bfloat16 (model.to(torch.bfloat16)) or float32")
        self.bf16 = prec == "bf16"
        self.precision = "bf16" if self.bf16 else getattr(engine, "precision", "fp32")
        self.x3 = self.precision == "x3"     # split fp32 operands on the fp16 matrix cores
        # qualified names of the model's modules: everything the plan keeps from the model is a _Ref
        self._names = {id(m): n for n, m in model.named_modules()}
        self._cur = model                # the model (or DataParallel replica) whose tensors are valid right now
        self.program_steps = []  # ProgramStep: runs of small-M convs as one persistent launch
        with _device_ctx(dev):
            self._build(model)
            self._fuse_programs()
            if self.ws_bytes:
                self.ws = torch.zeros(self.ws_bytes // 4, device=dev, dtype=torch.float32)
                self.ws_ptr = _ptr(self.ws)
            if self.nl_ws_bytes:
                self.nl_ws = torch.empty(self.nl_ws_bytes // 4, device=dev, dtype=torch.float32)
                self.nl_ws_ptr = _ptr(self.nl_ws)
        self._cur = None

    # ---------------------------------------------------------------- model references
    def ref(self, module):
        name = self._names.get(id(module))
        return _Ref(name) if name is not None else _Ref(None, module)

    def get(self, ref):
        if ref.name is None:
            return ref.obj
        if self._cur is None:
            raise PtxError("plan used outside a bound model (internal error)")
        return self._cur.get_submodule(ref.name) if ref.name else self._cur

    def bind(self, model):
        self._cur = model

    # ---------------------------------------------------------------- building blocks
    def pack(self, convs, bn, fold_kw=False, scale=None, f16=False, x3=None, stem4=False, fold_hw=False, pad8=False):
        """scale: (module, attribute name) of a scalar Parameter multiplying the filter.
        x3: force (True) / forbid (False) split operands for this filter; None = the plan's precision.
        pad8: Co-concatenated filters each start on an 8-row boundary (zero rows in between)."""
        if not isinstance(convs, (list, tuple)):
            convs = [convs]
        key = (tuple(id(c) for c in convs), id(bn), fold_kw, None if scale is None else (id(scale[0]), scale[1]), bool(f16), x3,
               bool(stem4), bool(fold_hw)) + (("pad8",) if pad8 else ())
        if key not in self._pack_cache:
            p = Packed(self, convs, bn, fold_kw, scale, f16, x3, stem4, fold_hw, pad8)
            self._pack_cache[key] = p
            self.packs.append(p)
        return self._pack_cache[key]

    def pack_dual(self, conv, bn, conv2, bn2):
        key = ("dual", id(conv), id(bn), id(conv2), id(bn2))
        if key not in self._pack_cache:
            p = PackedDual(self, conv, bn, conv2, bn2)
            self._pack_cache[key] = p
            self.packs.append(p)
        return self._pack_cache[key]

    def act(self, N, T, H, W, C_, ld=None, f16=False):
        a = Act(self.dev, N, T, H, W, C_, ld, f16, bf16=bool(f16) and self.bf16)
        self.acts.append(a)      # steps hold raw pointers: the plan owns every buffer
        return a

    def conv(self, x, pk, stride, padding, relu=False, res=None, res_kind=None, res_stride=1,
             label="conv", y=None, x2=None, x2_stride=1, same=False, up2=False, affine=None, out_f16=False,
             raw=False, tanh=False, pro_affine=None):
        """Fused generator-stage extras (fp16-operand convs only, ptx_conv3d_fused_fwd):
        up2      the conv slides over the nearest-2x upsampled input (the loader does the upsampling);
        affine   (scale_ptr, shift_ptr, ld): per-sample affine after bias (+ skip) -- the NEXT layer's cBN, folded;
        out_f16  y is written as halfs;  raw: also return the pre-affine output as a second (halfs) activation;
        tanh     tanh on the output."""
        kT, kH, kW = pk.k_eff
        sT, sH, sW = stride
        if self.bf16:        # bf16 plans: every conv reads and writes bf16 activations (one rounding per output)
            out_f16 = True
        xT, xH, xW = x.T, x.H * (2 if up2 else 1), x.W * (2 if up2 else 1)
        if same:        # TF-"SAME": out = ceil(in/stride), `padding` is ignored, front pad = total // 2
            (To, Ho, Wo), padding = _same_geometry((xT, xH, xW), (kT, kH, kW), stride)
        pT, pH, pW = padding
        if not same:
            To = (xT + 2 * pT - kT) // sT + 1
            Ho = (xH + 2 * pH - kH) // sH + 1
            Wo = (xW + 2 * pW - kW) // sW + 1
        if y is None:
            y = self.act(x.N, To, Ho, Wo, pk.Co, f16=out_f16)
        if bool(y.f16) != bool(out_f16):
            raise PtxError("%s: output precision mismatch" % label)
        if (y.N, y.T, y.H, y.W, y.C) != (x.N, To, Ho, Wo, pk.Co):
            raise PtxError("%s: output target %s does not match the conv result %s" % (
                label, (y.N, y.T, y.H, y.W, y.C), (x.N, To, Ho, Wo, pk.Co)))
        if y.ld != _r4(pk.Co) and pk.Co % 4 and not out_f16:
            raise PtxError("%s: a channel-slice output needs Co %% 4 == 0" % label)
        # PTX_SPLITK_FUSED=1: split-K launches reduce in-kernel (last-arriving block; the plan's workspace is allocated
        # ZEROED, its first 64 KiB are tile counters every launch leaves at zero).  Off by default: measured SLOWER than
        # the separate reduce launch on MI355X (layer4 3x3x3, split 6: 33 -> 54 us) -- the device-scope release / acquire
        # across the 8 XCD L2s and one block summing what 100+ blocks of the reduce kernel sum in parallel cost more than
        # the launch they save; the tuner answered by abandoning split-K (config 2: 1355 -> 1309 clips/s).
        flags = (PTX_EPI_RELU if relu else 0) | (PTX_SPLITK_FUSED if os.environ.get("PTX_SPLITK_FUSED", "0") == "1" else 0)
        d = ConvDesc()
        d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = x.N, xT, xH, xW, x.C, x.ld
        half = bool(getattr(x, "f16", False))
        if half != bool(getattr(pk, "f16", False)):
            raise PtxError("%s: activation and filter precisions differ" % label)
        bf16 = bool(getattr(x, "bf16", False))
        if bf16 != bool(getattr(pk, "bf16", False)):
            raise PtxError("%s: activation and filter precisions differ" % label)
        if half:        # fp16 operands: the descriptor counts 32-bit words (channel pairs)
            # bf16: an odd channel count reads its zero pad channel as the pair's second half (rows are 16-byte padded)
            if (x.C % 2 and not bf16) or x.ld % 8 or x2 is not None:
                raise PtxError("%s: fp16 operands need an even channel count and 16-byte rows" % label)
            flags |= PTX_F16_OPERANDS | (PTX_BF16_OPERANDS if bf16 else 0)
            d.Ci, d.ldx = (x.C + 1) // 2, x.ld // 2
        if getattr(pk, "x3", False):
            flags |= PTX_F16X3_OPERANDS
        fused = bool(up2 or affine is not None or out_f16 or raw or tanh or (res is not None and getattr(res, "f16", False)))
        if fused and not half:
            raise PtxError("%s: the fused generator-stage options need fp16 operands" % label)
        ext, raw_act = None, None
        if fused:
            from ._lib import (ConvFusedExt, PTX_EPI_AFFINE, PTX_EPI_DUAL_RAW, PTX_EPI_OUT_F16, PTX_EPI_TANH,
                               PTX_PRO_UP2, PTX_RES_F16)
            flags |= (PTX_PRO_UP2 if up2 else 0) | (PTX_EPI_OUT_F16 if out_f16 else 0) | (PTX_EPI_TANH if tanh else 0)
            if res is not None and getattr(res, "f16", False):
                flags |= PTX_RES_F16
            if affine is not None or raw:
                ext = ConvFusedExt()
                if affine is not None:
                    flags |= PTX_EPI_AFFINE
                    ext.scale, ext.shift, ext.ld_affine = affine[0], affine[1], int(affine[2])
                if raw:
                    raw_act = self.act(x.N, To, Ho, Wo, pk.Co, f16=True)
                    flags |= PTX_EPI_DUAL_RAW
                    ext.y_raw, ext.ld_raw = raw_act.t.data_ptr(), raw_act.ld
        # (a bf16 output of odd width writes its zero pad channel with the pair: bias / filter rows there are zero)
        d.To, d.Ho, d.Wo, d.Co, d.ldy = To, Ho, Wo, pk.Co + (pk.Co % 2 if bf16 else 0), y.ld
        d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = kT, kH, kW, sT, sH, sW, pT, pH, pW
        d.Kc, d.Co_pad = (pk.Kc // 2 if half else pk.Kc), pk.Co_pad
        d.groups = getattr(pk, "groups", 1)
        if d.groups > 1 and (x.C != pk.Ci * d.groups or pk.Ci % 4):
            raise PtxError("%s: grouped conv needs Ci/groups %% 4 == 0 and a %d-channel input" % (label, pk.Ci * d.groups))
        resptr = C.c_void_p(0)
        if res is not None:
            resptr = _ptr(res.t)
            d.ldr = res.ld
            if res_kind == "padA":
                flags |= PTX_EPI_RES_PADA
                d.res_C, d.res_T, d.res_H, d.res_W = res.C, res.T, res.H, res.W
                d.res_sT = d.res_sH = d.res_sW = int(res_stride)
            elif res_kind == "up":           # nearest-upsampled, channel-truncated skip; res_stride = log2 factors
                flags |= PTX_EPI_RES_PADA | PTX_EPI_RES_UP
                d.res_C, d.res_T, d.res_H, d.res_W = res.C, res.T, res.H, res.W
                d.res_sT, d.res_sH, d.res_sW = _t3(res_stride)
            else:
                flags |= PTX_EPI_RES_ADD
                assert (res.N, res.T, res.H, res.W, res.C) == (y.N, y.T, y.H, y.W, y.C), "residual shape"
        d.flags = flags
        st = ConvStep()
        st.d, st.x, st.w, st.b, st.res, st.y = d, _ptr(x.t), _ptr(pk.w), _ptr(pk.b), resptr, _ptr(y.t)
        st.plan, st.label = self, label
        st.macs = x.N * To * Ho * Wo * pk.Co * getattr(pk, "real_ci", pk.Ci) * pk.d.kT * pk.d.kH * pk.d.kW
        st.x2 = None
        st.ext, st.fused = ext, fused
        if x2 is not None:                      # K-concatenated second activation source (shortcut B)
            d.x2_C, d.x2_ld, d.x2_T, d.x2_H, d.x2_W = x2.C, x2.ld, x2.T, x2.H, x2.W
            d.x2_sT, d.x2_sH, d.x2_sW = _t3(x2_stride)
            st.x2 = _ptr(x2.t)
            st.macs += x.N * To * Ho * Wo * pk.Co * x2.C
        patch = None
        if pro_affine is not None:
            # the conv reads the RAW map and applies (scale, shift, ld) + ReLU to its input fragments: ptx_conv1x1_pro_f16_fwd only
            from ._lib import ConvFusedExt
            if not (fused and res is None and not raw and not tanh and x2 is None and self.lib.ptx_conv1x1_pro_f16_supported(C.byref(d))):
                raise PtxError("%s: an input affine needs the shapes ptx_conv1x1_pro_f16_fwd covers" % label)
            ps = PatchConvStep()
            ps.ext_in = ConvFusedExt()
            ps.ext_in.scale, ps.ext_in.shift, ps.ext_in.ld_affine = pro_affine[0], pro_affine[1], int(pro_affine[2])
            ps.d, ps.x, ps.w, ps.b, ps.y, ps.ext, ps.label = d, st.x, st.w, st.b, st.y, ext, label
            ps.res, ps.kernel = resptr, "conv1x1_pro_f16"
            ps.macs, ps.hbm_bytes = st.macs, 0
            self.steps.append(ps)
            self.patch_steps = getattr(self, "patch_steps", 0) + 1
            return y
        if fused and not tanh and x2 is None and not bf16:
            # generator stage: a GBlock's 3x3 convs (64 / 128 / 256 channels) and its closing 1x1 conv have their own fp16
            # kernels (gen_stage_f16.hip: no tile table, nothing to tune); PTX_CONV3X3_F16=0 / PTX_CONV1X1_F16=0: A/B runs
            if (res is None and not raw and os.environ.get("PTX_CONV3X3_F16", "1") != "0"
                    and self.lib.ptx_conv3x3_f16_supported(C.byref(d))):
                patch = "conv3x3_f16"
            elif os.environ.get("PTX_CONV1X1_F16", "1") != "0" and self.lib.ptx_conv1x1_skip_f16_supported(C.byref(d)):
                patch = "conv1x1_skip_f16"
        elif fused and not tanh and x2 is None and getattr(self, "gen_patch", False):
            # bf16 generator plans: the same two kernels on bf16 operands; PTX_CONV3X3_BF16=0 / PTX_CONV1X1_BF16=0: A/B runs
            if (res is None and not raw and os.environ.get("PTX_CONV3X3_BF16", "1") != "0"
                    and self.lib.ptx_conv3x3_bf16_supported(C.byref(d))):
                patch = "conv3x3_bf16"
            elif os.environ.get("PTX_CONV1X1_BF16", "1") != "0" and self.lib.ptx_conv1x1_skip_bf16_supported(C.byref(d)):
                patch = "conv1x1_skip_bf16"
        if patch is not None:
            ps = PatchConvStep()
            ps.d, ps.x, ps.w, ps.b, ps.y, ps.ext, ps.label = d, st.x, st.w, st.b, st.y, ext, label
            ps.res, ps.kernel, ps.ext_in = resptr, patch, None
            ps.macs, ps.hbm_bytes = st.macs, 0
            self.steps.append(ps)
            self.patch_steps = getattr(self, "patch_steps", 0) + 1
            return (y, raw_act) if raw else y
        key = json.dumps(d.key())
        # the patch-resident 3x3x3 body kernel (round 6): a second execution of the same problem, chosen per problem by
        # the tuner ("body:" keys) like a tile; PTX_CONV_BODY=0 keeps every 3x3x3 conv on the implicit-GEMM tiles (A/B runs),
        # =tall / =square force a shape wherever it is supported
        st.body, st.body_w, st.body_ok = None, None, ()
        if (not fused and x2 is None and not half and not getattr(pk, "x3", False) and (kT, kH, kW) in BODY_FILTERS
                and isinstance(pk, Packed) and not getattr(pk, "fold_kw", False) and os.environ.get("PTX_CONV_BODY", "1") != "0"):
            st.body_ok = tuple(sh for sh in (0, 1) if self.lib.ptx_conv_body_f32_supported(C.byref(d), sh))
        if st.body_ok:
            wb = torch.empty(int(self.lib.ptx_conv_body_f32_weight_elems(C.byref(d))), device=self.dev, dtype=torch.float32)
            self.keepalive.append(wb)
            st.body_w = _ptr(wb)
            lib_, wsrc, wdst = self.lib, _ptr(pk.w), st.body_w

            def repack_body(d=d, lib_=lib_, wsrc=wsrc, wdst=wdst):
                check(lib_.ptx_pack_conv_body_f32_weight(C.byref(d), wsrc, wdst, _stream()), "ptx_pack_conv_body_f32_weight")
            if torch.device(self.dev).type != "meta":
                self.refreshers.append(repack_body)
            force = os.environ.get("PTX_CONV_BODY", "1")
            known = body_lookup(key)
            if force in BODY_SHAPES and BODY_SHAPES.index(force) in st.body_ok:
                st.body = BODY_SHAPES.index(force)
            elif known is not None and known in st.body_ok:
                st.body = known
        tuned = tuned_lookup(key, _flags_kind(flags))
        if tuned is not None and not self.lib.ptx_conv3d_config_supported(C.byref(d), tuned[0]):
            tuned = None                 # a stale table entry is dropped here, at plan-build time
        st.from_table = tuned is not None
        if tuned is not None:
            st.cfg, st.split = tuned
        else:
            sk = C.c_int(1)
            st.cfg = self.lib.ptx_conv3d_pick_config(C.byref(d), C.byref(sk))
            st.split = sk.value
        # split-K workspace: room for the tuner's widest split on small problems, else the chosen one
        out_bytes = 4 * x.N * To * Ho * Wo * y.ld
        want = 8 if out_bytes * 8 <= (128 << 20) else st.split
        self.ws_bytes = max(self.ws_bytes, int(self.lib.ptx_conv3d_workspace_bytes(C.byref(d), want)))
        self.steps.append(st)
        self.conv_steps.append(st)
        return (y, raw_act) if raw else y

    def conv_chain(self, x, pk, stride, padding, pk2, relu1=True, relu2=False, res=None, label="chain", y=None):
        """conv(x, pk) -> [ReLU] -> 1x1x1 conv (pk2) -> [+ res] -> [ReLU] as ONE launch (ptx_conv3d_chain_fwd): returns (output
        activation, ChainStep) -- the step is NOT appended to the plan; the caller also emits the two separate launches into
        the same output and wraps both with Plan.alt() -- or None when the pair does not qualify.  Qualifies: dense unfolded
        filters of one operand kind (fp32, or split operands in an "x3" plan), a pointwise tail whose K axis is the first conv's output, at most 128 intermediate channels (one N tile
        holds the whole intermediate row), a same-shape residual (or none), and enough rows to fill the chip from M tiles
        alone (the tail's N slices run inside one workgroup: M >= PTX_CHAIN_MIN_M, default 8192)."""
        if not self.chain or isinstance(x, RawInput) or getattr(x, "f16", False):
            return None
        for p_ in (pk, pk2):
            if getattr(p_, "f16", False) or getattr(p_, "groups", 1) > 1 or getattr(p_, "fold_kw", False) or not isinstance(p_, Packed):
                return None
        x3 = bool(getattr(pk, "x3", False))
        if x3 != bool(getattr(pk2, "x3", False)):          # both GEMMs of a chained launch take the same operand kind
            return None
        rk = _r8 if x3 else _r4
        fx3 = PTX_F16X3_OPERANDS if x3 else 0
        # 32 .. PTX_CHAIN_MAX_N1 intermediate channels: narrower convs (SlowFast's fast pathway: 8 / 16 planes) keep their
        # 16-wide / direct tiles -- a 32-wide chained tile would pad their work 2-4x
        if pk2.k_eff != (1, 1, 1) or pk2.Ci != pk.Co or pk.Co < 32 or _r4(pk.Co) > min(128, int(os.environ.get("PTX_CHAIN_MAX_N1", "128"))):
            return None
        kT, kH, kW = pk.k_eff
        sT, sH, sW = stride
        pT, pH, pW = padding
        To, Ho, Wo = (x.T + 2 * pT - kT) // sT + 1, (x.H + 2 * pH - kH) // sH + 1, (x.W + 2 * pW - kW) // sW + 1
        M = x.N * To * Ho * Wo
        if min(To, Ho, Wo) < 1 or M < int(os.environ.get("PTX_CHAIN_MIN_M", "8192")):
            return None
        if res is not None and (res.N, res.T, res.H, res.W, res.C) != (x.N, To, Ho, Wo, pk2.Co):
            return None
        if y is not None and ((y.N, y.T, y.H, y.W, y.C) != (x.N, To, Ho, Wo, pk2.Co) or getattr(y, "f16", False)):
            return None
        d = ConvDesc()
        d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = x.N, x.T, x.H, x.W, x.C, x.ld
        d.To, d.Ho, d.Wo, d.Co, d.ldy = To, Ho, Wo, pk.Co, rk(pk.Co)
        d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = kT, kH, kW, sT, sH, sW, pT, pH, pW
        d.Kc, d.Co_pad, d.groups = pk.Kc, pk.Co_pad, 1
        d.flags = (PTX_EPI_RELU if relu1 else 0) | fx3
        ld_out = y.ld if y is not None else _r4(pk2.Co)
        d2 = ConvDesc()
        d2.N, d2.Ti, d2.Hi, d2.Wi, d2.Ci, d2.ldx = x.N, To, Ho, Wo, pk.Co, rk(pk.Co)
        d2.To, d2.Ho, d2.Wo, d2.Co, d2.ldy = To, Ho, Wo, pk2.Co, ld_out
        d2.kT = d2.kH = d2.kW = d2.sT = d2.sH = d2.sW = 1
        d2.Kc, d2.Co_pad, d2.groups = pk2.Kc, pk2.Co_pad, 1
        d2.flags = (PTX_EPI_RELU if relu2 else 0) | (PTX_EPI_RES_ADD if res is not None else 0) | fx3
        d2.ldr = res.ld if res is not None else 0
        key = chain_key(d, d2)
        cfg = chain_lookup(key)
        if cfg is None or not self.lib.ptx_conv3d_chain_supported(C.byref(d), C.byref(d2), cfg):
            cfg = self.lib.ptx_conv3d_chain_pick_config(C.byref(d), C.byref(d2))
        if cfg < 0 or not self.lib.ptx_conv3d_chain_supported(C.byref(d), C.byref(d2), cfg):
            return None
        if y is None:
            y = self.act(x.N, To, Ho, Wo, pk2.Co)
        if y.ld != _r4(pk2.Co) and pk2.Co % 4:
            raise PtxError("%s: a channel-slice output needs Co %% 4 == 0" % label)
        st = ChainStep()
        st.d, st.d2, st.cfg, st.key, st.plan, st.label = d, d2, cfg, key, self, label
        st.x, st.w, st.b, st.w2, st.b2, st.y = _ptr(x.t), _ptr(pk.w), _ptr(pk.b), _ptr(pk2.w), _ptr(pk2.b), _ptr(y.t)
        st.res = _ptr(res.t) if res is not None else C.c_void_p(0)
        st.macs = M * (pk.Co * getattr(pk, "real_ci", pk.Ci) * kT * kH * kW + pk2.Co * pk.Co)
        st.hbm_bytes = 0
        # the same pair on the patch-resident body kernel with its chained tail (round 6): a second execution of the chained
        # launch, chosen per pair by the tuner ("body:chain:" keys); PTX_CONV_BODY=0 / tall / square as for the plain convs
        st.body, st.body_ok, st.body_w, st.body_w2 = None, (), None, None
        if not x3 and (kT, kH, kW) in ((3, 3, 3), (1, 3, 3)) and os.environ.get("PTX_CONV_BODY", "1") != "0":
            st.body_ok = tuple(sh for sh in (0, 1) if self.lib.ptx_conv_body_chain_f32_supported(C.byref(d), C.byref(d2), sh))
        if st.body_ok:
            wb = torch.empty(int(self.lib.ptx_conv_body_f32_weight_elems(C.byref(d))), device=self.dev, dtype=torch.float32)
            wt = torch.empty(int(self.lib.ptx_conv_body_tail_f32_weight_elems(C.byref(d2))), device=self.dev, dtype=torch.float32)
            self.keepalive += [wb, wt]
            st.body_w, st.body_w2 = _ptr(wb), _ptr(wt)
            lib_, w1s, w2s = self.lib, _ptr(pk.w), _ptr(pk2.w)

            def repack_body_chain(d=d, d2=d2, lib_=lib_, w1s=w1s, w2s=w2s, w1d=st.body_w, w2d=st.body_w2):
                check(lib_.ptx_pack_conv_body_f32_weight(C.byref(d), w1s, w1d, _stream()), "ptx_pack_conv_body_f32_weight")
                check(lib_.ptx_pack_conv_body_tail_f32_weight(C.byref(d2), w2s, w2d, _stream()), "ptx_pack_conv_body_tail_f32_weight")
            if torch.device(self.dev).type != "meta":
                self.refreshers.append(repack_body_chain)
            force = os.environ.get("PTX_CONV_BODY", "1")
            known = body_lookup(key)
            if force in BODY_SHAPES and BODY_SHAPES.index(force) in st.body_ok:
                st.body = BODY_SHAPES.index(force)
            elif known is not None and known in st.body_ok:
                st.body = known
        self.chain_steps.append(st)
        return y, st

    def alt(self, chain, first_step, label):
        """Wrap the plan steps emitted since `first_step` (the two separate launches of a pair) and its chained launch into
        ONE AltStep; the choice comes from the tuned table, else the measured default (chained up to 64 mid channels)."""
        pair = self.steps[first_step:]
        del self.steps[first_step:]
        a = AltStep()
        a.chain, a.pair, a.label, a.key = chain, pair, label, chain.key
        known = alt_lookup(chain.key)
        a.use_chain = known if known is not None else (_r4(chain.d.Co) <= int(os.environ.get("PTX_CHAIN_DEFAULT_MAX_N1", "64")))
        force = os.environ.get("PTX_CHAIN_FORCE")          # "1" / "0": A/B runs
        if force in ("0", "1"):
            a.use_chain = force == "1"
        self.steps.append(a)
        self.alt_steps.append(a)
        return a

    def conv_bn(self, x, conv, bn, relu=False, res=None, res_kind=None, res_stride=1, label="conv", y=None):
        """nn.Conv{2,3}d or a (2+1)D pair, followed by `bn`, with the epilogue fused."""
        if hasattr(conv, "spatial_conv"):      # r2plus1d.py:85-88
            ks, ss, ps = _geom(conv.spatial_conv)
            fold = _foldable(conv.spatial_conv, x)
            kt, st_, pt = _geom(conv.temporal_conv)
            if not fold and ks == (1, 1, 1) and kt == (1, 1, 1) and res_kind is None and ps == (0, 0, 0) and pt == (0, 0, 0):
                # a "1x1x1" SpatioTemporalConv = two pointwise GEMMs through the mid channels (r2plus1d.py:68-88): ONE chained
                # launch, strides composed (the pair's output positions index the input directly)
                yc = self.conv_chain(x, self.pack(conv.spatial_conv, conv.bn), tuple(a * b for a, b in zip(ss, st_)), (0, 0, 0),
                                     self.pack(conv.temporal_conv, bn), relu1=True, relu2=relu, res=res, label=label + ".pair", y=y)
                if yc is not None:
                    y, first = yc[0], len(self.steps)
                    mid = self.conv(x, self.pack(conv.spatial_conv, conv.bn), ss, ps, relu=True, label=label + ".spatial")
                    self.conv(mid, self.pack(conv.temporal_conv, bn), st_, pt, relu=relu, res=res, label=label + ".temporal", y=y)
                    self.alt(yc[1], first, label + ".pair")
                    return y
            mid = self.stem_direct(x, conv.spatial_conv, conv.bn, True, label + ".spatial") if fold else None
            if mid is None:
                mid = self.conv(x if not fold else self.fold_input(x, conv.spatial_conv),
                            self.pack(conv.spatial_conv, conv.bn, fold),
                            (ss[0], ss[1], 1) if fold else ss, (ps[0], ps[1], 0) if fold else ps,
                            relu=True, label=label + ".spatial")
            kt, st_, pt = _geom(conv.temporal_conv)
            return self.conv(mid, self.pack(conv.temporal_conv, bn), st_, pt, relu=relu, res=res,
                             res_kind=res_kind, res_stride=res_stride, label=label + ".temporal", y=y)
        k, s, p = _geom(conv)
        same = bool(getattr(conv, "tf_same", False))       # I3D's Unit3D: explicit "SAME" padding
        fold = _foldable(conv, x)
        if fold and res is None and y is None:
            direct = self.stem_direct(x, conv, bn, relu, label)
            if direct is not None:
                return direct
        if fold:
            if same:    # the fold consumes the W axis with its own SAME front pad; T/H stay SAME in the conv
                _, pf = _same_geometry((x.T, x.H, x.W), k, s)
                x = self.fold_input(x, conv, same_pad=pf[2])
            else:
                x = self.fold_input(x, conv)
            s, p = (s[0], s[1], 1), (p[0], p[1], 0)
        return self.conv(x, self.pack(conv, bn, fold), s, p, relu=relu, res=res, res_kind=res_kind,
                         res_stride=res_stride, label=label, y=y, same=same)

    def stem_direct(self, raw, conv, bn, relu, label):
        """Split-operand stems skip the kW fold: the input becomes [N,T,H,W,4] (16-byte positions) and
        ptx_conv_stem_x3_fwd serves every (kh, kw) tap of a temporal tap from one staged input patch.  Returns None when
        the kernel does not cover the geometry (the folded implicit-GEMM path then runs)."""
        if os.environ.get("PTX_STEM_DIRECT", "1") == "0":
            return None
        if self.bf16:
            return self.stem_bf16(raw, conv, bn, relu, label)
        if raw.norm is not None and os.environ.get("PTX_STEM_DIRECT_U8", "1") == "0":
            return None                  # uint8 frames on the round-1 path: normalise + kW fold in one pass
        if not self.x3:
            return self.stem_direct_f32(raw, conv, bn, relu, label)
        if raw.t_step != 1:
            return None
        if not isinstance(conv, (nn.Conv3d, nn.Conv2d)) or raw.C > 4:
            return None
        (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = _geom(conv)
        if getattr(conv, "tf_same", False):     # I3D's Unit3D: out = ceil(in / stride), front pad = total // 2
            (To, Ho, Wo), (pT, pH, pW) = _same_geometry((raw.T, raw.H, raw.W), (kT, kH, kW), (sT, sH, sW))
        else:
            To, Ho, Wo = (raw.T + 2 * pT - kT) // sT + 1, (raw.H + 2 * pH - kH) // sH + 1, (raw.W + 2 * pW - kW) // sW + 1
        d = ConvDesc()
        d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = raw.N, raw.T, raw.H, raw.W, raw.C, 4
        d.To, d.Ho, d.Wo, d.Co = To, Ho, Wo, conv.out_channels
        d.ldy = _r4(conv.out_channels)
        d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = kT, kH, kW, sT, sH, sW, pT, pH, pW
        d.Kc, d.Co_pad = 32, _r128(conv.out_channels)
        d.flags = PTX_F16X3_OPERANDS | (PTX_EPI_RELU if relu else 0)
        if min(To, Ho, Wo) < 1 or not self.lib.ptx_conv_stem_x3_supported(C.byref(d)):
            return None
        lib, Nn, Cc, Ss = self.lib, raw.N, raw.C, raw.T * raw.H * raw.W
        src = self.stem_source(raw, pitch=raw.W)        # uint8 frames: normalised to fp32 NCDHW first (one 1 B -> 4 B pass)
        pk = self.pack(conv, bn, fold_kw=True, x3=True, stem4=True)
        planar = os.environ.get("PTX_STEM_X3P", "1") != "0" and bool(lib.ptx_conv_stem_x3p_supported(C.byref(d)))
        if planar:
            # six half planes per frame (c0 c1 c2 hi | lo): 12 bytes per pixel, a (kh, channel) run of 8 columns is one MFMA operand
            x4 = torch.empty(raw.N * raw.T * 6 * raw.H * raw.W, device=self.dev, dtype=torch.float16)
            self.keepalive.append(x4)
            x4p, Tt, Hh, Ww = _ptr(x4), raw.T, raw.H, raw.W

            def to_planes(st, self=self):
                check(lib.ptx_ncdhw_to_split_planes(src if src is not None else self.in_ptr, x4p, Nn, Cc, Tt, Hh, Ww, st),
                      "ptx_ncdhw_to_split_planes")
            self.steps.append(_tag(to_planes, "ncdhw_to_split_planes", 4 * Nn * Cc * Ss + 12 * Nn * Ss))
            w2 = torch.empty(lib.ptx_stem_x3p_weight_elems(C.byref(d)), device=self.dev, dtype=torch.float32)
            self.keepalive.append(w2)
            wsrc, w2p = _ptr(pk.w), _ptr(w2)

            def repack():
                check(lib.ptx_pack_stem_x3p_weight(C.byref(d), wsrc, w2p, _stream()), "ptx_pack_stem_x3p_weight")
            self.refreshers.append(repack)
            wptr = w2p
        else:
            # one 16-byte position per pixel, already split into (hi4 | lo4) halfs: the NCDHW edge does the split once
            x4 = self.act(raw.N, raw.T, raw.H, raw.W, 4)
            x4p = _ptr(x4.t)

            def to_split4(st, self=self):
                check(lib.ptx_ncdhw_to_split4(src if src is not None else self.in_ptr, x4p, Nn, Cc, Ss, st), "ptx_ncdhw_to_split4")
            self.steps.append(_tag(to_split4, "ncdhw_to_split4", 4 * Nn * Cc * Ss + 16 * Nn * Ss))
            wptr = _ptr(pk.w)
        y = self.act(raw.N, To, Ho, Wo, conv.out_channels)
        st = StemStep()
        st.d, st.x, st.w, st.b, st.y, st.label, st.planar = d, x4p, wptr, _ptr(pk.b), _ptr(y.t), label, planar
        st.macs = raw.N * To * Ho * Wo * conv.out_channels * raw.C * kT * kH * kW
        st.hbm_bytes = 0
        self.steps.append(st)
        self.stem_steps = getattr(self, "stem_steps", 0) + 1
        return y

    def stem_bf16(self, raw, conv, bn, relu, label):
        """bf16 RGB stem (conv1 of ResNet3D, resnet3D.py:153-155; the (1,7,7) spatial stem of R2Plus1D, r2plus1d.py:73-88):
        ptx_im2col_hw_bf16 folds the (kh, kw) taps of the caller's bf16 NCDHW clip into 147 channels (rows padded to 160),
        and the stem becomes a (kT, 1, 1) conv over them on the bf16 tiles -- 160 / 147 = 1.09x the algorithmic MACs
        issued (plus tile padding), no torch layout pass."""
        if raw.norm is not None or raw.t_step != 1 or not isinstance(conv, nn.Conv3d):
            raise PtxError("%s: the bf16 stem reads a bf16 NCDHW clip (uint8 frames / frame sub-sampling are fp32 only)" % label)
        (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = _geom(conv)
        if getattr(conv, "tf_same", False):
            raise PtxError("%s: SAME-padded stems are not supported in bf16" % label)
        Ho, Wo = (raw.H + 2 * pH - kH) // sH + 1, (raw.W + 2 * pW - kW) // sW + 1
        if min(Ho, Wo) < 1:
            raise PtxError("%s: input too small for the stem" % label)
        K = kH * kW * raw.C
        xf = self.act(raw.N, raw.T, Ho, Wo, K, ld=(K + 31) // 32 * 32, f16=True)
        lib, yp = self.lib, _ptr(xf.t)
        N, Cc, T, H, W, ld = raw.N, raw.C, raw.T, raw.H, raw.W, xf.ld

        def im2col(st, self=self):
            check(lib.ptx_im2col_hw_bf16(self.in_ptr, yp, N, Cc, T, H, W, kH, kW, sH, sW, pH, pW, Ho, Wo, ld, st), "ptx_im2col_hw_bf16")
        self.steps.append(_tag(im2col, "im2col_hw_bf16", 2 * N * Cc * T * H * W + 2 * xf.t.numel()))
        y = self.conv(xf, self.pack(conv, bn, fold_hw=True), (sT, 1, 1), (pT, 0, 0), relu=relu, label=label)
        self.stem_bf16_step = self.conv_steps[-1]
        self.stem_steps = getattr(self, "stem_steps", 0) + 1
        return y

    def stem_direct_f32(self, raw, conv, bn, relu, label):
        """fp32 stems skip the kW fold as well: ptx_conv_stem_f32_fwd LDS-DMAs the input patch of a temporal tap from the
        user's NCDHW tensor (frame sub-sampling is a stride) and serves every (kh, kw) tap from it.  Returns None when the
        kernel does not cover the geometry (the folded implicit-GEMM path then runs)."""
        if not isinstance(conv, (nn.Conv3d, nn.Conv2d)) or raw.C != 3 or getattr(self, "f16", False):
            return None
        if conv.out_channels <= 32:       # 64-wide channel tiles: SlowFast's 8-channel fast stem keeps the narrow tiles
            return None
        (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = _geom(conv)
        if getattr(conv, "tf_same", False):     # I3D's Unit3D: out = ceil(in / stride), front pad = total // 2
            (To, Ho, Wo), (pT, pH, pW) = _same_geometry((raw.T, raw.H, raw.W), (kT, kH, kW), (sT, sH, sW))
        else:
            To, Ho, Wo = (raw.T + 2 * pT - kT) // sT + 1, (raw.H + 2 * pH - kH) // sH + 1, (raw.W + 2 * pW - kW) // sW + 1
        pitch = _r4(raw.W)               # rows of a width that is not a multiple of 4 get a zero-padded 16-byte pitch
        d = ConvDesc()
        d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = raw.N, raw.T, raw.H, raw.W, 3, (pitch if pitch != raw.W else 0)
        d.To, d.Ho, d.Wo, d.Co = To, Ho, Wo, conv.out_channels
        d.ldy = _r4(conv.out_channels)
        d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = kT, kH, kW, sT, sH, sW, pT, pH, pW
        d.Co_pad = _r128(conv.out_channels)
        d.flags = PTX_EPI_RELU if relu else 0
        plane = raw.H * pitch
        strides = (raw.C * raw.T_full * plane, raw.T_full * plane, raw.t_step * plane)
        if min(To, Ho, Wo) < 1 or not self.lib.ptx_conv_stem_f32_supported(C.byref(d), *strides):
            return None
        src = self.stem_source(raw, pitch)
        pk = self.pack(conv, bn, fold_kw=True, x3=False)          # [tap][Co_pad][Kc], k = kw * 3 + c, BN folded
        d.Kc = pk.Kc
        w2 = torch.empty(self.lib.ptx_stem_f32_weight_elems(C.byref(d)), device=self.dev, dtype=torch.float32)
        self.keepalive.append(w2)
        lib, wf, w2p, Kc = self.lib, _ptr(pk.w), _ptr(w2), pk.Kc

        def repack():
            check(lib.ptx_pack_stem_f32_weight(C.byref(d), wf, Kc, w2p, _stream()), "ptx_pack_stem_f32_weight")
        self.refreshers.append(repack)
        y = self.act(raw.N, To, Ho, Wo, conv.out_channels)
        st = StemF32Step()
        st.d, st.plan, st.strides, st.w, st.b, st.y, st.label = d, self, strides, w2p, _ptr(pk.b), _ptr(y.t), label
        st.src = src
        st.macs = raw.N * To * Ho * Wo * conv.out_channels * raw.C * kT * kH * kW
        st.hbm_bytes = 0
        self.steps.append(st)
        self.stem_steps = getattr(self, "stem_steps", 0) + 1
        return y

    def stem_source(self, raw, pitch):
        """The fp32 NCDHW tensor a direct stem kernel reads, as a device pointer -- or None when that is the caller's own
        tensor (fp32 clips whose rows already have a 16-byte pitch: bound per run, plan.in_ptr).  Otherwise the plan owns
        it and fills it first: decoded uint8 frames [N,T,H,W,C] are normalised by ptx_frames_u8_to_ncdhw (TransformImage's
        tensor half, transforms/utils.py:72-75; bit-identical to the CPU ops) -- 1 B in, 4 B out per sample, ~5 % of the
        bytes the kW fold moved -- and rows whose width is not a multiple of 4 are copied to a zero-padded pitch
        (ptx_pad_rows).  Built once per plan: both SlowFast pathways read the same buffer through their own frame stride."""
        key = (raw.norm is not None, pitch)
        cache = self.__dict__.setdefault("_stem_src", {})
        if key in cache:
            return cache[key]
        lib = self.lib
        N, Cc, Tf, H, W = raw.N, raw.C, raw.T_full, raw.H, raw.W
        src = None
        if raw.norm is not None:
            norm = raw.norm
            buf = torch.empty((N, Cc, Tf, H, W), device=self.dev, dtype=torch.float32)
            self.keepalive += [norm, buf]
            bp = _ptr(buf)

            def to_f32(st, self=self):
                check(lib.ptx_frames_u8_to_ncdhw(self.in_ptr, bp, N, Tf, H, W, Cc, C.byref(norm), st), "ptx_frames_u8_to_ncdhw")
            self.steps.append(_tag(to_f32, "frames_u8_to_ncdhw", 5 * N * Cc * Tf * H * W))
            src = bp
        if pitch != W:
            rows = N * Cc * Tf * H
            buf2 = torch.empty((rows, pitch), device=self.dev, dtype=torch.float32)
            self.keepalive.append(buf2)
            b2p, prev = _ptr(buf2), src

            def pad(st, self=self):
                check(lib.ptx_pad_rows(prev if prev is not None else self.in_ptr, b2p, rows, W, pitch, st), "ptx_pad_rows")
            self.steps.append(_tag(pad, "pad_rows", 4 * rows * (W + pitch)))
            src = b2p
        cache[key] = src
        return src

    def fold_input(self, raw, conv, same_pad=None):
        """raw: RawInput (NCDHW user tensor or uint8 frames).  Emits the fold kernel."""
        (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = _geom(conv)
        if same_pad is not None:
            pW, Wo = same_pad, -(-raw.W // sW)
        else:
            Wo = (raw.W + 2 * pW - kW) // sW + 1
        ld = max(_r4(kW * raw.C), 32 if self.x3 else _stem_ld()) if kW * raw.C <= 24 else (_r8 if self.x3 else _r4)(kW * raw.C)
        # C = live folded columns (kW * Cin = 21 for the RGB stem); the kernel drops the MFMAs that
        # would only multiply the zero pad columns [C, ld)
        y = self.act(raw.N, raw.T, raw.H, Wo, kW * raw.C, ld)
        lib, yp = self.lib, _ptr(y.t)
        N, C_, T, H, W = raw.N, raw.C, raw.T, raw.H, raw.W
        step_t, T_full = raw.t_step, raw.T_full
        if raw.norm is not None:         # decoded uint8 frames [N,T,H,W,C]: normalise + fold in one pass
            norm = raw.norm
            self.keepalive.append(norm)

            def step(st, self=self):
                check(lib.ptx_fold_kw_frames_u8(self.in_ptr, yp, N, C_, T, H, W, step_t, T_full, kW, sW, pW, Wo, ld,
                                                C.byref(norm), st), "ptx_fold_kw_frames_u8")
        else:                            # NCDHW fp32; `input[:, :, ::step]` is a stride, not a copy
            plane = H * W
            sn, sc, stt = C_ * T_full * plane, T_full * plane, step_t * plane

            def step(st, self=self):
                check(lib.ptx_fold_kw_strided(self.in_ptr, yp, N, C_, T, H, W, sn, sc, stt, kW, sW, pW, Wo, ld, st),
                      "ptx_fold_kw_strided")
        in_bytes = N * C_ * T * H * W * (1 if raw.norm is not None else 4)
        self.steps.append(_tag(step, "fold_kw", in_bytes + 4 * y.t.numel()))
        return y

    def to_channels_last(self, raw):
        if self.bf16:        # bf16 plans: the caller's bf16 NCDHW input, channels [C, ld) zero-filled
            y = self.act(raw.N, raw.T, raw.H, raw.W, raw.C, f16=True)
            lib, yp = self.lib, _ptr(y.t)
            N, C_, S, ld = raw.N, raw.C, raw.T * raw.H * raw.W, y.ld

            def step(st, self=self):
                check(lib.ptx_ncdhw_to_ndhwc_bf16(self.in_ptr, yp, N, C_, S, ld, st), "ptx_ncdhw_to_ndhwc_bf16")
            self.steps.append(_tag(step, "ncdhw_to_ndhwc_bf16", 2 * N * C_ * S + 2 * y.t.numel()))
            return y
        y = self.act(raw.N, raw.T, raw.H, raw.W, raw.C)
        lib, yp = self.lib, _ptr(y.t)
        N, C_, S, ld = raw.N, raw.C, raw.T * raw.H * raw.W, y.ld

        def step(st, self=self):
            check(lib.ptx_ncdhw_to_ndhwc(self.in_ptr, yp, N, C_, S, ld, st), "ptx_ncdhw_to_ndhwc")
        self.steps.append(_tag(step, "ncdhw_to_ndhwc", 4 * N * C_ * S + 4 * y.t.numel()))
        return y

    def maxpool(self, x, k, s, p=None, y=None, same=False):
        """max_pool3d.  same=True: TF-"SAME" geometry (out = ceil(in/stride), front pad = total//2) with
        zero-valued padding -- F.pad followed by an unpadded MaxPool3d, as I3D ports do."""
        if same:
            To, Ho, Wo = (-(-x.T // s[0]), -(-x.H // s[1]), -(-x.W // s[2]))
            p = tuple(max((o - 1) * st + kk - i, 0) // 2 for o, st, kk, i in zip((To, Ho, Wo), s, k, (x.T, x.H, x.W)))
        else:
            To = (x.T + 2 * p[0] - k[0]) // s[0] + 1
            Ho = (x.H + 2 * p[1] - k[1]) // s[1] + 1
            Wo = (x.W + 2 * p[2] - k[2]) // s[2] + 1
        bf16 = bool(getattr(x, "bf16", False))
        if y is None:
            y = self.act(x.N, To, Ho, Wo, x.C, x.ld, f16=bf16)
        assert (y.N, y.T, y.H, y.W, y.C) == (x.N, To, Ho, Wo, x.C), "pool output shape"
        assert bool(getattr(y, "bf16", False)) == bf16, "pool output precision"
        d = PoolDesc(x.N, x.T, x.H, x.W, x.C, x.ld, To, Ho, Wo, k[0], k[1], k[2], s[0], s[1], s[2], p[0], p[1], p[2],
                     y.ld, ((PTX_POOL_SAME | PTX_POOL_PAD_ZERO) if same else 0) | (PTX_POOL_BF16 if bf16 else 0))
        lib, xp, yp = self.lib, _ptr(x.t), _ptr(y.t)
        self.keepalive.append(d)

        def step(st):
            check(lib.ptx_maxpool3d_fwd(C.byref(d), xp, yp, st), "ptx_maxpool3d_fwd")
        esz = 2 if getattr(x, "f16", False) else 4
        self.steps.append(_tag(step, "maxpool3d", esz * (x.N * x.S * x.C + y.N * To * Ho * Wo * x.C)))
        return y

    def attention(self, th, ph, g, y, scale_only=False, f16=False, relu=False):
        """y = softmax(th . ph^T) . g  (or (th . ph^T / Nk) . g, or (relu(th . ph^T) / Nk) . g) per sample, as one
        ptx_nonlocal_fwd launch.  th [N, Sq, d], ph [N, Sk, d], g [N, Sk, dv], y [N, Sq, dv]: channels-last activations
        (possibly channel slices).  Returns False -- nothing emitted -- when the fused kernel does not cover the shape
        (d > 1024) or PTX_NL_FUSED=0 asks for the unfused bgemm / softmax / bgemm chain."""
        from ._lib import NonlocalDesc, PTX_NL_F16, PTX_NL_RELU, PTX_NL_SCALE, PTX_NL_SOFTMAX, PTX_NL_X3
        if self.bf16:
            return self.attention_bf16(th, ph, g, y, scale_only, relu)
        d = NonlocalDesc()
        d.batch, d.Nq, d.Nk, d.d, d.dv = th.N, th.S, ph.S, th.C, g.C
        d.ld_theta, d.ld_phi, d.ld_g, d.ld_y = th.ld, ph.ld, g.ld, y.ld
        d.bs_theta, d.bs_phi, d.bs_g, d.bs_y = th.S * th.ld, ph.S * ph.ld, g.S * g.ld, y.S * y.ld
        d.mode = PTX_NL_SCALE if scale_only else PTX_NL_SOFTMAX
        if relu:
            if not scale_only:
                raise PtxError("attention: relu modifies the scale-only affinity")
            d.mode |= PTX_NL_RELU
        if f16 and not scale_only and th.C <= 64:      # fp16-operand MFMAs (the generator's fp16 plan)
            d.mode |= PTX_NL_F16
            if getattr(y, "f16", False):               # ... whose output conv reads halfs
                from ._lib import PTX_NL_OUT_F16
                d.mode |= PTX_NL_OUT_F16
        elif self.x3 and os.environ.get("PTX_NL_X3", "1") != "0":      # split operands, like the plan's convs
            d.mode |= PTX_NL_X3
        if getattr(y, "f16", False) and not (d.mode & PTX_NL_F16):
            raise PtxError("attention: a half output needs the fp16-operand kernel (d <= 64, softmax)")
        if os.environ.get("PTX_NL_FUSED", "1") == "0" or not self.lib.ptx_nonlocal_supported(C.byref(d)):
            return False
        lib, tp, pp, gp, yp = self.lib, _ptr(th.t), _ptr(ph.t), _ptr(g.t), _ptr(y.t)
        self.keepalive.append(d)
        # long sequences run the stream-K form over a scratch buffer of the plan (one for all its attention launches: they
        # follow each other on one stream; NOT the split-K workspace, whose head may hold arrival counters)
        self.nl_ws_bytes = max(self.nl_ws_bytes, int(lib.ptx_nonlocal_workspace_bytes(C.byref(d))))

        def step(st, self=self):
            check(lib.ptx_nonlocal_ws_fwd(C.byref(d), tp, pp, gp, yp, self.nl_ws_ptr, self.nl_ws_bytes, st), "ptx_nonlocal_ws_fwd")
        self.steps.append(_tag(step, "nonlocal_attention", 4 * th.N * (th.S * th.C + ph.S * ph.C + g.S * g.C + th.S * g.C),
                               macs=th.N * th.S * ph.S * (th.C + g.C)))
        self.attn_steps = getattr(self, "attn_steps", 0) + 1
        return True

    def attention_bf16(self, th, ph, g, y, scale_only=False, relu=False):
        """bf16 plans: the same attention as one ptx_nonlocal_bf16_fwd launch (bf16 operands on the bf16 matrix cores, fp32
        accumulate and softmax state; P and y rounded to bf16 once).  Every operand is a bf16 activation whose pad channels
        up to round8(C) are zero (the kernel contracts over them); y's columns [0, round8(dv)) are written."""
        from ._lib import NonlocalDesc, PTX_NL_BF16, PTX_NL_RELU, PTX_NL_SCALE, PTX_NL_SOFTMAX
        if not all(getattr(a, "bf16", False) for a in (th, ph, g, y)):
            raise PtxError("attention: a bf16 plan's operands are bf16 activations")
        if relu and not scale_only:
            raise PtxError("attention: relu modifies the scale-only affinity")
        d = NonlocalDesc()
        d.batch, d.Nq, d.Nk, d.d, d.dv = th.N, th.S, ph.S, th.C, g.C
        d.ld_theta, d.ld_phi, d.ld_g, d.ld_y = th.ld, ph.ld, g.ld, y.ld
        d.bs_theta, d.bs_phi, d.bs_g, d.bs_y = th.S * th.ld, ph.S * ph.ld, g.S * g.ld, y.S * y.ld
        d.mode = PTX_NL_BF16 | (PTX_NL_SCALE if scale_only else PTX_NL_SOFTMAX) | (PTX_NL_RELU if relu else 0)
        if not self.lib.ptx_nonlocal_supported(C.byref(d)):
            raise PtxError("attention: the bf16 kernel does not cover d=%d (d <= 1024)" % th.C)
        lib, tp, pp, gp, yp = self.lib, _ptr(th.t), _ptr(ph.t), _ptr(g.t), _ptr(y.t)
        self.keepalive.append(d)

        def step(st):
            check(lib.ptx_nonlocal_bf16_fwd(C.byref(d), tp, pp, gp, yp, st), "ptx_nonlocal_bf16_fwd")
        self.steps.append(_tag(step, "nonlocal_attention", 2 * th.N * (th.S * th.C + ph.S * ph.C + g.S * g.C + th.S * g.C),
                               macs=th.N * th.S * ph.S * (th.C + g.C)))
        self.attn_steps = getattr(self, "attn_steps", 0) + 1
        self.attn_descs = getattr(self, "attn_descs", []) + [d]
        self.attn_operands = getattr(self, "attn_operands", []) + [(th, ph, g, y)]
        return True

    def concat_rows_bf16(self, th, ph, nl, label):
        """bf16 'concatenation' affinity rows: (a_i, 1, 0, ..) and (1, b_j, 0, ..) as one bf16 1x1x1 conv each (Co = 8,
        zero rows 2..7), so relu(a_i + b_j) / Nk is the PTX_NL_SCALE | PTX_NL_RELU mode of the bf16 attention at d = 8.
        a_i and b_j are rounded to bf16 by the conv epilogue (the 1s are exact)."""
        pa = _ConcatRowsPack(self, nl, th.C, "a")
        pb = _ConcatRowsPack(self, nl, th.C, "b")
        self.packs += [pa, pb]
        one, zero = (1, 1, 1), (0, 0, 0)
        ta = self.conv(th, pa, one, zero, label=label + ".concat_a")
        tb = self.conv(ph, pb, one, zero, label=label + ".concat_b")
        return ta, tb

    def concat_attention(self, th, ph, g, y, nl, label):
        """The 'concatenation' affinity (nonlocalnet.py:213-243) on the fused attention kernel.  The 1x1 conv over
        cat([theta_i, phi_j]) is a_i + b_j with a = theta . w[:ci], b = phi . w[ci:] -- the dot product of the 2-vectors
        (a_i, 1) and (1, b_j) -- so f = relu(a_i + b_j) / N is ptx_nonlocal_fwd's PTX_NL_SCALE | PTX_NL_RELU mode on
        4-float rows (two live columns), and f . g runs in the same launch: the [N, Sq, Sk] affinity never reaches
        HBM.  Two small GEMMs produce the rows: Linear(ci -> 4) with weight rows (w_theta, 0, 0, 0) / bias (0, 1, 0, 0)
        and weight rows (0, w_phi, 0, 0) / bias (1, 0, 0, 0).  Returns False (nothing emitted) under PTX_NL_FUSED=0."""
        if self.bf16:
            ta, pb = self.concat_rows_bf16(th, ph, nl, label)
            return self.attention_bf16(ta, pb, g, y, scale_only=True, relu=True)
        if os.environ.get("PTX_NL_FUSED", "1") == "0":
            return False
        ci = th.C
        f32 = dict(device=self.dev, dtype=torch.float32)
        wa, wb = torch.zeros((4, ci), **f32), torch.zeros((4, ci), **f32)
        ba, bb = torch.zeros(4, **f32), torch.zeros(4, **f32)
        self.keepalive += [wa, wb, ba, bb]
        proj_ref = self.ref(nl.concat_project[0])

        def refresh():
            proj = self.get(proj_ref)
            w = proj.weight.detach().reshape(-1)
            wa.zero_(); wb.zero_(); ba.zero_(); bb.zero_()
            wa[0].copy_(w[:ci])
            wb[1].copy_(w[ci:])
            ba[1], bb[0] = 1.0, 1.0
            if proj.bias is not None:
                ba[0] = proj.bias.detach().reshape(())
        if torch.device(self.dev).type != "meta":
            self.refreshers.append(refresh)
        ta = self.act(th.N, th.T, th.H, th.W, 4)
        pb = self.act(ph.N, ph.T, ph.H, ph.W, 4)
        lib = self.lib
        thp, php, tap, pbp = _ptr(th.t), _ptr(ph.t), _ptr(ta.t), _ptr(pb.t)
        wap, wbp, bap, bbp = _ptr(wa), _ptr(wb), _ptr(ba), _ptr(bb)
        Mq, Mk, ldt, ldp = th.N * th.S, ph.N * ph.S, th.ld, ph.ld

        def step(st):
            check(lib.ptx_linear_fwd(thp, wap, bap, tap, Mq, ci, 4, ldt, 4, 0, st), label + ".concat_a")
            check(lib.ptx_linear_fwd(php, wbp, bbp, pbp, Mk, ci, 4, ldp, 4, 0, st), label + ".concat_b")
        self.steps.append(_tag(step, "nonlocal_concat_ab", 4 * (Mq + Mk) * (ci + 4), macs=(Mq + Mk) * ci))
        if not self.attention(ta, pb, g, y, scale_only=True, relu=True):
            raise PtxError("%s: the fused concatenation attention refused a supported shape" % label)
        return True

    def pool_target(self, x, win):
        """A compact bf16 output for the non-local block's 2x2x2 sub-sampling pool of x (stride = window, no padding)."""
        To, Ho, Wo = ((e - w) // w + 1 for e, w in zip((x.T, x.H, x.W), win))
        return self.act(x.N, To, Ho, Wo, x.C, f16=True)

    def nonlocal_block(self, x, nl, label):
        """Non-local block (nonlocalnet.py:139-243): pointwise projections in one launch, f = theta^T phi on
        MFMA, row softmax (or 1/N scaling), y = f g on MFMA, W projection (+BN) + residual in one launch.
        Modes: embedded_gaussian (:143-166), dot_product (:192-211, f / N), gaussian (:168-190, theta = phi = x),
        concatenation (:213-243: relu(w . cat(theta_i, phi_j)) / N = relu(a_i + b_j) / N with two GEMVs);
        `sub_sample` max-pools phi and g 2x2x2 (:126-131)."""
        mode = getattr(nl, "mode", "embedded_gaussian")
        sub = bool(getattr(nl, "sub_sample", False))
        if mode not in ("embedded_gaussian", "dot_product", "gaussian", "concatenation"):
            raise PtxError("unknown non-local mode %r" % mode)
        lib = self.lib
        first = (lambda m: m[0]) if sub else (lambda m: m)        # Sequential(conv, max_pool) when sub-sampling
        g_conv = first(nl.g)
        ci = g_conv.out_channels
        one, zero = (1, 1, 1), (0, 0, 0)
        if mode == "gaussian":
            g_act = self.conv(x, self.pack(g_conv, None), one, zero, label=label + ".g")
            th_act = ph_act = x                                   # theta = phi = the input itself
        elif self.bf16 and mode == "concatenation":
            # bf16 'concatenation': theta and phi feed the two row convs (concat_rows_bf16), and a conv reads every channel
            # of its input row (ldx), so they are compact activations of their own here rather than slices of one output
            th_act = self.conv(x, self.pack(nl.theta, None), one, zero, label=label + ".theta")
            ph_act = self.conv(x, self.pack(first(nl.phi), None), one, zero, label=label + ".phi")
            g_act = self.conv(x, self.pack(g_conv, None), one, zero, label=label + ".g")
        elif self.bf16:
            # bf16: theta | phi | g each on an 8-channel boundary (zero filter rows / bias between): 16-byte aligned slices
            # whose pad channels are zero -- what the bf16 attention contracts over
            c8 = _r8(ci)
            tpg = self.conv(x, self.pack([nl.theta, first(nl.phi), g_conv], None, pad8=True), one, zero,
                            label=label + ".theta_phi_g")
            th_act, ph_act, g_act = tpg.slice(0, ci), tpg.slice(c8, ci), tpg.slice(2 * c8, ci)
        else:
            tpg = self.conv(x, self.pack([nl.theta, first(nl.phi), g_conv], None), one, zero, label=label + ".theta_phi_g")
            th_act, ph_act, g_act = tpg.slice(0, ci), tpg.slice(ci, ci), tpg.slice(2 * ci, ci)
        if sub:
            # nn.MaxPool{1,2,3}d(kernel_size=2): stride 2, floor -- over the block's own axes (a 2-D block runs as T = 1)
            dim = int(getattr(nl, "dimension", 3))
            win = (1,) * (3 - dim) + (2,) * dim
            pool = (win, win, (0, 0, 0))
            if any(e < w for e, w in zip((x.T, x.H, x.W), win)):
                raise PtxError("%s: sub_sample needs at least 2 positions along every pooled axis" % label)
            if self.bf16:
                # compact outputs; the bf16 pool writes channels [0, round8(C)) as maxima over the input's pad channels,
                # which are zero (zero filter rows, or the zero-filled pad of x), and the buffers start zeroed
                ph_act = self.maxpool(ph_act, *pool, y=self.pool_target(ph_act, win))
                g_act = self.maxpool(g_act, *pool, y=self.pool_target(g_act, win))
            else:
                ph_act = self.maxpool(ph_act, *pool)
                g_act = self.maxpool(g_act, *pool)
        N, Sq, Sk, K = x.N, x.S, ph_act.S, th_act.C
        yatt = self.act(x.N, x.T, x.H, x.W, ci, f16=self.bf16)
        fused = False
        if mode == "concatenation":
            fused = self.concat_attention(th_act, ph_act, g_act, yatt, nl, label)
        else:
            fused = self.attention(th_act, ph_act, g_act, yatt, scale_only=(mode == "dot_product"))
        if fused:
            # theta^T phi -> softmax (or 1/N) -> . g in ONE launch: the [N, Sq, Sk] affinity never reaches HBM
            if getattr(nl, "bn_layer", True):
                return self.conv(yatt, self.pack(nl.W[0], nl.W[1]), one, zero, res=x, label=label + ".W")
            return self.conv(yatt, self.pack(nl.W, None), one, zero, res=x, label=label + ".W")
        ldf = _r4(Sk)
        f = torch.empty((N, Sq, ldf), device=self.dev, dtype=torch.float32)
        gT = torch.empty((N, ci, ldf), device=self.dev, dtype=torch.float32)
        self.keepalive += [f, gT]
        th, ph, gp = _ptr(th_act.t), _ptr(ph_act.t), _ptr(g_act.t)
        lda, ldb, ldg = th_act.ld, ph_act.ld, g_act.ld
        fp, gtp, yp, yld = _ptr(f), _ptr(gT), _ptr(yatt.t), yatt.ld
        scale_only = int(mode == "dot_product")
        if mode == "concatenation":
            av = torch.empty(N * Sq, device=self.dev, dtype=torch.float32)
            bv = torch.empty(N * Sk, device=self.dev, dtype=torch.float32)
            self.keepalive += [av, bv]
            avp, bvp, proj_ref = _ptr(av), _ptr(bv), self.ref(nl.concat_project[0])

        def step(st):
            if mode == "concatenation":
                w = self.get(proj_ref).weight.detach().reshape(-1).contiguous()          # [2*ci]: theta half | phi half
                check(lib.ptx_linear_fwd(th, _ptr(w), None, avp, N * Sq, ci, 1, lda, 1, 0, st), "concat a")
                check(lib.ptx_linear_fwd(ph, _ptr(w, ci), None, bvp, N * Sk, ci, 1, ldb, 1, 0, st), "concat b")
                check(lib.ptx_outer_sum_relu(avp, bvp, fp, N, Sq, Sk, ldf, st), "concat f")
            else:
                check(lib.ptx_bgemm_nt(th, ph, fp, N, Sq, Sk, K, lda, ldb, ldf, Sq * lda, Sk * ldb, Sq * ldf, st), "bgemm f")
                check(lib.ptx_softmax_rows(fp, N * Sq, Sk, ldf, scale_only, st), "softmax")
            check(lib.ptx_transpose_last2(gp, gtp, N, Sk, ci, ldg, ldf, st), "transpose g")
            check(lib.ptx_bgemm_nt(fp, gtp, yp, N, Sq, ci, Sk, ldf, ldf, yld, Sq * ldf, ci * ldf, Sq * yld, st), "bgemm y")
        self.steps.append(_tag(step, "nonlocal_unfused", macs=N * Sq * Sk * (K + ci)))
        if getattr(nl, "bn_layer", True):
            return self.conv(yatt, self.pack(nl.W[0], nl.W[1]), one, zero, res=x, label=label + ".W")
        return self.conv(yatt, self.pack(nl.W, None), one, zero, res=x, label=label + ".W")

    # ---------------------------------------------------------------- network
    def _build(self, model):
        kind = getattr(model, "plan_kind", "resnet")
        if self.bf16:
            name = str(getattr(model, "arch_name", None) or type(model).__name__)
            arch = getattr(model, "arch", None)
            # the standalone non-local blocks and MNISTNonLocalNet run on the bf16 attention kernel
            if kind not in BF16_NL_KINDS + BF16_GEN_KINDS and (
                    kind != "resnet" or name.split("@")[0] not in BF16_FAMILIES or arch is None or arch.nonlocal_layers
                    or arch.dims != 3 or arch.block not in ("basic", "bottleneck")):
                raise PtxError("bf16 inference covers the ResNet3D (resnet3d10..200) and R(2+1)D (r2plus1d10..50) families, "
                               "the non-local blocks and the BigGAN-deep generator; "
                               "%s (plan kind %r) has bf16 parameters: run it in float32" % (name, kind))
        if kind == "nlblock":                    # a standalone NonLocalBlock3D: [B,C,T,H,W] -> [B,C,T,H,W]
            N, Cc, T, H, W = self.shape
            self.feat = self.nonlocal_block(self.to_channels_last(RawInput(N, Cc, T, H, W)), model, "nl")
            self.pooled = None
            return
        if kind != "resnet":                     # SlowFast / I3D / BigGAN-deep: plans.py
            from . import plans
            return getattr(plans, "build_" + kind)(self, model)
        arch = model.arch
        shp = self.shape
        if arch.dims == 2:
            N, Cin, H, W = shp
            T = 1
        else:
            N, Cin, T, H, W = shp
        raw = RawInput(N, Cin, T, H, W, norm=self.norm)
        x = self.conv_bn(raw, model.conv1, model.bn1, relu=True, label="conv1")
        if arch.dims == 2:
            x = self.maxpool(x, (1, 3, 3), (1, 2, 2), (0, 1, 1))
        else:
            x = self.maxpool(x, (3, 3, 3), (2, 2, 2), (1, 1, 1))
        for li in range(4):
            for bi, blk in enumerate(getattr(model, "layer%d" % (li + 1))):
                x = self._block(arch, blk, x, "layer%d.%d" % (li + 1, bi))
        self.feat = x
        # head buffers
        self.pooled = torch.empty((x.N, x.C), device=self.dev, dtype=torch.float32)

    def _block(self, arch, blk, x, name, out=None):
        """One residual block.  `out`: optional pre-allocated target (a channel slice of the next
        stage's concatenated input, slowfast.py:145-151) for the block's final conv."""
        s = blk.stride
        if arch.block.startswith("preact"):
            return self._block_preact(arch, blk, x, name)
        # (bf16 plans: shortcut B runs as its own conv + a fused residual add -- the dual-source GEMM is fp32 / x3 only)
        fuse = (self.fuse_shortcut and not self.bf16 and blk.has_shortcut and arch.shortcut == "B" and arch.block in ("bottleneck", "resnext", "wide")
                and isinstance(blk.conv3, (nn.Conv3d, nn.Conv2d)) and isinstance(blk.downsample[0], (nn.Conv3d, nn.Conv2d)))
        if fuse:
            # conv3 + bn3 and the shortcut conv + bn share the output tile: one GEMM over the
            # concatenated K = [conv2 output channels | block input channels (strided gather)], no
            # residual tensor is materialised (reference resnet3D.py:135-142 + :176-185)
            o = self.conv_bn(x, blk.conv1, blk.bn1, relu=True, label=name + ".conv1")
            o = self.conv_bn(o, blk.conv2, blk.bn2, relu=True, label=name + ".conv2")
            pk = self.pack_dual(blk.conv3, blk.bn3, blk.downsample[0], blk.downsample[1])
            o = self.conv(o, pk, (1, 1, 1), (0, 0, 0), relu=True, x2=x, x2_stride=_geom(blk.downsample[0])[1], y=out,
                          label=name + ".conv3+downsample")
            if blk.has_nl:
                o = self.nonlocal_block(o, blk.nonlocalblock, name + ".nonlocalblock")
            return o
        if blk.has_shortcut and arch.shortcut == "B":
            res = self.conv_bn(x, blk.downsample[0], blk.downsample[1], label=name + ".downsample")
            kind = None
        elif blk.has_shortcut:
            res, kind = x, "padA"
        else:
            res, kind = x, None
        if arch.block in ("bottleneck", "resnext", "wide"):
            o = self.conv_bn(x, blk.conv1, blk.bn1, relu=True, label=name + ".conv1")
            tail = None
            if (kind is None and isinstance(blk.conv2, (nn.Conv3d, nn.Conv2d)) and isinstance(blk.conv3, (nn.Conv3d, nn.Conv2d))
                    and not getattr(blk.conv2, "tf_same", False)):
                # the bottleneck's tail conv2 -> bn2 -> relu -> conv3 -> bn3 -> += residual -> relu (resnet3D.py:129-142)
                # as one chained launch: conv2's output tile never leaves the workgroup
                k2, s2, p2 = _geom(blk.conv2)
                # conv_chain composes conv2's geometry with a UNIT-stride, unpadded pointwise tail: anything else keeps
                # the two launches (the reference's bottlenecks qualify, resnet3D.py:117-119; a user-edited block may not)
                plain_tail = _geom(blk.conv3) == ((1, 1, 1), (1, 1, 1), (0, 0, 0)) and not getattr(blk.conv3, "tf_same", False)
                tail = None if not plain_tail else self.conv_chain(o, self.pack(blk.conv2, blk.bn2), s2, p2, self.pack(blk.conv3, blk.bn3), relu1=True,
                                       relu2=True, res=res, label=name + ".conv2+conv3", y=out)
            first = len(self.steps)
            o2 = self.conv_bn(o, blk.conv2, blk.bn2, relu=True, label=name + ".conv2")
            o = self.conv_bn(o2, blk.conv3, blk.bn3, relu=True, res=res, res_kind=kind, res_stride=s,
                             label=name + ".conv3", y=out if tail is None else tail[0])
            if tail is not None:
                self.alt(tail[1], first, name + ".conv2+conv3")
        else:
            o = self.conv_bn(x, blk.conv1, blk.bn1, relu=True, label=name + ".conv1")
            o = self.conv_bn(o, blk.conv2, blk.bn2, relu=True, res=res, res_kind=kind, res_stride=s,
                             label=name + ".conv2", y=out)
        if blk.has_nl:
            o = self.nonlocal_block(o, blk.nonlocalblock, name + ".nonlocalblock")
        return o

    def bn_relu(self, x, bn, label):
        """Eval-mode BN -> ReLU as one HBM pass ahead of a conv (pre-activation blocks): the BN is folded to
        a per-channel affine by ptx_cbn_fold whenever the weights change."""
        f32 = dict(device=self.dev, dtype=torch.float32)
        sc, sh = torch.empty(x.C, **f32), torch.empty(x.C, **f32)
        self.keepalive += [sc, sh]
        lib, eps, C_, bn_ref = self.lib, float(bn.eps), x.C, self.ref(bn)

        def refresh():
            bn = self.get(bn_ref)
            ts = [t.contiguous() for t in (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var)]
            check(lib.ptx_cbn_fold(_ptr(ts[0]), _ptr(ts[1]), _ptr(ts[2]), _ptr(ts[3]), C.c_float(eps), _ptr(sc), _ptr(sh),
                                   1, C_, 0, 0, C_, 0, _stream()), "bn fold " + label)
        if torch.device(self.dev).type != "meta":
            self.refreshers.append(refresh)
        y = self.act(x.N, x.T, x.H, x.W, x.C)
        xp, yp, scp, shp = _ptr(x.t), _ptr(y.t), _ptr(sc), _ptr(sh)
        rows, ldx, ldy = x.N * x.T * x.H, x.ld, y.ld

        def step(st):
            # [N*T*H, W] rows: the kernel's (n, h, w) decomposition only matters for upsampling
            check(lib.ptx_affine_act_upsample(xp, yp, scp, shp, 0, 1, rows, x.W, C_, ldx, ldy, 1, 1, st), label)
        self.steps.append(_tag(step, "affine_act", 8 * x.N * x.S * x.C))
        return y

    def _block_preact(self, arch, blk, x, name):
        """pre_act_resnet3D.py:41-57 / :76-96: BN -> ReLU precede every conv, the residual joins un-activated.
        bn1 reads the block input (which the residual also needs): one affine pass; bn2 / bn3 follow a conv
        whose output nothing else reads: folded into that conv's filter, ReLU in its epilogue."""
        s = blk.stride
        if blk.has_shortcut and arch.shortcut == "B":
            res, kind = self.conv_bn(x, blk.downsample[0], blk.downsample[1], label=name + ".downsample"), None
        elif blk.has_shortcut:
            res, kind = x, "padA"
        else:
            res, kind = x, None
        a = self.bn_relu(x, blk.bn1, name + ".bn1")
        o = self.conv_bn(a, blk.conv1, blk.bn2, relu=True, label=name + ".conv1")
        if arch.block == "preact_bottleneck":
            o = self.conv_bn(o, blk.conv2, blk.bn3, relu=True, label=name + ".conv2")
            return self.conv_bn(o, blk.conv3, None, res=res, res_kind=kind, res_stride=s, label=name + ".conv3")
        return self.conv_bn(o, blk.conv2, None, res=res, res_kind=kind, res_stride=s, label=name + ".conv2")

    def _fuse_programs(self):
        """Replace every run of >= PTX_PROGRAM_MIN_STAGES consecutive plain fp32 ConvSteps with at most PTX_PROGRAM_MAX_M
        output rows by ONE ProgramStep (conv_program.hip).  A run ends at anything that is not such a conv (attention,
        pooling, chained pairs, fp16 / split-operand stages) and at a conv the library refuses (its message names the
        rule); the replaced ConvSteps stay inside the ProgramStep as its fallback and as the record of what it computes."""
        # PTX_PROGRAM: "0" (default) never build programs -- every measurement of round 5 has the launches ahead (configs 2 / 3 at
        # 8 clips: -3.7 % / -13 %; 1-4 clips: -7 % .. -24 %); "auto" build them and run whichever of {program,
        # its launches} the tuner measured faster (tuned table "prog:" keys); "1" / "force" always the program
        mode = os.environ.get("PTX_PROGRAM", "0")
        if mode == "0" or torch.device(self.dev).type != "cuda" or self.x3:
            return
        max_m = int(os.environ.get("PTX_PROGRAM_MAX_M", "4096"))
        min_n = int(os.environ.get("PTX_PROGRAM_MIN_STAGES", "2"))
        wgs = int(os.environ.get("PTX_PROGRAM_WGS", "2"))
        lib = self.lib
        tile_ids = {lib.ptx_conv_program_tile_name(i).decode(): i for i in range(lib.ptx_conv_program_num_tiles())}
        use_tuned = os.environ.get("PTX_PROGRAM_TILES", "auto") == "tuned"

        def eligible(st):
            if not isinstance(st, ConvStep) or st.fused or getattr(st, "body", None) is not None:
                return False
            d = st.d
            ok_flags = PTX_EPI_RELU | PTX_EPI_RES_ADD | PTX_SPLITK_FUSED
            return (d.flags & ~ok_flags) == 0 and d.groups <= 1 and d.N * d.To * d.Ho * d.Wo <= max_m

        def make(run):
            import hashlib
            key = hashlib.sha1(json.dumps([list(c.d.key()) for c in run]).encode()).hexdigest()[:20]
            if mode == "auto" and prog_lookup(key) is False:
                return False                 # measured before: the launches win -- no program, no workspace
            arr = (ConvStage * len(run))()
            for i, st in enumerate(run):
                e = arr[i]
                C.memmove(C.byref(e.desc), C.byref(st.d), C.sizeof(ConvDesc))
                e.x, e.x2, e.w_packed, e.bias, e.res, e.y = st.x, st.x2, st.w, st.b, st.res, st.y
                name = lib.ptx_conv3d_config_name(st.cfg).decode()
                e.tile = tile_ids.get(name, -1) if use_tuned else -1
                e.split_k = st.split if (use_tuned and e.tile >= 0) else 0
            info = ConvProgramInfo()
            if lib.ptx_conv_program_plan(arr, len(run), C.byref(info)) != 0:
                return None
            ps = ProgramStep()
            ps.ws = torch.zeros((int(info.workspace_bytes) + 255) // 4 + 64, device=self.dev, dtype=torch.float32)
            off = (-ps.ws.data_ptr()) % 256 // 4
            ps.ws = ps.ws[off:]
            host = (C.c_char * int(info.image_bytes))()
            check(lib.ptx_conv_program_build(arr, len(run), _ptr(ps.ws), int(info.workspace_bytes), host, int(info.image_bytes),
                                             C.byref(info)), "conv program build")
            ps.image = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(self.dev)
            ps.info, ps.stages, ps.convs, ps.plan, ps.wgs = info, arr, list(run), self, wgs
            ps.label = "%s..%s" % (run[0].label, run[-1].label)
            ps.macs, ps.hbm_bytes = sum(c.macs for c in run), 0
            ps.kernel = "conv_program/%dstages/%dtiles" % (len(run), info.total_items)
            ps.key = key
            known = prog_lookup(ps.key)
            ps.use_program = mode in ("1", "force") or (known is True)
            return ps

        out, run = [], []

        def flush():
            # the library may refuse a run as a whole (buffer reuse, a foreign row layout): retry without its first conv
            # until something sticks or the run is too short
            r = list(run)
            del run[:]
            while len(r) >= min_n:
                ps = make(r)
                if ps is False:
                    break
                if ps is not None:
                    out.append(ps)
                    self.program_steps.append(ps)
                    return
                out.append(r.pop(0))
            out.extend(r)

        for st in self.steps:
            if eligible(st):
                run.append(st)
            else:
                flush()
                out.append(st)
        flush()
        self.steps = out

    # ---------------------------------------------------------------- running
    def run_head(self, engine, model):
        """feature map -> logits: the default global-average-pool + classifier, or the plan's own tail."""
        if self.head is not None:
            return self.head(engine, model)
        if getattr(self, "head_error", None):
            raise PtxError(self.head_error)
        f = self.feat
        if self.bf16:
            check(self.lib.ptx_global_avgpool_bf16(_ptr(f.t), _ptr(self.pooled), f.N, f.C, f.S, f.ld, _stream()),
                  "ptx_global_avgpool_bf16")
            return engine._head_bf16(model, self.pooled, self)
        check(self.lib.ptx_global_avgpool(_ptr(f.t), _ptr(self.pooled), f.N, f.C, f.S, f.ld, 0, _stream()),
              "ptx_global_avgpool")
        out = engine._head(model, _ptr(self.pooled), f.N, f.C, self.dev)
        if out is None:     # user-supplied head module (Identity, Dropout, custom nn.Module): theirs to run
            out = model.head_module(self.pooled.clone())
        return out

    def all_convs(self):
        """Every convolution launch of the plan in execution order: the implicit-GEMM steps (`conv_steps`, what the
        autotuner owns) and the direct stem kernels."""
        out = []
        for s in self.steps:
            for t in (s.active() if isinstance(s, (AltStep, ProgramStep)) else [s]):
                if isinstance(t, (ConvStep, ChainStep, StemStep, StemF32Step, PatchConvStep, ProgramStep)):
                    out.append(t)
        return out

    def refresh_weights(self, model):
        """Re-pack every filter (and rebuild the weight-derived tables) from `model`'s current tensors."""
        self.bind(model)
        keep = []
        for p in self.packs:
            keep.append(p.refresh())
        for fn in self.refreshers:
            fn()
        if self.bf16 and getattr(self, "head32", None) is not None:
            self.head32_refresh(model)
        return keep

    def head32_refresh(self, model):
        """bf16 plans: the fp32 copy of the classifier (`last_linear` / `fc`) the fp32 ptx_linear_fwd reads, made when the
        plan is packed and refreshed with it (in place: a captured graph keeps reading the same buffers)."""
        head = model.head_module
        if not isinstance(head, nn.Linear):
            self.head32 = None
            return None
        key = (id(head), head.weight.data_ptr(), head.weight._version,
               None if head.bias is None else (head.bias.data_ptr(), head.bias._version))
        cur = getattr(self, "head32", None)
        if cur is not None and cur[1].shape == head.weight.shape and (cur[2] is None) == (head.bias is None):
            cur[1].copy_(head.weight.detach())
            if head.bias is not None:
                cur[2].copy_(head.bias.detach())
            self.head32 = (key, cur[1], cur[2])
        else:
            self.head32 = (key, head.weight.detach().float().contiguous(),
                           head.bias.detach().float().contiguous() if head.bias is not None else None)
        return self.head32

    @contextlib.contextmanager
    def exclusive(self):
        """A plan owns ONE set of activation buffers: concurrent callers (host threads on their own HIP
        streams, e.g. DataParallel-style workers sharing a device) are serialised -- on the host by a lock,
        on the device by making this run wait for the event that closed the previous one."""
        if torch.cuda.is_current_stream_capturing():
            yield
            return
        with self._run_lock:
            st = torch.cuda.current_stream()
            if self._last_done is not None and self._last_stream != st.cuda_stream:
                st.wait_event(self._last_done)
            try:
                yield
            finally:
                if self._last_done is None:
                    self._last_done = torch.cuda.Event()
                self._last_done.record(st)
                self._last_stream = st.cuda_stream

    def run_features(self, x):
        self.in_ptr = _ptr(x)
        st = _stream()
        for s in self.steps:
            s(st)
        return self.feat


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


def _foldable(conv, x):
    """Small-Cin first conv reading the raw NCDHW input: fold kW into the channel axis."""
    return isinstance(x, RawInput)


def _dense16(x):
    """Contiguous and 16-byte aligned: the kernels read the caller's tensor in 16-byte pieces (a contiguous view whose storage
    offset is not a multiple of 4 floats gets one aligned copy)."""
    x = x.contiguous()
    return x.clone() if x.data_ptr() % 16 else x


def _is_replica(model):
    return bool(getattr(model, "_is_replica", False))


def _first_weight(model):
    """A weight tensor of the model: works for DataParallel replicas too, whose `parameters()` is empty
    (replicate() stores the broadcast copies as plain attributes)."""
    for m in model.modules():
        w = getattr(m, "weight", None)
        if isinstance(w, torch.Tensor):
            return w
    raise PtxError("model has no weights")


class Engine:
    """Per-model executor, shared by the model and its torch.nn.DataParallel replicas (a replica's __dict__
    is a copy of the model's, so `_engine` is the same object).  Plans -- packed filters, activation buffers,
    launch lists -- are keyed by (input shape, device); whether the packed filters are current is decided from
    the OWNER model's parameters (replicas are rebuilt on every forward and carry fresh broadcast copies of
    the same values), and a re-pack reads the tensors of whichever model / replica is executing on that
    device."""

    def __init__(self, model=None):
        self._plans = collections.OrderedDict()
        # a plan owns every activation buffer of one (input shape, device): serving with many distinct
        # shapes must not grow without bound -- least-recently-used plans are dropped beyond this count
        self.max_plans = int(os.environ.get("PTX_MAX_PLANS", "16"))
        self._lock = threading.RLock()
        self._sig = {}
        self._owner = weakref.ref(model) if model is not None else None
        self._epoch = 0                  # bumped by invalidate(): load_state_dict / .to() / refresh()
        self._tensors = None             # (epoch, flat list of the owner's parameters and buffers)
        self.plan_builds = 0             # diagnostics: plans compiled / filter re-packs so far
        self.weight_refreshes = 0
        self.last_profile = None         # calibration record of the last profile_steps() call
        # How a forward decides whether the packed (BN-folded) filters are still current:
        #   True / "version"  (default) compare (data_ptr, _version) of every parameter and buffer of the owner
        #                     model -- catches load_state_dict, optimizer-style in-place updates, copy_();
        #                     ~50 us of host time per forward for ResNet3D-50 (the tensor list is cached)
        #   "checksum"        additionally compare a device-side checksum of the parameter bytes
        #                     (ptx_checksum_f32): also catches edits through `.data`, which bypass the version
        #                     counters (`p.data.fill_(1)` leaves p._version unchanged); one extra launch + a
        #                     device->host sync per forward
        #   False             O(1): only invalidate() / model.refresh() / load_state_dict / .to() re-pack
        self.check_weights = os.environ.get("PTX_CHECK_WEIGHTS", "version")
        if self.check_weights in ("0", "false", "False"):
            self.check_weights = False
        # tile configurations of conv problems that are not in the tuned table are timed (HIP events,
        # < 1 s per network) the first time a plan runs; PTX_AUTOTUNE=0 keeps the heuristic defaults
        self.auto_tune = os.environ.get("PTX_AUTOTUNE", "1") != "0"
        # opt-in hipGraph replay of forward(): the whole plan (+ pool + classifier) is captured once per
        # (shape, device) and replayed -- one host call instead of ~90 launches.  Pays off for
        # launch-bound shapes (small clips / batch 1); neutral at config-2 size.
        self.use_graph = os.environ.get("PTX_GRAPH", "0") == "1"
        # Arithmetic of the dense convolutions:
        #   "fp32"  (default) fp32 operands on v_mfma_f32_32x32x2_f32 -- the reference's own arithmetic;
        #   "x3"    fp32-accurate split operands on the fp16 matrix cores (PTX_F16X3_OPERANDS: a = hi + lo halfs,
        #           a.b = hi.hi + hi.lo + lo.hi, fp32 accumulate): same |dlogits| vs the CPU reference as "fp32"
        #           (1e-5 class), 3 / 16 of its matrix-core time.  Activations, epilogues and every other kernel stay
        #           fp32.  Operand magnitudes must stay inside the half range (|v| < 65504).
        # Changing it drops the compiled plans (set it before the first forward, or call invalidate()).
        # It governs float32 models only: a model whose parameters are bfloat16 runs the bf16 plans (bf16 operands on the
        # bf16 matrix cores, fp32 accumulate, bf16 activations) whatever it is set to (INTEGRATION.md, bf16 inference).
        self._precision = os.environ.get("PTX_PRECISION", "fp32")
        # Opt-in autograd routing (eager.wanted): with grad mode on and trainable parameters, eval-mode calls run the
        # zoo's torch.nn children and return a differentiable output, as the reference does (frozen-BN fine-tuning).
        # Off by default: every nn.Parameter requires grad, so plain inference without torch.no_grad() would leave
        # the HIP engine.
        self.autograd = os.environ.get("PTX_AUTOGRAD", "0") == "1"
        # Clip lanes (forward() only): the batch is cut into `lanes` equal contiguous slices, each slice runs through
        # ITS OWN plan (own activation buffers and split-K workspace) on its own HIP stream, and the logits are concatenated
        # in clip order.  The slices are independent chains of launches, so one lane's launch gaps, tile tails and
        # HBM-bound passes overlap the other's matrix-bound kernels: +2.0-2.5 % on configs 2 and 4 with two lanes on MI355X,
        # nothing on config 3, a loss with four.
        #   "auto" (default, round 6)  what the tuned table holds for this (architecture, input shape): 2 where
        #                              Engine.autotune measured two lanes >= 1 % faster than one ("lanes:" keys, the same
        #                              kind of measured accept rule as the chained launches' "alt:" keys), else 1;
        #   1 .. 8                     forced.
        # Per-clip results with n lanes are those of the slice-sized batch (another tile / split-K choice than the full
        # batch: same 1e-5 class, not the same bits).
        self._lanes = "auto"
        self._lane_streams = {}          # device index -> side streams of lanes 1 .. n-1 (lane 0 runs on the caller's stream)
        env = os.environ.get("PTX_LANES", "auto")
        self.lanes = "auto" if env == "auto" else int(env)

    @property
    def lanes(self):
        return self._lanes

    @lanes.setter
    def lanes(self, value):
        if value == "auto" and isinstance(value, str):
            self._lanes = "auto"
            return
        if not isinstance(value, int) or isinstance(value, bool) or not 1 <= value <= 8:
            raise PtxError("Engine.lanes must be \"auto\" or an integer in 1..8 (got %r)" % (value,))
        self._lanes = value

    def lanes_for(self, batch, model=None, shape=None):
        """Lanes forward() uses for a batch of this size: `lanes` ("auto": the tuned table's entry for this model and input
        shape, 1 without one) when it cuts the batch into equal non-empty slices and the hipGraph replay is off, else 1
        (the plain single-plan path -- never an error)."""
        n = self._lanes
        if n == "auto":
            n = 1
            if model is not None and shape is not None and not self.use_graph:
                n = lanes_lookup(lanes_key(model, shape, self.precision_of(model))) or 1
        return n if (n > 1 and not self.use_graph and batch >= n and batch % n == 0) else 1

    def tune_lanes(self, model, x, iters=8, verbose=False):
        """Measure forward(model, x) with one and with two clip lanes (each on its own tuned plans) and record the verdict in
        the tuned table: two lanes must win by 1 % (the lanes double the activation buffers; config 2 gains 1.4-2.2 % across the
        boxes of rounds 5 and 6, which a 1.5 % bar turned into a coin flip).  Returns the lanes kept."""
        x = _dense16(x)
        key = lanes_key(model, x.shape, self.precision_of(model))
        if self.use_graph or x.shape[0] < 2 or x.shape[0] % 2:
            return 1
        keep = self._lanes
        ms = {1: [], 2: []}
        try:
            for n in (1, 2):                     # plans compiled, tiles tuned, clocks up
                self._lanes = n
                for _ in range(3):
                    self.forward(model, x)
            # interleaved rounds (1, 2, 1, 2, ...): clock / thermal drift hits both arms alike; the verdict is the MEDIAN round
            for _ in range(5):
                for n in (1, 2):
                    self._lanes = n
                    torch.cuda.synchronize(x.device)
                    t0 = time.perf_counter()
                    for _ in range(iters):
                        self.forward(model, x)
                    torch.cuda.synchronize(x.device)
                    ms[n].append(1e3 * (time.perf_counter() - t0) / iters)
        finally:
            self._lanes = keep
        ms = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
        best = 2 if ms[2] < 0.99 * ms[1] else 1
        lanes_store(key, best)
        if verbose:
            print("tune clip lanes %s: 1 lane %.3f ms | 2 lanes %.3f ms -> %d" % (key, ms[1], ms[2], best))
        return best

    @property
    def precision(self):
        return self._precision

    def precision_of(self, model):
        """The arithmetic a forward of `model` runs: "bf16" for a model whose parameters are bfloat16 (whatever
        `precision` says), else `precision` ("fp32" / "x3")."""
        return "bf16" if model is not None and model_precision(model) == "bf16" else self._precision

    @precision.setter
    def precision(self, value):
        if value not in ("fp32", "x3"):
            raise PtxError("Engine.precision must be 'fp32' or 'x3' (got %r)" % (value,))
        if value != self._precision:
            self._precision = value
            self.invalidate()

    def __deepcopy__(self, memo):
        return Engine()

    def __getstate__(self):
        return {}

    def __setstate__(self, s):
        self.__init__()

    def invalidate(self):
        with self._lock:
            self._plans.clear()
            self._sig.clear()
            self._epoch += 1
            self._tensors = None

    def owner(self, model):
        """The model whose parameters define weight identity: the constructed model itself; for a
        DataParallel replica the model it was replicated from."""
        if not _is_replica(model):
            if self._owner is None or self._owner() is not model:
                self._owner = weakref.ref(model)      # deep copies / unpickled models bind on first use
                self._tensors = None
            return model
        own = self._owner() if self._owner is not None else None
        return own if own is not None else model

    def dry_plan(self, model, shape):
        """Compile a plan on the 'meta' device: every descriptor, tile choice and buffer shape is
        produced, nothing is allocated or launched.  Host-logic tests use this without a GPU."""
        return Plan(self, model, shape, torch.device("meta"))

    # ------------------------------------------------------------------------------------
    @staticmethod
    def _validate(model, x, dims):
        if model.training:
            raise PtxError("pretorched-x_amd is a forward-only (inference) engine: call model.eval() first; "
                           "there is no training-mode / autograd path")
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise PtxError("input must be a CUDA (ROCm) tensor -- there is no CPU fallback in this package")
        p = _first_weight(model)
        if p.dtype == torch.bfloat16:       # bf16 model: bf16 in, bf16 out (dtype mismatches raise, as in torch)
            if x.dtype != torch.bfloat16:
                raise PtxError("the model's parameters are bfloat16: the input must be bfloat16 too (got %s)" % x.dtype)
        elif x.dtype != torch.float32:
            raise PtxError("input must be float32 (got %s)" % x.dtype)
        want = 4 if dims == 2 else 5
        if x.dim() != want:
            raise PtxError("expected a %d-D input, got shape %s" % (want, tuple(x.shape)))
        if p.device != x.device:
            raise PtxError("input on %s but parameters on %s" % (x.device, p.device))

    def _owner_tensors(self, root):
        """Flat list of the owner's parameters and buffers, cached until the next invalidate() OR the next parameter /
        buffer / sub-module registration anywhere in the process (`_struct_epoch`: a trunk Parameter or module replaced
        by assignment gives the list new tensors, whose data_ptr then differs from the packed filters' signature).
        Walking the module tree costs ~0.4 ms per call for ResNet3D-50, reading 480 version counters ~50 us."""
        cached = self._tensors
        # without torch's global registration hooks (older torch) the tree is walked on every forward
        epoch = (self._epoch, _struct_epoch[0]) if _STRUCT_HOOKS else None
        if cached is None or epoch is None or cached[0] != epoch or cached[1] is not root:
            ts = list(root.parameters()) + list(root.buffers())
            if not ts and _is_replica(root):             # an orphan replica: its broadcast copies
                ts = [t for m in root.modules() for t in getattr(m, "_former_parameters", {}).values()]
                ts += list(root.buffers())
            cached = self._tensors = (epoch, root, ts)
        return cached[2]

    def _signature(self, model):
        root = self.owner(model)
        ts = self._owner_tensors(root)
        sig = tuple((t.data_ptr(), t._version) for t in ts)
        if self.check_weights == "checksum":
            sig = (sig, self._checksum(ts))
        return sig

    def _checksum(self, ts):
        """Order-independent 64-bit sum of the bit patterns of every floating-point tensor -- fp32 (ptx_checksum_f32) and
        16-bit (bf16 / fp16: ptx_checksum_b16) -- computed on the device the tensors live on; synchronises on the result."""
        fl = [t for t in ts if t.is_cuda and t.dtype == torch.float32 and t.numel() > 0]
        hl = [t for t in ts if t.is_cuda and t.dtype in (torch.bfloat16, torch.float16) and t.numel() > 0]
        if not fl and not hl:
            return 0
        dev = (fl or hl)[0].device
        with torch.cuda.device(dev):
            out = torch.zeros(1, dtype=torch.int64, device=dev)
            for lst, fn in ((fl, "ptx_checksum_f32"), (hl, "ptx_checksum_b16")):
                if lst:
                    tab = torch.tensor([[t.data_ptr(), t.numel()] for t in lst], dtype=torch.int64).to(dev)
                    check(getattr(_lib.lib(), fn)(C.c_void_p(tab.data_ptr()), len(lst), C.c_void_p(out.data_ptr()), _stream()), fn)
            return int(out.item())

    def plan_for(self, model, x, shape=None, norm=None, lane=0):
        """shape / norm: the NCDHW view and NormDesc of a uint8-frames input (forward_frames).  lane: which of the
        Engine.lanes concurrent slices this plan serves -- lanes of one shape are separate plans (separate buffers)."""
        shape = tuple(x.shape) if shape is None else tuple(shape)
        nkey = None if norm is None else (tuple(norm.mean), tuple(norm.std), norm.swap_rb, norm.to_255)
        key = (shape, x.device.index, nkey) + ((lane,) if lane else ())
        if model_precision(model) == "bf16":
            key += ("bf16",)
        with self._lock:
            plan = self._plans.get(key)
            fresh = plan is None
            if fresh:
                plan = Plan(self, model, shape, x.device, norm)
                self.plan_builds += 1
                self._plans[key] = plan
                while len(self._plans) > max(1, self.max_plans):
                    old, _ = self._plans.popitem(last=False)         # LRU eviction frees the plan's buffers
                    self._sig.pop(old, None)
            else:
                self._plans.move_to_end(key)
            if fresh or self.check_weights:
                sig = self._signature(model)
                if fresh or self._sig.get(key) != sig:
                    # the re-pack writes the filters other host threads' runs may still be reading
                    with torch.cuda.device(x.device), plan.exclusive():
                        plan.refresh_weights(model)
                    self.weight_refreshes += 1
                    self._sig[key] = sig
            return plan

    # ------------------------------------------------------------------------------------
    def features(self, model, x):
        """NCDHW in -> NCDHW feature map out (contiguous), like the reference's `features`."""
        self._validate(model, x, model.arch.dims)
        big = self._chunked(self.features, model, x)
        if big is not None:
            return big
        x = _dense16(x)
        with torch.cuda.device(x.device):
            plan = self.plan_for(model, x)
            self._maybe_tune(model, plan, x)
            with plan.exclusive():
                plan.bind(model)
                f = plan.run_features(x)
                dt = torch.bfloat16 if f.bf16 else torch.float32
                if model.arch.dims == 2:
                    out = torch.empty((f.N, f.C, f.H, f.W), device=x.device, dtype=dt)
                else:
                    out = torch.empty((f.N, f.C, f.T, f.H, f.W), device=x.device, dtype=dt)
                if f.bf16:
                    check(_lib.lib().ptx_ndhwc_to_ncdhw_bf16(_ptr(f.t), _ptr(out), f.N, f.C, f.S, f.ld, _stream()),
                          "ptx_ndhwc_to_ncdhw_bf16")
                else:
                    check(_lib.lib().ptx_ndhwc_to_ncdhw(_ptr(f.t), _ptr(out), f.N, f.C, f.S, f.ld, _stream()),
                          "ptx_ndhwc_to_ncdhw")
        return out

    def _head(self, model, pooled_ptr, N, Cf, dev):
        head = model.head_module
        pooled = None
        if isinstance(head, nn.Linear) and head.weight.is_cuda and head.weight.dtype == torch.float32:
            out = torch.empty((N, head.out_features), device=dev, dtype=torch.float32)
            w = head.weight.detach().contiguous()
            b = head.bias.detach().contiguous() if head.bias is not None else None
            check(_lib.lib().ptx_linear_fwd(pooled_ptr, _ptr(w), _ptr(b) if b is not None else C.c_void_p(0),
                                            _ptr(out), N, Cf, head.out_features, Cf, head.out_features, 0,
                                            _stream()), "ptx_linear_fwd")
            return out
        return None

    def _head_bf16(self, model, pooled, plan=None):
        """bf16 models: the classifier runs as the fp32 ptx_linear_fwd on the fp32 pooled vector with an fp32 copy of
        `last_linear` / `fc` (the plan's, refreshed with its filters); the logits are rounded to bf16 once.  A user-supplied
        head module gets the pooled vector as bf16."""
        N, Cf = pooled.shape
        dev = pooled.device
        head = model.head_module
        if isinstance(head, nn.Linear) and head.weight.is_cuda and head.weight.dtype == torch.bfloat16:
            holder = plan if plan is not None else self
            cur = getattr(holder, "head32", None)
            key = (id(head), head.weight.data_ptr(), head.weight._version,
                   None if head.bias is None else (head.bias.data_ptr(), head.bias._version))
            if cur is None or cur[0] != key:
                cur = Plan.head32_refresh(holder, model)
            w32, b32 = cur[1], cur[2]
            out32 = torch.empty((N, head.out_features), device=dev, dtype=torch.float32)
            check(_lib.lib().ptx_linear_fwd(_ptr(pooled), _ptr(w32), _ptr(b32) if b32 is not None else C.c_void_p(0),
                                            _ptr(out32), N, Cf, head.out_features, Cf, head.out_features, 0, _stream()),
                  "ptx_linear_fwd")
            out = torch.empty((N, head.out_features), device=dev, dtype=torch.bfloat16)
            check(_lib.lib().ptx_f32_to_bf16(_ptr(out32), _ptr(out), out32.numel(), _stream()), "ptx_f32_to_bf16")
            return out
        p16 = torch.empty((N, Cf), device=dev, dtype=torch.bfloat16)
        check(_lib.lib().ptx_f32_to_bf16(_ptr(pooled), _ptr(p16), pooled.numel(), _stream()), "ptx_f32_to_bf16")
        return head(p16)       # user-supplied head module (Identity, custom nn.Module): theirs to run

    def logits(self, model, feats):
        """NCDHW feature map -> [N, classes]: global average pool + `last_linear` read at call time
        (users replace it with another Linear or an Identity, reference README "last_linear")."""
        self._validate(model, feats, model.arch.dims)
        if feats.dtype == torch.bfloat16:
            # bf16: NCDHW -> channels-last (ptx_ncdhw_to_ndhwc_bf16), then the forward's own pool kernel, so
            # logits(features(x)) has forward(x)'s bits
            feats = _dense16(feats)
            N, Cf = feats.shape[0], feats.shape[1]
            S = feats.numel() // (N * Cf)
            with torch.cuda.device(feats.device):
                ld = (Cf + 7) // 8 * 8
                cl = torch.empty((N, S, ld), device=feats.device, dtype=torch.bfloat16)
                check(_lib.lib().ptx_ncdhw_to_ndhwc_bf16(_ptr(feats), _ptr(cl), N, Cf, S, ld, _stream()), "ptx_ncdhw_to_ndhwc_bf16")
                pooled = torch.empty((N, Cf), device=feats.device, dtype=torch.float32)
                check(_lib.lib().ptx_global_avgpool_bf16(_ptr(cl), _ptr(pooled), N, Cf, S, ld, _stream()), "ptx_global_avgpool_bf16")
                return self._head_bf16(model, pooled)
        feats = feats.contiguous()
        N, Cf = feats.shape[0], feats.shape[1]
        S = feats.numel() // (N * Cf)
        with torch.cuda.device(feats.device):
            pooled = torch.empty((N, Cf), device=feats.device, dtype=torch.float32)
            check(_lib.lib().ptx_global_avgpool(_ptr(feats), _ptr(pooled), N, Cf, S, Cf, 1, _stream()),
                  "ptx_global_avgpool")
            out = self._head(model, _ptr(pooled), N, Cf, feats.device)
            if out is None:     # user-supplied head module (Identity, custom nn.Module): theirs to run
                out = model.head_module(pooled)
        return out

    LIMIT_BYTES = (1 << 31) - (1 << 20)      # libptx_amd uses 32-bit buffer offsets: < 2 GiB per tensor

    def max_batch(self, model, sample_shape):
        """Largest batch whose biggest plan tensor stays under the 2 GiB per-launch limit."""
        one = Plan(self, model, (1,) + tuple(sample_shape), torch.device("meta"))
        per_clip = max(a.t.numel() * a.t.element_size() for a in one.acts)
        return max(1, int(self.LIMIT_BYTES // per_clip))

    def _chunked(self, fn, model, x):
        """Run `fn(model, chunk)` over batch slices that respect the per-launch size limit."""
        key = ("maxb", tuple(x.shape[1:]))
        with self._lock:
            mb = self._sig.get(key)
            if mb is None:
                mb = self._sig[key] = self.max_batch(model, x.shape[1:])
        if x.shape[0] <= mb:
            return None
        n_chunks = -(-x.shape[0] // mb)
        size = -(-x.shape[0] // n_chunks)
        return torch.cat([fn(model, x[i:i + size]) for i in range(0, x.shape[0], size)], 0)

    def _maybe_tune(self, model, plan, x):
        """First use of a plan: time the tile configurations of conv problems the tuned table does not know.
        Runs under the plan's exclusive lock (the tuner relaunches convs into the plan's buffers and edits
        the steps' tile choices), and `plan.tuned` is set only when it is done, so a second thread arriving
        meanwhile waits instead of running a half-tuned plan."""
        if not self.auto_tune or plan.tuned:
            return
        with plan.exclusive():
            if plan.tuned:
                return
            if os.environ.get("PTX_RETUNE") == "1":          # re-time EVERY problem (new tiles in the build): tuning sessions
                self._autotune(model, x, iters=2, only_untuned=False, plan=plan)
                plan.tuned = True
                return
            if any(tuned_lookup(json.dumps(s.d.key()), _flags_kind(s.d.flags)) is None
                   or (getattr(s, "body_ok", ()) and body_lookup(json.dumps(s.d.key())) is None)
                   for s in plan.conv_steps) or any(chain_lookup(s.key) is None or (getattr(s, "body_ok", ()) and body_lookup(s.key) is None)
                                                    for s in plan.chain_steps) \
                    or any(alt_lookup(a.key) is None for a in plan.alt_steps) \
                    or (os.environ.get("PTX_PROGRAM", "0") == "auto" and any(prog_lookup(p.key) is None for p in plan.program_steps)):
                self._autotune(model, x, iters=2, only_untuned=True, plan=plan)
            plan.tuned = True

    def _forward_graph(self, model, plan, x):
        """Capture (once) and replay forward() as a hipGraph.  The input is staged into a static
        buffer; the logits are copied out of the graph's private pool."""
        head = model.head_module
        key = (id(head), head.weight.data_ptr() if isinstance(head, nn.Linear) else 0)
        g = plan.graph
        if g is None or g["key"] != key:
            static_x = torch.empty_like(x)
            static_x.copy_(x)
            self._forward_eager(model, plan, static_x)            # warm-up: everything allocated / tuned
            torch.cuda.synchronize(x.device)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_out = self._forward_eager(model, plan, static_x)
            g = plan.graph = dict(key=key, graph=graph, x=static_x, out=static_out)
        g["x"].copy_(x)
        g["graph"].replay()
        return g["out"].clone()

    def _forward_eager(self, model, plan, x):
        with plan.exclusive():
            plan.bind(model)
            plan.run_features(x)
            out = plan.run_head(self, model)
            # conv programs (experimental, PTX_PROGRAM=1 / force / auto): a dependency wait that ran out of polls leaves its
            # stages partially written and only sets the program's error word -- read it before the logits are handed out
            # (one stream synchronisation per forward, paid by the opt-in mode only; PTX_PROGRAM_CHECK=0 skips it)
            if getattr(plan, "program_steps", None) and os.environ.get("PTX_PROGRAM_CHECK", "1") != "0":
                for ps in plan.program_steps:
                    if ps.use_program:
                        err = ps.error()
                        if err is not None:
                            raise PtxError("%s: the conv program stopped with error %s (code, waiting stage, queue index, "
                                           "producer stage): its outputs are incomplete" % (ps.label, err))
            return out

    def forward(self, model, x):
        """features -> logits without leaving channels-last."""
        self._validate(model, x, model.arch.dims)
        big = self._chunked(self.forward, model, x)
        if big is not None:
            return big
        x = _dense16(x)
        with torch.cuda.device(x.device):
            n = self.lanes_for(x.shape[0], model, x.shape)
            if n > 1:
                return self._forward_lanes(model, x, n)
            plan = self.plan_for(model, x)
            self._maybe_tune(model, plan, x)
            if self.use_graph:
                return self._forward_graph(model, plan, x)
            out = self._forward_eager(model, plan, x)
        return out

    def lane_plans(self, model, x):
        """The plans forward(model, x) runs, lane 0 first (one plan unless Engine.lanes cuts this batch)."""
        x = _dense16(x)
        n = self.lanes_for(x.shape[0], model, x.shape)
        per = x.shape[0] // n
        plans = []
        with torch.cuda.device(x.device):
            for i in range(n):
                part = _dense16(x[i * per:(i + 1) * per])
                plans.append(self.plan_for(model, part, lane=i))
                self._maybe_tune(model, plans[i], part)
        return plans

    def _forward_lanes(self, model, x, n):
        """forward() over `n` clip lanes: slice i of the batch on stream i (lane 0 on the caller's stream, the others on the
        engine's side streams, which first wait for the caller's stream -- the input is ready there -- and which the caller's
        stream waits for before the logits are concatenated).  Every lane is an ordinary eager forward of its own plan."""
        dev = x.device
        cur = torch.cuda.current_stream(dev)
        side = self._lane_streams.get(dev.index)
        if side is None or len(side) < n - 1:
            side = self._lane_streams[dev.index] = [torch.cuda.Stream(dev) for _ in range(n - 1)]
        per = x.shape[0] // n
        parts = [_dense16(x[i * per:(i + 1) * per]) for i in range(n)]
        plans = []
        for i in range(n):
            # first use: lane 0 is compiled and times what the tuned table lacks BEFORE the next lane is compiled -- a plan
            # picks its tiles at compile time, so every lane ends up on the same (tuned) tiles and computes the same bits
            plans.append(self.plan_for(model, parts[i], lane=i))
            self._maybe_tune(model, plans[i], parts[i])
        ready = cur.record_event()
        outs = [None] * n
        for i in range(1, n):
            st = side[i - 1]
            st.wait_event(ready)
            with torch.cuda.stream(st):
                outs[i] = self._forward_eager(model, plans[i], parts[i])
        outs[0] = self._forward_eager(model, plans[0], parts[0])
        for i in range(1, n):
            cur.wait_stream(side[i - 1])
        if not all(torch.is_tensor(o) for o in outs):
            raise PtxError("Engine.lanes: the model's head must return one tensor per call (batch on dim 0) to be concatenated")
        for o in outs[1:]:
            o.record_stream(cur)                 # allocated under a side stream, consumed (and freed) under the caller's
        return torch.cat(outs, 0)

    # ------------------------------------------------------------------------------------
    def generate(self, model, z, y):
        """BigGAN-deep generator: z [B,dim_z], y [B,shared_dim] (= model.shared(labels)) -> images [B,3,R,R].  A generator
        whose parameters are bfloat16 takes bf16 z / y and returns bf16 images; otherwise everything is float32."""
        if model.training:
            raise PtxError("pretorched-x_amd is a forward-only (inference) engine: call model.eval() first")
        prec = model_precision(model)
        want = torch.bfloat16 if prec == "bf16" else torch.float32
        for t, d, nm in ((z, model.dim_z, "z"), (y, model.shared_dim, "y")):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != want:
                raise PtxError("generate: %s must be a %s CUDA tensor (no CPU fallback)%s" % (
                    nm, "bfloat16" if prec == "bf16" else "float32",
                    "; the generator's parameters are bfloat16" if prec == "bf16" else ""))
            if t.dim() != 2 or t.shape[1] != d:
                raise PtxError("generate: %s must be [B, %d], got %s" % (nm, d, tuple(t.shape)))
        if z.shape[0] != y.shape[0] or z.device != y.device:
            raise PtxError("generate: z and y must share batch size and device")
        z, y = z.contiguous(), y.contiguous()
        N = z.shape[0]
        key = ("maxb", ("biggan", prec))
        with self._lock:
            mb = self._sig.get(key)
            if mb is None:
                one = Plan(self, model, (1, model.dim_z), torch.device("meta"))
                mb = self._sig[key] = max(1, int(self.LIMIT_BYTES // max(a.t.numel() * a.t.element_size() for a in one.acts)))
        if N > mb:      # balanced chunks (64 -> 32 + 32, not 63 + 1): every chunk keeps the GEMMs' M large
            size = -(-N // (-(-N // mb)))
            starts = list(range(0, N, size))
            n = min(self._lanes, len(starts)) if (not self.use_graph and self._lanes != "auto") else 1
            if n > 1:
                # clip lanes (Engine.lanes): chunk k through plan k % n on stream k % n -- the chunks are
                # independent chains of launches and the generator mixes HBM-bound and matrix-bound kernels
                dev = z.device
                with torch.cuda.device(dev):
                    cur = torch.cuda.current_stream(dev)
                    side = self._lane_streams.get(dev.index)
                    if side is None or len(side) < n - 1:
                        side = self._lane_streams[dev.index] = [torch.cuda.Stream(dev) for _ in range(n - 1)]
                    ready = cur.record_event()
                    for st in side[:n - 1]:
                        st.wait_event(ready)
                    outs = []
                    for k, i in enumerate(starts):
                        lane = k % n
                        with torch.cuda.stream(cur if lane == 0 else side[lane - 1]):
                            outs.append(self._generate_one(model, z[i:i + size], y[i:i + size], lane))
                    for st in side[:n - 1]:
                        cur.wait_stream(st)
                    for k, o in enumerate(outs):
                        if k % n:
                            o.record_stream(cur)
                    return torch.cat(outs, 0)
            return torch.cat([self._generate_one(model, z[i:i + size], y[i:i + size]) for i in starts], 0)
        return self._generate_one(model, z, y)

    def _generate_one(self, model, z, y, lane=0):
        N = z.shape[0]
        with torch.cuda.device(z.device):
            plan = self.plan_for(model, z, lane=lane)
            plan.in_ptr2 = _ptr(y)
            self._maybe_tune(model, plan, z)
            with plan.exclusive():
                plan.bind(model)
                plan.in_ptr2 = _ptr(y)
                f = plan.run_features(z)
                if f.bf16:       # bf16 plans: the tanh conv wrote bf16, the layout pass keeps it
                    out = torch.empty((N, 3, f.H, f.W), device=z.device, dtype=torch.bfloat16)
                    check(_lib.lib().ptx_ndhwc_to_ncdhw_bf16(_ptr(f.t), _ptr(out), N, 3, f.H * f.W, f.ld, _stream()),
                          "ptx_ndhwc_to_ncdhw_bf16")
                else:
                    out = torch.empty((N, 3, f.H, f.W), device=z.device, dtype=torch.float32)
                    check(_lib.lib().ptx_ndhwc_to_ncdhw(_ptr(f.t), _ptr(out), N, 3, f.H * f.W, f.ld, _stream()),
                          "ptx_ndhwc_to_ncdhw")
        return out

    def forward_frames(self, model, frames, opts=None, transform=None):
        """Decoded uint8 frames [N,T,H,W,C] (NHWC for 2-D models) -> logits.  The tensor half of the
        reference's TransformImage (ToTensor, ToSpaceBGR, ToRange255, Normalize; transforms/utils.py:72-75)
        is fused into the stem's fold kernel: no fp32 NCDHW clip is ever materialised.  `opts`: anything
        with mean / std / input_space / input_range (default: the model's own pretrained settings).
        `transform`: a `transforms.TransformFrames(.., out="frames")` applied to the frames first (resize + crop of
        frames of any size on the device, utils.py:53-64); None: the frames already have the input size."""
        if transform is not None:
            from .transforms import apply_frames_transform
            frames = apply_frames_transform(transform, frames)
        opts = model if opts is None else opts
        get = (lambda k: opts[k]) if isinstance(opts, dict) else (lambda k: getattr(opts, k))
        try:
            norm = NormDesc.make(get("mean"), get("std"), get("input_space"), get("input_range"))
        except (AttributeError, KeyError):
            raise PtxError("forward_frames: no mean/std/input_space/input_range on the model (they exist only for "
                           "pretrained models, torchvision_models.py:162-166): pass opts=pretrained_settings[...]")
        if model.training:
            raise PtxError("pretorched-x_amd is a forward-only (inference) engine: call model.eval() first")
        if model_precision(model) != "fp32":
            raise PtxError("forward_frames runs float32 models only (this model's parameters are %s)" % model_precision(model))
        dims = model.arch.dims
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8:
            raise PtxError("forward_frames: frames must be a uint8 CUDA tensor")
        if frames.dim() != dims + 2:
            raise PtxError("forward_frames: expected %s, got shape %s" % (
                "[N,T,H,W,C]" if dims == 3 else "[N,H,W,C]", tuple(frames.shape)))
        if frames.shape[-1] != 3:
            raise PtxError("forward_frames: the stems take 3 channels")
        frames = frames.contiguous()
        if dims == 3:
            N, T, H, W, Cc = frames.shape
            shape = (N, Cc, T, H, W)
        else:
            N, H, W, Cc = frames.shape
            shape = (N, Cc, H, W)
        key = ("maxb", shape[1:])
        with self._lock:
            mb = self._sig.get(key)
            if mb is None:
                mb = self._sig[key] = self.max_batch(model, shape[1:])
        if N > mb:
            size = -(-N // (-(-N // mb)))
            return torch.cat([self.forward_frames(model, frames[i:i + size], opts) for i in range(0, N, size)], 0)
        with torch.cuda.device(frames.device):
            plan = self.plan_for(model, frames, shape=shape, norm=norm)
            self._maybe_tune(model, plan, frames)
            return self._forward_eager(model, plan, frames)

    def forward_views(self, model, video, opts=None, views=None, reduce="softmax", chunk=None):
        """Decoded uint8 video [N,Tv,H,W,3] (or [Tv,H,W,3]: one video) -> fp32 [N, classes]: the mean over `views`
        (a `transforms.SampleViews`: clips x crops, sampled on the device) of softmax(logits) (reduce="softmax"), of the
        logits ("logits"), or the logits of every view [N, V, classes] in the model's dtype (None).
        float32 models take the views as uint8 frames through forward_frames (views.out == "frames", `opts` as there);
        bfloat16 models take the normalised bf16 clip through forward() (views: out="tensor", dtype=torch.bfloat16).
        Views are produced `chunk` at a time (default `views_chunk(N, V, max_batch)`: as many as the per-launch size
        limit allows), so only one chunk of views exists at any time."""
        prec = model_precision(model)
        if prec not in ("fp32", "bf16"):
            raise PtxError("forward_views runs float32 and bfloat16 models (this model's parameters are %s)" % prec)
        check_views(views, model, "frames" if prec == "fp32" else "bf16")
        if getattr(model.arch, "dims", 3) != 3:
            raise PtxError("forward_views: a 2-D model takes images, not clips (TRN.forward_views runs a 2-D backbone on the "
                           "frames of a clip)")
        S = views.size
        key = ("maxb", (3, views.num_frames, S, S))
        with self._lock:
            mb = self._sig.get(key)
            if mb is None:
                mb = self._sig[key] = self.max_batch(model, key[1])
        if prec == "fp32":
            run = lambda frames: self.forward_frames(model, frames, opts)
        else:
            run = lambda clip: self.forward(model, clip)
        return run_views(video, views, run, mb, reduce, chunk)

    def autotune(self, model, x, iters=3, verbose=False, persist=False, only_untuned=False, plan=None):
        """Time every compiled tile configuration (x a few split-K factors) for each distinct conv
        problem of the plan with HIP events and keep the fastest.  Holds the plan's exclusive lock: the
        tuner relaunches convs into the plan's buffers."""
        own_plan = plan is not None
        if plan is None:
            self._validate(model, x, model.arch.dims)
            with torch.cuda.device(x.device):
                plan = self.plan_for(model, _dense16(x))
        with torch.cuda.device(x.device), plan.exclusive():
            plan = self._autotune(model, x, iters, verbose, persist, only_untuned, plan)
        # the clip-lanes verdict of this (architecture, shape), measured on the tuned tiles of both launch shapes -- only for
        # the engine's own full-batch plan and only when the knob is on "auto"
        if (self._lanes == "auto" and not own_plan and not self.use_graph and x.shape[0] >= 2 and x.shape[0] % 2 == 0
                and os.environ.get("PTX_TUNE_LANES", "1") != "0"
                and not (only_untuned and lanes_lookup(lanes_key(model, _dense16(x).shape, self.precision_of(model))) is not None)):
            with torch.cuda.device(x.device):
                half = _dense16(_dense16(x)[:x.shape[0] // 2])
                hp = self.plan_for(model, half)
                with hp.exclusive():
                    self._autotune(model, half, iters, verbose, False, only_untuned, hp)
                self.tune_lanes(model, x, verbose=verbose)
            if persist:
                save_tuned_table()
        return plan

    def _autotune(self, model, x, iters=3, verbose=False, persist=False, only_untuned=False, plan=None):
        lib = _lib.lib()
        # timed launches per candidate: 2 keeps a first-use tune under a second per network; tuning sessions that feed the
        # shipped table ask for more (PTX_TUNE_ITERS) -- many candidates differ by 1-2 %, the noise of a 2-launch average
        iters = max(iters, int(os.environ.get("PTX_TUNE_ITERS", "0")))
        with torch.cuda.device(x.device):
            if plan is None:
                plan = self.plan_for(model, _dense16(x))
            plan.bind(model)
            plan.run_features(_dense16(x))      # make every buffer hold sane data
            ncfg = lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16()
            seen, seen_body = {}, {}
            log = open(os.environ["PTX_TUNE_LOG"], "w") if os.environ.get("PTX_TUNE_LOG") else None
            for stp in plan.conv_steps:
                key = json.dumps(stp.d.key())
                if key in seen:
                    stp.cfg, stp.split = seen[key]
                    if key in seen_body:
                        stp.body = seen_body[key]
                    continue
                kind = _flags_kind(stp.d.flags)
                if only_untuned and tuned_lookup(key, kind) is not None and (not getattr(stp, "body_ok", ()) or body_lookup(key) is not None):
                    continue
                best = None
                # PTX_TUNE_CANDIDATES="dma4/re,dma3/re": a targeted session -- only tiles whose name holds one of the
                # substrings are timed, next to the table's incumbent, which keeps its place unless beaten by 2 %
                cands = [c for c in os.environ.get("PTX_TUNE_CANDIDATES", "").split(",") if c]
                inc = tuned_lookup(key, kind) if cands else None
                inc_ms = None
                if inc is not None:
                    # the incumbent is timed EXPLICITLY, up front: its split need not be among the splits the sweep below
                    # tries for that tile, and without its time the 2 % rule would be skipped silently
                    keep_cfg = (stp.cfg, stp.split, getattr(stp, "from_table", False))
                    stp.cfg, stp.split, stp.from_table = inc[0], inc[1], False
                    try:
                        stp(_stream())
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(iters):
                            stp(_stream())
                        e1.record()
                        e1.synchronize()
                        inc_ms = e0.elapsed_time(e1) / iters
                    except PtxError:
                        inc = None                       # a stale entry this build refuses: nothing to defend
                    stp.cfg, stp.split, stp.from_table = keep_cfg
                stp.body = None                  # the tile sweep times the implicit-GEMM path
                steps_k = stp.d.kT * stp.d.kH * stp.d.kW * ((stp.d.Kc + 31) // 32)
                M = stp.d.N * stp.d.To * stp.d.Ho * stp.d.Wo
                ncol = _r4(stp.d.Co)                          # columns written (ldy is only the row stride)
                for cfg in range(ncfg):
                    name = lib.ptx_conv3d_config_name(cfg).decode()
                    if _tile_kind(name) != kind:
                        continue                         # fp16-operand / split-operand problems <-> their own tiles
                    if cands and not (any(c in name for c in cands) or (inc is not None and cfg == inc[0])):
                        continue
                    bm, bn_, bk = [int(v) for v in name.split("/")[0].split("x")]
                    narrow = bn_ <= 32 and bk == 32 and bm >= 128 and not name.endswith("/dma")   # Mx16 / Mx32 tiles
                    if (bk == 24) != (stp.d.Kc == 24) and not (stp.d.Kc == 24 and narrow):
                        continue                         # BK = 24 tiles are for the kW-folded stem only
                    if narrow and ncol > 32 and stp.d.groups <= 1:
                        continue
                    if bk == 64 and stp.d.Kc % 64 and kind != "x3":     # BK = 64 tiles: long, 64-aligned K only
                        continue
                    if name.endswith("/direct") and ncol > 32 and stp.d.groups <= 1:   # VALU kernels: narrow outputs
                        continue
                    if stp.d.groups > 1 and not name.endswith("/direct") and (stp.d.Co // stp.d.groups) % bn_:
                        continue                         # grouped: direct tiles, or MFMA tiles inside one group
                    if bn_ > 64 and ncol <= 64:
                        continue
                    if bn_ < 32 and ncol > 32 and name.endswith("/f16"):
                        continue
                    if bn_ % 48 == 0 and ncol % 48 != 0:          # 48/96-wide tiles: (2+1)D widths only
                        continue
                    if bm >= 128 and M < 8192:
                        continue
                    if stp is getattr(plan, "stem_bf16_step", None) and issued_conv_flop(stp.d, (bm, bn_, bk), 2) > 3.2 * stp.macs:
                        continue                         # the bf16 stem issues at most 1.6x its algorithmic MACs
                    blocks = ((M + bm - 1) // bm) * ((ncol + bn_ - 1) // bn_)
                    splits = [1]
                    if blocks < 512:
                        splits += [s for s in (2, 3, 4, 6, 8) if steps_k // s >= 4 and blocks * s <= 2048]
                    for sk in splits:
                        if sk > 1 and lib.ptx_conv3d_workspace_bytes(C.byref(stp.d), sk) > plan.ws_bytes:
                            continue
                        stp.cfg, stp.split, stp.from_table = cfg, sk, False     # a refusal must surface here, not fall back
                        try:
                            stp(_stream())      # warm-up + validity
                        except PtxError:
                            continue
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(iters):
                            stp(_stream())
                        e1.record()
                        e1.synchronize()
                        ms = e0.elapsed_time(e1) / iters
                        if log is not None:
                            log.write("%s\tM=%d\tN=%d\tK=%d\t%s\tsplit=%d\t%.4f ms\t%.1f TF\n" % (
                                stp.label, M, stp.d.Co, stp.d.Kc * stp.d.kT * stp.d.kH * stp.d.kW, name, sk, ms,
                                2e-9 * stp.macs / ms))
                        if best is None or ms < best[0]:
                            best = (ms, cfg, sk)
                        if inc is not None and (cfg, sk) == tuple(inc):
                            inc_ms = ms
                if inc_ms is not None and best is not None and best[1] != inc[0] and best[0] > 0.98 * inc_ms:
                    best = (inc_ms, inc[0], inc[1])
                if best is None:                 # nothing admissible was timed: keep the heuristic default
                    sk = C.c_int(1)
                    best = (float("nan"), lib.ptx_conv3d_pick_config(C.byref(stp.d), C.byref(sk)), sk.value)
                stp.cfg, stp.split = best[1], best[2]
                # the body kernel's shapes against the best tile: same 2 % bar an incumbent defends itself with
                if getattr(stp, "body_ok", ()) and os.environ.get("PTX_CONV_BODY", "1") not in ("0",) + BODY_SHAPES:
                    stp.body = None
                    t_best, pick = best[0], -1
                    for sh in stp.body_ok:
                        stp.body = sh
                        stp(_stream())
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(max(iters, 3)):
                            stp(_stream())
                        e1.record()
                        e1.synchronize()
                        ms = e0.elapsed_time(e1) / max(iters, 3)
                        if log is not None:
                            log.write("%s\tconv_body_f32/%s\t%.4f ms\t%.1f TF\n" % (stp.label, BODY_SHAPES[sh], ms, 2e-9 * stp.macs / ms))
                        if verbose:
                            print("tune %-34s body/%-6s %.4f ms  %.1f TF  (best tile %.4f ms)" % (stp.label, BODY_SHAPES[sh], ms, 2e-9 * stp.macs / ms, best[0]))
                        if ms < 0.98 * t_best:
                            t_best, pick = ms, sh
                    stp.body = pick if pick >= 0 else None
                    body_store(key, pick)
                    seen_body[key] = stp.body
                seen[key] = (best[1], best[2])
                tuned_store(key, best[1], best[2])
                if verbose:
                    print("tune %-34s M=%-8d N=%-5d K=%-6d -> %-20s split=%d  %.3f ms  %.1f TF" % (
                        stp.label, M, stp.d.Co, stp.d.Kc * stp.d.kT * stp.d.kH * stp.d.kW,
                        lib.ptx_conv3d_config_name(best[1]).decode(), best[2], best[0],
                        2e-9 * stp.macs / best[0]))
            # chained launches: time every chained tile that holds the intermediate row
            seen_c, seen_cb = {}, {}
            for stp in plan.chain_steps:
                if stp.key in seen_c:
                    stp.cfg = seen_c[stp.key]
                    if stp.key in seen_cb:
                        stp.body = seen_cb[stp.key]
                    continue
                if only_untuned and chain_lookup(stp.key) is not None and (not getattr(stp, "body_ok", ()) or body_lookup(stp.key) is not None):
                    continue
                best = None
                stp.body = None                  # the chained-tile sweep times the implicit-GEMM chain
                for cfg in range(lib.ptx_conv3d_chain_num_configs()):
                    if not lib.ptx_conv3d_chain_supported(C.byref(stp.d), C.byref(stp.d2), cfg):
                        continue
                    keep, stp.cfg = stp.cfg, cfg
                    try:
                        stp(_stream())
                    except PtxError:
                        stp.cfg = keep
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        stp(_stream())
                    e1.record()
                    e1.synchronize()
                    ms = e0.elapsed_time(e1) / iters
                    if log is not None:
                        log.write("%s\t%s\t%.4f ms\t%.1f TF\n" % (stp.label, lib.ptx_conv3d_chain_config_name(cfg).decode(), ms,
                                                                  2e-9 * stp.macs / ms))
                    if best is None or ms < best[0]:
                        best = (ms, cfg)
                    stp.cfg = keep
                if best is not None:
                    stp.cfg = best[1]
                    # ... and the body kernel's chained form against the best chained tile (2 % bar)
                    if getattr(stp, "body_ok", ()) and os.environ.get("PTX_CONV_BODY", "1") not in ("0",) + BODY_SHAPES:
                        t_best, pick = best[0], -1
                        for sh in stp.body_ok:
                            stp.body = sh
                            stp(_stream())
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(max(iters, 3)):
                                stp(_stream())
                            e1.record()
                            e1.synchronize()
                            ms = e0.elapsed_time(e1) / max(iters, 3)
                            if log is not None:
                                log.write("%s\tconv_body_chain_f32/%s\t%.4f ms\t%.1f TF\n" % (stp.label, BODY_SHAPES[sh], ms, 2e-9 * stp.macs / ms))
                            if verbose:
                                print("tune %-34s body-chain/%-6s %.4f ms  %.1f TF  (best chained tile %.4f ms)" % (
                                    stp.label, BODY_SHAPES[sh], ms, 2e-9 * stp.macs / ms, best[0]))
                            if ms < 0.98 * t_best:
                                t_best, pick = ms, sh
                        stp.body = pick if pick >= 0 else None
                        body_store(stp.key, pick)
                        seen_cb[stp.key] = stp.body
                    seen_c[stp.key] = best[1]
                    chain_store(stp.key, best[1])
                    if verbose:
                        print("tune %-34s -> %-28s %.3f ms  %.1f TF" % (stp.label, lib.ptx_conv3d_chain_config_name(best[1]).decode(),
                                                                       best[0], 2e-9 * stp.macs / best[0]))
            # chained launch vs the two launches it replaces: time both executions of every pair, keep the faster
            force = os.environ.get("PTX_CHAIN_FORCE")
            seen_a = {}
            for a in plan.alt_steps:
                if a.key in seen_a:
                    a.use_chain = seen_a[a.key]
                    continue
                if force in ("0", "1") or (only_untuned and alt_lookup(a.key) is not None):
                    continue
                ms2 = []
                for run in (a.chain, lambda st_: [s_(st_) for s_ in a.pair]):
                    run(_stream())
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(max(iters, 3)):
                        run(_stream())
                    e1.record()
                    e1.synchronize()
                    ms2.append(e0.elapsed_time(e1) / max(iters, 3))
                # the chained launch has to win by a margin: timed alone in a loop it looks ~2 % better than inside the
                # forward (measured: config 2 x3, layer2 tails -- chosen at parity by the tuner, 1.2 % slower in the step)
                a.use_chain = ms2[0] < 0.97 * ms2[1]
                seen_a[a.key] = a.use_chain
                alt_store(a.key, a.use_chain)
                if log is not None:
                    log.write("%s\tchain %.4f ms\tpair %.4f ms\t-> %s\n" % (a.label, ms2[0], ms2[1], "chain" if a.use_chain else "pair"))
                if verbose:
                    print("tune %-34s chain %.4f ms | pair %.4f ms -> %s" % (a.label, ms2[0], ms2[1], "chain" if a.use_chain else "pair"))
            # conv program vs the launches it replaces: time both executions of every run, keep the faster (same margin rule)
            pmode = os.environ.get("PTX_PROGRAM", "0")
            dissolved = []
            for ps in list(plan.program_steps):
                if pmode != "auto":
                    continue
                known = prog_lookup(ps.key)
                if only_untuned and known is not None:      # an identical run of convs was measured a moment ago: same verdict
                    ps.use_program = known
                    if not known:
                        i = plan.steps.index(ps)
                        plan.steps[i:i + 1] = ps.convs
                        dissolved.append(ps)
                    continue
                ms2 = []
                for flag in (True, False):
                    ps.use_program = flag
                    ps(_stream())
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(max(iters, 5)):
                        ps(_stream())
                    e1.record()
                    e1.synchronize()
                    ms2.append(e0.elapsed_time(e1) / max(iters, 5))
                ps.use_program = ms2[0] < 0.97 * ms2[1]
                if ps.error() is not None:
                    ps.use_program = False
                prog_store(ps.key, ps.use_program)
                if not ps.use_program:       # the launches it stood for take its place; its workspace and image are freed
                    i = plan.steps.index(ps)
                    plan.steps[i:i + 1] = ps.convs
                    dissolved.append(ps)
                if log is not None:
                    log.write("%s\tprogram %.4f ms\tlaunches %.4f ms\t-> %s\n" % (ps.label, ms2[0], ms2[1], "program" if ps.use_program else "launches"))
                if verbose:
                    print("tune %-44s program %.4f ms | %d launches %.4f ms -> %s" % (ps.label, ms2[0], len(ps.convs), ms2[1],
                                                                                      "program" if ps.use_program else "launches"))
            plan.program_steps = [p_ for p_ in plan.program_steps if p_ not in dissolved]
            plan.run_features(_dense16(x))
            plan.tuned = True
            if log is not None:
                log.close()
        if persist:
            save_tuned_table()
        return plan

    def profile_convs(self, model, x, iters=5, plan=None):
        """Per-conv-launch timing with HIP events on the current stream: the launches the forward RUNS (`plan.all_convs()`:
        the active side of every chain-or-pair decision, chained launches and direct stems included), as rows of
        (label, MACs, ms, tile / kernel name, split-K).  `plan`: an already compiled (and run) plan, for models whose input
        is not one NCDHW tensor."""
        with torch.cuda.device(x.device):
            if plan is None:
                self._validate(model, x, model.arch.dims)
                plan = self.plan_for(model, _dense16(x))
                plan.bind(model)
                plan.run_features(_dense16(x))
            live = set(id(s) for s in plan.all_convs())
            rows = []
            for r in self.profile_steps(plan, iters):
                if r[1] in ("conv", "stem", "chain"):
                    rows.append((r[0], r[3], r[4], r[5], r[6].split if r[1] == "conv" else 1))
            if len(rows) != len(live):
                raise PtxError("profile_convs: %d timed launches for %d live conv steps" % (len(rows), len(live)))
        return rows


    def profile_steps(self, plan, iters=5, isolated=None):
        """HIP-event time of EVERY launch of a compiled (and run) plan on the current stream, convs and HBM-bound
        passes alike: rows of (label, kind, algorithmic bytes, MACs, ms, tile / kernel name).  kind is "conv" for the
        implicit-GEMM launches, "stem" for the direct stem kernels, "mem" for tagged HBM passes, "mfma" for the fused attention, "other" for the rest.

        Method (round 6).  The launches are timed INSIDE ordinary passes over the plan -- the caches and the clock / power
        state of a forward -- by a CHAIN of events, one after every launch: interval i = event i -> event i + 1, so the
        intervals of a pass sum to that pass by construction.  An event between two launches costs the stream a marker
        packet, so an instrumented pass is longer than a plain one; the same call therefore also times `iters` PLAIN passes
        (two events around all of them) and removes the difference as a constant per launch:
            overhead = (instrumented pass - plain pass) / launches,   ms_i = interval_i - overhead
        so that sum(ms_i) == the plain pass (rows are rescaled by a common factor if a clamp at 25 % of the raw interval
        was hit).  `self.last_profile` keeps the calibration: {"plain_pass_ms", "instrumented_pass_ms", "launches",
        "overhead_us_per_launch", "raw_sum_ms", "clamped"}.  Round 5 bracketed each launch with its OWN pair of events and
        reported the raw brackets: they summed to 5.76 ms in a 5.39 ms step.

        `isolated=True` (or PTX_PROFILE_ISOLATED=1) is the round-1..4 method, every launch repeated `iters` times back to back
        on its own: it over-states the MFMA-bound launches by 5-19 % (five identical matrix-bound launches in a row pull
        the clock down)."""
        if isolated is None:
            isolated = os.environ.get("PTX_PROFILE_ISOLATED", "0") == "1"
        st = _stream()
        flat = [t for s in plan.steps for t in (s.active() if isinstance(s, (AltStep, ProgramStep)) else [s])]
        ms_of = []
        self.last_profile = None
        if isolated:
            for stp in flat:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stp(st)
                e0.record()
                for _ in range(iters):
                    stp(st)
                e1.record()
                e1.synchronize()
                ms_of.append(e0.elapsed_time(e1) / iters)
        else:
            n = len(flat)
            # untimed passes first: every launch has run in this order and the clocks are back up -- the caller may have left
            # the GPU idle for seconds (bench.py's CPU leg), and the first tens of milliseconds after an idle period run at a
            # lower clock (measured: a pass 1.9 % slower than the timed steps of the same plan when only two passes preceded it)
            t_warm = time.perf_counter()
            for k in range(64):
                for stp in flat:
                    stp(st)
                if k >= 3 and (k & 3) == 3:
                    torch.cuda.synchronize()
                    if time.perf_counter() - t_warm > 0.25:
                        break
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(n + 1)] for _ in range(iters)]
            pa, pb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            pc, pd = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def plain(e0, e1, k):
                e0.record()
                for _ in range(k):
                    for stp in flat:
                        stp(st)
                e1.record()
            half = max(1, iters // 2)
            plain(pa, pb, half)                 # plain passes on BOTH sides of the instrumented ones (clock drift)
            for it in range(iters):
                ev[it][0].record()
                for i, stp in enumerate(flat):
                    stp(st)
                    ev[it][i + 1].record()
            plain(pc, pd, half)
            torch.cuda.synchronize()
            plain_ms = (pa.elapsed_time(pb) + pc.elapsed_time(pd)) / (2 * half)
            raw = [sum(ev[it][i].elapsed_time(ev[it][i + 1]) for it in range(iters)) / iters for i in range(n)]
            inst_ms = sum(ev[it][0].elapsed_time(ev[it][n]) for it in range(iters)) / iters
            over = max(0.0, (inst_ms - plain_ms) / max(n, 1))
            ms_of = [max(r - over, 0.25 * r) for r in raw]
            clamped = sum(1 for r in raw if r - over < 0.25 * r)
            tot = sum(ms_of)
            if tot > 0 and (clamped or inst_ms < plain_ms):
                ms_of = [m * plain_ms / tot for m in ms_of]
            self.last_profile = {"method": "event chain inside ordinary passes, constant per-launch marker overhead removed",
                                 "iters": iters, "launches": n, "plain_pass_ms": plain_ms, "instrumented_pass_ms": inst_ms,
                                 "raw_sum_ms": sum(raw), "overhead_us_per_launch": 1e3 * over, "clamped": clamped}
        rows = []
        for stp, ms in zip(flat, ms_of):
            if isinstance(stp, ConvStep) and getattr(stp, "body", None) is not None:       # a direct kernel, like the stems
                rows.append((stp.label, "stem", 0, stp.macs, ms, stp.kernel))
            elif isinstance(stp, ConvStep):
                rows.append((stp.label, "conv", 0, stp.macs, ms, _lib.lib().ptx_conv3d_config_name(stp.cfg).decode(), stp))
            elif isinstance(stp, (StemStep, StemF32Step, PatchConvStep)):      # direct (patch) kernels are convs too
                rows.append((stp.label, "stem", 0, stp.macs, ms, stp.kernel))
            elif isinstance(stp, (ChainStep, ProgramStep)):     # several convs in one launch, their own tile tables
                rows.append((stp.label, "chain", 0, stp.macs, ms, stp.kernel))
            else:
                nb, macs = getattr(stp, "hbm_bytes", 0), getattr(stp, "macs", 0)
                kind = "mem" if nb and not macs else "mfma" if macs else "other"
                rows.append((getattr(stp, "label", getattr(stp, "__name__", "step")), kind, nb, macs, ms, ""))
        return rows


# ---------------------------------------------------------------------------------------------
# multi-view inference: decoded video -> transforms.SampleViews -> model, chunk by chunk -> ptx_views_mean
# ---------------------------------------------------------------------------------------------
def views_chunk(N, V, max_batch):
    """Views per chunk of forward_views for N videos of V views each: every chunk is N * views_chunk clips, the most
    that `max_batch` clips allow (at least one view, at most all V)."""
    return max(1, min(int(V), int(max_batch) // max(int(N), 1)))


def views_mean(logits, N, V, mode="softmax"):
    """[N*V, K] (or [N, V, K]) fp32 / bf16 CUDA logits -> fp32 [N, K]: the mean over a video's views of softmax(row)
    (mode "softmax") or of the rows (mode "logits"), one ptx_views_mean launch."""
    if mode not in ("softmax", "logits"):
        raise PtxError("views_mean: mode must be 'softmax' or 'logits', got %r" % (mode,))
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.dtype not in (torch.float32, torch.bfloat16):
        raise PtxError("views_mean: logits must be a float32 or bfloat16 CUDA tensor (no CPU fallback)")
    K = logits.shape[-1]
    if logits.numel() != N * V * K or logits.stride(-1) != 1:
        raise PtxError("views_mean: expected %d x %d rows, got shape %s" % (N, V, tuple(logits.shape)))
    rows = logits.reshape(N * V, K) if logits.dim() != 2 else logits
    if rows.shape[0] > 1 and rows.stride(0) < K:
        rows = rows.contiguous()
    with torch.cuda.device(logits.device):
        y = torch.empty((N, K), device=logits.device, dtype=torch.float32)
        check(_lib.lib().ptx_views_mean(C.c_void_p(rows.data_ptr()), _ptr(y), N, V, K, rows.stride(0) if rows.shape[0] > 1 else K,
                                        int(logits.dtype == torch.bfloat16), 0 if mode == "softmax" else 1, _stream()),
              "ptx_views_mean")
    return y


def run_views(video, views, run, max_batch, reduce="softmax", chunk=None, who="forward_views"):
    """The loop behind every forward_views: `views.sample` produces views [v0, v0 + nv) of every video, `run` turns
    the N * nv clips into logits, the logits of all chunks land in one [N*V, K] buffer, ptx_views_mean reduces it."""
    if reduce not in ("softmax", "logits", None):
        raise PtxError("%s: reduce must be 'softmax', 'logits' or None, got %r" % (who, reduce))
    if not isinstance(video, torch.Tensor) or video.dim() not in (4, 5):
        raise PtxError("%s: video must be a uint8 CUDA tensor [N,Tv,H,W,3] or [Tv,H,W,3]" % who)
    N, V = (video.shape[0] if video.dim() == 5 else 1), views.num_views
    nv = views_chunk(N, V, max_batch) if chunk is None else chunk
    if not isinstance(nv, int) or isinstance(nv, bool) or nv < 1:
        raise PtxError("%s: chunk must be a positive number of views, got %r" % (who, chunk))
    buf = None
    for v0 in range(0, V, nv):
        n = min(nv, V - v0)
        x = views.sample(video, v0, n)                        # rank 4: [n, ...]; rank 5: [N, n, ...]
        out = run(x.reshape((N * n,) + tuple(x.shape[-4:])))
        if not isinstance(out, torch.Tensor) or out.numel() % (N * n) or out.dtype not in (torch.float32, torch.bfloat16):
            raise PtxError("%s: the model's head must return one float32 / bfloat16 row of logits per clip" % who)
        out = out.reshape(N, n, -1)
        if buf is None:
            buf = torch.empty((N, V, out.shape[-1]), device=out.device, dtype=out.dtype)
        buf[:, v0:v0 + n] = out
    return buf if reduce is None else views_mean(buf, N, V, reduce)


def check_views(views, model, want_out, who="forward_views"):
    from .transforms import SampleViews
    if not isinstance(views, SampleViews):
        raise PtxError("%s: views must be a pretorched.transforms.SampleViews, got %r" % (who, views))
    if want_out == "frames" and views.out != "frames":
        raise PtxError("%s: a float32 model takes the views as uint8 frames (forward_frames): build the SampleViews with "
                       "out='frames'" % who)
    if want_out == "bf16" and (views.out != "tensor" or views.dtype != torch.bfloat16):
        raise PtxError("%s: a bfloat16 model takes the views as the normalised bf16 clip: build the SampleViews with "
                       "out='tensor', dtype=torch.bfloat16" % who)


class EngineOwner:
    """nn.Module plumbing shared by every HIP-executed model class: the per-model Engine and the hooks
    that tell it the weights changed.  Mixed in ahead of nn.Module."""

    def _init_engine(self):
        self._engine = Engine(self)

    def engine(self):
        return self._engine

    def refresh(self):
        """Drop every compiled plan and packed (BN-folded) filter: the next forward re-reads the parameters.
        load_state_dict(), .to()/.cuda() and in-place updates that bump a tensor's version counter are noticed
        automatically; edits made through `.data` (e.g. `m.weight.data.fill_(1)`), replaced trunk modules and
        `engine().check_weights = False` need this call (or `engine().check_weights = "checksum"`)."""
        self._engine.invalidate()
        return self

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._engine.invalidate()
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        if "_engine" in self.__dict__:
            self._engine.invalidate()
        return r


# ---------------------------------------------------------------------------------------------
# TRN relation MLP (trn.py:39-45): ReLU -> Linear -> ReLU -> Linear
# ---------------------------------------------------------------------------------------------
def linear(x, lin, flags=0):
    """y = x @ W^T + b through ptx_linear_fwd for any [..., K] float32 CUDA tensor (TRN classifier,
    trn.py:257-258)."""
    if not isinstance(lin, torch.nn.Linear):
        return lin(x)                                   # user-replaced head: theirs to run
    from . import eager
    if eager.wanted(lin, x):                            # train() / autograd / CPU model (eager.py)
        return lin(x)
    if not x.is_cuda or x.dtype != torch.float32:
        raise PtxError("linear: input must be a float32 CUDA tensor (no CPU fallback)")
    K = lin.in_features
    flat = x.contiguous().view(-1, K)
    M = flat.shape[0]
    with torch.cuda.device(x.device):
        out = torch.empty((M, lin.out_features), device=x.device, dtype=torch.float32)
        w = lin.weight.detach().contiguous()
        b = lin.bias.detach().contiguous() if lin.bias is not None else None
        check(_lib.lib().ptx_linear_fwd(_ptr(flat), _ptr(w), _ptr(b) if b is not None else C.c_void_p(0),
                                        _ptr(out), M, K, lin.out_features, K, lin.out_features, flags,
                                        _stream()), "ptx_linear_fwd")
    return out.view(tuple(x.shape[:-1]) + (lin.out_features,))


def relation_scale(x, subsets, lin1, lin2, out=None, accumulate=False):
    """All frame subsets of ONE relation scale in two launches (reference trn.py:101-110 runs one MLP per
    subset): launch 1 gathers the frames inside the kernel and reads W1 once for every subset, launch 2
    applies W2 to the sum of the hidden vectors (linearity of `stack(output).sum(0)`) and accumulates
    into `out`.  x: [B, T, F] fp32 CUDA; subsets: tuples of frame indices, all of one length."""
    if not x.is_cuda or x.dtype != torch.float32:
        raise PtxError("relation_scale: input must be a float32 CUDA tensor (no CPU fallback)")
    B, T, F_ = x.shape
    d = _lib.RelationDesc()
    d.B, d.n_sets, d.n_frames, d.frame_len = B, len(subsets), len(subsets[0]), F_
    for r, sub in enumerate(subsets):
        for f, i in enumerate(sub):
            d.idx[r][f] = int(i)
    lib = _lib.lib()
    hid_n, out_n = lin1.out_features, lin2.out_features
    with torch.cuda.device(x.device):
        hid = torch.empty((len(subsets) * B, hid_n), device=x.device, dtype=torch.float32)
        res = out if out is not None else torch.empty((B, out_n), device=x.device, dtype=torch.float32)
        w1, b1 = lin1.weight.detach().contiguous(), lin1.bias.detach().contiguous()
        w2, b2 = lin2.weight.detach().contiguous(), lin2.bias.detach().contiguous()
        check(lib.ptx_relation_linear_fwd(C.byref(d), _ptr(x), T * F_, _ptr(w1), _ptr(b1), _ptr(hid), hid_n, hid_n,
                                          PTX_PRO_RELU | PTX_EPI_RELU, _stream()), "relation.linear1")
        check(lib.ptx_linear_setsum_fwd(_ptr(hid), _ptr(w2), _ptr(b2), _ptr(res), B, len(subsets), hid_n, out_n, hid_n,
                                        out_n, PTX_EPI_ACCUM if accumulate else 0, _stream()), "relation.linear2")
    return res


def relation_mlp(flat, lin1, lin2, out=None, accumulate=False):
    if not flat.is_cuda or flat.dtype != torch.float32:
        raise PtxError("relation_mlp: input must be a float32 CUDA tensor (no CPU fallback)")
    flat = flat.contiguous()
    M, K = flat.shape
    lib = _lib.lib()
    with torch.cuda.device(flat.device):
        hid = torch.empty((M, lin1.out_features), device=flat.device, dtype=torch.float32)
        res = out if out is not None else torch.empty((M, lin2.out_features), device=flat.device,
                                                      dtype=torch.float32)
        w1, b1 = lin1.weight.detach().contiguous(), lin1.bias.detach().contiguous()
        w2, b2 = lin2.weight.detach().contiguous(), lin2.bias.detach().contiguous()
        # ReLU(in) -> Linear -> ReLU fused into launch 1; Linear into launch 2
        check(lib.ptx_linear_fwd(_ptr(flat), _ptr(w1), _ptr(b1), _ptr(hid), M, K, lin1.out_features, K,
                                 lin1.out_features, PTX_PRO_RELU | PTX_EPI_RELU, _stream()), "relation.linear1")
        check(lib.ptx_linear_fwd(_ptr(hid), _ptr(w2), _ptr(b2), _ptr(res), M, lin1.out_features,
                                 lin2.out_features, lin1.out_features, lin2.out_features,
                                 PTX_EPI_ACCUM if accumulate else 0, _stream()), "relation.linear2")
    return res
