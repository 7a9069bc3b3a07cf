"""The plan compiler: a zoo model + input shape -> the list of libptx_amd launches that computes it.

`Plan` owns every activation buffer, packed filter and launch record (steps.py) of one (input shape, device); its building
blocks -- conv / conv_chain / conv_bn / maxpool / attention / nonlocal_block -- are what the family builders of plans.py
(SlowFast, I3D, BigGAN-deep, MNISTNonLocalNet) are written in.  Tile and kernel choices come from the tuned table
(tuned.py), else from the library's own heuristics.
"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import threading

import torch
import torch.nn as nn

from . import _lib, plans
from ._lib import (ConvDesc, ConvFusedExt, ConvProgramInfo, ConvStage, NonlocalDesc, PoolDesc, PTX_BF16_OPERANDS, PTX_EPI_AFFINE,
                   PTX_EPI_DUAL_RAW, PTX_EPI_OUT_F16, PTX_EPI_RELU, PTX_EPI_RES_ADD, PTX_EPI_RES_PADA, PTX_EPI_RES_UP, PTX_EPI_TANH,
                   PTX_F16_OPERANDS, PTX_F16X3_OPERANDS, PTX_NL_BF16, PTX_NL_F16, PTX_NL_OUT_F16, PTX_NL_RELU, PTX_NL_SCALE,
                   PTX_NL_SOFTMAX, PTX_NL_X3, PTX_POOL_BF16, PTX_POOL_PAD_ZERO, PTX_POOL_SAME, PTX_PRO_UP2, PTX_RES_F16,
                   PTX_SPLITK_FUSED, PTX_STEM_SRC_BF16_NCDHW, PTX_STEM_SRC_U8_NTHWC, PtxError, check)
from ._lib import BnApplyDesc
from .steps import BnApplyStep, BnStatsStep, BnUpdateStep
from .steps import DwConvStep, PackedDw
from .steps import (Act, AltStep, ChainStep, ConvStep, Packed, PackedDual, PatchConvStep, ProgramStep, RawInput, StemBf16Step, StemF32Step, StemTfirStep, TFIR_SCHEMES, Wino4Step, WinoStep, _WinoExec,
                    StemStep, _ConcatRowsPack, _Ref, _device_ctx, _geom, _ptr, _r4, _r8, _r128, _same_geometry, _stem_ld, _stream,
                    _t3, _tag)
from .tuned import (BODY_FILTERS, BODY_SHAPES, _flags_kind, alt_lookup, body_lookup, chain_key, chain_lookup, prog_lookup,
                    tfir_lookup, tuned_lookup, wino4_lookup, wino_lookup)

# bf16 inference (a model whose floating-point parameters are torch.bfloat16): the families whose plans run end to end on the
# bf16 kernels.  Everything else raises at plan build time.
BF16_FAMILIES = ("resnet3d10", "resnet3d18", "resnet3d34", "resnet3d50", "resnet3d101", "resnet3d152", "resnet3d200",
                 "r2plus1d10", "r2plus1d18", "r2plus1d34", "r2plus1d50")
# ... and the plan kinds built from non-local blocks alone: NonLocalBlock1D / 2D / 3D and MNISTNonLocalNet
BF16_NL_KINDS = ("nlblock", "mnist_nl")
# ... and, under Engine.bf16_stem = "direct" only, the networks that embed non-local blocks in one of the families above
# (arch.nonlocal_layers: nonlocalresnet3d18 .. 101, NonLocalResNet3D(nonlocal_layers=...), nonlocal_r2plus1d50; Plan._build).
# Under the default "fold" stem they keep raising.
# ... and, under Engine.bf16_stem = "direct" only, the 2-D ResNets (TRN's per-frame backbone): the Conv2d stem is the direct
# kernel's kT = 1 case on T = 1, and there is no fold route behind it
BF16_FAMILIES_2D = ("resnet18", "resnet34", "resnet50", "resnet101", "resnet152")
# ... and the BigGAN-deep generator (every resolution and width; plans.build_biggan's bf16 flow)
BF16_GEN_KINDS = ("biggan",)
# ... and, under Engine.bf16_stem = "direct" only, plan kind "slowfast" (SlowFast / SlowOnly / FastOnly: Plan._build)


def _bf16_base(name):
    """The BF16_FAMILIES entry a non-local network is built on: 'nonlocalresnet3d50' -> 'resnet3d50', 'nonlocal_r2plus1d50' ->
    'r2plus1d50' (arch keys: the '/5', '/nl0-1-1-0' placement and '@B' shortcut suffixes dropped)."""
    name = name.split("@")[0].split("/")[0]
    for prefix in ("nonlocal_", "nonlocal"):
        if name.startswith(prefix):
            return name[len(prefix):]
    return name


def model_precision(model):
    """"bf16" when the model's floating-point parameters are torch.bfloat16, "fp16" for torch.float16, else "fp32" -- read
    from the first weight (a generator step, not a walk of the tree: this runs on every forward)."""
    w = next(iter(model.parameters()), None)
    if w is None:
        w = next((getattr(m, "weight", None) for m in model.modules() if isinstance(getattr(m, "weight", None), torch.Tensor)), None)
    return {torch.bfloat16: "bf16", torch.float16: "fp16"}.get(getattr(w, "dtype", None), "fp32")


# Batch-statistics plans (Plan(batch_stats=True): what Engine.update_bn runs) cover float32 models of plan kind "resnet" whose
# convs are nn.Conv3d / nn.Conv2d / (2+1)D pairs and that hold no non-local block
BATCH_STATS_SCOPE = ("float32 resnet3d10..200, r2plus1d10..50, resnext3d10..200, wideresnet3d50, preact_resnet3d10..200 and the 2-D "
                     "resnet18..152 (either shortcut type), built by this package and living on the GPU -- not bfloat16 / float16 "
                     "models, non-local networks, MultiViewConv networks, SlowFast, I3D, TRN, BigGAN or adopted instances")


def check_batch_stats_scope(model):
    """Raise PtxError unless `model` is one a batch-statistics plan can be compiled for (BATCH_STATS_SCOPE)."""
    name = str(getattr(model, "arch_name", None) or type(model).__name__)
    arch = getattr(model, "arch", None)
    why = None
    if getattr(model, "_engine", None) is None:
        why = "it does not run on the HIP engine"
    elif name.startswith("adopted:") or "_ptx_twin" in getattr(model, "__dict__", {}):
        why = "it is an adopted instance"
    elif getattr(model, "plan_kind", "resnet") != "resnet" or arch is None or not hasattr(arch, "block"):
        why = "its plan kind is %r" % getattr(model, "plan_kind", None)
    elif model_precision(model) != "fp32":
        why = "its parameters are %s" % model_precision(model)
    elif arch.nonlocal_layers:
        why = "it holds non-local blocks"
    elif arch.conv == "mv":
        why = "its convs are MultiViewConv"
    elif arch.block.startswith("csn"):
        why = "its 3x3x3 convs are depthwise (channel-separated)"
    if why is not None:
        raise PtxError("update_bn does not cover %s (%s): it runs %s" % (name, why, BATCH_STATS_SCOPE))


def _foldable(conv, x):
    """Small-Cin first conv reading the raw NCDHW input: fold kW into the channel axis."""
    return isinstance(x, RawInput)


class Plan:
    def __init__(self, engine, model, shape, dev, norm=None, batch_stats=False):
        # batch_stats: the second plan flavour of a (shape, device) -- every BatchNorm normalises with the moments of THIS batch
        # (train()-mode F.batch_norm) and moves its running statistics: conv_bn becomes the raw conv + statistics + update +
        # apply, nothing is fused across a BN (no chained pairs, no dual-source shortcut GEMM, no conv programs), the
        # arithmetic is fp32 whatever Engine.precision says, and the plan ends at the trunk's features (Engine.update_bn)
        self.batch_stats = bool(batch_stats)
        if self.batch_stats:
            check_batch_stats_scope(model)
            if norm is not None:
                raise PtxError("update_bn takes float32 clips, not uint8 frames")
        self.bn_steps = []               # BnStatsStep per BatchNorm, in execution order (batch-statistics plans)
        self.bn_refs, self.bn_sizes = [], []      # ... their modules (_Ref) and (offset into bn_run, channels)
        self.bn_f = []                   # ... the factor f of their running-statistics update (set per batch by the pass)
        self.bn_run = None               # (running_mean, running_var) of every BN, concatenated: the plan's own scratch pair
        self.bn_own_run = None           # ... unless a pass points bn_run at its buffers (Engine.update_bn)
        self.bn_ws_bytes, self.bn_ws, self.bn_ws_ptr = 0, None, C.c_void_p(0)         # partial sums of the statistics kernel
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
        self.chain = os.environ.get("PTX_CHAIN", "1") != "0" and not self.batch_stats
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
        self.fuse_shortcut = os.environ.get("PTX_FUSE_SHORTCUT", "1") != "0" and not self.batch_stats
        # arithmetic: the model's parameter dtype decides bf16 (every conv on the bf16 tiles, bf16 activations); for fp32
        # models Engine.precision picks fp32 / x3
        prec = model_precision(model)
        if prec == "fp16":
            raise PtxError("fp16 models (model.half()) are not supported: use bfloat16 (model.to(torch.bfloat16)) or float32")
        self.bf16 = prec == "bf16"
        self.precision = "bf16" if self.bf16 else "fp32" if self.batch_stats else engine.precision
        self.x3 = self.precision == "x3"     # split fp32 operands on the fp16 matrix cores
        # qualified names of the model's modules: everything the plan keeps from the model is a _Ref
        self._names = {id(m): n for n, m in model.named_modules()}
        self._cur = model                # the model (or DataParallel replica) whose tensors are valid right now
        self.program_steps = []  # ProgramStep: runs of small-M convs as one persistent launch
        self.wino_steps = []     # WinoStep: direct launch | Winograd transforms around a grouped conv, chosen by measurement
        self.wino4_steps = []    # every step with a Winograd F(4x4) form: those of wino_steps, then the F(4x4)-only Wino4Steps
        self.wino_bytes, self.wino_arena = 0, None       # V / M arena of the Winograd steps (the largest need of either form)
        self.stem_tfir_steps = []        # StemF32Steps with temporal fast-FIR executions (V in the Winograd arena)
        self.stem_bf16_step = None       # the bf16 stem's ConvStep (the tuner bounds its issued work)
        self.bf16_stem = getattr(engine, "bf16_stem", "fold")            # "fold" | "direct" (ptx_conv_stem_bf16_fwd)
        self.stem_steps = self.patch_steps = self.attn_steps = 0         # launches outside conv_steps, by kind
        self.attn_descs, self.attn_operands = [], []                     # bf16 attention launches: descriptors, (th, ph, g, y)
        self.attn_variants = []          # ... and the kernel form the dispatcher picks for each (ptx_nonlocal_bf16_variant, at build time)
        self._stem_src = {}              # stem_source()'s buffers by (uint8 frames?, row pitch)
        self.feat = self.pooled = None   # set by the family's builder
        self.head_error = None           # why the default / custom head cannot run on this shape (raised by run_head)
        self.head32 = None               # bf16 plans: fp32 copy of the classifier (head32_refresh)
        self.kind = None                 # the model's plan_kind (set by _build)
        self.half_plan = self.gen_patch = False      # BigGAN-deep plans (plans.build_biggan): fp16 operands / patch kernels
        with _device_ctx(dev):
            self._build(model)
            if not self.batch_stats:
                self._fuse_programs()
            self._bind_wino_arena()
            if self.bn_steps:
                f32 = dict(device=dev, dtype=torch.float32)
                total = sum(_r4(c) for _, c in self.bn_sizes)
                self.bn_own_run = self.bn_run = (torch.zeros(total, **f32), torch.ones(total, **f32))
                self.bn_ws = torch.empty(self.bn_ws_bytes // 4, **f32)
                self.bn_ws_ptr = _ptr(self.bn_ws)
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
        if self.bf16:        # bf16 plans: every conv reads and writes bf16 activations (one rounding per output)
            out_f16 = True
        xin, out, padding = self._conv_geometry(x, pk, stride, padding, same, up2)
        y = self._conv_output(x, pk, out, y, out_f16, label)
        d, resptr, fused, ext, raw_act = self._conv_desc(x, pk, y, xin, out, stride, padding, relu, res, res_kind, res_stride,
                                                         x2, x2_stride, (up2, affine, out_f16, raw, tanh), label)
        st = ConvStep()
        st.d, st.x, st.w, st.b, st.res, st.y = d, _ptr(x.t), _ptr(pk.w), _ptr(pk.b), resptr, _ptr(y.t)
        st.plan, st.label = self, label
        st.macs = x.N * out[0] * out[1] * out[2] * pk.Co * pk.real_ci * pk.d.kT * pk.d.kH * pk.d.kW
        st.ext, st.fused = ext, fused
        if x2 is not None:                      # K-concatenated second activation source (shortcut B)
            st.x2 = _ptr(x2.t)
            st.macs += x.N * out[0] * out[1] * out[2] * pk.Co * x2.C
        patch = self._patch_kernel(d, fused, x.bf16, res, raw, tanh, x2, pro_affine, label)
        if patch is not None:
            ps = PatchConvStep()
            if pro_affine is not None:
                ps.ext_in = ConvFusedExt()
                ps.ext_in.scale, ps.ext_in.shift, ps.ext_in.ld_affine = pro_affine[0], pro_affine[1], int(pro_affine[2])
            ps.d, ps.x, ps.w, ps.b, ps.y, ps.ext, ps.label = d, st.x, st.w, st.b, st.y, ext, label
            ps.res, ps.kernel = resptr, patch
            ps.macs, ps.hbm_bytes = st.macs, 0
            self.steps.append(ps)
            self.patch_steps += 1
            return (y, raw_act) if raw else y
        self._body_kernel(st, pk, x2)
        self._pick_tile(st, 4 * x.N * out[0] * out[1] * out[2] * y.ld)
        self.steps.append(self._wino(st, pk, x2) or st)
        self.conv_steps.append(st)
        return (y, raw_act) if raw else y

    @staticmethod
    def _conv_geometry(x, pk, stride, padding, same, up2):
        """(input extents the conv slides over, output extents, padding) as (T, H, W) triples."""
        xin = (x.T, x.H * (2 if up2 else 1), x.W * (2 if up2 else 1))
        if same:        # TF-"SAME": out = ceil(in/stride), `padding` is ignored, front pad = total // 2
            out, padding = _same_geometry(xin, pk.k_eff, stride)
        else:
            out = tuple((i + 2 * p_ - k) // s + 1 for i, p_, k, s in zip(xin, padding, pk.k_eff, stride))
        return xin, out, padding

    def _conv_output(self, x, pk, out, y, out_f16, label):
        """The conv's output activation: a new one, or the caller's target `y` checked against the result."""
        To, Ho, Wo = out
        if y is None:
            y = self.act(x.N, To, Ho, Wo, pk.Co, f16=out_f16)
        if bool(y.f16) != bool(out_f16):
            raise PtxError("%s: output precision mismatch" % label)
        if (y.N, y.T, y.H, y.W, y.C) != (x.N, To, Ho, Wo, pk.Co):
            raise PtxError("%s: output target %s does not match the conv result %s" % (
                label, (y.N, y.T, y.H, y.W, y.C), (x.N, To, Ho, Wo, pk.Co)))
        if y.ld != _r4(pk.Co) and pk.Co % 4 and not out_f16:
            raise PtxError("%s: a channel-slice output needs Co %% 4 == 0" % label)
        return y

    def _conv_desc(self, x, pk, y, xin, out, stride, padding, relu, res, res_kind, res_stride, x2, x2_stride, stage, label):
        """Fill the ConvDesc of one launch: operands, fused-stage flags (`stage`: Plan.conv's up2 / affine / out_f16 / raw /
        tanh), output, residual, second source.  Returns (descriptor, residual pointer, fused, ConvFusedExt, raw activation)."""
        # PTX_SPLITK_FUSED=1: split-K launches reduce in-kernel (last-arriving block; the plan's workspace is allocated
        # ZEROED, its first 64 KiB are tile counters every launch leaves at zero).  Off by default: measured SLOWER than
        # the separate reduce launch on MI355X (layer4 3x3x3, split 6: 33 -> 54 us) -- the device-scope release / acquire
        # across the 8 XCD L2s and one block summing what 100+ blocks of the reduce kernel sum in parallel cost more than
        # the launch they save; the tuner answered by abandoning split-K (config 2: 1355 -> 1309 clips/s).
        flags = (PTX_EPI_RELU if relu else 0) | (PTX_SPLITK_FUSED if os.environ.get("PTX_SPLITK_FUSED", "0") == "1" else 0)
        d = ConvDesc()
        d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = x.N, xin[0], xin[1], xin[2], x.C, x.ld
        half, bf16 = bool(x.f16), bool(x.bf16)
        if half != bool(pk.f16):
            raise PtxError("%s: activation and filter precisions differ" % label)
        if bf16 != bool(pk.bf16):
            raise PtxError("%s: activation and filter precisions differ" % label)
        if half:        # fp16 operands: the descriptor counts 32-bit words (channel pairs)
            # bf16: an odd channel count reads its zero pad channel as the pair's second half (rows are 16-byte padded)
            if (x.C % 2 and not bf16) or x.ld % 8 or x2 is not None:
                raise PtxError("%s: fp16 operands need an even channel count and 16-byte rows" % label)
            flags |= PTX_F16_OPERANDS | (PTX_BF16_OPERANDS if bf16 else 0)
            d.Ci, d.ldx = (x.C + 1) // 2, x.ld // 2
        if pk.x3:
            flags |= PTX_F16X3_OPERANDS
        stage_flags, fused, ext, raw_act = self._conv_fused(x, pk, out, half, res, stage, label)
        flags |= stage_flags
        # (a bf16 output of odd width writes its zero pad channel with the pair: bias / filter rows there are zero)
        (d.To, d.Ho, d.Wo), d.Co, d.ldy = out, pk.Co + (pk.Co % 2 if bf16 else 0), y.ld
        (d.kT, d.kH, d.kW), (d.sT, d.sH, d.sW), (d.pT, d.pH, d.pW) = pk.k_eff, stride, padding
        d.Kc, d.Co_pad = (pk.Kc // 2 if half else pk.Kc), pk.Co_pad
        d.groups = pk.groups
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
        if x2 is not None:                      # K-concatenated second activation source (shortcut B)
            d.x2_C, d.x2_ld, d.x2_T, d.x2_H, d.x2_W = x2.C, x2.ld, x2.T, x2.H, x2.W
            d.x2_sT, d.x2_sH, d.x2_sW = _t3(x2_stride)
        return d, resptr, fused, ext, raw_act

    def _conv_fused(self, x, pk, out, half, res, stage, label):
        """Flags and ConvFusedExt of a fused generator stage (ptx_conv3d_fused_fwd): (flags, fused, ext, raw activation)."""
        up2, affine, out_f16, raw, tanh = stage
        fused = bool(up2 or affine is not None or out_f16 or raw or tanh or (res is not None and res.f16))
        if fused and not half:
            raise PtxError("%s: the fused generator-stage options need fp16 operands" % label)
        if not fused:
            return 0, False, None, None
        ext, raw_act = None, None
        flags = (PTX_PRO_UP2 if up2 else 0) | (PTX_EPI_OUT_F16 if out_f16 else 0) | (PTX_EPI_TANH if tanh else 0)
        if res is not None and res.f16:
            flags |= PTX_RES_F16
        if affine is not None or raw:
            ext = ConvFusedExt()
            if affine is not None:
                flags |= PTX_EPI_AFFINE
                ext.scale, ext.shift, ext.ld_affine = affine[0], affine[1], int(affine[2])
            if raw:
                raw_act = self.act(x.N, out[0], out[1], out[2], pk.Co, f16=True)
                flags |= PTX_EPI_DUAL_RAW
                ext.y_raw, ext.ld_raw = raw_act.t.data_ptr(), raw_act.ld
        return flags, True, ext, raw_act

    def _patch_kernel(self, d, fused, bf16, res, raw, tanh, x2, pro_affine, label):
        """Name of the generator-stage kernel (gen_stage_f16.hip: no tile table, nothing to tune) that runs this conv instead
        of an implicit-GEMM tile, or None."""
        if pro_affine is not None:
            # the conv reads the RAW map and applies (scale, shift, ld) + ReLU to its input fragments: ptx_conv1x1_pro_f16_fwd only
            if not (fused and res is None and not raw and not tanh and x2 is None and self.lib.ptx_conv1x1_pro_f16_supported(C.byref(d))):
                raise PtxError("%s: an input affine needs the shapes ptx_conv1x1_pro_f16_fwd covers" % label)
            return "conv1x1_pro_f16"
        if not fused or tanh or x2 is not None:
            return None
        lib = self.lib
        if not bf16:
            # generator stage: a GBlock's 3x3 convs (64 / 128 / 256 channels) and its closing 1x1 conv have their own fp16
            # kernels; PTX_CONV3X3_F16=0 / PTX_CONV1X1_F16=0: A/B runs
            kind, ok3x3, ok1x1 = "f16", lib.ptx_conv3x3_f16_supported, lib.ptx_conv1x1_skip_f16_supported
        elif self.gen_patch:
            # bf16 generator plans: the same two kernels on bf16 operands; PTX_CONV3X3_BF16=0 / PTX_CONV1X1_BF16=0: A/B runs
            kind, ok3x3, ok1x1 = "bf16", lib.ptx_conv3x3_bf16_supported, lib.ptx_conv1x1_skip_bf16_supported
        else:
            return None
        if res is None and not raw and os.environ.get("PTX_CONV3X3_" + kind.upper(), "1") != "0" and ok3x3(C.byref(d)):
            return "conv3x3_" + kind
        if os.environ.get("PTX_CONV1X1_" + kind.upper(), "1") != "0" and ok1x1(C.byref(d)):
            return "conv1x1_skip_" + kind
        return None

    @staticmethod
    def _body_choice(key, body_ok):
        """Body-kernel shape a step starts on: PTX_CONV_BODY=tall / =square force a shape wherever it is supported, else the
        tuned table's verdict ("body:" keys), else None (the implicit-GEMM tile)."""
        force = os.environ.get("PTX_CONV_BODY", "1")
        known = body_lookup(key)
        if force in BODY_SHAPES and BODY_SHAPES.index(force) in body_ok:
            return BODY_SHAPES.index(force)
        return known if known is not None and known in body_ok else None

    def _body_kernel(self, st, pk, x2):
        """The patch-resident 3x3x3 body kernel (round 6): a second execution of the same problem, chosen per problem by
        the tuner ("body:" keys) like a tile; PTX_CONV_BODY=0 keeps every 3x3x3 conv on the implicit-GEMM tiles (A/B runs)."""
        d = st.d
        if (not st.fused and x2 is None and not pk.f16 and not pk.x3 and (d.kT, d.kH, d.kW) in BODY_FILTERS
                and isinstance(pk, Packed) and not pk.fold_kw and os.environ.get("PTX_CONV_BODY", "1") != "0"):
            st.body_ok = tuple(sh for sh in (0, 1) if self.lib.ptx_conv_body_f32_supported(C.byref(d), sh))
        if not st.body_ok:
            return
        wb = torch.empty(int(self.lib.ptx_conv_body_f32_weight_elems(C.byref(d))), device=self.dev, dtype=torch.float32)
        self.keepalive.append(wb)
        st.body_w = _ptr(wb)
        lib_, wsrc, wdst = self.lib, _ptr(pk.w), st.body_w

        def repack_body(d=d, lib_=lib_, wsrc=wsrc, wdst=wdst):
            check(lib_.ptx_pack_conv_body_f32_weight(C.byref(d), wsrc, wdst, _stream()), "ptx_pack_conv_body_f32_weight")
        if torch.device(self.dev).type != "meta":
            self.refreshers.append(repack_body)
        st.body = self._body_choice(json.dumps(d.key()), st.body_ok)

    def _wino(self, st, pk, x2):
        """Winograd F(2x2,3x3) and F(4x4,3x3) (csrc/conv_wino_f32.hip): further executions of a stride-1 (kT,3,3) fp32 conv as
        three launches each -- input transform, a 16- / 36-group (kT,1,1) conv on the ordinary tiles, output transform -- chosen
        per problem by the tuner ("wino:" / "wino4:" keys; default direct).  Returns the WinoStep (Wino4Step where only F(4x4)
        takes the frame: odd H or W) that stands for `st` in the plan, or None when the conv is not eligible or
        PTX_CONV_WINO=0.  The grouped convs are NOT among `conv_steps`: the tuner sweeps their tiles in the Winograd phase, only
        where a verdict is being measured."""
        mode = os.environ.get("PTX_CONV_WINO", "auto")
        d, lib_ = st.d, self.lib
        if (mode == "0" or st.fused or x2 is not None or not isinstance(pk, Packed) or pk.f16 or pk.x3 or pk.fold_kw or pk.groups > 1
                or (d.kH, d.kW) != (3, 3)):
            return None
        ok2, ok4 = bool(lib_.ptx_conv_wino_f32_supported(C.byref(d))), bool(lib_.ptx_conv_wino4_f32_supported(C.byref(d)))
        if not (ok2 or ok4):
            return None
        w = WinoStep() if ok2 else Wino4Step()
        w.direct, w.label, w.key = [st], st.label, json.dumps(d.key())
        if ok2:
            self._wino_form(w, st, pk, 2)
            self.wino_steps.append(w)
        if ok4:
            self._wino_form(w, st, pk, 4)
            self.wino4_steps.append(w)
        self._wino_choice(w)
        return w

    def _wino_form(self, w, st, pk, m):
        """Compile the F(m x m) execution of `st` into `w`: the grouped ConvStep and the two transform launches."""
        d, lib_, tag = st.d, self.lib, "wino" if m == 2 else "wino4"
        fn = {n: getattr(lib_, n % tag) for n in ("ptx_conv_%s_f32_gemm_desc", "ptx_%s_f32_weight_elems", "ptx_pack_%s_f32_weight",
                                                  "ptx_conv_%s_f32_workspace_bytes", "ptx_%s_in_f32", "ptx_%s_out_f32")}
        gd = ConvDesc()
        check(fn["ptx_conv_%s_f32_gemm_desc"](C.byref(d), C.byref(gd)), "ptx_conv_%s_f32_gemm_desc" % tag)
        g = ConvStep()
        g.d, g.b, g.res, g.plan, g.label, g.macs = gd, C.c_void_p(0), C.c_void_p(0), self, "%s.%s_gemm" % (st.label, tag), st.macs
        tuned = tuned_lookup(json.dumps(gd.key()), "")
        if tuned is not None and lib_.ptx_conv3d_config_supported(C.byref(gd), tuned[0]):
            g.cfg, g.from_table = tuned[0], True
        else:
            g.cfg = lib_.ptx_conv3d_pick_config(C.byref(gd), None)
        arena = int(fn["ptx_conv_%s_f32_workspace_bytes"](C.byref(d)))
        v_bytes = arena - 4 * gd.N * gd.To * gd.Ho * gd.Wo * gd.ldy
        w.arena_bytes = max(w.arena_bytes or 0, arena)
        self.wino_bytes = max(self.wino_bytes, arena)
        xp, bp, rp, yp, label = st.x, st.b, st.res, st.y, st.label
        t_in, t_out, mslot = fn["ptx_%s_in_f32"], fn["ptx_%s_out_f32"], "m_ptr" if m == 2 else "m4_ptr"

        def wino_in(stream, w=w, d=d, xp=xp, label=label):
            check(t_in(C.byref(d), xp, w.v_ptr, stream), "%s.%s_in" % (label, tag))

        def wino_out(stream, w=w, d=d, bp=bp, rp=rp, yp=yp, label=label):
            check(t_out(C.byref(d), getattr(w, mslot), bp, rp, yp, stream), "%s.%s_out" % (label, tag))
        pos, tiles = d.N * d.Ti * d.Hi * d.Wi, gd.N * gd.To * gd.Ho * gd.Wo
        form = [_tag(wino_in, tag + "_in", 4 * (pos * d.Ci + tiles * gd.ldx)), g,
                _tag(wino_out, tag + "_out", 4 * (tiles * gd.ldy + pos * d.Co * (2 if d.flags & PTX_EPI_RES_ADD else 1)))]
        wsrc, n_u = _ptr(pk.w), int(fn["ptx_%s_f32_weight_elems"](C.byref(d)))
        pack = fn["ptx_pack_%s_f32_weight"]

        def weights(now=False):
            """Allocate the transformed filter, point the grouped conv at it and register its repack (`now`: the packed
            filters are already in place -- transform this one right away)."""
            u = torch.empty(n_u, device=self.dev, dtype=torch.float32)
            self.keepalive.append(u)
            g.w = wdst = _ptr(u)

            def repack_wino(d=d, wsrc=wsrc, wdst=wdst):
                check(pack(C.byref(d), wsrc, wdst, _stream()), "ptx_pack_%s_f32_weight" % tag)
            if torch.device(self.dev).type != "meta":
                self.refreshers.append(repack_wino)
                if now:
                    repack_wino()
        if m == 2:
            w.wino, w.gemm, w.v_bytes = form, g, v_bytes
            weights()
        else:           # U4 of a 256-channel conv is 28 MB: only where the step can run (wino4_weights)
            w.wino4, w.gemm4, w.v4_bytes, w.need_u4 = form, g, v_bytes, weights

    def wino4_weights(self, w, now=False):
        """Make the F(4x4) execution of `w` runnable: allocate and pack U4 once (a stored verdict, the forced mode, or the tuner
        about to time it)."""
        if w.need_u4 is not None:
            need, w.need_u4 = w.need_u4, None
            need(now)

    def _wino_choice(self, w):
        """The execution of a Winograd-capable step at compile time: PTX_CONV_WINO=1 / =4 force F(2x2) / F(4x4) wherever that
        form exists (a conv without the forced form keeps its `auto` behaviour), else the tuned table's verdicts -- "wino4:"
        first, a missing one means not F(4x4)."""
        mode = os.environ.get("PTX_CONV_WINO", "auto")
        has2, has4 = w.wino is not None, w.wino4 is not None
        if mode == "1" and has2:
            w.use_wino, w.use_wino4 = True, False
        elif mode == "4" and has4:
            w.use_wino, w.use_wino4 = False, True
        else:
            w.use_wino4 = has4 and bool(wino4_lookup(w.key))
            w.use_wino = has2 and not w.use_wino4 and bool(wino_lookup(w.key))

    def _bind_wino_arena(self):
        """One arena for V and M of every Winograd step, sized for the largest need of either form: a step's two buffers are
        live only between its own three launches.  Also the point where the selected F(4x4) steps get their filters."""
        if not self.wino_bytes:
            return
        for w in self.wino4_steps:       # the choice is final here (a pair re-keys its first conv): U4 only where F(4x4) runs
            if w.use_wino4:
                self.wino4_weights(w)
        self.wino_arena = torch.empty(self.wino_bytes // 4, device=self.dev, dtype=torch.float32)
        for st in self.stem_tfir_steps:  # the stem's transformed input: the arena is free while the stem runs
            for form in st.tfir.values():
                form[1].v = _ptr(self.wino_arena)
        for w in set(self.wino_steps + self.wino4_steps):
            w.v_ptr = _ptr(self.wino_arena)
            if w.gemm is not None:
                w.m_ptr = _ptr(self.wino_arena, w.v_bytes // 4)
                w.gemm.x, w.gemm.y = w.v_ptr, w.m_ptr
            if w.gemm4 is not None:
                w.m4_ptr = _ptr(self.wino_arena, w.v4_bytes // 4)
                w.gemm4.x, w.gemm4.y = w.v_ptr, w.m4_ptr

    def _pick_tile(self, st, out_bytes):
        """Tile configuration and split-K of a ConvStep: the tuned table's entry when this build can run it, else the library's
        own pick; and room in the split-K workspace."""
        d = st.d
        tuned = tuned_lookup(json.dumps(d.key()), _flags_kind(d.flags))
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
        want = 8 if out_bytes * 8 <= (128 << 20) else st.split
        self.ws_bytes = max(self.ws_bytes, int(self.lib.ptx_conv3d_workspace_bytes(C.byref(d), want)))

    def conv_chain(self, x, pk, stride, padding, pk2, relu1=True, relu2=False, res=None, label="chain", y=None):
        """conv(x, pk) -> [ReLU] -> 1x1x1 conv (pk2) -> [+ res] -> [ReLU] as ONE launch (ptx_conv3d_chain_fwd): returns (output
        activation, ChainStep) -- the step is NOT appended to the plan; the caller also emits the two separate launches into
        the same output and wraps both with Plan.alt() -- or None when the pair does not qualify.  Qualifies: dense unfolded
        filters of one operand kind (fp32, or split operands in an "x3" plan), a pointwise tail whose K axis is the first conv's output, at most 128 intermediate channels (one N tile
        holds the whole intermediate row), a same-shape residual (or none), and enough rows to fill the chip from M tiles
        alone (the tail's N slices run inside one workgroup: M >= PTX_CHAIN_MIN_M, default 8192)."""
        if not self.chain or isinstance(x, RawInput) or x.f16:
            return None
        for p_ in (pk, pk2):
            if not isinstance(p_, Packed) or p_.f16 or p_.groups > 1 or p_.fold_kw:
                return None
        x3 = bool(pk.x3)
        if x3 != bool(pk2.x3):          # both GEMMs of a chained launch take the same operand kind
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
        if y is not None and ((y.N, y.T, y.H, y.W, y.C) != (x.N, To, Ho, Wo, pk2.Co) or y.f16):
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
        st.macs = M * (pk.Co * pk.real_ci * kT * kH * kW + pk2.Co * pk.Co)
        # the same pair on the patch-resident body kernel with its chained tail (round 6): a second execution of the chained
        # launch, chosen per pair by the tuner ("body:chain:" keys); PTX_CONV_BODY=0 / tall / square as for the plain convs
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
            st.body = self._body_choice(key, st.body_ok)
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
        for w in pair:
            if isinstance(w, _WinoExec):     # the pair's first conv also has a Winograd form: its verdict is the pair's
                w.alt, w.key = a, chain.key
                self._wino_choice(w)
                if w.use_wino or w.use_wino4:
                    a.use_chain = False
        force = os.environ.get("PTX_CHAIN_FORCE")          # "1" / "0": A/B runs
        if force in ("0", "1"):
            a.use_chain = force == "1"
        if a.use_chain:                                    # (a forced chain: the pair's Winograd form does not run)
            for w in pair:
                if isinstance(w, _WinoExec):
                    w.use_wino = w.use_wino4 = False
        self.steps.append(a)
        self.alt_steps.append(a)
        return a

    def conv_bn(self, x, conv, bn, relu=False, res=None, res_kind=None, res_stride=1, label="conv", y=None):
        """nn.Conv{2,3}d or a (2+1)D pair, followed by `bn`, with the epilogue fused."""
        if self.batch_stats and bn is not None:
            return self._conv_bn_batch(x, conv, bn, relu, res, res_kind, res_stride, label, y)
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
        if isinstance(conv, nn.Conv3d) and conv.groups > 1 and conv.groups == conv.in_channels == conv.out_channels:
            return self.conv_dw(x, conv, bn, relu=relu, res=res, label=label, y=y)
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

    def conv_dw(self, x, conv, bn, relu=False, res=None, label="conv_dw", y=None):
        """A depthwise nn.Conv3d (groups == in_channels == out_channels) + `bn` (+ ReLU): one ptx_conv3d_dw_f32_fwd launch on
        its own tap-major pack (include/ptx_amd_dw.h).  fp32 whatever the plan's precision: an "x3" plan runs the same kernel."""
        if self.bf16 or not isinstance(x, Act) or x.f16:
            raise PtxError("%s: the depthwise conv runs on float32 channels-last activations only" % label)
        if res is not None:
            raise PtxError("%s: the depthwise conv takes no residual" % label)
        key = ("dw", id(conv), id(bn))
        if key not in self._pack_cache:
            self._pack_cache[key] = PackedDw(self, conv, bn)
            self.packs.append(self._pack_cache[key])
        pk = self._pack_cache[key]
        k, s, p = _geom(conv)
        if x.C != pk.C:
            raise PtxError("%s: a %d-channel depthwise conv on a %d-channel input" % (label, pk.C, x.C))
        out = tuple((i + 2 * p_ - k_) // s_ + 1 for i, p_, k_, s_ in zip((x.T, x.H, x.W), p, k, s))
        if y is None:
            y = self.act(x.N, out[0], out[1], out[2], pk.C)
        if (y.N, y.T, y.H, y.W, y.C) != (x.N,) + out + (pk.C,) or y.f16:
            raise PtxError("%s: output target %s does not match the conv result %s" % (
                label, (y.N, y.T, y.H, y.W, y.C), (x.N,) + out + (pk.C,)))
        d = ConvDesc()
        d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = x.N, x.T, x.H, x.W, x.C, x.ld
        (d.To, d.Ho, d.Wo), d.Co, d.ldy = out, pk.C, y.ld
        (d.kT, d.kH, d.kW), (d.sT, d.sH, d.sW), (d.pT, d.pH, d.pW) = k, s, p
        d.groups, d.flags = pk.C, (PTX_EPI_RELU if relu else 0)
        if min(out) < 1 or not self.lib.ptx_conv3d_dw_f32_supported(C.byref(d)):
            raise PtxError("%s: %s" % (label, self.lib.ptx_last_error().decode(errors="replace") if min(out) >= 1 else "empty output"))
        st = DwConvStep()
        st.d, st.x, st.w, st.b, st.y, st.label = d, _ptr(x.t), _ptr(pk.w), _ptr(pk.b), _ptr(y.t), label
        npos = x.N * out[0] * out[1] * out[2]
        st.macs = npos * pk.C * k[0] * k[1] * k[2]
        st.hbm_bytes = 4 * pk.C * (x.N * x.S + npos)
        self.steps.append(st)
        return y

    def _conv_bn_batch(self, x, conv, bn, relu, res, res_kind, res_stride, label, y):
        """conv_bn of a batch-statistics plan: the raw conv (bn=None: no fold, no activation, no residual -- on whatever
        tiles / Winograd execution the library picks), then the BN on this batch's own moments, in place on the conv's output."""
        if y is not None:
            raise PtxError("%s: a batch-statistics plan writes no channel-slice targets" % label)
        if hasattr(conv, "spatial_conv"):      # (2+1)D pair: its inner conv.bn takes batch statistics as well
            mid = self.conv_bn(x, conv.spatial_conv, conv.bn, relu=True, label=label + ".spatial")
            raw = self.conv_bn(mid, conv.temporal_conv, None, label=label + ".temporal")
        elif isinstance(conv, (nn.Conv3d, nn.Conv2d)):
            raw = self.conv_bn(x, conv, None, label=label)
        else:
            raise PtxError("%s: update_bn does not cover %s convs: it runs %s" % (label, type(conv).__name__, BATCH_STATS_SCOPE))
        return self.bn_batch(raw, bn, relu, res, res_kind, res_stride, label + ".bn", y=raw)

    def bn_batch(self, x, bn, relu, res=None, res_kind=None, res_stride=1, label="bn", y=None):
        """Train()-mode BatchNorm of a batch-statistics plan on activation x, as three steps: the batch moments
        (ptx_bn_batch_stats_f32), this batch's scale / shift + the running-statistics update (ptx_bn_batch_update_f32),
        and y = act(x * scale + shift [+ res]) (ptx_bn_apply_f32; y may be x itself)."""
        if not isinstance(bn, (nn.BatchNorm3d, nn.BatchNorm2d)) or not bn.track_running_stats or bn.running_mean is None:
            raise PtxError("%s: update_bn needs nn.BatchNorm2d / nn.BatchNorm3d layers that track running statistics (got %s)" % (
                label, type(bn).__name__))
        if x.f16 or bn.num_features != x.C:
            raise PtxError("%s: a %d-feature BatchNorm on a %d-channel %s activation" % (label, bn.num_features, x.C, x.t.dtype))
        n = x.N * x.S
        if n <= 1:      # F.batch_norm(training=True) raises ValueError here; the shapes are known now, nothing is launched
            raise PtxError("%s: Expected more than 1 value per channel when computing batch statistics, got input size [%d, %d, %d, %d, %d]"
                           % (label, x.N, x.C, x.T, x.H, x.W))
        if y is None:
            y = self.act(x.N, x.T, x.H, x.W, x.C)
        f32 = dict(device=self.dev, dtype=torch.float32)
        mean, var, scale, shift = (torch.empty(_r4(x.C), **f32) for _ in range(4))
        self.keepalive += [mean, var, scale, shift]
        index = len(self.bn_steps)
        off = sum(_r4(c) for _, c in self.bn_sizes)
        ref = self.ref(bn)
        self.bn_refs.append(ref)
        self.bn_sizes.append((off, x.C))
        self.bn_f.append(1.0)
        self.bn_ws_bytes = max(self.bn_ws_bytes, int(self.lib.ptx_bn_batch_stats_workspace_bytes(n, x.C)))
        st = BnStatsStep()
        st.plan, st.index, st.x, st.rows, st.C, st.ld, st.mean, st.var = self, index, _ptr(x.t), n, x.C, x.ld, _ptr(mean), _ptr(var)
        st.label, st.hbm_bytes = label + ".stats", 4 * n * x.C
        up = BnUpdateStep()
        up.plan, up.index, up.off, up.n, up.C, up.eps, up.bn = self, index, off, n, x.C, float(bn.eps), ref
        up.mean, up.var, up.scale, up.shift, up.label = st.mean, st.var, _ptr(scale), _ptr(shift), label + ".update"
        d = BnApplyDesc()
        d.N, d.T, d.H, d.W, d.C, d.ldx, d.ldy = x.N, x.T, x.H, x.W, x.C, x.ld, y.ld
        d.flags = PTX_EPI_RELU if relu else 0
        if res is not None:
            d.ldr = res.ld
            if res_kind == "padA":
                d.flags |= PTX_EPI_RES_PADA
                d.res_C, d.res_T, d.res_H, d.res_W = res.C, res.T, res.H, res.W
                d.res_sT = d.res_sH = d.res_sW = int(res_stride)
            elif res_kind is None:
                d.flags |= PTX_EPI_RES_ADD
                assert (res.N, res.T, res.H, res.W, res.C) == (x.N, x.T, x.H, x.W, x.C), "residual shape"
            else:
                raise PtxError("%s: residual kind %r has no batch-statistics form" % (label, res_kind))
        ap = BnApplyStep()
        ap.d, ap.raw, ap.scale, ap.shift, ap.y, ap.label = d, st.x, up.scale, up.shift, _ptr(y.t), label + ".apply"
        ap.res = _ptr(res.t) if res is not None else C.c_void_p(0)
        ap.hbm_bytes = 4 * n * x.C * (3 if res is not None else 2)
        self.steps += [st, up, ap]
        self.bn_steps.append(st)
        return y

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
        self.stem_steps += 1
        return y

    def stem_bf16(self, raw, conv, bn, relu, label):
        """bf16 RGB stem (conv1 of ResNet3D, resnet3D.py:153-155; the (1,7,7) spatial stem of R2Plus1D, r2plus1d.py:73-88):
        ptx_im2col_hw_bf16 folds the (kh, kw) taps of the caller's bf16 NCDHW clip into 147 channels (rows padded to 160),
        and the stem becomes a (kT, 1, 1) conv over them on the bf16 tiles -- 160 / 147 = 1.09x the algorithmic MACs
        issued (plus tile padding), no torch layout pass."""
        direct = self.bf16_stem == "direct"
        # a sub-sampled stem (input[:, :, ::step]) and every SlowFast stem: the direct kernel's frame-strided entry, and no
        # fold fallback (a time-strided im2col does not exist; at 224 x 224 the fold would write 13x the fast clip)
        strided = direct and isinstance(conv, nn.Conv3d) and (raw.t_step != 1 or self.kind == "slowfast")
        # a 2-D ResNet's Conv2d stem: the direct kernel's kT = 1 case on T = 1 (Plan._build lets 2-D models in under "direct" only)
        conv2d = direct and isinstance(conv, nn.Conv2d) and raw.T == 1 and raw.t_step == 1
        if (raw.norm is not None and not direct) or (raw.t_step != 1 and not strided) or not (isinstance(conv, nn.Conv3d) or conv2d):
            raise PtxError("%s: the bf16 stem reads a bf16 NCDHW clip (uint8 frames / frame sub-sampling are fp32 only%s)" % (
                label, "" if direct else "; Engine.bf16_stem = 'direct' reads uint8 frames"))
        (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = _geom(conv)
        if getattr(conv, "tf_same", False):
            raise PtxError("%s: SAME-padded stems are not supported in bf16" % label)
        Ho, Wo = (raw.H + 2 * pH - kH) // sH + 1, (raw.W + 2 * pW - kW) // sW + 1
        if min(Ho, Wo) < 1:
            raise PtxError("%s: input too small for the stem" % label)
        if direct:
            y = self.stem_bf16_direct(raw, conv, bn, relu, label, strided)
            if y is not None:
                return y
        if conv2d:                       # no fold route behind a Conv2d stem
            raise PtxError("%s: the direct bf16 stem cannot run this 2-D stem: %s" % (
                label, self.lib.ptx_last_error().decode(errors="replace")))
        K = kH * kW * raw.C
        xf = self.act(raw.N, raw.T, Ho, Wo, K, ld=(K + 31) // 32 * 32, f16=True)
        lib, yp = self.lib, _ptr(xf.t)
        N, Cc, T, H, W, ld = raw.N, raw.C, raw.T, raw.H, raw.W, xf.ld

        def im2col(st, self=self):
            check(lib.ptx_im2col_hw_bf16(self.in_ptr, yp, N, Cc, T, H, W, kH, kW, sH, sW, pH, pW, Ho, Wo, ld, st), "ptx_im2col_hw_bf16")
        self.steps.append(_tag(im2col, "im2col_hw_bf16", 2 * N * Cc * T * H * W + 2 * xf.t.numel()))
        y = self.conv(xf, self.pack(conv, bn, fold_hw=True), (sT, 1, 1), (pT, 0, 0), relu=relu, label=label)
        self.stem_bf16_step = self.conv_steps[-1]
        self.stem_steps += 1
        return y

    def stem_bf16_direct(self, raw, conv, bn, relu, label, strided=False):
        """Engine.bf16_stem = "direct": ONE ptx_conv_stem_bf16_fwd launch reads the caller's bf16 NCDHW clip -- or the decoded
        uint8 frames, normalised while the patch is staged -- and serves every (kh, kw) tap from an LDS-resident patch: no
        im2col pass, no 160-channel copy.  The filter is the fold path's own packed filter (same BN fold, same single
        rounding), re-laid bit-exactly into the kernel's fragment order.  Returns None when the kernel refuses a bf16-clip
        geometry (the fold path then runs); a refused uint8 geometry raises with the kernel's reason.
        strided: ptx_conv_stem_bf16_strided_fwd on every raw.t_step-th of raw.T_full frames (SlowFast's pathways); a refused
        geometry raises for either source -- there is no fold path behind a sub-sampled stem."""
        (kT, kH, kW), (sT, sH, sW), (pT, pH, pW) = _geom(conv)
        To, Ho, Wo = (raw.T + 2 * pT - kT) // sT + 1, (raw.H + 2 * pH - kH) // sH + 1, (raw.W + 2 * pW - kW) // sW + 1
        Co = conv.out_channels
        d = ConvDesc()
        d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = raw.N, raw.T, raw.H, raw.W, raw.C, 0
        d.To, d.Ho, d.Wo, d.Co, d.ldy = To, Ho, Wo, Co, _r8(Co)
        d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = kT, kH, kW, sT, sH, sW, pT, pH, pW
        d.Co_pad = _r128(Co)
        d.flags = PTX_F16_OPERANDS | PTX_BF16_OPERANDS | PTX_EPI_OUT_F16 | (PTX_EPI_RELU if relu else 0)
        src = PTX_STEM_SRC_U8_NTHWC if raw.norm is not None else PTX_STEM_SRC_BF16_NCDHW
        lib = self.lib
        if strided:
            if To < 1 or not lib.ptx_conv_stem_bf16_strided_supported(C.byref(d), src, raw.t_step, raw.T_full):
                raise PtxError("%s: the direct bf16 stem cannot read frames 0, %d, .. of %d %s: %s" % (
                    label, raw.t_step, raw.T_full, "bf16 frames" if raw.norm is None else "uint8 frames",
                    lib.ptx_last_error().decode(errors="replace") if To >= 1 else "input too short for the stem"))
        elif To < 1 or not lib.ptx_conv_stem_bf16_supported(C.byref(d), src):
            if raw.norm is not None:
                raise PtxError("%s: the direct bf16 stem cannot read these uint8 frames: %s" % (
                    label, lib.ptx_last_error().decode(errors="replace") if To >= 1 else "input too short for the stem"))
            return None
        pk = self.pack(conv, bn, fold_hw=True)           # [kT][Co_pad][Kc] bf16, k = (kh*kW + kw)*Cin + c: the fold path's filter
        w2 = torch.empty(lib.ptx_stem_bf16_weight_elems(C.byref(d)), device=self.dev, dtype=torch.bfloat16)
        self.keepalive.append(w2)
        wsrc, w2p = _ptr(pk.w), _ptr(w2)

        def relay():
            check(lib.ptx_pack_stem_bf16_weight(C.byref(d), wsrc, w2p, _stream()), "ptx_pack_stem_bf16_weight")
        self.refreshers.append(relay)
        y = self.act(raw.N, To, Ho, Wo, Co, f16=True)
        st = StemBf16Step()
        st.d, st.plan, st.src, st.w, st.b, st.y, st.label = d, self, src, w2p, _ptr(pk.b), _ptr(y.t), label
        if raw.norm is not None:
            st.norm = raw.norm
            self.keepalive.append(raw.norm)
        if strided:
            st.frame_step, st.T_full = raw.t_step, raw.T_full
        st.macs = raw.N * To * Ho * Wo * Co * raw.C * kT * kH * kW
        # compulsory traffic: the clip (or the frames; the raw.T = ceil(T_full / t_step) frames that are read) once in, the
        # bf16 activation out, the filter
        st.hbm_bytes = raw.N * raw.C * raw.T * raw.H * raw.W * (1 if raw.norm is not None else 2) + 2 * y.t.numel() + 2 * w2.numel()
        self.steps.append(st)
        self.stem_steps += 1
        return y

    def stem_direct_f32(self, raw, conv, bn, relu, label):
        """fp32 stems skip the kW fold as well: ptx_conv_stem_f32_fwd LDS-DMAs the input patch of a temporal tap from the
        user's NCDHW tensor (frame sub-sampling is a stride) and serves every (kh, kw) tap from it.  Returns None when the
        kernel does not cover the geometry (the folded implicit-GEMM path then runs)."""
        if not isinstance(conv, (nn.Conv3d, nn.Conv2d)) or raw.C != 3:
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
        self._stem_tfir(st, raw, w2p)
        self.steps.append(st)
        self.stem_steps += 1
        return y

    def _stem_tfir(self, st, raw, w_stem):
        """Temporal fast-FIR executions of a 7x7x7 stride-1-in-time fp32 stem (csrc/conv_stem_tfir_f32.hip): per scheme two
        launches, the temporal input transform into V and the forward over V, chosen against the direct launch by the tuner
        ("tfir:" keys; default direct).  PTX_STEM_TFIR=0 compiles none, =1|2|3 forces a scheme where the library takes the
        problem, auto compiles the schemes the tuner may time (TFIR_SCHEMES).  Decoded uint8 frames and padded-pitch clips run the same
        forms from the plan-owned fp32 buffer, under the same key, so frames and clips keep producing identical bits.  V lives
        in the Winograd arena; the transformed filters (about 1 MB each) are packed with the plan."""
        mode = os.environ.get("PTX_STEM_TFIR", "auto")
        if mode == "0":
            return
        d, lib_ = st.d, self.lib
        schemes = (int(mode),) if mode in ("1", "2", "3") else TFIR_SCHEMES
        forms = {}
        for sid in schemes:
            if not lib_.ptx_conv_stem_tfir_f32_supported(C.byref(d), *st.strides, sid):
                continue
            m, P = C.c_int32(), C.c_int32()
            check(lib_.ptx_stem_tfir_scheme(sid, C.byref(m), C.byref(P), None, None, None), "ptx_stem_tfir_scheme")
            u = torch.empty(lib_.ptx_stem_tfir_f32_weight_elems(C.byref(d), sid), device=self.dev, dtype=torch.float32)
            self.keepalive.append(u)
            up = _ptr(u)

            def repack_tfir(sid=sid, up=up):
                check(lib_.ptx_pack_stem_tfir_f32_weight(C.byref(d), sid, w_stem, up, _stream()), "ptx_pack_stem_tfir_f32_weight")
            if torch.device(self.dev).type != "meta":
                self.refreshers.append(repack_tfir)
            v_bytes = int(lib_.ptx_stem_tfir_f32_workspace_bytes(C.byref(d), sid))
            self.wino_bytes = max(self.wino_bytes, v_bytes)
            f = StemTfirStep()
            f.d, f.scheme, f.m, f.P, f.w, f.b, f.y, f.macs = d, sid, m.value, P.value, up, st.b, st.y, st.macs
            f.label = "%s.tfir%d" % (st.label, sid)

            def tfir_in(stream, f=f, sid=sid, st=st):
                x = st.src if st.src is not None else self.in_ptr
                check(lib_.ptx_stem_tfir_in_f32(C.byref(d), sid, x, *st.strides, f.v, stream), f.label + "_in")
            forms[sid] = [_tag(tfir_in, "tfir%d_in" % sid, 4 * raw.N * 3 * raw.T * raw.H * _r4(raw.W) + v_bytes), f]
        if not forms:
            return
        st.tfir, st.key = forms, json.dumps(d.key() + tuple(st.strides))
        if mode in ("1", "2", "3"):
            st.use_tfir = int(mode)
        else:
            known = tfir_lookup(st.key)
            st.use_tfir = known if known in forms else 0
        self.stem_tfir_steps.append(st)

    def stem_source(self, raw, pitch):
        """The fp32 NCDHW tensor a direct stem kernel reads, as a device pointer -- or None when that is the caller's own
        tensor (fp32 clips whose rows already have a 16-byte pitch: bound per run, plan.in_ptr).  Otherwise the plan owns
        it and fills it first: decoded uint8 frames [N,T,H,W,C] are normalised by ptx_frames_u8_to_ncdhw (TransformImage's
        tensor half, transforms/utils.py:72-75; bit-identical to the CPU ops) -- 1 B in, 4 B out per sample, ~5 % of the
        bytes the kW fold moved -- and rows whose width is not a multiple of 4 are copied to a zero-padded pitch
        (ptx_pad_rows).  Built once per plan: both SlowFast pathways read the same buffer through their own frame stride."""
        key = (raw.norm is not None, pitch)
        cache = self._stem_src
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
        # (bf16 plans: the caller's bf16 NCDHW input, channels [C, ld) zero-filled)
        y = self.act(raw.N, raw.T, raw.H, raw.W, raw.C, f16=self.bf16)
        name, esz = ("ncdhw_to_ndhwc_bf16", 2) if self.bf16 else ("ncdhw_to_ndhwc", 4)
        fn, yp = getattr(self.lib, "ptx_" + name), _ptr(y.t)
        N, C_, S, ld = raw.N, raw.C, raw.T * raw.H * raw.W, y.ld

        def step(st, self=self):
            check(fn(self.in_ptr, yp, N, C_, S, ld, st), "ptx_" + name)
        self.steps.append(_tag(step, name, esz * N * C_ * S + esz * y.t.numel()))
        return y

    def maxpool(self, x, k, s, p=None, y=None, same=False):
        """max_pool3d.  same=True: TF-"SAME" geometry (out = ceil(in/stride), front pad = total//2) with
        zero-valued padding -- F.pad followed by an unpadded MaxPool3d, as I3D ports do."""
        if same:
            (To, Ho, Wo), p = _same_geometry((x.T, x.H, x.W), k, s)
        else:
            To = (x.T + 2 * p[0] - k[0]) // s[0] + 1
            Ho = (x.H + 2 * p[1] - k[1]) // s[1] + 1
            Wo = (x.W + 2 * p[2] - k[2]) // s[2] + 1
        bf16 = bool(x.bf16)
        if y is None:
            y = self.act(x.N, To, Ho, Wo, x.C, x.ld, f16=bf16)
        assert (y.N, y.T, y.H, y.W, y.C) == (x.N, To, Ho, Wo, x.C), "pool output shape"
        assert bool(y.bf16) == bf16, "pool output precision"
        d = PoolDesc(x.N, x.T, x.H, x.W, x.C, x.ld, To, Ho, Wo, k[0], k[1], k[2], s[0], s[1], s[2], p[0], p[1], p[2],
                     y.ld, ((PTX_POOL_SAME | PTX_POOL_PAD_ZERO) if same else 0) | (PTX_POOL_BF16 if bf16 else 0))
        lib, xp, yp = self.lib, _ptr(x.t), _ptr(y.t)
        self.keepalive.append(d)

        def step(st):
            check(lib.ptx_maxpool3d_fwd(C.byref(d), xp, yp, st), "ptx_maxpool3d_fwd")
        esz = 2 if x.f16 else 4
        self.steps.append(_tag(step, "maxpool3d", esz * (x.N * x.S * x.C + y.N * To * Ho * Wo * x.C)))
        return y

    def attention(self, th, ph, g, y, scale_only=False, f16=False, relu=False):
        """y = softmax(th . ph^T) . g  (or (th . ph^T / Nk) . g, or (relu(th . ph^T) / Nk) . g) per sample, as one
        ptx_nonlocal_fwd launch.  th [N, Sq, d], ph [N, Sk, d], g [N, Sk, dv], y [N, Sq, dv]: channels-last activations
        (possibly channel slices).  Returns False -- nothing emitted -- when the fused kernel does not cover the shape
        (d > 1024) or PTX_NL_FUSED=0 asks for the unfused bgemm / softmax / bgemm chain."""
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
            if y.f16:                                  # ... whose output conv reads halfs
                d.mode |= PTX_NL_OUT_F16
        elif self.x3 and os.environ.get("PTX_NL_X3", "1") != "0":      # split operands, like the plan's convs
            d.mode |= PTX_NL_X3
        if y.f16 and not (d.mode & PTX_NL_F16):
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
        self.attn_steps += 1
        return True

    def attention_bf16(self, th, ph, g, y, scale_only=False, relu=False):
        """bf16 plans: the same attention as one ptx_nonlocal_bf16_fwd launch (bf16 operands on the bf16 matrix cores, fp32
        accumulate and softmax state; P and y rounded to bf16 once).  Every operand is a bf16 activation whose pad channels
        up to round8(C) are zero (the kernel contracts over them); y's columns [0, round8(dv)) are written."""
        if not all(a.bf16 for a in (th, ph, g, y)):
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
        self.attn_steps += 1
        self.attn_descs.append(d)
        self.attn_variants.append(int(lib.ptx_nonlocal_bf16_variant(C.byref(d))))
        self.attn_operands.append((th, ph, g, y))
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


        def project():       # W (+ BN) + residual in one launch
            wpk = self.pack(nl.W[0], nl.W[1]) if getattr(nl, "bn_layer", True) else self.pack(nl.W, None)
            return self.conv(yatt, wpk, one, zero, res=x, label=label + ".W")
        if mode == "concatenation":
            fused = self.concat_attention(th_act, ph_act, g_act, yatt, nl, label)
        else:
            fused = self.attention(th_act, ph_act, g_act, yatt, scale_only=(mode == "dot_product"))
        if fused:
            # theta^T phi -> softmax (or 1/N) -> . g in ONE launch: the [N, Sq, Sk] affinity never reaches HBM
            return project()
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
        return project()

    # ---------------------------------------------------------------- network
    def _build(self, model):
        kind = self.kind = getattr(model, "plan_kind", "resnet")
        if self.bf16:
            name = str(getattr(model, "arch_name", None) or type(model).__name__)
            arch = getattr(model, "arch", None)
            # SlowFast / SlowOnly / FastOnly: only on the frame-strided direct stem (both pathways read input[:, :, ::step])
            if kind == "slowfast" and self.bf16_stem != "direct":
                raise PtxError("bf16 SlowFast runs on the direct bf16 stem only (its pathways sub-sample the clip in time): set "
                               "Engine.bf16_stem = 'direct' (PTX_BF16_STEM=direct), or run %s in float32" % name)
            # a ResNet3D / R(2+1)D with non-local blocks: on the direct bf16 stem only (the contract SlowFast got)
            nl_net = (kind == "resnet" and arch is not None and bool(arch.nonlocal_layers) and _bf16_base(name) in BF16_FAMILIES
                      and arch.dims == 3 and arch.block in ("basic", "bottleneck"))
            if nl_net and self.bf16_stem != "direct":
                raise PtxError("bf16 non-local ResNets run on the direct bf16 stem only: set Engine.bf16_stem = 'direct' "
                               "(PTX_BF16_STEM=direct), or run %s in float32" % name)
            # the 2-D ResNets (resnet18..152): on the direct bf16 stem only, as well
            net_2d = (kind == "resnet" and arch is not None and arch.dims == 2 and name in BF16_FAMILIES_2D
                      and not arch.nonlocal_layers and arch.block in ("basic", "bottleneck"))
            if net_2d and self.bf16_stem != "direct":
                raise PtxError("bf16 2-D ResNets run on the direct bf16 stem only (its kT = 1 case; there is no fold route for a "
                               "Conv2d stem): set Engine.bf16_stem = 'direct' (PTX_BF16_STEM=direct), or run %s in float32" % name)
            # the standalone non-local blocks and MNISTNonLocalNet run on the bf16 attention kernel
            if not nl_net and not net_2d and kind not in BF16_NL_KINDS + BF16_GEN_KINDS + ("slowfast",) and (
                    kind != "resnet" or name.split("@")[0] not in BF16_FAMILIES or arch is None or arch.nonlocal_layers
                    or arch.dims != 3 or arch.block not in ("basic", "bottleneck")):
                raise PtxError("bf16 inference covers the ResNet3D (resnet3d10..200) and R(2+1)D (r2plus1d10..50) families, "
                               "the non-local blocks, the BigGAN-deep generator and (under bf16_stem = 'direct') SlowFast, "
                               "the non-local ResNets and the 2-D ResNets (resnet18..152); "
                               "%s (plan kind %r) has bf16 parameters: run it in float32" % (name, kind))
        if kind == "nlblock":                    # a standalone NonLocalBlock3D: [B,C,T,H,W] -> [B,C,T,H,W]
            N, Cc, T, H, W = self.shape
            self.feat = self.nonlocal_block(self.to_channels_last(RawInput(N, Cc, T, H, W)), model, "nl")
            self.pooled = None
            return
        if kind != "resnet":                     # SlowFast / I3D / BigGAN-deep: plans.py
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
        if arch.dims == 2 or arch.block.startswith("csn"):       # (the CSN stem keeps every frame: MaxPool3d((1,3,3), (1,2,2), (0,1,1)))
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
        if arch.block.startswith("csn"):
            return self._block_csn(arch, blk, x, name, out)
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
                # (a batch-statistics plan chains nothing, and must not even pack the BN-folded filters of the pair)
                tail = None if not plain_tail or self.batch_stats else self.conv_chain(o, self.pack(blk.conv2, blk.bn2), s2, p2, self.pack(blk.conv3, blk.bn3), relu1=True,
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

    def _block_csn(self, arch, blk, x, name, out=None):
        """A channel-separated bottleneck (Tran et al., ICCV 2019): conv1 1x1x1 + bn1 + ReLU -> [ip-CSN: conv2_pw 1x1x1 + bn2_pw]
        -> conv2 DEPTHWISE 3x3x3 (the block's stride) + bn2 + ReLU -> conv3 1x1x1 + bn3 + residual + ReLU.  The pointwise convs
        are the GEMMs every bottleneck runs -- shortcut B folded into conv3's K axis where the plan fuses shortcuts -- and the
        depthwise conv is one streaming launch (conv_dw)."""
        o = self.conv_bn(x, blk.conv1, blk.bn1, relu=True, label=name + ".conv1")
        if arch.block == "csn_ip":
            o = self.conv_bn(o, blk.conv2_pw, blk.bn2_pw, label=name + ".conv2_pw")
        o = self.conv_bn(o, blk.conv2, blk.bn2, relu=True, label=name + ".conv2")
        if blk.has_shortcut and self.fuse_shortcut and arch.shortcut == "B":
            pk = self.pack_dual(blk.conv3, blk.bn3, blk.downsample[0], blk.downsample[1])
            return self.conv(o, pk, (1, 1, 1), (0, 0, 0), relu=True, x2=x, x2_stride=_geom(blk.downsample[0])[1], y=out,
                             label=name + ".conv3+downsample")
        if blk.has_shortcut and arch.shortcut == "B":
            res, kind = self.conv_bn(x, blk.downsample[0], blk.downsample[1], label=name + ".downsample"), None
        else:
            res, kind = x, ("padA" if blk.has_shortcut else None)
        return self.conv_bn(o, blk.conv3, blk.bn3, relu=True, res=res, res_kind=kind, res_stride=blk.stride,
                            label=name + ".conv3", y=out)

    def bn_relu(self, x, bn, label):
        """Eval-mode BN -> ReLU as one HBM pass ahead of a conv (pre-activation blocks): the BN is folded to
        a per-channel affine by ptx_cbn_fold whenever the weights change."""
        if self.batch_stats:    # this batch's own moments; x stays as it is (the residual reads it)
            return self.bn_batch(x, bn, True, label=label)
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
            if not isinstance(st, ConvStep) or st.fused or st.body is not None:
                return False
            d = st.d
            ok_flags = PTX_EPI_RELU | PTX_EPI_RES_ADD | PTX_SPLITK_FUSED
            return (d.flags & ~ok_flags) == 0 and d.groups <= 1 and d.N * d.To * d.Ho * d.Wo <= max_m

        def make(run):
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
        if self.head_error:
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
            for t in (s.active() if isinstance(s, (AltStep, ProgramStep, _WinoExec, StemF32Step)) else [s]):
                if isinstance(t, (ConvStep, ChainStep, StemStep, StemF32Step, StemTfirStep, StemBf16Step, PatchConvStep, ProgramStep)):
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
        if self.bf16 and self.head32 is not None:
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
        cur = self.head32
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
