"""Forward-pass engine: runs a zoo model as the list of libptx_amd launches its plan holds.

Design (MI355X-first, not a translation of the reference's nn.Module graphs):
  * one *plan* per (input shape, device): every activation buffer is allocated once
    (channels-last NDHWC fp32, sized for 288 GB of HBM -- no reuse games), every conv descriptor,
    tile configuration and split-K factor is fixed at compile time, weights are BN-folded and
    re-laid-out K-major once (`ptx_pack_conv_weight`) and only re-packed when a parameter changes;
  * running a plan is a straight sequence of asynchronous C-ABI calls on torch's current HIP
    stream -- no synchronisation, no allocation except the returned tensor -- so a forward can be
    captured into a hipGraph and replayed (`Engine.use_graph`, PTX_GRAPH=1);
  * there is no eager / CPU fallback: CPU tensors, training mode or a missing library raise.

torch is used for device memory (torch.empty), streams and parameter storage only.

Module layout: this module keeps `Engine` (the per-model executor: plan cache, weight signatures, the forward entry
points) and `EngineOwner`.  The tuned table is tuned.py, the launch records steps.py, the plan compiler plan.py (family
builders: plans.py), autotune and profiling tuner.py, the launches outside a plan heads.py.  Their names are re-exported
here, so `pretorched_x_amd.engine` stays the one import point for tests and scripts.
"""
import collections
import ctypes as C
import json
import os
import threading
import weakref

import torch
import torch.nn as nn

from . import _lib, tuner
from ._lib import NormDesc, PtxError, check
from .heads import check_views, linear, relation_mlp, relation_scale, run_views, views_chunk, views_mean  # noqa: F401
from .plan import BATCH_STATS_SCOPE, BF16_FAMILIES, BF16_GEN_KINDS, BF16_NL_KINDS, Plan, _foldable, check_batch_stats_scope, model_precision  # noqa: F401
from .steps import (Act, AltStep, ChainStep, ConvStep, Packed, PackedDual, PatchConvStep, ProgramStep, RawInput, Wino4Step, WinoStep, _WinoExec,  # noqa: F401
                    StemBf16Step, StemF32Step, StemStep, StemTfirStep, _ConcatRowsPack, _Ref, _dense16, _device_ctx, _geom, _ptr, _r4, _r8, _r128,
                    _same_geometry, _stem_ld, _stream, _t3, _tag, _tile_dims, issued_conv_flop)
from .tuned import (BODY_FILTERS, BODY_SHAPES, _TUNED_PATH, _chain_config_index, _config_index, _flags_kind,  # noqa: F401
                    _tile_kind, _tuned_table, alt_lookup, alt_store, body_lookup, body_store, chain_key, chain_lookup,
                    chain_store, lanes_key, lanes_lookup, lanes_store, prog_lookup, prog_store, save_tuned_table, tuned_lookup,
                    tuned_merge, tuned_replace, tuned_snapshot, tuned_store)


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
        self.head32 = None               # bf16 logits(): fp32 copy of the classifier (Plan.head32_refresh, held here)
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
        # Stem of the bf16 plans (opt-in, like PTX_PROGRAM / PTX_NL_STREAMK):
        #   "fold"    (default) ptx_im2col_hw_bf16 + a (kT,1,1) conv on the generic bf16 tiles; bf16 models take bf16 clips only;
        #   "direct"  ptx_conv_stem_bf16_fwd: one patch-resident kernel that reads the bf16 clip -- or decoded uint8 frames,
        #             normalised while they are staged, so forward_frames / frames-out forward_views accept bf16 models.
        #             It also reads every step-th frame (ptx_conv_stem_bf16_strided_fwd): bf16 SlowFast runs under it only.
        #             A Conv2d stem is its kT = 1 case: the bf16 2-D ResNets (and so a bf16 TRN) run under it only as well.
        # Changing it drops the compiled plans.  Same operands as "fold", another summation order.
        self._bf16_stem = "fold"
        self.bf16_stem = os.environ.get("PTX_BF16_STEM", "fold")
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

    @property
    def bf16_stem(self):
        return self._bf16_stem

    @bf16_stem.setter
    def bf16_stem(self, value):
        if value not in ("fold", "direct"):
            raise PtxError("Engine.bf16_stem must be 'fold' or 'direct' (got %r)" % (value,))
        if value != self._bf16_stem:
            self._bf16_stem = value
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

    def dry_plan(self, model, shape, batch_stats=False):
        """Compile a plan on the 'meta' device: every descriptor, tile choice and buffer shape is
        produced, nothing is allocated or launched.  Host-logic tests use this without a GPU.
        batch_stats: the batch-statistics flavour update_bn runs -- always ONE plan for the whole batch, whatever `lanes` says."""
        return Plan(self, model, shape, torch.device("meta"), batch_stats=batch_stats)

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

    def plan_for(self, model, x, shape=None, norm=None, lane=0, batch_stats=False):
        """shape / norm: the NCDHW view and NormDesc of a uint8-frames input (forward_frames).  lane: which of the
        Engine.lanes concurrent slices this plan serves -- lanes of one shape are separate plans (separate buffers).
        batch_stats: the batch-statistics flavour of this shape (update_bn), a plan of its own next to the eval plan."""
        shape = tuple(x.shape) if shape is None else tuple(shape)
        nkey = None if norm is None else (tuple(norm.mean), tuple(norm.std), norm.swap_rb, norm.to_255)
        key = (shape, x.device.index, nkey) + ((lane,) if lane else ()) + (("batch_stats",) if batch_stats else ())
        if model_precision(model) == "bf16":
            key += ("bf16",) + (("direct",) if self._bf16_stem == "direct" else ())
        with self._lock:
            plan = self._plans.get(key)
            fresh = plan is None
            if fresh:
                plan = Plan(self, model, shape, x.device, norm, batch_stats=batch_stats)
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
                self._to_ncdhw(f, out, f.C)
        return out

    @staticmethod
    def _to_ncdhw(f, out, channels):
        """The first `channels` channels of channels-last activation f -> the NCDHW tensor `out`, in f's precision."""
        name = "ptx_ndhwc_to_ncdhw_bf16" if f.bf16 else "ptx_ndhwc_to_ncdhw"
        check(getattr(_lib.lib(), name)(_ptr(f.t), _ptr(out), f.N, channels, f.S, f.ld, _stream()), name)

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
            cur = holder.head32
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

    def _max_batch(self, model, sample_shape, key=None):
        """max_batch(), computed once per sample shape (kept with the weight signatures: invalidate() drops it)."""
        key = ("maxb", tuple(sample_shape) if key is None else key)
        with self._lock:
            mb = self._sig.get(key)
            if mb is None:
                mb = self._sig[key] = self.max_batch(model, sample_shape)
        return mb

    def _chunked(self, fn, model, x):
        """Run `fn(model, chunk)` over batch slices that respect the per-launch size limit."""
        mb = self._max_batch(model, x.shape[1:])
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
                   or (s.body_ok and body_lookup(json.dumps(s.d.key())) is None)
                   for s in plan.conv_steps) or any(chain_lookup(s.key) is None or (s.body_ok and body_lookup(s.key) is None)
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
            if plan.program_steps and os.environ.get("PTX_PROGRAM_CHECK", "1") != "0":
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
        mb = self._max_batch(model, (model.dim_z,), key=("biggan", prec))
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
                # (bf16 plans: the tanh conv wrote bf16, the layout pass keeps it)
                out = torch.empty((N, 3, f.H, f.W), device=z.device, dtype=torch.bfloat16 if f.bf16 else torch.float32)
                self._to_ncdhw(f, out, 3)
        return out

    def _frames_input(self, model, frames, opts, transform, who="forward_frames"):
        """What forward_frames (and cam_frames) run on: the transform applied, the frames checked and made contiguous, the NCDHW /
        NCHW view of their shape and the NormDesc of `opts` (default: the model's own pretrained settings)."""
        from .transforms import YUV420, apply_frames_transform
        if transform is not None or isinstance(frames, YUV420):
            frames = apply_frames_transform(transform, frames)
        opts = model if opts is None else opts
        get = (lambda k: opts[k]) if isinstance(opts, dict) else (lambda k: getattr(opts, k))
        try:
            norm = NormDesc.make(get("mean"), get("std"), get("input_space"), get("input_range"))
        except (AttributeError, KeyError):
            raise PtxError("%s: no mean/std/input_space/input_range on the model (they exist only for "
                           "pretrained models, torchvision_models.py:162-166): pass opts=pretrained_settings[...]" % who)
        if model.training:
            raise PtxError("pretorched-x_amd is a forward-only (inference) engine: call model.eval() first")
        prec = model_precision(model)
        if prec != "fp32" and not (prec == "bf16" and self._bf16_stem == "direct"):
            raise PtxError("%s runs float32 models only (this model's parameters are %s)%s" % (
                who, prec, "; engine().bf16_stem = 'direct' lets a bfloat16 model read the frames in its stem" if prec == "bf16" else ""))
        dims = model.arch.dims
        if not isinstance(frames, torch.Tensor) or not frames.is_cuda or frames.dtype != torch.uint8:
            raise PtxError("%s: frames must be a uint8 CUDA tensor" % who)
        if frames.dim() != dims + 2:
            raise PtxError("%s: expected %s, got shape %s" % (
                who, "[N,T,H,W,C]" if dims == 3 else "[N,H,W,C]", tuple(frames.shape)))
        if frames.shape[-1] != 3:
            raise PtxError("%s: the stems take 3 channels" % who)
        frames = frames.contiguous()
        if dims == 3:
            N, T, H, W, Cc = frames.shape
            shape = (N, Cc, T, H, W)
        else:
            N, H, W, Cc = frames.shape
            shape = (N, Cc, H, W)
        return frames, shape, norm

    def forward_frames(self, model, frames, opts=None, transform=None):
        """Decoded uint8 frames [N,T,H,W,C] (NHWC for 2-D models) -> logits.  The tensor half of the
        reference's TransformImage (ToTensor, ToSpaceBGR, ToRange255, Normalize; transforms/utils.py:72-75)
        is fused into the stem's fold kernel: no fp32 NCDHW clip is ever materialised.  `opts`: anything
        with mean / std / input_space / input_range (default: the model's own pretrained settings).
        `transform`: a `transforms.TransformFrames(.., out="frames")` applied to the frames first (resize + crop of
        frames of any size on the device, utils.py:53-64), or a `transforms.SampleClips(.., out="frames")`, for which
        `frames` is a batch of VIDEOS of any sizes and lengths (a list) that it samples clips from; None: the frames
        already have the input size.
        `frames` may be a `transforms.YUV420` source (NV12 / I420 planes); it needs a transform, whose kernel converts
        the colours while it stages the rows."""
        frames, shape, norm = self._frames_input(model, frames, opts, transform)
        N = frames.shape[0]
        mb = self._max_batch(model, shape[1:])
        if N > mb:
            size = -(-N // (-(-N // mb)))
            return torch.cat([self.forward_frames(model, frames[i:i + size], opts) for i in range(0, N, size)], 0)
        with torch.cuda.device(frames.device):
            plan = self.plan_for(model, frames, shape=shape, norm=norm)
            self._maybe_tune(model, plan, frames)
            return self._forward_eager(model, plan, frames)

    def forward_views(self, model, video, opts=None, views=None, reduce="softmax", chunk=None):
        """Decoded uint8 video [N,Tv,H,W,3] (or [Tv,H,W,3]: one video; or a `transforms.YUV420` source with planes
        [N,Tv,H,W] / [Tv,H,W]) -> fp32 [N, classes]: the mean over `views`
        (a `transforms.SampleViews`: clips x crops, sampled on the device) of softmax(logits) (reduce="softmax"), of the
        logits ("logits"), or the logits of every view [N, V, classes] in the model's dtype (None).
        float32 models take the views as uint8 frames through forward_frames (views.out == "frames", `opts` as there);
        bfloat16 models take the normalised bf16 clip through forward() (views: out="tensor", dtype=torch.bfloat16) -- and,
        under bf16_stem = "direct", also a frames-out sampler through forward_frames.
        Views are produced `chunk` at a time (default `views_chunk(N, V, max_batch)`: as many as the per-launch size
        limit allows), so only one chunk of views exists at any time."""
        prec = model_precision(model)
        if prec not in ("fp32", "bf16"):
            raise PtxError("forward_views runs float32 and bfloat16 models (this model's parameters are %s)" % prec)
        frames_in = prec == "fp32" or (self._bf16_stem == "direct" and getattr(views, "out", None) == "frames")
        check_views(views, model, "frames" if frames_in else "bf16", bf16_stem=self._bf16_stem)
        if getattr(model.arch, "dims", 3) != 3:
            raise PtxError("forward_views: a 2-D model takes images, not clips (TRN.forward_views runs a 2-D backbone on the "
                           "frames of a clip)")
        S = views.size
        mb = self._max_batch(model, (3, views.num_frames, S, S))
        if frames_in:
            run = lambda frames: self.forward_frames(model, frames, opts)
        else:
            run = lambda clip: self.forward(model, clip)
        return run_views(video, views, run, mb, reduce, chunk)

    # ------------------------------------------------------------------------------------
    def update_bn(self, model, loader, device=None, momentum=None, reset=True):
        """torch.optim.swa_utils.update_bn(loader, model, device) on the HIP engine: one forward-only pass over `loader` in which
        every BatchNorm of the trunk normalises with the batch's own mean and biased variance and moves its running_mean /
        running_var / num_batches_tracked, as train()-mode F.batch_norm does.  `loader` yields clips, or lists / tuples
        whose first element is the clip; with `device` each clip is moved there first.  reset: running statistics are reset
        first (as torch does).  momentum None: the cumulative average over the pass, every batch with equal weight (what
        torch's update_bn sets); a float: that factor for every layer.  Neither model.training nor any BN's `.momentum` is
        touched, and no torch.nn forward runs.  The running statistics of the pass live in buffers of the pass and are
        copied into the BatchNorm buffers when the loader is exhausted (copy_ bumps their version counters, so the next
        eval-mode forward re-folds the filters without refresh()).  Each batch runs through ONE batch-statistics plan
        (Plan(batch_stats=True)): never clip lanes, never chunks -- both would compute part-batch statistics -- and always
        the fp32 tiles (`precision = "x3"` is ignored)."""
        check_batch_stats_scope(model)
        if momentum is not None and not (isinstance(momentum, (int, float)) and not isinstance(momentum, bool) and 0.0 <= momentum <= 1.0):
            raise PtxError("update_bn: momentum must be None or a number in [0, 1] (got %r)" % (momentum,))
        bns = [m for m in model.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)]
        for bn in bns:
            if not bn.track_running_stats or bn.running_mean is None:
                raise PtxError("update_bn: every BatchNorm must track running statistics")
            if reset:
                bn.reset_running_stats()         # in place: zero_() / fill_(1) / zero_()
        run = sizes = tracked = dev = None
        dims = model.arch.dims
        for batch in loader:
            x = batch[0] if isinstance(batch, (list, tuple)) else batch
            if device is not None:
                x = x.to(device)
            if not isinstance(x, torch.Tensor) or not x.is_cuda:
                raise PtxError("update_bn: clips must be CUDA (ROCm) tensors -- there is no CPU path in this call (pass device=...)")
            if x.dtype != torch.float32 or x.dim() != (4 if dims == 2 else 5):
                raise PtxError("update_bn: expected a float32 %d-D clip batch, got %s %s" % (4 if dims == 2 else 5, x.dtype, tuple(x.shape)))
            if _first_weight(model).device != x.device or (dev is not None and dev != x.device):
                raise PtxError("update_bn: clips on %s but parameters on %s (one device per pass)" % (x.device, _first_weight(model).device))
            dev = x.device
            if x.shape[0] > self._max_batch(model, x.shape[1:]):
                raise PtxError("update_bn: a batch of %d clips of %s exceeds the 2 GiB per-launch limit (%d clips); batch statistics "
                               "need the whole batch in one plan -- use smaller batches" % (
                                   x.shape[0], tuple(x.shape[1:]), self._max_batch(model, x.shape[1:])))
            x = _dense16(x)
            with torch.cuda.device(dev):
                plan = self.plan_for(model, x, batch_stats=True)
                self._maybe_tune(model, plan, x)
                with plan.exclusive():
                    plan.bind(model)
                    if run is None:
                        if {id(plan.get(r)) for r in plan.bn_refs} != {id(bn) for bn in bns} or len(plan.bn_refs) != len(bns):
                            raise PtxError("update_bn: the model holds BatchNorm layers outside its trunk (or one used twice)")
                        sizes = list(plan.bn_sizes)
                        run = tuple(torch.zeros_like(t) for t in plan.bn_own_run)
                        layers = [plan.get(r) for r in plan.bn_refs]
                        for (off, c), bn in zip(sizes, layers):
                            run[0][off:off + c].copy_(bn.running_mean)
                            run[1][off:off + c].copy_(bn.running_var)
                        tracked = [0] * len(layers) if reset else [int(v) for v in torch.stack([bn.num_batches_tracked for bn in layers]).tolist()]
                    elif list(plan.bn_sizes) != sizes:
                        raise PtxError("update_bn: the BatchNorm layers of this batch's plan differ from the first batch's (internal error)")
                    tracked = [t + 1 for t in tracked]
                    plan.bn_f[:] = [float(momentum) if momentum is not None else 1.0 / t for t in tracked]
                    plan.bn_run = run
                    try:
                        plan.run_features(x)
                    finally:
                        plan.bn_run = plan.bn_own_run
        if run is not None:
            with torch.cuda.device(dev), torch.no_grad():
                for (off, c), bn, t in zip(sizes, layers, tracked):
                    bn.running_mean.copy_(run[0][off:off + c])
                    bn.running_var.copy_(run[1][off:off + c])
                    bn.num_batches_tracked.fill_(t)

    # ------------------------------------------------------------------------------------ tuner.py
    def autotune(self, model, x, iters=3, verbose=False, persist=False, only_untuned=False, plan=None):
        return tuner.autotune(self, model, x, iters, verbose, persist, only_untuned, plan)

    def _autotune(self, model, x, iters=3, verbose=False, persist=False, only_untuned=False, plan=None):
        return tuner._autotune(self, model, x, iters, verbose, persist, only_untuned, plan)

    def tune_lanes(self, model, x, iters=8, verbose=False):
        return tuner.tune_lanes(self, model, x, iters, verbose)

    def profile_convs(self, model, x, iters=5, plan=None):
        return tuner.profile_convs(self, model, x, iters, plan)

    def profile_steps(self, plan, iters=5, isolated=None):
        return tuner.profile_steps(self, plan, iters, isolated)


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

    def update_bn(self, loader, momentum=None, reset=True):
        """Recompute the running statistics of every BatchNorm with a forward-only pass over `loader` on the HIP engine
        (Engine.update_bn; `pretorched_x_amd.update_bn(loader, model, device)` is torch.optim.swa_utils.update_bn's signature)."""
        return self._engine.update_bn(self, loader, momentum=momentum, reset=reset)

    # class activation maps (cam.py): defined for a global average pool + one Linear, which VideoResNet overrides these for
    def cam(self, *a, **k):
        from .cam import unsupported
        raise unsupported(self)

    def cam_frames(self, *a, **k):
        from .cam import unsupported
        raise unsupported(self)

    def logits_map(self, *a, **k):
        from .cam import unsupported
        raise unsupported(self, "logits maps")

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self._engine.invalidate()
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        if "_engine" in self.__dict__:
            self._engine.invalidate()
        return r
