"""Class activation maps (Zhou et al., "Learning Deep Features for Discriminative Localization", CVPR 2016) of the VideoResNet
families: "where and when" next to the engine's "which class".

Every `VideoResNet` ends in a global average pool and one `nn.Linear`.  For exactly that head the map of class c is the classifier
row applied at every position of the final feature map,

    scores[n, j, t, h, w] = b[c] + sum_ch W[c, ch] * features[n, ch, t, h, w],      c = classes[n, j]

and its mean over the positions is the logit.  `model.cam(x)` runs ONE forward: the plan's channels-last feature map stays where it
is, the head runs as usual, then `ptx_cam_scores` reads the map once (k classifier rows in LDS) and `ptx_cam_quantize` makes one
uint8 map per (clip, class).  `transforms.CamOverlay` draws the maps over the frames, equal to Pillow bit for bit.

The launches live here, the entry points on the models (`VideoResNet.cam` / `cam_frames` / `logits_map`); CPU and train()-mode
models answer through eager.py with the same definition in plain torch.
"""
import collections
import ctypes as C

import torch
import torch.nn as nn

from . import _lib
from ._lib import PtxError, check
from .steps import _dense16, _ptr, _stream

SUPPORTED = ("the VideoResNet families (3-D, (2+1)D, ResNeXt / wide / pre-activation / multi-view, the non-local nets, the "
             "channel-separated nets and the 2-D ResNets) with an nn.Linear head")

CamResult = collections.namedtuple("CamResult", ("logits", "classes", "scores", "maps", "frames"))
CamResult.__doc__ = """What `model.cam` / `model.cam_frames` return.
logits:  the bits of `model(input)` ([N, classes], the model's dtype).
classes: int64 [N, k], the classes the maps belong to (the top-k of the logits unless the caller named them).
scores:  fp32 [N, k, T', H', W'] ([N, k, H', W'] for the 2-D nets): the class scores at every position of the final feature map.
maps:    uint8, same shape: every map stretched to 0 .. 255 on its own (`transforms.cam_quantize_numpy`).
frames:  `cam_frames` only: the uint8 frames the model saw (the transform's output), what `transforms.CamOverlay` takes."""


def unsupported(model, what="class activation maps"):
    """PtxError for a model outside the supported set (every family but VideoResNet, adopted instances, another head)."""
    name = getattr(model, "arch_name", None) or type(model).__name__
    return PtxError("%s are defined for %s; %s is not one of them" % (what, SUPPORTED, name))


def check_model(model, what="class activation maps"):
    """The head this call reads: raises unless `model` is a VideoResNet of the zoo whose head is an nn.Linear."""
    from .zoo import VideoResNet
    if not isinstance(model, VideoResNet) or str(getattr(model, "arch_name", "")).startswith("adopted:"):
        raise unsupported(model, what)
    head = model.head_module
    if not isinstance(head, nn.Linear):
        raise PtxError("%s are defined for %s: this model's head is %s, for which the map of a class is not defined" % (
            what, SUPPORTED, type(head).__name__))
    return head


def class_list(classes, topk, logits, num_classes):
    """The [N, k] int64 class list of a call, on the logits' device: the top-k of the logits (classes None), one class for every clip
    (an int) or the caller's [N][k] indices (checked against the classifier on the host)."""
    N = logits.shape[0]
    if classes is None:
        if isinstance(topk, bool) or not isinstance(topk, int) or not 1 <= topk <= num_classes:
            raise PtxError("cam: topk must be an integer in 1..%d (got %r)" % (num_classes, topk))
        return logits.detach().float().topk(topk, dim=1).indices
    if isinstance(classes, int) and not isinstance(classes, bool):
        cl = torch.full((N, 1), classes, dtype=torch.int64)
    else:
        cl = torch.as_tensor(classes).detach().cpu()
        if cl.dtype in (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.bool) or cl.dim() != 2 or cl.shape[0] != N or cl.shape[1] < 1:
            raise PtxError("cam: classes must be None, an int or [N=%d][k] integer indices (got %s %s)" % (N, cl.dtype, tuple(cl.shape)))
        cl = cl.to(torch.int64)
    if int(cl.min()) < 0 or int(cl.max()) >= num_classes:
        raise PtxError("cam: a class index is outside [0, %d)" % num_classes)
    return cl.to(logits.device)


def scores_expression(features, weight, bias, classes):
    """The definition in plain torch (the CPU / train() path, and what the tests restate): features [N, C, *positions], the
    classifier's weight / bias, classes int64 [N, k] -> [N, k, *positions]."""
    out = torch.einsum("nkc,nc...->nk...", weight[classes], features)
    if bias is not None:
        out = out + bias[classes].reshape(classes.shape + (1,) * (features.dim() - 2))
    return out


def launch_scores(feat, w32, b32, classes, num_classes):
    """ptx_cam_scores + ptx_cam_quantize on a plan's channels-last feature map `feat` (steps.Act; fp32 or bf16), on the current
    stream: fp32 scores and uint8 maps [N, k, S].  Class lists beyond PTX_CAM_MAX_CLASSES (or beyond what the classifier rows'
    LDS holds) run in column groups."""
    lib = _lib.lib()
    N, S, k = feat.N, feat.S, classes.shape[1]
    dev = feat.t.device
    group = min(_lib.PTX_CAM_MAX_CLASSES, _lib.PTX_CAM_MAX_LDS_BYTES // (4 * ((feat.C + 3) // 4 * 4)))
    if group < 1:
        raise PtxError("cam: one classifier row of %d channels exceeds the %d bytes of LDS a ptx_cam_scores launch holds" % (
            feat.C, _lib.PTX_CAM_MAX_LDS_BYTES))
    cls32 = classes.to(torch.int32)
    parts = []
    for j0 in range(0, k, group):
        cj = cls32[:, j0:j0 + group].contiguous()
        kj = cj.shape[1]
        if not lib.ptx_cam_scores_supported(N, S, feat.C, feat.ld, kj, num_classes, int(feat.bf16)):
            raise PtxError("cam: %s" % lib.ptx_last_error().decode(errors="replace"))
        y = torch.empty((N, kj, S), device=dev, dtype=torch.float32)
        check(lib.ptx_cam_scores(_ptr(feat.t), int(feat.bf16), _ptr(w32), _ptr(b32) if b32 is not None else C.c_void_p(0), _ptr(cj),
                                 _ptr(y), N, S, feat.C, feat.ld, kj, num_classes, _stream()), "ptx_cam_scores")
        parts.append(y)
    scores = parts[0] if len(parts) == 1 else torch.cat(parts, 1)
    maps = torch.empty((N, k, S), device=dev, dtype=torch.uint8)
    check(lib.ptx_cam_quantize(_ptr(scores), _ptr(maps), N * k, S, _stream()), "ptx_cam_quantize")
    return scores, maps


def _run_plan(engine, model, plan, x, classes, topk):
    """One forward of `plan` on `x` plus the maps, under the plan's lock (the feature map is the plan's buffer)."""
    head = model.head_module
    with plan.exclusive():
        plan.bind(model)
        f = plan.run_features(x)
        logits = plan.run_head(engine, model)
        cl = class_list(classes, topk, logits, head.out_features)
        if f.bf16:
            cur = plan.head32                    # the fp32 copy the bf16 head just read (Engine._head_bf16 keeps it current)
            if cur is None:
                raise PtxError("cam: the bf16 plan holds no fp32 copy of the classifier (internal error)")
            w32, b32 = cur[1], cur[2]
        else:
            if not head.weight.is_cuda or head.weight.dtype != torch.float32:
                raise PtxError("cam: the classifier must be a float32 nn.Linear on the model's device")
            w32 = head.weight.detach().contiguous()
            b32 = head.bias.detach().contiguous() if head.bias is not None else None
        scores, maps = launch_scores(f, w32, b32, cl, head.out_features)
        shape = (f.N, cl.shape[1]) + ((f.H, f.W) if model.arch.dims == 2 else (f.T, f.H, f.W))
    return CamResult(logits, cl, scores.view(shape), maps.view(shape), None)


def _cat(results, frames=None):
    if len(results) == 1:
        return results[0]._replace(frames=frames)
    return CamResult(*(torch.cat([getattr(r, n) for r in results], 0) for n in ("logits", "classes", "scores", "maps")), frames)


def _rows(classes, i0, i1):
    """Clips [i0, i1) of a caller's class list (None and ints serve every clip)."""
    if classes is None or (isinstance(classes, int) and not isinstance(classes, bool)):
        return classes
    return torch.as_tensor(classes)[i0:i1]


def cam(engine, model, x, classes=None, topk=1):
    """Engine side of `VideoResNet.cam`: the plans, lanes and chunks of `Engine.forward`, so `logits` has its bits."""
    check_model(model)
    engine._validate(model, x, model.arch.dims)
    mb = engine._max_batch(model, x.shape[1:])
    if x.shape[0] > mb:
        n_chunks = -(-x.shape[0] // mb)
        size = -(-x.shape[0] // n_chunks)
        return _cat([cam(engine, model, x[i:i + size], _rows(classes, i, i + size), topk) for i in range(0, x.shape[0], size)])
    x = _dense16(x)
    with torch.cuda.device(x.device):
        n = engine.lanes_for(x.shape[0], model, x.shape)
        if n == 1:
            plan = engine.plan_for(model, x)
            engine._maybe_tune(model, plan, x)
            return _run_plan(engine, model, plan, x, classes, topk)
        # clip lanes, as Engine._forward_lanes runs them: slice i through its own plan on stream i, the maps of a slice behind its head
        dev = x.device
        cur = torch.cuda.current_stream(dev)
        side = engine._lane_streams.get(dev.index)
        if side is None or len(side) < n - 1:
            side = engine._lane_streams[dev.index] = [torch.cuda.Stream(dev) for _ in range(n - 1)]
        per = x.shape[0] // n
        parts = [_dense16(x[i * per:(i + 1) * per]) for i in range(n)]
        plans = []
        for i in range(n):
            plans.append(engine.plan_for(model, parts[i], lane=i))
            engine._maybe_tune(model, plans[i], parts[i])
        ready = cur.record_event()
        out = [None] * n
        for i in range(1, n):
            side[i - 1].wait_event(ready)
            with torch.cuda.stream(side[i - 1]):
                out[i] = _run_plan(engine, model, plans[i], parts[i], _rows(classes, i * per, (i + 1) * per), topk)
        out[0] = _run_plan(engine, model, plans[0], parts[0], _rows(classes, 0, per), topk)
        for i in range(1, n):
            cur.wait_stream(side[i - 1])
        for r in out[1:]:
            for t in r[:4]:
                t.record_stream(cur)             # allocated under a side stream, consumed (and freed) under the caller's
    return _cat(out)


def cam_frames(engine, model, frames, opts=None, transform=None, classes=None, topk=1):
    """Engine side of `VideoResNet.cam_frames`: `Engine.forward_frames`' route (transform, fused normalisation, chunks)."""
    check_model(model)
    frames, shape, norm = engine._frames_input(model, frames, opts, transform, "cam_frames")
    N = frames.shape[0]
    mb = engine._max_batch(model, shape[1:])
    size = N if N <= mb else -(-N // (-(-N // mb)))
    out = []
    with torch.cuda.device(frames.device):
        for i in range(0, N, size):
            part = frames[i:i + size]
            plan = engine.plan_for(model, part, shape=(part.shape[0],) + tuple(shape[1:]), norm=norm)
            engine._maybe_tune(model, plan, part)
            out.append(_run_plan(engine, model, plan, part, _rows(classes, i, i + size) if size < N else classes, topk))
    return _cat(out, frames)


def logits_map(engine, model, feats):
    """Engine side of `VideoResNet.logits_map`: NCDHW fp32 features -> every class at every position [N, classes, *positions]:
    the layout pass, `ptx_linear_fwd` on N * S rows, the layout pass back."""
    head = check_model(model, "logits maps")
    engine._validate(model, feats, model.arch.dims)
    if not head.weight.is_cuda or head.weight.dtype != torch.float32:
        raise PtxError("logits_map: the classifier must be a float32 nn.Linear on the model's device")
    feats = feats.contiguous()
    N, Cf = feats.shape[0], feats.shape[1]
    if Cf != head.in_features:
        raise PtxError("logits_map: the classifier takes %d channels, the features have %d" % (head.in_features, Cf))
    S = feats.numel() // (N * Cf)
    K = head.out_features
    if N * S * (max(Cf, K) + 3) * 4 > engine.LIMIT_BYTES:
        raise PtxError("logits_map: %d x %d positions of %d channels / %d classes exceed the 2 GiB per-launch limit: pass fewer clips" % (
            N, S, Cf, K))
    lib = _lib.lib()
    ldc, ldk = (Cf + 3) // 4 * 4, (K + 3) // 4 * 4               # the layout passes take row pitches that are multiples of 4
    with torch.cuda.device(feats.device):
        cl = torch.empty((N, S, ldc), device=feats.device, dtype=torch.float32)
        check(lib.ptx_ncdhw_to_ndhwc(_ptr(feats), _ptr(cl), N, Cf, S, ldc, _stream()), "ptx_ncdhw_to_ndhwc")
        rows = torch.empty((N, S, ldk), device=feats.device, dtype=torch.float32)
        w = head.weight.detach().contiguous()
        b = head.bias.detach().contiguous() if head.bias is not None else None
        check(lib.ptx_linear_fwd(_ptr(cl), _ptr(w), _ptr(b) if b is not None else C.c_void_p(0), _ptr(rows), N * S, Cf, K, ldc, ldk, 0,
                                 _stream()), "ptx_linear_fwd")
        out = torch.empty((N, K) + tuple(feats.shape[2:]), device=feats.device, dtype=torch.float32)
        check(lib.ptx_ndhwc_to_ncdhw(_ptr(rows), _ptr(out), N, K, S, ldk, _stream()), "ptx_ndhwc_to_ncdhw")
    return out
