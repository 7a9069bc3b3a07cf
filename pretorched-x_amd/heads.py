"""Launches that are not part of a plan: the multi-view reduction behind every forward_views, and the Linear / TRN
relation heads that run straight through ptx_linear_fwd."""
import ctypes as C

import torch

from . import _lib
from ._lib import PTX_EPI_ACCUM, PTX_EPI_RELU, PTX_PRO_RELU, PtxError, check
from .steps import _ptr, _stream


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
    from .transforms import YUV420
    if isinstance(video, YUV420):                                  # planes [N,Tv,H,W] or [Tv,H,W]: the source knows N
        if video.lead not in (2, 3):
            raise PtxError("%s: a YUV420 video has planes [N,Tv,H,W] or [Tv,H,W]" % who)
        N = video.N if video.lead == 3 else 1
    elif not isinstance(video, torch.Tensor) or video.dim() not in (4, 5):
        raise PtxError("%s: video must be a uint8 CUDA tensor [N,Tv,H,W,3] or [Tv,H,W,3] (or a transforms.YUV420)" % who)
    else:
        N = video.shape[0] if video.dim() == 5 else 1
    V = views.num_views
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


def check_views(views, model, want_out, who="forward_views", bf16_stem="fold"):
    """want_out: "frames" (the views go through forward_frames) or "bf16" (the normalised bf16 clip through forward()).
    bf16_stem: the engine's switch -- under "direct" a bfloat16 model takes either kind, and the message says so."""
    from .transforms import SampleViews
    if not isinstance(views, SampleViews):
        raise PtxError("%s: views must be a pretorched.transforms.SampleViews, got %r" % (who, views))
    if want_out == "frames" and views.out != "frames":
        raise PtxError("%s: a float32 model takes the views as uint8 frames (forward_frames): build the SampleViews with "
                       "out='frames'" % who)
    if want_out == "bf16" and (views.out != "tensor" or views.dtype != torch.bfloat16):
        raise PtxError("%s: a bfloat16 model takes the views as the normalised bf16 clip: build the SampleViews with "
                       "out='tensor', dtype=torch.bfloat16%s" % (who, " (or out='frames': bf16_stem = 'direct' reads them in the stem)"
                                                                if bf16_stem == "direct" else ""))


# ---------------------------------------------------------------------------------------------
# TRN relation MLP (trn.py:39-45): ReLU -> Linear -> ReLU -> Linear
# ---------------------------------------------------------------------------------------------
def _bf16_head(who, x, *lins):
    """True when this head call runs on the bf16-weight kernels (include/ptx_amd_linear_bf16.h): every Linear holds bfloat16
    parameters and x is a bfloat16 CUDA tensor.  A dtype mismatch in either direction raises; float32 calls return False."""
    wd = {t.dtype for lin in lins for t in (lin.weight, lin.bias) if t is not None}
    if torch.bfloat16 not in wd:
        if isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16:
            raise PtxError("%s: the input is bfloat16 but the Linear parameters are %s: convert the module with "
                           ".to(torch.bfloat16), or pass a float32 input" % (who, sorted(str(d) for d in wd)))
        return False
    if wd != {torch.bfloat16}:
        raise PtxError("%s: the Linear parameters mix %s" % (who, sorted(str(d) for d in wd)))
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.bfloat16:
        raise PtxError("%s: the Linear parameters are bfloat16: the input must be a bfloat16 CUDA tensor too (got %s; no CPU "
                       "fallback)" % (who, getattr(x, "dtype", type(x))))
    return True


def _wb(lin):
    """The live bf16 parameters of a Linear (no copies: nothing to refresh)."""
    w = lin.weight.detach()
    b = lin.bias.detach() if lin.bias is not None else None
    return (w if w.is_contiguous() else w.contiguous()), (None if b is None else b.contiguous())


def _bp(t):
    return _ptr(t) if t is not None else C.c_void_p(0)


def _workspace(M, K, Nout, dev):
    """(tensor or None, pointer, bytes): the split-K partial tiles of one bf16-weight launch."""
    n = int(_lib.lib().ptx_linear_bf16w_workspace_bytes(M, K, Nout))
    if n == 0:
        return None, C.c_void_p(0), 0
    ws = torch.empty((n + 3) // 4, device=dev, dtype=torch.float32)
    return ws, _ptr(ws), n


def _dense_bf16w(x, x_kind, lin, y, flags, what):
    """y (fp32 [M, Nout], contiguous) (+)= act(x) @ W^T + b through ptx_linear_bf16w_fwd; x: contiguous [M, K] bf16 / fp32."""
    M, K = x.shape
    w, b = _wb(lin)
    ws, wsp, wsn = _workspace(M, K, lin.out_features, x.device)
    check(_lib.lib().ptx_linear_bf16w_fwd(_ptr(x), x_kind, _ptr(w), _bp(b), _ptr(y), M, K, lin.out_features, K, y.stride(0), flags,
                                          wsp, wsn, _stream()), what)


def round_bf16(y32):
    """fp32 -> bf16, one round-to-nearest-even per element (ptx_f32_to_bf16)."""
    out = torch.empty(y32.shape, device=y32.device, dtype=torch.bfloat16)
    with torch.cuda.device(y32.device):
        check(_lib.lib().ptx_f32_to_bf16(_ptr(y32), _ptr(out), y32.numel(), _stream()), "ptx_f32_to_bf16")
    return out


def linear(x, lin, flags=0):
    """y = x @ W^T + b through ptx_linear_fwd for any [..., K] float32 CUDA tensor (TRN classifier,
    trn.py:257-258)."""
    if not isinstance(lin, torch.nn.Linear):
        return lin(x)                                   # user-replaced head: theirs to run
    from . import eager
    if eager.wanted(lin, x):                            # train() / autograd / CPU model (eager.py)
        return lin(x)
    if _bf16_head("linear", x, lin):
        # bf16 parameters on bf16 features: ptx_linear_bf16w_fwd on the live weights, fp32 accumulate, logits rounded once
        flat = x.contiguous().view(-1, lin.in_features)
        with torch.cuda.device(x.device):
            out32 = torch.empty((flat.shape[0], lin.out_features), device=x.device, dtype=torch.float32)
            _dense_bf16w(flat, _lib.PTX_LIN_X_BF16, lin, out32, flags, "ptx_linear_bf16w_fwd")
        return round_bf16(out32).view(tuple(x.shape[:-1]) + (lin.out_features,))
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
    into `out`.  x: [B, T, F] fp32 CUDA; subsets: tuples of frame indices, all of one length.
    bf16 parameters take a bf16 x through the bf16-weight twins of the two launches; hidden vector and `out` stay fp32."""
    if _bf16_head("relation_scale", x, lin1, lin2):
        return _relation_scale_bf16(x, subsets, lin1, lin2, out, accumulate)
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


def _relation_scale_bf16(x, subsets, lin1, lin2, out, accumulate):
    B, T, F_ = x.shape
    x = x.contiguous()
    d = _lib.RelationDesc()
    d.B, d.n_sets, d.n_frames, d.frame_len = B, len(subsets), len(subsets[0]), F_
    for r, sub in enumerate(subsets):
        for f, i in enumerate(sub):
            d.idx[r][f] = int(i)
    lib = _lib.lib()
    hid_n, out_n = lin1.out_features, lin2.out_features
    M, K = len(subsets) * B, len(subsets[0]) * F_
    with torch.cuda.device(x.device):
        hid = torch.empty((M, hid_n), device=x.device, dtype=torch.float32)
        res = out if out is not None else torch.empty((B, out_n), device=x.device, dtype=torch.float32)
        (w1, b1), (w2, b2) = _wb(lin1), _wb(lin2)
        ws, wsp, wsn = _workspace(M, K, hid_n, x.device)
        check(lib.ptx_relation_linear_bf16w_fwd(C.byref(d), _ptr(x), T * F_, _ptr(w1), _bp(b1), _ptr(hid), hid_n, hid_n,
                                                PTX_PRO_RELU | PTX_EPI_RELU, wsp, wsn, _stream()), "relation.linear1 (bf16 weights)")
        check(lib.ptx_linear_setsum_bf16w_fwd(_ptr(hid), _ptr(w2), _bp(b2), _ptr(res), B, len(subsets), hid_n, out_n, hid_n,
                                              out_n, PTX_EPI_ACCUM if accumulate else 0, _stream()), "relation.linear2 (bf16 weights)")
    return res


def relation_mlp(flat, lin1, lin2, out=None, accumulate=False):
    """ReLU -> lin1 -> ReLU -> lin2 on [M, K] rows, fp32 [M, out] back (accumulated into `out` when asked).  bf16 parameters
    take a bf16 `flat`: the hidden vector and the result stay fp32 (the relation module rounds its output once)."""
    if _bf16_head("relation_mlp", flat, lin1, lin2):
        flat = flat.contiguous()
        M = flat.shape[0]
        with torch.cuda.device(flat.device):
            hid = torch.empty((M, lin1.out_features), device=flat.device, dtype=torch.float32)
            res = out if out is not None else torch.empty((M, lin2.out_features), device=flat.device, dtype=torch.float32)
            _dense_bf16w(flat, _lib.PTX_LIN_X_BF16, lin1, hid, PTX_PRO_RELU | PTX_EPI_RELU, "relation.linear1 (bf16 weights)")
            _dense_bf16w(hid, _lib.PTX_LIN_X_F32, lin2, res, PTX_EPI_ACCUM if accumulate else 0, "relation.linear2 (bf16 weights)")
        return res
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
