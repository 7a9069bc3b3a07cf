"""Footprint tests of the pooling / head entry points (pool_head.hip, linear_bf16.hip): every operand carved out of one
guarded arena (tests/arena.py) at the weakest alignment its entry accepts, once under each fill.  Per case: guards and
inputs intact, nothing non-finite written, the layout contract, the values against a float64 reference at the tolerance of
the entry's existing test (named per case), bit-identical outputs under the two fills.  No launch of this module adds into
its output with floating-point atomics: none is excused from bit-equality.

Alignment switches reached here (pretorched-x_amd/csrc):
  pool_head.hip ptx_linear_fwd     MFMA route <- x|w|y|b 16-byte aligned, M >= 32; skinny route <- x|w aligned; else scalar
  pool_head.hip linear_smallm_kernel `vec` (device side): the host sends this kernel only what fails the skinny route's test,
                                   which is the same test plus M * ldx < 2^31 -- its `vec` side needs an 8 GiB x and is not
                                   reachable at a test's size; the scalar side runs in the x-off / w-off / K = 62 cases
  pool_head.hip affine_act_upsample_kernel `vec4` <- scale|shift 16-byte aligned, C % 4 == 0, ld_scale % 4 == 0
  linear_bf16.hip rows16 (ptx_linear_bf16w_fwd): bf16 x -> MFMA kernel, else VALU kernel with a.vec = rows16
  linear_bf16.hip a.vec (ptx_linear_setsum_bf16w_fwd)"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from footprint import P, ST, cl, judge, r4, rnd, run

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
S = slice(None)


def _lib(ptx):
    return ptx._lib.lib()


# ---- ptx_linear_fwd: tolerance 1e-5 of test_gpu_kernels.py::test_avgpool_and_linear ------------------------------------------
# (M, K, Nout, ldx, ldy, flags, (align x, w, b, y), route)
LINEAR = [
    ("mfma_all_aligned", 40, 68, 36, 72, 40, "relu", (16, 16, 16, 16)),       # M >= 32, every condition holds: the MFMA tiles
    ("only_x_off", 40, 68, 36, 72, 40, "relu", (4, 16, 16, 16)),              # -> scalar kernel (x|w decides both vector routes)
    ("only_w_off", 40, 68, 36, 72, 40, "relu", (16, 4, 16, 16)),              # -> scalar kernel
    ("only_y_off", 40, 68, 36, 72, 40, "relu", (16, 16, 16, 4)),              # -> skinny kernel (16-byte loads, scalar stores)
    ("only_b_off", 40, 68, 36, 72, 40, "relu", (16, 16, 4, 16)),              # -> skinny kernel: the MFMA epilogue reads b as quads
    ("skinny_small_m", 5, 36, 7, 40, 9, "pro|relu|accum", (16, 16, 4, 4)),    # the GEMV route at its weakest alignment
    ("scalar_odd_k", 9, 62, 7, 63, 9, "pro|relu", (4, 4, 4, 4)),              # K % 4 != 0: everything at 4 bytes
    ("scalar_accum", 9, 62, 7, 62, 7, "accum", (4, 4, 4, 4)),
]


@pytest.mark.parametrize("case", LINEAR, ids=[c[0] for c in LINEAR])
def test_linear(ptx, case):
    L, lib = ptx._lib, _lib(ptx)
    _, M, K, N, ldx, ldy, fl, (ax, aw, ab, ay) = case
    flags = (L.PTX_PRO_RELU if "pro" in fl else 0) | (L.PTX_EPI_RELU if "relu" in fl else 0) | (L.PTX_EPI_ACCUM if "accum" in fl else 0)
    x = torch.zeros(M, ldx)
    x[:, :K] = rnd(M, K, seed=32)
    x[:, K:] = float("nan")                                        # columns [K, ldx) belong to a neighbour: never read
    w, b = rnd(N, K, seed=33, scale=K ** -0.5), rnd(N, seed=34)
    y0 = rnd(M, ldy, seed=35)
    xi = F.relu(x[:, :K].double()) if "pro" in fl else x[:, :K].double()
    want = xi @ w.double().t() + b.double()
    if "accum" in fl:
        want = want + y0[:, :N].double()
    want = F.relu(want) if "relu" in fl else want
    accum = "accum" in fl
    specs = [("x", x, None, ax, "in"), ("w", w, None, aw, "in"), ("b", b, None, ab, "in"),
             ("y", y0, None, ay, "inout") if accum else ("y", (M, ldy), F32, ay, "out")]

    def launch(v, ar):
        L.check(lib.ptx_linear_fwd(P(v["x"]), P(v["w"]), P(v["b"]), P(v["y"]), M, K, N, ldx, ldy, flags, ST()), "linear")

    res = run(specs, launch)
    judge(res, "y", want, 1e-5, (S, slice(0, N)), untouched=() if accum else [(S, slice(N, ldy))])
    if accum and ldy > N:
        for out in res:
            assert torch.equal(out["y"][:, N:], y0[:, N:]), "columns [Nout, ldy) of an accumulated y must stay as they were"


def test_relation_linear_and_setsum(ptx):
    """x and w at 16 bytes (relation_linear / linear_setsum refuse less), b and y at 4.  Tolerance 2e-5 of
    test_gpu_kernels.py::test_skinny_linear_gather_and_setsum, whose shapes these are."""
    L, lib = ptx._lib, _lib(ptx)
    B, T, Fd, hid = 5, 8, 64, 48
    x, w, b = rnd(B, T, Fd, seed=103), rnd(hid, 4 * Fd, seed=104, scale=0.06), rnd(hid, seed=105)
    subsets = [(0, 2, 3, 7), (1, 2, 5, 6), (0, 1, 2, 3)]
    d = L.RelationDesc()
    d.B, d.n_sets, d.n_frames, d.frame_len = B, 3, 4, Fd
    for r, sub in enumerate(subsets):
        for f, i in enumerate(sub):
            d.idx[r][f] = i
    want = torch.cat([F.relu(F.relu(x[:, list(sub)].reshape(B, -1).double()) @ w.double().t() + b.double()) for sub in subsets], 0)
    ldy = hid + 3

    def launch(v, ar):
        L.check(lib.ptx_relation_linear_fwd(C.byref(d), P(v["x"]), T * Fd, P(v["w"]), P(v["b"]), P(v["y"]), hid, ldy,
                                            L.PTX_PRO_RELU | L.PTX_EPI_RELU, ST()), "relation linear")

    res = run([("x", x, None, 16, "in"), ("w", w, None, 16, "in"), ("b", b, None, 4, "in"), ("y", (3 * B, ldy), F32, 4, "out")], launch)
    judge(res, "y", want, 2e-5, (S, slice(0, hid)), untouched=[(S, slice(hid, ldy))])
    xs, ws = torch.zeros(B * T * Fd + 4, device="cuda:0"), torch.zeros(hid * 4 * Fd + 4, device="cuda:0")
    for ox, ow in ((1, 0), (0, 1)):                                  # the refusal is a host-side return: nothing is launched
        st = lib.ptx_relation_linear_fwd(C.byref(d), P(xs, ox), T * Fd, P(ws, ow), None, P(xs), hid, hid, 0, ST())
        assert st == 1 and b"misaligned" in lib.ptx_last_error()
    # the second Linear over the summed subsets; h = the float32 hidden rows of the reference
    h = want.float()
    w2, b2, y0 = rnd(20, hid, seed=106, scale=0.1), rnd(20, seed=107), rnd(B, 23, seed=108)
    want2 = sum(h[r * B:(r + 1) * B].double() for r in range(3)) @ w2.double().t() + 3 * b2.double() + y0[:, :20].double()

    def launch2(v, ar):
        L.check(lib.ptx_linear_setsum_fwd(P(v["h"]), P(v["w2"]), P(v["b2"]), P(v["y"]), B, 3, hid, 20, hid, 23, L.PTX_EPI_ACCUM, ST()),
                "setsum")

    res = run([("h", h, None, 16, "in"), ("w2", w2, None, 16, "in"), ("b2", b2, None, 4, "in"), ("y", y0, None, 4, "inout")], launch2)
    judge(res, "y", want2, 2e-5, (S, slice(0, 20)))
    for out in res:
        assert torch.equal(out["y"][:, 20:], y0[:, 20:])


# ---- ptx_maxpool3d_fwd: exact (test_gpu_kernels.py::test_maxpool); x and y 16-byte aligned (pool_head.hip: "maxpool3d: misaligned pointer")
MAXPOOL = [
    ("tile_kernel", 2, 5, 8, 8, 20, (3, 3, 3), (2, 2, 2), (1, 1, 1)),          # row 3 of test_maxpool: 2 x 2 patches
    ("slide_kernel", 1, 4, 6, 19, 8, (2, 2, 3), (2, 2, 1), (1, 1, 1)),         # row 7: W-sliding kernel (kH != 3)
    ("generic_kernel", 1, 2, 6, 9, 8, (1, 3, 2), (1, 1, 2), (0, 1, 1)),        # row 9: generic kernel (kW != 3)
]


@pytest.mark.parametrize("case", MAXPOOL, ids=[c[0] for c in MAXPOOL])
def test_maxpool(ptx, case):
    L, lib = ptx._lib, _lib(ptx)
    _, N, T, H, W, Cc, k, s, p = case
    x = rnd(N, Cc, T, H, W, seed=30)
    want = F.max_pool3d(x, k, s, p)
    To, Ho, Wo = want.shape[2:]
    xc = cl(x)
    ld = xc.shape[-1]
    d = L.PoolDesc(N, T, H, W, Cc, ld, To, Ho, Wo, *k, *s, *p)

    def launch(v, ar):
        L.check(lib.ptx_maxpool3d_fwd(C.byref(d), P(v["x"]), P(v["y"]), ST()), "maxpool")

    res = run([("x", xc, None, 16, "in"), ("y", (N, To, Ho, Wo, ld), F32, 16, "out")], launch)
    judge(res, "y", want.permute(0, 2, 3, 4, 1), 0, (Ellipsis, slice(0, Cc)), written=(Ellipsis, slice(0, r4(Cc))))


def test_maxpool_same_into_a_channel_slice(ptx):
    """TF-"SAME" pooling with zero-valued padding into a channel slice of a wider row (first row of
    test_gpu_kernels.py::test_maxpool_same_slices_copy_and_window_mean; exact): the columns outside the slice keep the fill."""
    L, lib = ptx._lib, _lib(ptx)
    N, T, H, W, Cc, k, s = 2, 5, 14, 14, 24, (1, 3, 3), (1, 2, 2)
    x = rnd(N, Cc, T, H, W, seed=90) - 0.5
    out = [-(-i // st) for i, st in zip((T, H, W), s)]
    tot = [max((o - 1) * st + kk - i, 0) for o, st, kk, i in zip(out, s, k, (T, H, W))]
    fr = [t // 2 for t in tot]
    want = F.max_pool3d(F.pad(x, (fr[2], tot[2] - fr[2], fr[1], tot[1] - fr[1], fr[0], tot[0] - fr[0])), k, s)
    xc = cl(x)
    total, c0 = Cc + 40, 8
    d = L.PoolDesc(N, T, H, W, Cc, xc.shape[-1], *out, *k, *s, *fr, total, L.PTX_POOL_SAME | L.PTX_POOL_PAD_ZERO)

    def launch(v, ar):
        L.check(lib.ptx_maxpool3d_fwd(C.byref(d), P(v["x"]), P(v["cat"], c0), ST()), "maxpool same")

    res = run([("x", xc, None, 16, "in"), ("cat", (N, *out, total), F32, 16, "out")], launch)
    judge(res, "cat", want.permute(0, 2, 3, 4, 1), 0, (Ellipsis, slice(c0, c0 + Cc)),
          untouched=[(Ellipsis, slice(0, c0)), (Ellipsis, slice(c0 + Cc, total))])


def test_window_mean_copy2d_outer_sum(ptx):
    L, lib = ptx._lib, _lib(ptx)
    # window mean, any 4-byte alignment (scalar kernel; nothing checked): 1e-6 of test_maxpool_same_slices_copy_and_window_mean
    x = rnd(3, 8, 21, seed=93)

    def launch(v, ar):
        L.check(lib.ptx_window_mean(P(v["x"]), P(v["y"]), 3, 8, 21, 2, 1, ST()), "window_mean")
        L.check(lib.ptx_window_mean(P(v["x"]), P(v["z"]), 3, 8, 21, 8, 1, ST()), "window_mean all")

    res = run([("x", x, None, 4, "in"), ("y", (3, 7, 21), F32, 4, "out"), ("z", (3, 1, 21), F32, 4, "out")], launch)
    judge(res, "y", (x[:, :-1].double() + x[:, 1:].double()) / 2, 1e-6, Ellipsis)
    judge(res, "z", x.double().mean(1, keepdim=True), 1e-6, Ellipsis)
    # copy2d into a column window: 16-byte pointers (pool_head.hip "copy2d: misaligned pointer"); a copy is exact
    src = rnd(7, 24, seed=92)

    def launch2(v, ar):
        L.check(lib.ptx_copy2d(P(v["src"]), P(v["dst"], 12), 7, 24, 24, 40, ST()), "copy2d")

    res = run([("src", src, None, 16, "in"), ("dst", (7, 40), F32, 16, "out")], launch2)
    judge(res, "dst", src, 0, (S, slice(12, 36)), untouched=[(S, slice(0, 12)), (S, slice(36, 40))])
    # outer sum: 4-byte pointers, pad column zero: 1e-6 of test_outer_sum_relu
    a, b = rnd(3, 10, seed=150), rnd(3, 7, seed=151)

    def launch3(v, ar):
        L.check(lib.ptx_outer_sum_relu(P(v["a"]), P(v["b"]), P(v["f"]), 3, 10, 7, 8, ST()), "outer_sum_relu")

    res = run([("a", a, None, 4, "in"), ("b", b, None, 4, "in"), ("f", (3, 10, 8), F32, 4, "out")], launch3)
    judge(res, "f", F.relu(a.double()[:, :, None] + b.double()[:, None, :]) / 7, 1e-6, (Ellipsis, slice(0, 7)), written=Ellipsis,
          zero=[(Ellipsis, slice(7, 8))])


def test_global_avgpool(ptx):
    """Both layouts and the bf16 map at element-size alignment (scalar kernels, no check in the entries): 1e-5 of
    test_gpu_kernels.py::test_avgpool_and_linear, whose shape this is."""
    L, lib = ptx._lib, _lib(ptx)
    x = rnd(3, 100, 2, 7, 7, seed=31)
    want = x.double().mean((2, 3, 4))
    xc = cl(x, 104)
    xc[..., 100:] = float("nan")                                   # channels [C, ld) are a neighbour's: never read
    xb = cl(x, 104).to(BF16)
    wantb = xb[..., :100].double().mean((1, 2, 3))

    def launch(v, ar):
        L.check(lib.ptx_global_avgpool(P(v["xc"]), P(v["y"]), 3, 100, 98, 104, 0, ST()), "avgpool cl")
        L.check(lib.ptx_global_avgpool(P(v["xf"]), P(v["y2"]), 3, 100, 98, 100, 1, ST()), "avgpool cf")
        L.check(lib.ptx_global_avgpool_bf16(P(v["xb"]), P(v["y3"]), 3, 100, 98, 104, ST()), "avgpool bf16")

    res = run([("xc", xc, None, 4, "in"), ("xf", x.contiguous(), None, 4, "in"), ("xb", xb, None, 2, "in"),
               ("y", (3, 100), F32, 4, "out"), ("y2", (3, 100), F32, 4, "out"), ("y3", (3, 100), F32, 4, "out")], launch)
    judge(res, "y", want, 1e-5, Ellipsis)
    judge(res, "y2", want, 1e-5, Ellipsis)
    judge(res, "y3", wantb, 1e-5, Ellipsis)


# ---- cBN fold and the affine / activation / upsample pass: 1e-5 of test_cbn_fold_affine_upsample_and_upsampled_skip ----------
def test_cbn_fold(ptx):
    L, lib = ptx._lib, _lib(ptx)
    N, tot = 3, 30
    gain, bias = rnd(N, tot, seed=111, scale=0.3), rnd(N, tot, seed=112, scale=0.3)
    mean, var = rnd(tot, seed=113, scale=0.2), torch.rand(tot, generator=torch.Generator().manual_seed(114)) + 0.5
    ldo = tot + 2
    sc = (1 + gain.double()) / torch.sqrt(var.double() + 1e-5)
    sh = bias.double() - mean.double() * sc

    def launch(v, ar):
        L.check(lib.ptx_cbn_fold(P(v["gain"]), P(v["bias"]), P(v["mean"]), P(v["var"]), C.c_float(1e-5), P(v["sc"]), P(v["sh"]),
                                 N, tot, tot, tot, ldo, 1, ST()), "fold")

    res = run([("gain", gain, None, 4, "in"), ("bias", bias, None, 4, "in"), ("mean", mean, None, 4, "in"), ("var", var, None, 4, "in"),
               ("sc", (N, ldo), F32, 4, "out"), ("sh", (N, ldo), F32, 4, "out")], launch)
    judge(res, "sc", sc, 1e-5, (S, slice(0, tot)), untouched=[(S, slice(tot, ldo))])
    judge(res, "sh", sh, 1e-5, (S, slice(0, tot)), untouched=[(S, slice(tot, ldo))])


AFFINE = [
    # name, C, ld_scale, first table column, alignment of the table rows, up, act
    ("vec4", 12, 32, 8, 16, 2, 1),                # C % 4 == 0, ld_scale % 4 == 0, tables 16-byte aligned: quad loads
    ("scalar_tables_off", 12, 32, 8, 4, 2, 1),    # the same extents, tables 4 bytes off: only the pointers decide
    ("scalar_odd_c", 10, 31, 12, 4, 1, 2),        # the existing test's C = 10 with an odd table pitch, tanh
]


@pytest.mark.parametrize("case", AFFINE, ids=[c[0] for c in AFFINE])
def test_affine_act_upsample(ptx, case):
    L, lib = ptx._lib, _lib(ptx)
    _, Cc, lds, off, at, up, act = case
    N, H, W = 3, 5, 6
    x = rnd(N, Cc, 1, H, W, seed=110)
    table_sc, table_sh = rnd(N, lds, seed=111, scale=0.3) + 1, rnd(N, lds, seed=112, scale=0.3)
    xc = cl(x)
    ld = xc.shape[-1]
    if ld > Cc:
        xc[..., Cc:] = 7.0                                          # pad channels of x may hold anything: y's are written as zero
    # the tables are windows [off, off + C) of wider rows; 4 * off is a multiple of 32, so the window is exactly as aligned as the row
    tsc, tsh = table_sc, table_sh
    ref = x[:, :, 0].double() * tsc[:, off:off + Cc].double()[:, :, None, None] + tsh[:, off:off + Cc].double()[:, :, None, None]
    ref = F.relu(ref) if act == 1 else (torch.tanh(ref) if act == 2 else ref)
    ref = F.interpolate(ref, scale_factor=up) if up > 1 else ref

    def launch(v, ar):
        L.check(lib.ptx_affine_act_upsample(P(v["x"]), P(v["y"]), P(v["sc"], off), P(v["sh"], off), lds, N, H, W, Cc, ld, ld, up, act,
                                            ST()), "affine")

    res = run([("x", xc, None, 16, "in"), ("sc", tsc, None, at, "in"), ("sh", tsh, None, at, "in"),
               ("y", (N, H * up, W * up, ld), F32, 16, "out")], launch)
    judge(res, "y", ref.permute(0, 2, 3, 1), 1e-5, (Ellipsis, slice(0, Cc)), written=Ellipsis, zero=[(Ellipsis, slice(Cc, ld))])


# ---- bf16-weight linears (linear_bf16.hip): 2e-5 / 5e-3 per route, as tests/test_gpu_trn_bf16.py ------------------------------
def _bf(t):
    return t.to(BF16)


LBW = [
    # name, x kind, M, K, Nout, ldx, (align x, w, b, y), route
    ("mfma_bf16_x", "bf16", 19, 264, 37, 272, (16, 16, 2, 4)),           # rows16 and bf16 x: matrix cores, split K with a workspace
    ("valu_vec_f32_x", "f32", 9, 264, 37, 268, (16, 16, 2, 4)),          # rows16, fp32 x: VALU kernel, a.vec = 1
    ("valu_scalar_f32_x_off", "f32", 9, 264, 37, 268, (4, 16, 2, 4)),    # the same extents, x 4 bytes off: a.vec = 0
    ("valu_scalar_w_off", "f32", 9, 264, 37, 268, (16, 2, 2, 4)),        # w 2 bytes off
    ("valu_scalar_bf16_x_off", "bf16", 19, 264, 37, 272, (2, 16, 2, 4)),  # bf16 x 2 bytes off: VALU kernel, scalar loads
    ("valu_scalar_odd_k", "bf16", 9, 61, 7, 61, (2, 2, 2, 4)),           # K % 8 != 0
]


@pytest.mark.parametrize("case", LBW, ids=[c[0] for c in LBW])
def test_linear_bf16w(ptx, case):
    """Reference: float64 on the bf16-rounded operands (what the kernels multiply); the products are exact in fp32 and only the
    summation order differs, so the fp32 linear tolerance 2e-5 of test_skinny_linear_gather_and_setsum applies
    (tests/test_gpu_trn_bf16.py compares these kernels with it as well)."""
    L, lib = ptx._lib, _lib(ptx)
    _, kind, M, K, N, ldx, (ax, aw, ab, ay) = case
    xk = L.PTX_LIN_X_BF16 if kind == "bf16" else L.PTX_LIN_X_F32
    x = torch.zeros(M, ldx)
    x[:, :K] = rnd(M, K, seed=200)
    x = _bf(x) if kind == "bf16" else x
    w, b = _bf(rnd(N, K, seed=201, scale=K ** -0.5)), _bf(rnd(N, seed=202))
    ldy = N + 3
    want = F.relu(F.relu(x[:, :K].double()) @ w.double().t() + b.double())
    ws_bytes = lib.ptx_linear_bf16w_workspace_bytes(M, K, N)
    specs = [("x", x, None, ax, "in"), ("w", w, None, aw, "in"), ("b", b, None, ab, "in"), ("y", (M, ldy), F32, ay, "out")]
    if ws_bytes:
        specs.append(("ws", (ws_bytes // 4,), F32, 16, "scratch"))

    def launch(v, ar):
        ws = v.get("ws")
        L.check(lib.ptx_linear_bf16w_fwd(P(v["x"]), xk, P(v["w"]), P(v["b"]), P(v["y"]), M, K, N, ldx, ldy,
                                         L.PTX_PRO_RELU | L.PTX_EPI_RELU, P(ws) if ws is not None else None, ws_bytes, ST()), "linear_bf16w")

    res = run(specs, launch)
    judge(res, "y", want, 2e-5, (S, slice(0, N)), untouched=[(S, slice(N, ldy))])


@pytest.mark.parametrize("ax,aw", [(16, 16), (4, 16), (16, 2)], ids=["vec", "scalar_x_off", "scalar_w_off"])
def test_linear_setsum_bf16w(ptx, ax, aw):
    L, lib = ptx._lib, _lib(ptx)
    B, n_sets, K, N, ldx = 5, 3, 72, 21, 76
    x = torch.zeros(n_sets * B, ldx)
    x[:, :K] = rnd(n_sets * B, K, seed=210)
    w, b = _bf(rnd(N, K, seed=211, scale=K ** -0.5)), _bf(rnd(N, seed=212))
    y0 = rnd(B, N + 2, seed=213)
    want = sum(x[r * B:(r + 1) * B, :K].double() for r in range(n_sets)) @ w.double().t() + n_sets * b.double() + y0[:, :N].double()

    def launch(v, ar):
        L.check(lib.ptx_linear_setsum_bf16w_fwd(P(v["x"]), P(v["w"]), P(v["b"]), P(v["y"]), B, n_sets, K, N, ldx, N + 2, L.PTX_EPI_ACCUM,
                                                ST()), "setsum_bf16w")

    res = run([("x", x, None, ax, "in"), ("w", w, None, aw, "in"), ("b", b, None, 2, "in"), ("y", y0, None, 4, "inout")], launch)
    judge(res, "y", want, 2e-5, (S, slice(0, N)))
    for out in res:
        assert torch.equal(out["y"][:, N:], y0[:, N:])


def test_relation_linear_bf16w(ptx):
    """x and w at 16 bytes (the entry refuses less: "x and w need 16 bytes"), b at 2, y at 4; a refusal for each of x and w."""
    L, lib = ptx._lib, _lib(ptx)
    B, T, Fd, hid = 5, 8, 64, 45
    x, w, b = _bf(rnd(B, T, Fd, seed=220)), _bf(rnd(hid, 4 * Fd, seed=221, scale=0.06)), _bf(rnd(hid, seed=222))
    subsets = [(0, 2, 3, 7), (1, 2, 5, 6), (0, 1, 2, 3)]
    d = L.RelationDesc()
    d.B, d.n_sets, d.n_frames, d.frame_len = B, 3, 4, Fd
    for r, sub in enumerate(subsets):
        for f, i in enumerate(sub):
            d.idx[r][f] = i
    want = torch.cat([F.relu(F.relu(x[:, list(sub)].reshape(B, -1).double()) @ w.double().t() + b.double()) for sub in subsets], 0)
    ws_bytes = lib.ptx_linear_bf16w_workspace_bytes(3 * B, 4 * Fd, hid)
    specs = [("x", x, None, 16, "in"), ("w", w, None, 16, "in"), ("b", b, None, 2, "in"), ("y", (3 * B, hid + 1), F32, 4, "out")]
    if ws_bytes:
        specs.append(("ws", (ws_bytes // 4,), F32, 16, "scratch"))

    def launch(v, ar):
        ws = v.get("ws")
        L.check(lib.ptx_relation_linear_bf16w_fwd(C.byref(d), P(v["x"]), T * Fd, P(v["w"]), P(v["b"]), P(v["y"]), hid, hid + 1,
                                                  L.PTX_PRO_RELU | L.PTX_EPI_RELU, P(ws) if ws is not None else None, ws_bytes, ST()),
                "relation_linear_bf16w")
        for ox, ow in ((1, 0), (0, 1)):                            # a host-side return: nothing is launched
            st = lib.ptx_relation_linear_bf16w_fwd(C.byref(d), P(v["x"], ox), T * Fd, P(v["w"], ow), P(v["b"]), P(v["y"]), hid, hid + 1,
                                                   0, None, 0, ST())
            assert st == 1 and b"x and w need 16 bytes" in lib.ptx_last_error()

    res = run(specs, launch)
    judge(res, "y", want, 2e-5, (S, slice(0, hid)), untouched=[(S, slice(hid, hid + 1))])
