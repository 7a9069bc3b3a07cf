"""Footprint tests of the layout / pack entry points (pack_layout.hip): operands in a guarded arena (tests/arena.py) at the
weakest alignment each entry accepts, once under each fill; guards and inputs intact, the layout contract, exact values
(these entries move or round values: every comparison is bit-exact, as in test_gpu_kernels.py::test_layout_transforms),
bit-identical outputs under the two fills.  The checksums add into *out with INTEGER atomics (exact in any order): not
excused from bit-equality either.

Alignment switch reached here: pack_layout.hip ptx_ncdhw_to_ndhwc writes whole 16-byte positions when C <= 4, ld == 4 and
`((uintptr_t)y & 15) == 0`, else runs the 32 x 32 tile transpose: one case on each side, same extents."""
import ctypes as C

import numpy as np
import pytest
import torch

from arena import FILLS, Arena, arena_bytes, assert_same_bits
from footprint import DEV, P, ST, judge, r4, rnd, run

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
S = slice(None)


def _lib(ptx):
    return ptx._lib.lib()


@pytest.mark.parametrize("N,Cc,Sp,ay", [(1, 70, 37, 4), (2, 3, 37, 16), (2, 3, 37, 4)],
                         ids=["tile_transpose_70x37", "rgb_y_aligned_positions", "rgb_y_4_bytes_off_tiles"])
def test_ncdhw_ndhwc_round_trip(ptx, N, Cc, Sp, ay):
    """x at any 4-byte alignment (scalar loads; check_layout_args checks no pointer)."""
    L, lib = ptx._lib, _lib(ptx)
    x = rnd(N, Cc, Sp, seed=40)
    ld = r4(Cc)

    def launch(v, ar):
        L.check(lib.ptx_ncdhw_to_ndhwc(P(v["x"]), P(v["y"]), N, Cc, Sp, ld, ST()), "to cl")
        L.check(lib.ptx_ndhwc_to_ncdhw(P(v["y"]), P(v["z"]), N, Cc, Sp, ld, ST()), "to cf")

    res = run([("x", x, None, 4, "in"), ("y", (N, Sp, ld), F32, ay, "out"), ("z", (N, Cc, Sp), F32, 4, "out")], launch)
    judge(res, "y", x.permute(0, 2, 1), 0, (Ellipsis, slice(0, Cc)), written=Ellipsis, zero=[(Ellipsis, slice(Cc, ld))])
    judge(res, "z", x, 0, Ellipsis)


def test_ncdhw_ndhwc_bf16_round_trip(ptx):
    """(1, 70, 37), ld = 72: the channels-last side 16-byte aligned ("layout_bf16: the channels-last tensor must be 16-byte
    aligned"), the NCDHW side at 2 bytes."""
    L, lib = ptx._lib, _lib(ptx)
    N, Cc, Sp, ld = 1, 70, 37, 72
    x = rnd(N, Cc, Sp, seed=40).to(BF16)

    def launch(v, ar):
        L.check(lib.ptx_ncdhw_to_ndhwc_bf16(P(v["x"]), P(v["y"]), N, Cc, Sp, ld, ST()), "to cl")
        L.check(lib.ptx_ndhwc_to_ncdhw_bf16(P(v["y"]), P(v["z"]), N, Cc, Sp, ld, ST()), "to cf")
        st = lib.ptx_ncdhw_to_ndhwc_bf16(P(v["x"]), P(v["y"], 1), N, Cc, Sp, ld, ST())       # host-side return, nothing launched
        assert st == 1 and b"16-byte aligned" in lib.ptx_last_error()

    res = run([("x", x, None, 2, "in"), ("y", (N, Sp, ld), BF16, 16, "out"), ("z", (N, Cc, Sp), BF16, 2, "out")], launch)
    judge(res, "y", x.permute(0, 2, 1), 0, (Ellipsis, slice(0, Cc)), written=Ellipsis, zero=[(Ellipsis, slice(Cc, ld))])
    judge(res, "z", x, 0, Ellipsis)


def test_transpose_last2_and_pad_rows(ptx):
    """Both at any 4-byte alignment (scalar kernels, no pointer check).  transpose: the case of test_layout_transforms
    ([2][50][24] with 22 live columns -> [2][22][52], rows [50, 52) zero); columns [22, 24) of x are never read."""
    L, lib = ptx._lib, _lib(ptx)
    x = rnd(2, 50, 24, seed=41)
    x[..., 22:] = float("nan")

    def launch(v, ar):
        L.check(lib.ptx_transpose_last2(P(v["x"]), P(v["y"]), 2, 50, 22, 24, 52, ST()), "transpose")

    res = run([("x", x, None, 4, "in"), ("y", (2, 22, 52), F32, 4, "out")], launch)
    judge(res, "y", x[:, :, :22].permute(0, 2, 1), 0, (Ellipsis, slice(0, 50)), written=Ellipsis, zero=[(Ellipsis, slice(50, 52))])
    rows, W, ld = 5, 37, 40
    x = rnd(rows, W, seed=42)

    def launch2(v, ar):
        L.check(lib.ptx_pad_rows(P(v["x"]), P(v["y"]), rows, W, ld, ST()), "pad_rows")

    res = run([("x", x, None, 4, "in"), ("y", (rows, ld), F32, 4, "out")], launch2)
    judge(res, "y", x, 0, (S, slice(0, W)), written=Ellipsis, zero=[(S, slice(W, ld))])


def test_ncdhw_to_split4(ptx):
    """x at 4 bytes, y at 16 ("ncdhw_to_split4: ... 16-byte aligned output": refused otherwise).  This entry has no alignment
    SWITCH: pack_layout.hip:954 is the switch of ptx_ncdhw_to_ndhwc (covered on both sides by test_ncdhw_ndhwc_round_trip);
    ptx_ncdhw_to_split4 has only the refusal at pack_layout.hip:943, asserted here with its message.  hi = half(v),
    lo = half((v - hi) * 2^12): the same fp32 operations on the host give the same bits."""
    L, lib = ptx._lib, _lib(ptx)
    N, Cc, Sp = 2, 3, 37
    x = rnd(N, Cc, Sp, seed=45)
    v4 = torch.zeros(N, Sp, 4)
    v4[..., :Cc] = x.permute(0, 2, 1)
    hi = v4.to(F16)
    want = torch.cat([hi, ((v4 - hi.float()) * 4096.0).to(F16)], -1)           # [N][S][8] halfs: hi c0..c3 | lo c0..c3

    def launch(v, ar):
        L.check(lib.ptx_ncdhw_to_split4(P(v["x"]), P(v["y"]), N, Cc, Sp, ST()), "split4")
        assert lib.ptx_ncdhw_to_split4(P(v["x"]), P(v["y"], 2), N, Cc, Sp, ST()) == 1       # host-side return, nothing launched
        assert b"16-byte aligned output" in lib.ptx_last_error()

    res = run([("x", x, None, 4, "in"), ("y", (N, Sp, 8), F16, 16, "out")], launch)
    judge(res, "y", want, 0, Ellipsis, zero=[(Ellipsis, slice(Cc, 4)), (Ellipsis, slice(4 + Cc, 8))])


def _special_f32():
    """37 values (not a multiple of any vector width): round-to-nearest-even ties both ways, +-0, denormals, +-Inf, NaN."""
    bits = [0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000,        # ties: to even down / up, and around them
            0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF,   # zeros, denormals
            0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000,                    # Inf, max (rounds to Inf), a tie at the top
            0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF]                                # quiet / signalling NaNs
    t = torch.tensor(np.array(bits, dtype=np.uint32).view(np.int32)).view(F32)
    return torch.cat([t, rnd(37 - len(bits), seed=46)])


def test_f32_to_bf16_and_back(ptx):
    """No direct test before this one.  Reference: torch's round-to-nearest-even conversion on the CPU; NaN stays NaN (payloads
    are not compared).  x of f32_to_bf16 at 4 bytes and y at 2; x of bf16_to_f32 at 2 and y at 4 (the entries' own checks)."""
    L, lib = ptx._lib, _lib(ptx)
    x = _special_f32()
    n = x.numel()
    assert n == 37
    want = x.to(BF16)
    xb = want.clone()

    def launch(v, ar):
        L.check(lib.ptx_f32_to_bf16(P(v["x"]), P(v["y"]), n, ST()), "f32_to_bf16")
        L.check(lib.ptx_bf16_to_f32(P(v["xb"]), P(v["z"]), n, ST()), "bf16_to_f32")

    res = run([("x", x, None, 4, "in"), ("xb", xb, None, 2, "in"), ("y", (n,), BF16, 2, "out"), ("z", (n,), F32, 4, "out")], launch)
    nan = torch.isnan(x)
    for out in res:
        y, z = out["y"], out["z"]
        assert torch.equal(torch.isnan(y.float()), nan) and torch.equal(torch.isnan(z), nan)
        assert torch.equal(y[~nan].view(torch.int16), want[~nan].view(torch.int16)), "f32_to_bf16 is not round-to-nearest-even"
        assert torch.equal(z[~nan].view(torch.int32), xb[~nan].float().view(torch.int32)), "bf16_to_f32 is not exact"
    assert_same_bits(res[0]["y"], res[1]["y"], "y")
    assert_same_bits(res[0]["z"], res[1]["z"], "z")


def _checksum(tensors, b16):
    """The sum of pack_layout.hip's checksum kernels in Python integers (mod 2^64)."""
    total = 0
    for t, a in enumerate(tensors):
        p = a.view(-1).view(torch.int16 if b16 else torch.int32).numpy().astype(np.uint16 if b16 else np.uint32).astype(object)
        acc = 0
        for i, v in enumerate(p):
            acc += (int(v) + (1 if b16 else 0)) * (((2654435761 * i) & 0xFFFFFFFF) | 1)
        total += (acc & 0xFFFFFFFFFFFFFFFF) * (2 * t + 1)
    return total & 0xFFFFFFFFFFFFFFFF


@pytest.mark.parametrize("b16", [False, True], ids=["f32", "b16"])
def test_checksum(ptx, b16):
    """The table holds the tensors' own addresses, so it is built after they are placed (Arena used directly; the same
    offsets under both fills).  table and out at 8 bytes, the tensors at their element size; the table and the tensors are
    `in` operands (untouched), *out is `inout`: zeroed by the caller, the only thing written."""
    L, lib = ptx._lib, _lib(ptx)
    dt = BF16 if b16 else F32
    tensors = [rnd(37, seed=47).to(dt), rnd(3, 101, seed=48).to(dt), rnd(1, seed=49).to(dt)]
    want = _checksum(tensors, b16)
    sizes = [t.numel() * t.element_size() for t in tensors] + [16 * len(tensors), 8]
    ar = Arena(arena_bytes(sizes), DEV, FILLS[0])
    got, addrs = [], None
    for fill in FILLS:
        ar.reset(fill)
        views = [ar.place(t, align=t.element_size(), role="in", name="t%d" % i) for i, t in enumerate(tensors)]
        table = torch.tensor([[v.data_ptr(), v.numel()] for v in views], dtype=torch.int64)
        tv = ar.place(table, align=8, role="in", name="table")
        out = ar.place(torch.zeros(1, dtype=torch.int64), align=8, role="inout", name="out")
        now = [v.data_ptr() for v in views + [tv, out]]
        assert addrs is None or addrs == now
        addrs = now
        fn = lib.ptx_checksum_b16 if b16 else lib.ptx_checksum_f32
        L.check(fn(P(tv), len(tensors), P(out), ST()), "checksum")
        torch.cuda.synchronize()
        got.append(int(ar.check()["out"].cpu().item()) & 0xFFFFFFFFFFFFFFFF)
    assert got[0] == want and got[1] == want, (got, want)


def test_pack_conv_weight_ragged(ptx):
    """ptx_pack_conv_weight (fp32 layout) at a ragged (Co, Ci) = (20, 10): Kc = 12, Co_pad = 128, three taps, conv bias and BN
    fold.  Every pointer at 4 bytes (scalar kernels, nothing checked).  The whole [taps][Co_pad][Kc] block and all Co_pad biases
    are written: zeros in the pad rows and columns.  Bars, derived: the folded filter w * (gamma * (1 / sqrt(var + eps))) is five
    fp32 roundings (sum, root, reciprocal, two products): (1 + 2^-24)^5 - 1 < 6 * 2^-24 relative; the bias
    beta + (b - mean) * s adds a difference, a product and a sum: 7 * 2^-24 (|beta| + |(b - mean) s|)."""
    L, lib = ptx._lib, _lib(ptx)
    Co, Ci, kT, Kc, Co_pad, eps = 20, 10, 3, 12, 128, 1e-5
    w, cb = rnd(Co, Ci, kT, 1, 1, seed=60), rnd(Co, seed=61)
    g = torch.Generator().manual_seed(62)
    gamma, beta = torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g) * 0.1
    mean, var = torch.randn(Co, generator=g) * 0.1, torch.rand(Co, generator=g) + 0.5
    pd = L.PackDesc(Co, Ci, kT, 1, 1, Kc, Co_pad, 0)
    assert lib.ptx_packed_weight_elems(C.byref(pd)) == kT * Co_pad * Kc

    def launch(v, ar):
        L.check(lib.ptx_pack_conv_weight(C.byref(pd), P(v["w"]), P(v["cb"]), P(v["gamma"]), P(v["beta"]), P(v["mean"]), P(v["var"]),
                                         C.c_float(eps), P(v["wp"]), P(v["bp"]), ST()), "pack")

    res = run([("w", w, None, 4, "in"), ("cb", cb, None, 4, "in"), ("gamma", gamma, None, 4, "in"), ("beta", beta, None, 4, "in"),
               ("mean", mean, None, 4, "in"), ("var", var, None, 4, "in"), ("wp", (kT, Co_pad, Kc), F32, 4, "out"),
               ("bp", (Co_pad,), F32, 4, "out")], launch)
    s = gamma.double() / (var.double() + float(np.float32(eps))).sqrt()
    want_w = torch.zeros(kT, Co_pad, Kc, dtype=torch.float64)
    want_w[:, :Co, :Ci] = (w.double()[:, :, :, 0, 0] * s[:, None, None]).permute(2, 0, 1)
    prod = (cb.double() - mean.double()) * s
    for out in res:
        wp, bp = out["wp"].double(), out["bp"].double()
        assert torch.isfinite(wp).all() and torch.isfinite(bp).all()
        assert bool(((wp - want_w).abs() <= 6 * 2.0 ** -24 * want_w.abs()).all())              # pad rows / columns: exactly zero
        assert bool(((bp[:Co] - (beta.double() + prod)).abs() <= 7 * 2.0 ** -24 * (beta.double().abs() + prod.abs())).all())
        assert bool((bp[Co:] == 0).all())
    assert_same_bits(res[0]["wp"], res[1]["wp"], "wp")
    assert_same_bits(res[0]["bp"], res[1]["bp"], "bp")


def test_ncdhw_to_split_planes(ptx):
    """x and y at 16 bytes with W % 8 == 0 ("ncdhw_to_split_planes: ... 16-byte aligned pointers": refused otherwise, asserted).
    Six half planes per frame: hi of c0 c1 c2, then lo = half((v - hi) * 2^12); C = 2 leaves the third pair zero.  Same fp32
    operations on the host: exact."""
    L, lib = ptx._lib, _lib(ptx)
    N, Cc, T, H, W = 2, 2, 3, 5, 24
    x = rnd(N, Cc, T, H, W, seed=50)
    v3 = torch.zeros(N, T, 3, H, W)
    v3[:, :, :Cc] = x.permute(0, 2, 1, 3, 4)
    hi = v3.to(F16)
    want = torch.cat([hi, ((v3 - hi.float()) * 4096.0).to(F16)], 2)              # [N][T][6][H][W]

    def launch(v, ar):
        L.check(lib.ptx_ncdhw_to_split_planes(P(v["x"]), P(v["y"]), N, Cc, T, H, W, ST()), "split planes")
        for ox, oy in ((1, 0), (0, 2)):                                          # host-side return, nothing launched
            assert lib.ptx_ncdhw_to_split_planes(P(v["x"], ox), P(v["y"], oy), N, Cc, T, H, W, ST()) == 1
            assert b"16-byte aligned pointers" in lib.ptx_last_error()

    res = run([("x", x, None, 16, "in"), ("y", (N, T, 6, H, W), F16, 16, "out")], launch)
    judge(res, "y", want, 0, Ellipsis, zero=[(S, S, slice(Cc, 3)), (S, S, slice(3 + Cc, 6))])


def test_fold_kw(ptx):
    """ptx_fold_kw_ncdhw and ptx_fold_kw_strided (every second frame): y[n][t][h][wo][kw * C + c] = x[n][c][t][h][wo * sW - pW + kw],
    zero outside the image and in columns [kW * C, ld).  x at 4 bytes (scalar loads into LDS), y at 16 ("fold_kw: misaligned
    output", asserted).  The stem's own geometry at a small odd size: C = 3, kW = 7, sW = 2, pW = 3, ld = 24.  A move: exact."""
    L, lib = ptx._lib, _lib(ptx)
    N, Cc, T, H, W, kW, sW, pW, ld = 2, 3, 4, 5, 13, 7, 2, 3, 24
    Wo = (W + 2 * pW - kW) // sW + 1
    x = rnd(N, Cc, T, H, W, seed=51)

    def ref(xs):
        n, c, t, h, w = xs.shape
        xp = torch.zeros(n, c, t, h, w + 2 * pW + sW)
        xp[..., pW:pW + w] = xs
        y = torch.zeros(n, t, h, Wo, ld)
        for wo in range(Wo):
            for kw in range(kW):
                y[:, :, :, wo, kw * c:(kw + 1) * c] = xp[..., wo * sW + kw].permute(0, 2, 3, 1)
        return y

    T2 = (T + 1) // 2

    def launch(v, ar):
        L.check(lib.ptx_fold_kw_ncdhw(P(v["x"]), P(v["y"]), N, Cc, T, H, W, kW, sW, pW, Wo, ld, ST()), "fold_kw")
        L.check(lib.ptx_fold_kw_strided(P(v["x"]), P(v["y2"]), N, Cc, T2, H, W, Cc * T * H * W, T * H * W, 2 * H * W, kW, sW, pW, Wo, ld, ST()),
                "fold_kw strided")
        assert lib.ptx_fold_kw_ncdhw(P(v["x"]), P(v["y"], 1), N, Cc, T, H, W, kW, sW, pW, Wo, ld, ST()) == 1
        assert b"misaligned output" in lib.ptx_last_error()

    res = run([("x", x, None, 4, "in"), ("y", (N, T, H, Wo, ld), F32, 16, "out"), ("y2", (N, T2, H, Wo, ld), F32, 16, "out")], launch)
    judge(res, "y", ref(x), 0, Ellipsis, zero=[(Ellipsis, slice(kW * Cc, ld))])
    judge(res, "y2", ref(x[:, :, ::2]), 0, Ellipsis, zero=[(Ellipsis, slice(kW * Cc, ld))])


def test_im2col_hw_bf16_x_two_bytes_off(ptx):
    """ptx_im2col_hw_bf16: x "at any 2-byte alignment" (placed 2 bytes off a 4-byte boundary), y at 16 ("im2col_hw_bf16:
    misaligned pointer", asserted).  y[n][t][ho][wo][(kh * kW + kw) * C + c] = x[n][c][t][ho * sH - pH + kh][wo * sW - pW + kw],
    zero outside the image and in columns [kH * kW * C, ld); ld = 160 for the 7 x 7 x 3 stem.  A move of bf16 values: exact."""
    L, lib = ptx._lib, _lib(ptx)
    N, Cc, T, H, W, k, s, p, ld = 1, 3, 2, 9, 11, 7, 2, 3, 160
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = rnd(N, Cc, T, H, W, seed=52).to(BF16)
    xp = torch.zeros(N, Cc, T, H + 2 * p + s, W + 2 * p + s, dtype=BF16)
    xp[..., p:p + H, p:p + W] = x
    want = torch.zeros(N, T, Ho, Wo, ld, dtype=BF16)
    for ho in range(Ho):
        for wo in range(Wo):
            patch = xp[..., ho * s:ho * s + k, wo * s:wo * s + k]                  # [N][C][T][kh][kw]
            want[:, :, ho, wo, :k * k * Cc] = patch.permute(0, 2, 3, 4, 1).reshape(N, T, k * k * Cc)

    def launch(v, ar):
        args = (N, Cc, T, H, W, k, k, s, s, p, p, Ho, Wo, ld, ST())
        L.check(lib.ptx_im2col_hw_bf16(P(v["x"]), P(v["y"]), *args), "im2col")
        assert lib.ptx_im2col_hw_bf16(P(v["x"]), P(v["y"], 4), *args) == 1 and b"misaligned pointer" in lib.ptx_last_error()

    res = run([("x", x, None, 2, "in"), ("y", (N, T, Ho, Wo, ld), BF16, 16, "out")], launch)
    judge(res, "y", want, 0, Ellipsis, zero=[(Ellipsis, slice(k * k * Cc, ld))])
