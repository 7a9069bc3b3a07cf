"""Footprint tests of the attention / soft-max entry points (nonlocal_attn.hip, ptx_softmax_rows, ptx_bgemm_nt): operands in a
guarded arena (tests/arena.py) at the weakest alignment each entry accepts, once under each fill; guards and inputs intact,
nothing non-finite written, the layout contract, a float64 reference at the existing test's tolerance, bit-identical outputs
under the two fills (no launch here uses floating-point atomics: none is excused).

Alignment switch reached here: nonlocal_attn.hip ptx_nonlocal_ws_fwd takes the stream-K form only with a 16-byte aligned
workspace (`!((uintptr_t)workspace & 15)`); a workspace 4 bytes off is the documented fallback to ptx_nonlocal_fwd's kernels."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import attention_cases as AC
from arena import assert_same_bits
from footprint import P, ST, judge, r4, rnd, run

pytestmark = pytest.mark.gpu

F32 = torch.float32
S = slice(None)


def _lib(ptx):
    return ptx._lib.lib()


@pytest.mark.parametrize("scale_only", [0, 1], ids=["softmax", "scale"])
def test_softmax_rows_in_place(ptx, scale_only):
    """cols = 37, ld = 40, in place (role inout), any 4-byte alignment (scalar kernel, the entry checks nothing): 1e-6 of
    test_gpu_kernels.py::test_softmax_and_bgemm.  Pad columns [cols, ld) are written as zero whatever they held."""
    L, lib = ptx._lib, _lib(ptx)
    rows, cols, ld = 5, 37, 40
    x = rnd(rows, ld, seed=42, scale=3.0)
    want = x[:, :cols].double() / cols if scale_only else F.softmax(x[:, :cols].double(), -1)
    x[:, cols:] = float("nan")

    def launch(v, ar):
        L.check(lib.ptx_softmax_rows(P(v["x"]), rows, cols, ld, scale_only, ST()), "softmax")

    res = run([("x", x, None, 4, "inout")], launch)
    judge(res, "x", want, 1e-6, (S, slice(0, cols)), written=Ellipsis, zero=[(S, slice(cols, ld))])


def test_bgemm_nt(ptx):
    """(1, 70, 33, 10) of test_gpu_kernels.py::test_softmax_and_bgemm at its 1e-4; A, B, C 16-byte aligned ("bgemm: misaligned
    pointer").  Columns [round_up(K, 4), lda) of A are a neighbour's (NaN here); columns [Nn, ldc) of C are written as zero."""
    L, lib = ptx._lib, _lib(ptx)
    B, M, Nn, K = 1, 70, 33, 10
    lda, ldb, ldc = r4(K) + 4, r4(K), r4(Nn)
    a, b = torch.zeros(B, M, lda), torch.zeros(B, Nn, ldb)
    a[..., :K], b[..., :K] = rnd(B, M, K, seed=43), rnd(B, Nn, K, seed=44)
    a[..., r4(K):] = float("nan")
    want = torch.matmul(a[..., :K].double(), b[..., :K].double().transpose(1, 2))

    def launch(v, ar):
        L.check(lib.ptx_bgemm_nt(P(v["a"]), P(v["b"]), P(v["c"]), B, M, Nn, K, lda, ldb, ldc, M * lda, Nn * ldb, M * ldc, ST()), "bgemm")

    res = run([("a", a, None, 16, "in"), ("b", b, None, 16, "in"), ("c", (B, M, ldc), F32, 16, "out")], launch)
    judge(res, "c", want, 1e-4, (Ellipsis, slice(0, Nn)), written=Ellipsis, zero=[(Ellipsis, slice(Nn, ldc))])


def _nl_inputs(B, Nq, Nk, d, dv, seed):
    """Operands as test_gpu_kernels.py::test_fused_nonlocal_attention builds them: channel slices of one fused projection."""
    g_ = torch.Generator().manual_seed(seed)
    ld = r4(2 * d + dv) + 4
    tq, tk = torch.randn(B, Nq, ld, generator=g_), torch.randn(B, Nk, ld, generator=g_)
    tq[..., :d] *= 3.0 / d ** 0.5
    tq[..., d:] = float("nan")                                     # the other slices of the query-side tensor are never read
    tk[..., :d] = float("nan")
    tk[..., 2 * d + dv:] = float("nan")
    theta, phi, gv = tq[..., :d].double(), tk[..., d:2 * d].double(), tk[..., 2 * d:2 * d + dv].double()
    want = torch.matmul(F.softmax(torch.matmul(theta, phi.transpose(1, 2)), dim=-1), gv)
    return tq, tk, ld, want


def _nl_desc(L, B, Nq, Nk, d, dv, ld, ldy):
    desc = L.NonlocalDesc()
    desc.batch, desc.Nq, desc.Nk, desc.d, desc.dv = B, Nq, Nk, d, dv
    desc.ld_theta = desc.ld_phi = desc.ld_g = ld
    desc.ld_y = ldy
    desc.bs_theta, desc.bs_phi, desc.bs_g, desc.bs_y = Nq * ld, Nk * ld, Nk * ld, Nq * ldy
    desc.mode = L.PTX_NL_SOFTMAX
    return desc


def test_nonlocal_fwd(ptx):
    """The smallest row of tests/attention_cases.py (tile64: 2 x 100 x 100 x 16 x 16), 16-byte aligned operands ("nonlocal:
    misaligned pointer"), 2e-5 of test_fused_nonlocal_attention.  Columns [dv, ld_y) are left untouched."""
    L, lib = ptx._lib, _lib(ptx)
    _, _, _, B, Nq, Nk, d, dv, _ = [r for r in AC.FP32_ROWS if r[0] == "tile64"][0]
    tq, tk, ld, want = _nl_inputs(B, Nq, Nk, d, dv, 1000 + Nq + d)
    ldy = r4(dv) + 8
    desc = _nl_desc(L, B, Nq, Nk, d, dv, ld, ldy)
    assert lib.ptx_nonlocal_supported(C.byref(desc))

    def launch(v, ar):
        L.check(lib.ptx_nonlocal_fwd(C.byref(desc), P(v["tq"]), P(v["tk"], d), P(v["tk"], 2 * d), P(v["y"]), ST()), "nonlocal")

    res = run([("tq", tq, None, 16, "in"), ("tk", tk, None, 16, "in"), ("y", (B, Nq, ldy), F32, 16, "out")], launch)
    judge(res, "y", want, 2e-5, (Ellipsis, slice(0, dv)), untouched=[(Ellipsis, slice(dv, ldy))])


@pytest.mark.parametrize("flavour", ["fp32", "x3"])
def test_nonlocal_ws_fwd_aligned_and_misaligned_workspace(ptx, monkeypatch, flavour):
    """(fp32 and the split-operand flavour PTX_NL_X3: launch_nl_sk<.., 0> and <.., 2>.)  The stream-K row of tests/attention_cases.py (1 x 530 x 1000 x 200 x 136) with PTX_NL_STREAMK=1, as
    test_nonlocal_attention_stream_k runs it (2e-5): the workspace is placed in the arena too -- 16-byte aligned (the
    stream-K form: scratch, nothing to zero) and 4 bytes off (the documented fallback, which must equal ptx_nonlocal_fwd
    bit for bit)."""
    L, lib = ptx._lib, _lib(ptx)
    _, _, _, B, Nq, Nk, d, dv, _ = AC.STREAMK_ROW
    monkeypatch.setenv("PTX_NL_STREAMK", "1")
    tq, tk, ld, want = _nl_inputs(B, Nq, Nk, d, dv, 2000 + Nq + d)
    ldy = r4(dv) + 8
    desc = _nl_desc(L, B, Nq, Nk, d, dv, ld, ldy)
    desc.mode |= L.PTX_NL_X3 if flavour == "x3" else 0
    need = lib.ptx_nonlocal_workspace_bytes(C.byref(desc))
    assert need > 0 and need % 16 == 0
    specs = [("tq", tq, None, 16, "in"), ("tk", tk, None, 16, "in"), ("ws", (need // 4,), F32, 16, "scratch"),
             ("ws_off", (need // 4,), F32, 4, "scratch"), ("y", (B, Nq, ldy), F32, 16, "out"),
             ("y_off", (B, Nq, ldy), F32, 16, "out"), ("y_plain", (B, Nq, ldy), F32, 16, "out")]

    def launch(v, ar):
        args = (C.byref(desc), P(v["tq"]), P(v["tk"], d), P(v["tk"], 2 * d))
        L.check(lib.ptx_nonlocal_ws_fwd(*args, P(v["y"]), P(v["ws"]), need, ST()), "nonlocal ws")
        L.check(lib.ptx_nonlocal_ws_fwd(*args, P(v["y_off"]), P(v["ws_off"]), need, ST()), "nonlocal ws, workspace 4 bytes off")
        L.check(lib.ptx_nonlocal_fwd(*args, P(v["y_plain"]), ST()), "nonlocal")
        torch.cuda.synchronize()
        assert bool((v["ws_off"].view(torch.uint8) == ar.fill).all()), "the fallback must not touch a workspace it refused"

    res = run(specs, launch)
    for name in ("y", "y_off", "y_plain"):
        judge(res, name, want, 2e-5, (Ellipsis, slice(0, dv)), untouched=[(Ellipsis, slice(dv, ldy))])
    for out in res:
        assert_same_bits(out["y_off"][..., :dv], out["y_plain"][..., :dv], "ws_fwd with a misaligned workspace vs nonlocal_fwd")


# ---- bf16 attention: the fused kernel (variant 0) and the key-split kernel (variant 1) ----------------------------------------
BF16_NL = [
    # id, variant, d, dv, Nq, Nk
    ("fused_smallest_odd", 0, 3, 3, 37, 9),            # smallest row of tests/test_gpu_nl_bf16.py::KERNEL_CASES
    ("fused_odd_widths", 0, 10, 10, 64, 64),
    ("ksplit_d32", 1, 32, 256, 37, 65),                # rows of tests/attention_cases.py::BF16_ROWS: Nk = 64 + 1
    ("ksplit_empty_group", 1, 256, 256, 64, 9),        # group 1 sees no key at all
]


@pytest.mark.parametrize("case", BF16_NL, ids=[c[0] for c in BF16_NL])
def test_nonlocal_bf16(ptx, case):
    """ptx_nonlocal_bf16_variant_fwd (variant 0 is what ptx_nonlocal_bf16_fwd launches) with the operands laid out as
    tests/test_gpu_nl_bf16.py::_run_kernel lays them: theta a channel slice at column 8 of a wider row, phi and g slices of one
    buffer whose columns past round8 hold NaN, y at column 8 of a wider row.  Pointers 16 bytes (header: "pointers 16-byte
    aligned"; "nonlocal: misaligned pointer").  Bar of that module: 2^-7 (max |g| + |ref|).  Columns [dv, round8(dv)) of y are
    zeros, everything else outside the slice keeps the fill."""
    L, lib = ptx._lib, _lib(ptx)
    _, variant, d, dv, Nq, Nk = case
    B = 2
    gen = torch.Generator().manual_seed(7 * d + dv)
    amp = (2.0 / d ** 0.5) ** 0.5
    BF = torch.bfloat16
    th = (torch.randn(B, Nq, d, generator=gen) * amp).to(BF)
    ph = (torch.randn(B, Nk, d, generator=gen) * amp).to(BF)
    g = torch.randn(B, Nk, dv, generator=gen).to(BF)
    ref = torch.softmax(th.double() @ ph.double().transpose(1, 2), -1) @ g.double()
    d8, dv8 = (d + 7) // 8 * 8, (dv + 7) // 8 * 8
    ldt, ldk, ldy = 8 + d8 + 8, d8 + dv8 + 8, 8 + dv8 + 16
    T = torch.zeros(B, Nq, ldt, dtype=BF)
    T[:, :, 8:8 + d] = th
    T[:, :, :8] = float("nan")
    T[:, :, 8 + d8:] = float("nan")
    K = torch.zeros(B, Nk, ldk, dtype=BF)
    K[:, :, :d] = ph
    K[:, :, d8:d8 + dv] = g
    K[:, :, d8 + dv8:] = float("nan")
    desc = L.NonlocalDesc()
    desc.batch, desc.Nq, desc.Nk, desc.d, desc.dv = B, Nq, Nk, d, dv
    desc.ld_theta, desc.ld_phi, desc.ld_g, desc.ld_y = ldt, ldk, ldk, ldy
    desc.bs_theta, desc.bs_phi, desc.bs_g, desc.bs_y = Nq * ldt, Nk * ldk, Nk * ldk, Nq * ldy
    desc.mode = L.PTX_NL_BF16 | L.PTX_NL_SOFTMAX
    assert lib.ptx_nonlocal_bf16_variant_supported(C.byref(desc), variant)

    def launch(v, ar):
        L.check(lib.ptx_nonlocal_bf16_variant_fwd(C.byref(desc), variant, P(v["T"], 8), P(v["K"]), P(v["K"], d8), P(v["y"], 8), ST()),
                "nonlocal bf16 variant %d" % variant)

    res = run([("T", T, None, 16, "in"), ("K", K, None, 16, "in"), ("y", (B, Nq, ldy), BF, 16, "out")], launch)
    live = (Ellipsis, slice(8, 8 + dv))
    bar = 2.0 ** -7 * float(g.abs().max()) + ref.abs() * 2.0 ** -7
    for out in res:
        err = (out["y"][live].double() - ref).abs()
        assert bool((err <= bar).all()), float((err - bar).max())
    judge(res, "y", ref, None, live, written=(Ellipsis, slice(8, 8 + dv8)), zero=[(Ellipsis, slice(8 + dv, 8 + dv8))],
          untouched=[(Ellipsis, slice(0, 8)), (Ellipsis, slice(8 + dv8, ldy))])
