"""Shared plumbing of the tests/test_gpu_footprint_*.py modules: one launch under both arena fills, then the five
assertions every case makes -- (a) guards and inputs intact (Arena.check inside both_fills), (b) nothing non-finite in the
written region, (c) the layout contract (zero pad columns, untouched columns still holding the fill), (d) the values against
a float64 CPU reference at the tolerance of the family's existing test, (e) bit-identical outputs under the two fills."""
import ctypes as C

import torch

from arena import FILLS, assert_finite, assert_holds_fill, assert_same_bits, both_fills

DEV = "cuda:0"


def P(t, off=0):
    """Pointer to element `off` of a placed view."""
    return C.c_void_p(t.data_ptr() + off * t.element_size())


def ST():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run(specs, launch):
    """-> (outputs under 0xFF, outputs under 0x00): {name: CPU tensor} each."""
    return both_fills(DEV, specs, launch)


def close64(got, want, tol, what):
    """The suite's `close` (tests/test_gpu_kernels.py) against a float64 reference: max |err| <= tol * max(1, max |want|)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    want = want.double()
    scale = max(1.0, want.abs().max().item())
    err = (got.double() - want).abs().max().item()
    assert err <= tol * scale, "%s: max err %.3e (scale %.3e) exceeds %.1e" % (what, err, scale, tol)


def judge(res, name, want, tol, live, written=None, zero=(), untouched=(), bits=True, absolute=False):
    """res: run()'s pair.  live: index of the values `want` describes; written: index of everything the entry writes
    (default: live); zero: indices that must hold 0; untouched: indices that must still hold the fill.
    tol: 0 = exact; a number = the suite's `close` bound (x max(1, max |want|)), or max |err| <= tol itself with `absolute`;
    None = the caller has compared the values with a bar of its own.
    bits=False only for the launches that add into their output with floating-point atomics."""
    written = live if written is None else written
    for out, fill in zip(res, FILLS):
        got = out[name]
        assert_finite(got[written], "%s under fill 0x%02x" % (name, fill))                  # (b)
        for z in zero:                                                                    # (c)
            assert bool((got[z] == 0).all()), "%s: pad columns must be written as zero (fill 0x%02x)" % (name, fill)
        for u in untouched:
            assert_holds_fill(got[u], fill, "%s: columns the entry must leave untouched" % name)
        if tol is None:                                                                   # (d)
            pass
        elif tol == 0:
            assert torch.equal(got[live].double(), want.double()), "%s: not exact (fill 0x%02x)" % (name, fill)
        elif absolute:
            err = (got[live].double() - want.double()).abs().max().item()
            assert got[live].shape == want.shape and err <= tol, "%s: max err %.3e exceeds %.1e (fill 0x%02x)" % (name, err, tol, fill)
        else:
            close64(got[live], want, tol, "%s (fill 0x%02x)" % (name, fill))
    if bits:                                                                              # (e)
        assert_same_bits(res[0][name][written], res[1][name][written], name)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def r4(v):
    return (v + 3) // 4 * 4


def cl(x, ld=None):
    """NCDHW cpu -> channels-last [N,T,H,W,ld] cpu, zero pad channels (tests/test_gpu_kernels.py to_cl, on the host)."""
    n, c = x.shape[:2]
    ld = r4(c) if ld is None else ld
    y = torch.zeros(n, *x.shape[2:], ld, dtype=x.dtype)
    y[..., :c] = x.permute(0, 2, 3, 4, 1)
    return y


def repack(fn, src, n_out, dtype=torch.float32, a_in=16):
    """One filter re-pack (fn(src pointer, dst pointer) issues it) in the arena: the source an `in` operand, the re-laid filter
    an `out` operand of n_out elements at 16 bytes.  Returns the filter of the 0xFF run after checking that every element was
    written (nothing non-finite survives) and that the 0x00 run gives the same bits.  The caller feeds it to the kernel under
    test, whose float64 comparison then covers the values."""
    out = run([("src", src, None, a_in, "in"), ("dst", (n_out,), dtype, 16, "out")], lambda v, ar: fn(P(v["src"]), P(v["dst"])))
    judge(out, "dst", None, None, Ellipsis)
    return out[0]["dst"]
