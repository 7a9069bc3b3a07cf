"""The integer-logit attention inputs of tests/attention_cases.py, checked on the CPU: the logits are exact integers in
every precision and summation order, the references alone sit well inside every bar test_gpu_attention_logits.py applies,
and the inputs tell a correct online softmax from two broken ones that today's Gaussian inputs let through."""
import pytest
import torch

import attention_cases as AC

F32_BAR, F16_BAR = 2e-5, 5e-3              # tests/test_gpu_kernels.py::test_fused_nonlocal_attention


def _shapes():
    """(id, B, Nq, Nk, d, dv, group_keys) of every attention launch of the GPU tests."""
    rows = [(r[0],) + r[3:] for r in AC.FP32_ROWS + [AC.STREAMK_ROW]]
    rows += [("bf16-%d-%d-%d-%d" % r, AC.BF16_BATCH, r[2], r[3], r[0], r[1], 32) for r in AC.BF16_ROWS]
    return rows


SHAPES = _shapes()
KIND = {r[0]: r[2] for r in AC.FP32_ROWS + [AC.STREAMK_ROW]}


def _bar32(want, tol=F32_BAR):
    return tol * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_logits_are_exact_integers(shape):
    _, B, Nq, Nk, d, dv, gk = shape
    perm = torch.randperm(d, generator=torch.Generator().manual_seed(d))
    for profile in AC.profiles_for(Nk, gk):
        for shift in (True, False):
            th, ph, g = AC.make_inputs(profile, B, Nq, Nk, d, dv, gk, shift)
            for t in (th, ph):
                assert float(t.abs().max()) <= 128 and torch.equal(t, t.round())
                assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.half().float(), t)
            s64 = AC.logits(th, ph)
            assert torch.equal(AC.logits(th, ph, torch.float32).double(), s64) and torch.equal(s64, s64.round())
            assert torch.equal(AC.logits(th[..., perm], ph[..., perm], torch.float32).double(), s64)
            assert float(s64.abs().max()) <= 252
            if profile != "uniform" and shift:
                assert float(s64.abs().max()) >= 100               # the regime the issue is about
            if not shift:                                          # the shifted run differs by exactly r_i per row
                s_sh = AC.logits(*AC.make_inputs(profile, B, Nq, Nk, d, dv, gk, True)[:2])
                assert torch.equal(s_sh - s64, AC.row_shift(Nq).double()[None, :, None].expand_as(s64))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s[0])
def test_references_are_inside_the_gpu_bars(shape):
    """fp32 torch against fp64 under the fp32 / split-operand bar; one rounding of P and y to bf16 under the bf16 bar; fp16
    operands and P under the PTX_NL_F16 bar.  The margins printed on failure are what the kernels have to spend."""
    name, B, Nq, Nk, d, dv, gk = shape
    kind = KIND.get(name, "softmax")
    for profile in AC.profiles_for(Nk, gk):
        th, ph, g = AC.make_inputs(profile, B, Nq, Nk, d, dv, gk)
        if name.startswith("bf16"):
            g = g.to(torch.bfloat16).float()
            want = AC.reference(th, ph, g)
            err = (AC.narrow_emulation(th, ph, g, torch.bfloat16) - want).abs()
            bar = 2.0 ** -7 * float(g.abs().max()) + want.abs() * 2.0 ** -7
            assert bool((err <= bar).all()), (profile, float((err - bar).max()))
            continue
        want = AC.reference(th, ph, g, kind)
        err = float((AC.reference(th, ph, g, kind, torch.float32).double() - want).abs().max())
        assert err <= 0.25 * _bar32(want), (profile, err, _bar32(want))
        if name == "f16":
            err = float((AC.narrow_emulation(th, ph, g, torch.float16) - want).abs().max())
            assert err <= 0.5 * _bar32(want, F16_BAR), (profile, err)


def test_one_hot_profiles_select_one_value_row():
    """late_peak / peak_group*: the gap to every other key is at least 96 - 2 * 12, so in fp32 l rounds to 1 and y to g[j*]."""
    for shape in SHAPES:
        _, B, Nq, Nk, d, dv, gk = shape
        for profile in AC.ONE_HOT:
            j = AC.peak_key(profile, Nk, gk)
            if j is None:
                continue
            th, ph, g = AC.make_inputs(profile, B, Nq, Nk, d, dv, gk)
            s = AC.logits(th, ph)
            rest = torch.cat([s[..., :j], s[..., j + 1:]], -1)
            assert Nk == 1 or float((s[..., j] - rest.max(-1).values).min()) >= 72
            if gk is not None and profile != "late_peak":
                assert (j % (2 * gk)) // gk == int(profile[-1])      # the key group that sees it


def test_relu_rows_that_are_all_negative_exist():
    name, _, kind, B, Nq, Nk, d, dv, gk = [r for r in AC.FP32_ROWS if r[2] == "relu"][0]
    th, ph, g = AC.make_inputs("late_peak", B, Nq, Nk, d, dv, gk)
    s = AC.logits(th, ph)
    dead = (s < 0).all(-1)
    assert bool(dead.any()) and not bool(dead.all())
    assert bool((AC.reference(th, ph, g, "relu")[dead] == 0).all())


MUTATIONS = ("shared_max", "no_max")


def _emulation_passes(data, mutation):
    want = AC.reference(*data)
    got = AC.online_softmax_emulation(*data, mutation=mutation).double()
    return bool(torch.isfinite(got).all()) and float((got - want).abs().max()) <= _bar32(want)


def test_mutants_pass_todays_inputs_and_fail_the_new_ones():
    """The fp32 emulation of the tiled online softmax (16-key tiles) at the smallest row of test_fused_nonlocal_attention,
    against that test's 2e-5 bar: correct, with one maximum shared by the 16 queries of a wave, and with no max subtraction."""
    B, Nq, Nk, d, dv = 2, 100, 100, 16, 16
    today = AC.todays_inputs(B, Nq, Nk, d, dv)
    assert _emulation_passes(today, None)
    for mutation in MUTATIONS:
        assert _emulation_passes(today, mutation), mutation       # the gap: today's inputs accept both
    for profile in AC.profiles_for(Nk, 16):
        data = AC.make_inputs(profile, B, Nq, Nk, d, dv, 16)
        assert _emulation_passes(data, None), profile
        if profile == "uniform":
            continue
        for mutation in MUTATIONS:
            assert not _emulation_passes(data, mutation), (profile, mutation)


def test_softmax_rows_logits():
    for cols in AC.SOFTMAX_COLS:
        x, n = AC.softmax_rows_logits(cols)
        assert x.shape == (8 * n, cols) and torch.equal(x, x.round()) and float(x.abs().max()) <= 252
        assert torch.equal(x.to(torch.bfloat16).float(), x)       # exact as bf16 logits too
        want = torch.softmax(x.double(), -1)
        assert float((torch.softmax(x, -1).double() - want).abs().max()) <= 0.25e-6
        for k in range(1, 8):                                     # a row shift does not change the softmax
            assert torch.equal(torch.softmax(x[k * n:(k + 1) * n].double(), -1), want[:n])
        hi, lo, zero = (AC.SOFTMAX_ROWS.index(p) for p in ("high", "low", "zero"))
        assert torch.equal(want[hi], want[lo]) and torch.equal(want[hi], want[zero])
