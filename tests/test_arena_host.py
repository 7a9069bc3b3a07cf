"""The footprint checker's own test (tests/arena.py), on a CPU arena with fake "kernels" written as torch CPU ops.  Four
planted errors must each be reported with the operand's name and the byte offset; a correct op must pass."""
import pytest
import torch

from arena import FILLS, GRAIN, MIN_GUARD, Arena, ArenaError, arena_bytes, assert_finite, assert_same_bits, both_fills

N = 37                                            # floats per operand: not a multiple of any vector width


def _x():
    return torch.arange(1, N + 1, dtype=torch.float32) / 8


def _flat(ar):
    """The whole arena as fp32 words (a fake kernel addresses past its operands through this)."""
    return ar.buf.view(torch.float32)


def _arena(fill, align_x=16, align_y=16):
    ar = Arena(arena_bytes([4 * N, 4 * N]), "cpu", fill)
    x = ar.place(_x(), align=align_x, role="in", name="x")
    y = ar.place((N,), torch.float32, align=align_y, role="out", name="y")
    return ar, x, y


def _w(ar, v):
    """Word index of a view's first element in the arena."""
    off = v.data_ptr() - ar.base
    assert off % 4 == 0
    return off // 4


@pytest.mark.parametrize("fill", FILLS)
def test_a_correct_op_passes(fill):
    ar, x, y = _arena(fill)
    torch.mul(x, 2.0, out=y)
    outs = ar.check()
    assert list(outs) == ["y"] and outs["y"].data_ptr() == y.data_ptr()
    assert torch.equal(outs["y"], _x() * 2)
    assert_finite(outs["y"], "y")


@pytest.mark.parametrize("fill", FILLS)
def test_store_one_element_past_the_output_is_reported(fill):
    ar, x, y = _arena(fill)
    torch.mul(x, 2.0, out=y)
    _flat(ar)[_w(ar, y) + N] = 1.23              # 0x3f9d70a4: no byte of it equals either fill
    with pytest.raises(ArenaError, match=r"1 bytes past the end of `y`"):
        ar.check()


@pytest.mark.parametrize("fill", FILLS)
def test_store_one_element_before_the_output_is_reported(fill):
    ar, x, y = _arena(fill)
    torch.mul(x, 2.0, out=y)
    _flat(ar)[_w(ar, y) - 1] = 1.23
    with pytest.raises(ArenaError, match=r"4 bytes before the start of `y`"):
        ar.check()


@pytest.mark.parametrize("fill", FILLS)
def test_an_input_modified_in_place_is_reported(fill):
    ar, x, y = _arena(fill)
    torch.mul(x, 2.0, out=y)
    x[5] = -x[5]                                   # the sign bit: byte 3 of element 5
    with pytest.raises(ArenaError, match=r"`in` operand `x` was modified at byte offset 23\b"):
        ar.check()


def _reads_one_past(views, ar):
    """y[i] = 2 x[i] + 0 * x[i + 1]: the last lane reads one element past `x` and multiplies it by zero."""
    x, y = views["x"], views["y"]
    nxt = _flat(ar)[_w(ar, x) + 1:_w(ar, x) + 1 + N]
    torch.add(x * 2.0, nxt * 0.0, out=y)


def test_a_zero_weighted_read_past_the_input_shows_in_both_ways():
    specs = [("x", _x(), None, 16, "in"), ("y", (N,), torch.float32, 16, "out")]
    ff, zz = both_fills("cpu", specs, _reads_one_past)         # no guard changed, no input changed: check() passes
    assert torch.isnan(ff["y"][N - 1]) and torch.isfinite(ff["y"][:N - 1]).all()
    with pytest.raises(AssertionError, match=r"y: 1 non-finite values, the first at element %d" % (N - 1)):
        assert_finite(ff["y"], "y")
    assert torch.equal(zz["y"], _x() * 2)
    with pytest.raises(AssertionError, match=r"depends on the fill: \d+ bytes differ .* byte offset %d" % (4 * (N - 1))):
        assert_same_bits(ff["y"], zz["y"], "y")
    ff, zz = both_fills("cpu", specs, lambda v, ar: torch.mul(v["x"], 2.0, out=v["y"]))
    assert_same_bits(ff["y"], zz["y"], "y")
    assert_finite(ff["y"], "y")


@pytest.mark.parametrize("align", [1, 2, 4, 8, 16, 32, 64, 128, 256, 512])
def test_place_is_exactly_that_aligned_and_no_better(align):
    dtype = torch.uint8 if align == 1 else torch.bfloat16 if align == 2 else torch.float32
    ar = Arena(arena_bytes([400, 400]), "cpu", 0xFF)
    a = ar.place((100,), dtype, align=align, role="out", name="a")
    b = ar.place(torch.zeros(100, dtype=dtype), align=align, role="in", name="b")
    for v in (a, b):
        assert v.data_ptr() % GRAIN == align % GRAIN
        assert v.data_ptr() % align == 0 and (align == GRAIN or v.data_ptr() % (2 * align) == align)
    ar.check()


def test_guards_never_overlap_operands_and_cover_the_largest_operand():
    big = 3 * MIN_GUARD + 20
    sizes = [big, 52, 4 * N, 7]
    ar = Arena(arena_bytes(sizes), "cpu", 0x00, guard=max(MIN_GUARD, big))
    ar.place((big,), torch.uint8, align=1, role="out", name="big")
    ar.place((13,), torch.float32, align=4, role="out", name="f")
    ar.place(_x(), align=16, role="in", name="x")
    ar.place((7,), torch.uint8, align=1, role="scratch", name="s", zero=True)
    spans, guards = ar.spans(), ar.guards()
    assert len(guards) == len(spans) + 1 and guards[0][0] == 0 and guards[-1][1] == ar.nbytes
    for i, (name, a, b) in enumerate(spans):
        assert guards[i][1] == a and guards[i + 1][0] == b          # guard | operand | guard, nothing shared
        assert b - a == sizes[i]
    for a, b in guards:
        assert b - a >= max(MIN_GUARD, big)
    covered = sorted([(a, b) for _, a, b in spans] + guards)
    assert covered[0][0] == 0 and all(covered[i][1] == covered[i + 1][0] for i in range(len(covered) - 1))
    ar.check()


def test_a_guard_shorter_than_a_later_larger_operand_is_refused():
    ar = Arena(arena_bytes([16, 4 * MIN_GUARD], guard=4 * MIN_GUARD), "cpu", 0xFF)
    ar.place((4,), torch.float32, align=16, role="out", name="small")          # its head guard is 64 KiB only
    ar.place((4 * MIN_GUARD,), torch.uint8, align=16, role="out", name="large")
    with pytest.raises(AssertionError, match="shorter than"):
        ar.check()


def test_scratch_is_zeroed_on_request_and_out_keeps_the_fill():
    ar = Arena(arena_bytes([64, 64, 64]), "cpu", 0xFF)
    s0 = ar.place((16,), torch.int32, align=16, role="scratch", name="counters", zero=True)
    s1 = ar.place((16,), torch.int32, align=16, role="scratch", name="partials")
    y = ar.place((16,), torch.float32, align=4, role="out", name="y")
    assert bool((s0 == 0).all()) and bool((s1 == -1).all()) and bool(torch.isnan(y).all())
    s1.fill_(3)                                      # scratch contents are the kernel's business
    assert set(ar.check()) == {"y"}
