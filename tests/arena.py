"""A guarded arena for footprint tests: every operand of a kernel launch is carved out of ONE owned allocation, at exactly
the alignment asked for and no better, with guard bands on both sides.  An access that leaves its operand then lands in
memory the test owns and shows up as a changed guard byte (a stray store), a changed `in` operand, or -- for a stray load
-- as a NaN under the 0xFF fill and as a difference between the runs under the two fills.  Nothing faults.

    ar = Arena(nbytes, "cuda:0", 0xFF)
    x = ar.place(x_cpu, align=16, role="in", name="x")
    y = ar.place((M, ldy), torch.float32, align=4, role="out", name="y")
    ... launch on x.data_ptr() / y.data_ptr() ...
    torch.cuda.synchronize()
    outs = ar.check()            # raises ArenaError naming the operand and the byte offset; returns {"y": view}

The two fills: 0xFF bytes are a NaN in fp32, fp16 and bf16 (and 255 in uint8); 0x00 is the other.  `both_fills` runs one
launch under each on the SAME allocation and the same offsets, so the addresses are identical between the two runs."""
import numpy as np
import torch

MIN_GUARD = 64 << 10
GRAIN = 512                       # torch allocations are 512-byte aligned: the arena's addresses are taken modulo this
ROLES = ("in", "out", "inout", "scratch")
FILLS = (0xFF, 0x00)


class ArenaError(AssertionError):
    pass


def nbytes_of(src, dtype=None):
    if isinstance(src, torch.Tensor):
        return src.numel() * src.element_size()
    n = 1
    for s in src:
        n *= int(s)
    return n * torch.empty(0, dtype=dtype).element_size()


def arena_bytes(sizes, guard=None):
    """Bytes that hold operands of these sizes with their guards (head and tail included) at any alignment."""
    guard = max([MIN_GUARD] + list(sizes)) if guard is None else guard
    return sum(sizes) + (len(sizes) + 1) * (guard + GRAIN) + GRAIN


class Arena:
    def __init__(self, nbytes, device="cpu", fill=0xFF, guard=MIN_GUARD):
        """`guard`: the least distance kept between operands; a placement raises it to the largest operand placed so
        far, and check() asserts that every gap covers max(64 KiB, the largest operand placed)."""
        assert guard >= MIN_GUARD
        self.device = torch.device(device)
        raw = torch.empty(nbytes + GRAIN, dtype=torch.uint8, device=self.device)
        head = (-raw.data_ptr()) % GRAIN               # host allocations are only 64-byte aligned: start on the grain
        self.buf = raw[head:head + nbytes]
        self.base = self.buf.data_ptr()
        assert self.base % GRAIN == 0
        self.nbytes = nbytes
        self.min_guard = guard
        self.reset(fill)

    def reset(self, fill):
        """Refill every byte and forget the placements: the same place() calls then return the same addresses."""
        assert 0 <= fill <= 255
        self.fill = fill
        self.buf.fill_(fill)
        self.ops = []                                  # dicts: name, off, nbytes, role, view, sent (uint8 numpy or None)
        self.largest = 0

    def place(self, src, dtype=None, align=16, role="in", name=None, zero=False):
        """src: a CPU tensor (uploaded; its dtype and shape are the view's) or a shape with `dtype`.  The view's address
        is congruent to `align` modulo 512: exactly that aligned and no better.  `zero`: a scratch operand whose contract
        says the caller zeroes it."""
        assert role in ROLES, role
        is_t = isinstance(src, torch.Tensor)
        assert is_t or role in ("out", "scratch"), "an `%s` operand needs its contents" % role
        dtype = src.dtype if is_t else dtype
        shape = tuple(src.shape) if is_t else tuple(int(s) for s in src)
        esz = torch.empty(0, dtype=dtype).element_size()
        n = nbytes_of(src, dtype)
        assert n > 0 and 0 < align <= GRAIN and align & (align - 1) == 0 and align % esz == 0, (n, align, esz)
        self.largest = max(self.largest, n)
        gap = max(self.min_guard, self.largest)
        lo = (self.ops[-1]["off"] + self.ops[-1]["nbytes"] if self.ops else 0) + gap
        off = lo + (align % GRAIN - lo) % GRAIN
        assert off + n + gap <= self.nbytes, "arena of %d bytes is too small for %r (%d bytes at %d, guard %d)" % (
            self.nbytes, name, n, off, gap)
        view = self.buf[off:off + n].view(dtype).view(shape)
        ptr = view.data_ptr()
        assert ptr == self.base + off and ptr % GRAIN == align % GRAIN, "placement is not exactly %d-byte aligned" % align
        assert align == GRAIN or (ptr % (2 * align)) != 0
        sent = None
        if is_t:
            view.copy_(src.contiguous())
            sent = src.contiguous().view(-1).view(torch.uint8).numpy().copy()
        elif zero:
            view.zero_()
        self.ops.append(dict(name=name or "op%d" % len(self.ops), off=off, nbytes=n, role=role, view=view, sent=sent))
        return view

    def spans(self):
        """[(name, first byte, one past the last byte)] of the placements, in address order."""
        return [(o["name"], o["off"], o["off"] + o["nbytes"]) for o in self.ops]

    def guards(self):
        """[(first byte, one past the last byte)] of the guard bands: head, between neighbours, tail."""
        edges = [0] + [e for _, a, b in self.spans() for e in (a, b)] + [self.nbytes]
        return [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2)]

    def _blame(self, pos):
        """Name a guard byte by its nearest operand."""
        best = None
        for name, a, b in self.spans():
            d = a - pos if pos < a else pos - b + 1
            if best is None or d < best[0]:
                best = (d, "%d bytes before the start of `%s`" % (a - pos, name) if pos < a else
                        "%d bytes past the end of `%s`" % (pos - b + 1, name))
        return best[1] if best else "in an empty arena"

    def check(self):
        """After the device is idle: every guard byte still holds the fill and every `in` operand is bit-identical to what
        was uploaded.  Returns {name: view} of the `out` / `inout` operands."""
        need = max(MIN_GUARD, self.largest)
        host = self.buf.cpu().numpy()
        for a, b in self.guards():
            assert b - a >= need, "guard [%d, %d) is shorter than max(64 KiB, largest operand) = %d" % (a, b, need)
            bad = np.flatnonzero(host[a:b] != self.fill)
            if bad.size:
                pos = a + int(bad[0])
                raise ArenaError("guard byte changed %s (arena byte %d): 0x%02x, fill 0x%02x; %d guard bytes differ in this band"
                                 % (self._blame(pos), pos, host[pos], self.fill, bad.size))
        for o in self.ops:
            if o["role"] != "in":
                continue
            bad = np.flatnonzero(host[o["off"]:o["off"] + o["nbytes"]] != o["sent"])
            if bad.size:
                k = int(bad[0])
                raise ArenaError("`in` operand `%s` was modified at byte offset %d: 0x%02x, uploaded 0x%02x; %d bytes differ"
                                 % (o["name"], k, host[o["off"] + k], o["sent"][k], bad.size))
        return {o["name"]: o["view"] for o in self.ops if o["role"] in ("out", "inout")}


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy()


def assert_finite(t, what):
    """No NaN / Inf in a written region (a float view, or a slice of one)."""
    f = t.detach().cpu().float()
    bad = torch.nonzero(~torch.isfinite(f).view(-1))
    assert bad.numel() == 0, "%s: %d non-finite values, the first at element %d (a load outside an operand met the 0xFF fill?)" % (
        what, bad.numel(), int(bad[0]))


def assert_holds_fill(t, fill, what):
    """Columns a header says are left untouched still hold the fill."""
    bad = np.flatnonzero(_bits(t) != fill)
    assert bad.size == 0, "%s: %d bytes no longer hold the fill 0x%02x, the first at byte %d" % (what, bad.size, fill, int(bad[0]) if bad.size else -1)


def assert_same_bits(a, b, what):
    """The outputs under the two fills: any difference means the result depends on memory outside the operands."""
    ba, bb = _bits(a), _bits(b)
    assert ba.shape == bb.shape
    bad = np.flatnonzero(ba != bb)
    assert bad.size == 0, "%s: the output depends on the fill: %d bytes differ between the 0xFF and 0x00 runs, the first at byte offset %d" % (
        what, bad.size, int(bad[0]) if bad.size else -1)


def both_fills(device, specs, launch, fills=FILLS):
    """Run `launch(views)` once per fill with every operand placed in ONE arena at the same offsets.

    specs: [(name, cpu tensor or shape, dtype or None, align, role)] (+ an optional sixth `zero` for scratch).
    launch(views, arena): views = {name: view}; it issues the entry's launches (and may return anything).
    Returns [{name: cpu clone of each out / inout operand}, ...] in the order of `fills`, after check()."""
    sizes = [nbytes_of(s[1], s[2]) for s in specs]
    guard = max([MIN_GUARD] + sizes)
    ar = Arena(arena_bytes(sizes, guard), device, fills[0], guard)
    results, addrs = [], None
    for fill in fills:
        ar.reset(fill)
        views = {}
        for s in specs:
            views[s[0]] = ar.place(s[1], s[2], s[3], s[4], name=s[0], zero=(len(s) > 5 and s[5]))
        now = [v.data_ptr() for v in views.values()]
        assert addrs is None or addrs == now, "the two fills must run at identical addresses"
        addrs = now
        launch(views, ar)
        if ar.device.type == "cuda":
            torch.cuda.synchronize()
        outs = ar.check()
        results.append({k: v.detach().cpu().clone() for k, v in outs.items()})
    return results
