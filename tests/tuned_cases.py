"""The shipped tuned table (pretorched-x_amd/tuned_gfx950.json) as test cases, shared by test_tuned_table_host.py and
test_gpu_tuned_table.py.  Pure Python: no library, no GPU.

The table decides, per production convolution, which tile runs and with how many K splits -- combinations of (tile,
geometry, flags, split) that the kernel tests, which vary one axis at a time, never run.  A tuned problem is far too
large for a float64 reference, so every entry is SHRUNK: whatever selects a code path stays (channels, strides of the
rows, filter, stride, padding, flags, groups, the residual / second-source strides and the whole W axis -- the kw-reuse
and row-major-epilogue tiles work on whole output rows), and the row count is cut: at most 2 samples (an M tile may
straddle the sample boundary), at most 2 output frames and 2 output rows (4 under PTX_PRO_UP2, which needs even
upsampled extents).  A shrunken axis gets the smallest input extent that yields the new output extent under the entry's
own rule (symmetric padding or SAME), plus the remainder (in + 2p - k) mod s the tuned shape had, so trailing input rows
no tap reads stay present.
"""
import collections
import json
import os

from pretorched_x_amd._lib import (ConvDesc, PTX_EPI_RES_ADD, PTX_EPI_RES_PADA, PTX_EPI_RES_UP, PTX_F16_OPERANDS,
                                   PTX_F16X3_OPERANDS, PTX_PRO_UP2)

TABLE_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pretorched-x_amd", "tuned_gfx950.json")
FIELDS = tuple(f for f, _ in ConvDesc._fields_)
NF = len(FIELDS)
# shrink() leaves these alone, whatever the entry (the W axis included)
KEPT = ("Ci", "Co", "Kc", "Co_pad", "ldx", "ldy", "ldr", "kT", "kH", "kW", "sT", "sH", "sW", "pT", "pH", "pW", "flags",
        "groups", "res_C", "res_sT", "res_sH", "res_sW", "x2_C", "x2_ld", "x2_sT", "x2_sH", "x2_sW", "Wi", "Wo", "res_W",
        "x2_W")
MAX_N, MAX_T, MAX_H, MAX_H_UP2 = 2, 2, 2, 4
# Entries that may drop out of cases() / chain_cases(): table key -> the reason.  Nothing else may be missing
# (test_tuned_table_host.py), and the list may hold at most MAX_EXCLUDED entries.
EXCLUDED = {}
MAX_EXCLUDED = 20

Case = collections.namedtuple("Case", "key desc tile split")            # desc: {field: int} of the SHRUNKEN problem
ChainCase = collections.namedtuple("ChainCase", "key desc tail tile")


def load_table():
    """The shipped file as {key: (name, number)}, read by path (PTX_TUNED_TABLE does not redirect it)."""
    with open(TABLE_PATH) as f:
        return {k: (v[0], int(v[1])) for k, v in json.load(f).items()}


def split_kinds(table=None):
    """{kind: {key: value}} with kind in conv, chain, alt, body, wino, wino4, lanes, prog, tfir (the key prefix)."""
    out = collections.defaultdict(dict)
    for k, v in (load_table() if table is None else table).items():
        out["conv" if k.startswith("[") else k.split(":", 1)[0]][k] = v
    return dict(out)


def key_ints(key):
    """The integer list a table key carries after its prefixes ("chain:", "alt:chain:", "wino:" ...)."""
    return json.loads(key[key.index("["):])


def to_desc(ints):
    assert len(ints) == NF, len(ints)
    return dict(zip(FIELDS, (int(v) for v in ints)))


def fill(desc):
    """A ctypes ConvDesc from a {field: int} dict."""
    d = ConvDesc()
    for f in FIELDS:
        setattr(d, f, desc[f])
    return d


def extent_ok(n_in, n_out, k, s, p):
    """validate_desc's rule for one axis: symmetric padding p, or SAME (out = ceil(in / s), p = the front pad)."""
    if n_out == (n_in + 2 * p - k) // s + 1:
        return True
    same = (n_in + s - 1) // s
    return n_out == same and p == max((same - 1) * s + k - n_in, 0) // 2


def _shrink_axis(n_in, n_out, k, s, p, new_out):
    """Input extent of the axis for `new_out` outputs (or the tuned pair when no shrunken form is valid)."""
    if new_out >= n_out:
        return n_in, n_out
    if n_out == (n_in + 2 * p - k) // s + 1:                       # symmetric
        new_in = (new_out - 1) * s + k - 2 * p + (n_in + 2 * p - k) % s
        if new_in >= 1 and new_out == (new_in + 2 * p - k) // s + 1:
            return new_in, new_out
        return n_in, n_out
    # SAME: ceil(in / s) = out with the same front pad; prefer the tuned extent's residue mod s
    cands = [v for v in range((new_out - 1) * s + 1, new_out * s + 1) if extent_ok(v, new_out, k, s, p)]
    cands.sort(key=lambda v: (v % s != n_in % s, v))
    return (cands[0], new_out) if cands else (n_in, n_out)


def _gathered(n_out, stride, tuned_out, tuned_ext):
    """Extent of a strided operand (shortcut-A residual, second source) read at out * stride: the last index read plus
    the trailing rows the tuned shape carried beyond its own last index."""
    slack = tuned_ext - ((tuned_out - 1) * stride + 1)
    return (n_out - 1) * stride + 1 + max(0, min(slack, stride - 1))


def shrink(desc):
    d = dict(desc)
    d["N"] = min(desc["N"], MAX_N)
    up2 = bool(desc["flags"] & PTX_PRO_UP2)
    d["Ti"], d["To"] = _shrink_axis(desc["Ti"], desc["To"], desc["kT"], desc["sT"], desc["pT"], min(desc["To"], MAX_T))
    d["Hi"], d["Ho"] = _shrink_axis(desc["Hi"], desc["Ho"], desc["kH"], desc["sH"], desc["pH"],
                                    min(desc["Ho"], MAX_H_UP2 if up2 else MAX_H))
    if up2 and d["Hi"] % 2:
        d["Hi"], d["Ho"] = desc["Hi"], desc["Ho"]
    if desc["flags"] & PTX_EPI_RES_PADA:
        if desc["flags"] & PTX_EPI_RES_UP:                          # index = out >> res_s*
            d["res_T"] = ((d["To"] - 1) >> desc["res_sT"]) + 1
            d["res_H"] = ((d["Ho"] - 1) >> desc["res_sH"]) + 1
        else:                                                       # index = out * res_s*
            d["res_T"] = _gathered(d["To"], desc["res_sT"], desc["To"], desc["res_T"])
            d["res_H"] = _gathered(d["Ho"], desc["res_sH"], desc["Ho"], desc["res_H"])
    if desc["x2_C"] > 0:
        d["x2_T"] = _gathered(d["To"], desc["x2_sT"], desc["To"], desc["x2_T"])
        d["x2_H"] = _gathered(d["Ho"], desc["x2_sH"], desc["Ho"], desc["x2_H"])
    return d


def shrink_chain(desc, tail):
    """(d, d2) of a chain entry: `desc` shrunk, the tail over its output positions."""
    d = shrink(desc)
    t = dict(tail)
    t["N"] = d["N"]
    t["Ti"], t["Hi"], t["Wi"] = d["To"], d["Ho"], d["Wo"]
    t["To"], t["Ho"], t["Wo"] = d["To"], d["Ho"], d["Wo"]
    return d, t


def tile_bk(name):
    """BK of a tile named "BMxBNxBK/...": K columns per step (32-bit words on the 16-bit tiles, as Kc counts them)."""
    return int(name.split("/")[0].split("x")[2])


def k_steps(desc, name):
    """k-steps of the tile on the problem: taps x ceil(K / BK), both sources of a dual conv counted."""
    bk = tile_bk(name)
    groups = max(desc["groups"], 1)
    k_a = desc["Ci"] // groups if groups > 1 else max(desc["ldx"], desc["Kc"])
    chunks = -(-k_a // bk) + (-(-desc["x2_ld"] // bk) if desc["x2_C"] > 0 else 0)
    return desc["kT"] * desc["kH"] * desc["kW"] * chunks


def conv_entries(table=None):
    """[(key, desc, tile, split)] of the conv verdicts in the current key format."""
    return [(k, to_desc(key_ints(k)), v[0], v[1]) for k, v in sorted(split_kinds(table).get("conv", {}).items())
            if len(key_ints(k)) == NF]


def chain_entries(table=None):
    """[(key, desc, tail, tile)] of the "chain:" verdicts."""
    out = []
    for k, v in sorted(split_kinds(table).get("chain", {}).items()):
        ints = key_ints(k)
        if len(ints) == 2 * NF:
            out.append((k, to_desc(ints[:NF]), to_desc(ints[NF:]), v[0]))
    return out


def cases(table=None):
    """{tile name: [Case]}: every conv verdict shrunk, one case per distinct (shrunken descriptor, tile, split)."""
    out, seen = collections.OrderedDict(), set()
    for key, desc, tile, split in conv_entries(table):
        if key in EXCLUDED:
            continue
        d = shrink(desc)
        ident = (tuple(d[f] for f in FIELDS), tile, split)
        if ident in seen:
            continue
        seen.add(ident)
        out.setdefault(tile, []).append(Case(key, d, tile, split))
    return out


def chain_cases(table=None):
    """{chained tile name: [ChainCase]}, de-duplicated like cases()."""
    out, seen = collections.OrderedDict(), set()
    for key, desc, tail, tile in chain_entries(table):
        if key in EXCLUDED:
            continue
        d, t = shrink_chain(desc, tail)
        ident = (tuple(d[f] for f in FIELDS), tuple(t[f] for f in FIELDS), tile)
        if ident in seen:
            continue
        seen.add(ident)
        out.setdefault(tile, []).append(ChainCase(key, d, t, tile))
    return out


def covered_keys(table=None):
    """Keys of the entries cases() / chain_cases() stand for (an entry whose shrunken form equals another's is covered)."""
    return ({k for k, *_ in conv_entries(table) if k not in EXCLUDED} |
            {k for k, *_ in chain_entries(table) if k not in EXCLUDED})


def operand_kind(flags):
    return "f16" if flags & PTX_F16_OPERANDS else "x3" if flags & PTX_F16X3_OPERANDS else "fp32"


def ref_flops(desc):
    """Multiply-adds x 2 of the float64 reference of one (shrunken) conv problem."""
    groups = max(desc["groups"], 1)
    words = 2 if desc["flags"] & PTX_F16_OPERANDS else 1
    k = desc["kT"] * desc["kH"] * desc["kW"] * desc["Ci"] * words // groups + desc["x2_C"]
    return 2 * desc["N"] * desc["To"] * desc["Ho"] * desc["Wo"] * desc["Co"] * k


__all__ = ["TABLE_PATH", "FIELDS", "KEPT", "EXCLUDED", "MAX_EXCLUDED", "Case", "ChainCase", "load_table", "split_kinds",
           "key_ints", "to_desc", "fill", "extent_ok", "shrink", "shrink_chain", "tile_bk", "k_steps", "conv_entries",
           "chain_entries", "cases", "chain_cases", "covered_keys", "operand_kind", "ref_flops", "PTX_EPI_RES_ADD"]
