"""The tuned table: what the autotuner measured, remembered per problem and shipped as tuned_gfx950.json.

One dict, key -> (name, number), behind one lock.  The entry kinds share it by key prefix:
    <conv key>          (tile configuration NAME, split-K)         tuned_lookup / tuned_store
    chain:<pair key>    (chained-tile configuration NAME, 1)       chain_lookup / chain_store
    alt:<pair key>      ("chain" | "pair", 1)                      alt_lookup / alt_store
    prog:<run hash>     ("program" | "launches", 1)                prog_lookup / prog_store
    body:<key>          ("tall" | "square" | "igemm", 1)           body_lookup / body_store
    wino:<key>          (grouped conv's tile NAME, 1 | 2)          wino_lookup / wino_store   (1 Winograd runs, 2 direct stays)
    wino4:<key>         (36-group conv's tile NAME, 1 | 2)         wino4_lookup / wino4_store (1 F(4x4) runs, 2 it does not)
    tfir:<key>          ("direct" | "fir", 0 | scheme)             tfir_lookup / tfir_store   (the fp32 stem: 0 direct, else the scheme)
    lanes:<model key>   ("lanes", n)                               lanes_lookup / lanes_store
Tiles are stored by NAME, so inserting / reordering the library's configuration tables cannot remap an entry silently.
"""
import json
import os
import threading

from . import _lib
from ._lib import PTX_BF16_OPERANDS, PTX_F16_OPERANDS, PTX_F16X3_OPERANDS

# PTX_TUNED_TABLE: another table file (tuning sessions: A/B a freshly dumped table against the shipped one on the same box)
_TUNED_PATH = os.environ.get("PTX_TUNED_TABLE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_gfx950.json")
_tuned = None                    # key -> (name, number); loaded from _TUNED_PATH on first use
_tuned_lock = threading.Lock()
_name_index = {}                 # "conv" / "chain" -> {configuration name: index into this build's table}


def _tuned_table():
    global _tuned
    with _tuned_lock:
        if _tuned is None:
            _tuned = {}
            if os.path.exists(_TUNED_PATH):
                try:
                    _tuned = {k: (str(v[0]), int(v[1])) for k, v in json.load(open(_TUNED_PATH)).items()
                              if isinstance(v[0], str)}
                except Exception:
                    _tuned = {}
        return _tuned


def _get(key):
    return _tuned_table().get(key)


def _put(key, name, number=1):
    table = _tuned_table()
    with _tuned_lock:
        table[key] = (str(name), int(number))


def tuned_snapshot():
    table = _tuned_table()
    with _tuned_lock:
        return dict(table)


def tuned_merge(entries):
    """Adopt another process's tuned entries (rank 0 tunes, every rank runs the same tiles)."""
    table = _tuned_table()
    with _tuned_lock:
        for k, v in entries.items():
            table[k] = (str(v[0]), int(v[1]))


def tuned_replace(entries):
    """Make `entries` the whole table (scripts/merge_tuned.py: merge files, then save)."""
    global _tuned
    with _tuned_lock:
        _tuned = {k: (str(v[0]), int(v[1])) for k, v in entries.items()}


def save_tuned_table(path=_TUNED_PATH):
    snap = tuned_snapshot()
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join('%s: ["%s", %d]' % (json.dumps(k), v[0], v[1]) for k, v in sorted(snap.items())) + "\n}\n")


# ---------------------------------------------------------------- tile names
def _index_of(table, name):
    """Index of a configuration by NAME in the loaded library's "conv" or "chain" table (None when this build has no such
    tile)."""
    idx = _name_index.get(table)
    if idx is None:
        lib = _lib.lib()
        if table == "conv":
            n = lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16()      # the bf16 tiles close the table
            idx = {lib.ptx_conv3d_config_name(i).decode(): i for i in range(n)}
        else:
            idx = {lib.ptx_conv3d_chain_config_name(i).decode(): i for i in range(lib.ptx_conv3d_chain_num_configs())}
        _name_index[table] = idx
    return idx.get(name)


def _config_index(name):
    return _index_of("conv", name)


def _chain_config_index(name):
    return _index_of("chain", name)


def _tile_kind(name):
    """Operand flavour of a tile configuration by name: "f16" (halfs), "bf16", "x3" (split fp32 on f16 MFMA) or "" (fp32)."""
    return "f16" if name.endswith("/f16") else "bf16" if name.endswith("/bf16") else "x3" if name.endswith("/x3") else ""


def _flags_kind(flags):
    if flags & PTX_BF16_OPERANDS:
        return "bf16"
    return "f16" if flags & PTX_F16_OPERANDS else "x3" if flags & PTX_F16X3_OPERANDS else ""


# ---------------------------------------------------------------- typed accessors
def tuned_lookup(key, kind=""):
    """(config index, split-K) of a tuned conv problem, or None: unknown keys, tiles this build does not
    have and entries of the wrong operand flavour all fall back to ptx_conv3d_pick_config."""
    kind = "f16" if kind is True else "" if kind is False else kind
    ent = _get(key)
    if ent is None or _tile_kind(ent[0]) != kind:
        return None
    idx = _config_index(ent[0])
    return None if idx is None else (idx, ent[1])


def tuned_store(key, cfg_index, split):
    _put(key, _lib.lib().ptx_conv3d_config_name(int(cfg_index)).decode(), split)


def chain_key(d, d2):
    return "chain:" + json.dumps(d.key() + d2.key())


def chain_lookup(key):
    """Tuned chained-tile index of a (conv, tail) problem pair, or None."""
    ent = _get(key)
    return None if ent is None else _chain_config_index(ent[0])


def chain_store(key, cfg_index):
    _put(key, _lib.lib().ptx_conv3d_chain_config_name(int(cfg_index)).decode())


def alt_lookup(key):
    ent = _get("alt:" + key)
    return None if ent is None else ent[0] == "chain"


def alt_store(key, use_chain):
    _put("alt:" + key, "chain" if use_chain else "pair")


def prog_lookup(key):
    ent = _get("prog:" + key)
    return None if ent is None else ent[0] == "program"


def prog_store(key, use_program):
    _put("prog:" + key, "program" if use_program else "launches")


BODY_SHAPES = ("tall", "square")      # ptx_conv_body_f32_fwd shapes 0 / 1
# filters the body kernels take: (1|3)x3x3 on the patch-resident tile; (3|5|7)x1x1 on the T-stacked tile (shape 0 only)
BODY_FILTERS = ((3, 3, 3), (1, 3, 3), (3, 1, 1), (5, 1, 1), (7, 1, 1))


def body_lookup(key):
    """Tuned verdict of a 3x3x3 problem on the patch-resident body kernel: shape index (0 tall, 1 square), -1 = the
    implicit-GEMM tile stays, None = never measured."""
    ent = _get("body:" + key)
    if ent is None:
        return None
    return BODY_SHAPES.index(ent[0]) if ent[0] in BODY_SHAPES else -1


def body_store(key, shape):
    _put("body:" + key, BODY_SHAPES[shape] if shape is not None and shape >= 0 else "igemm")


def wino_lookup(key):
    """Tuned verdict of a stride-1 (kT,3,3) problem (conv key, or the chain key of the pair it opens) on the Winograd
    launches: True = they run, False = the direct execution stays, None = never measured.  Like every entry the value names
    a tile -- the one the grouped conv was measured on -- and the number carries the verdict: 1 Winograd, 2 direct."""
    ent = _get("wino:" + key)
    return None if ent is None else ent[1] == 1


def wino_store(key, use_wino, cfg_index):
    _put("wino:" + key, _lib.lib().ptx_conv3d_config_name(int(cfg_index)).decode(), 1 if use_wino else 2)


def wino4_lookup(key):
    """Tuned verdict of the same problem on the Winograd F(4x4,3x3) launches: True = they run (instead of whatever the
    "wino:" verdict says), False = they do not, None = never measured -- which reads as False.  The name is the tile the
    36-group conv was measured on."""
    ent = _get("wino4:" + key)
    return None if ent is None else ent[1] == 1


def wino4_store(key, use_wino4, cfg_index):
    _put("wino4:" + key, _lib.lib().ptx_conv3d_config_name(int(cfg_index)).decode(), 1 if use_wino4 else 2)


def tfir_lookup(key):
    """Tuned verdict of an fp32 7x7x7 stem problem on the temporal fast-FIR launches: the scheme that runs (1..3), 0 = the
    direct launch stays, None = never measured -- which reads as 0."""
    ent = _get("tfir:" + key)
    return None if ent is None else int(ent[1])


def tfir_store(key, scheme):
    _put("tfir:" + key, "fir" if scheme else "direct", int(scheme))


def lanes_key(model, shape, precision="fp32"):
    """Tuned-table key of the clip-lanes decision: one per (architecture, input shape, arithmetic)."""
    name = getattr(model, "arch_name", None) or type(model).__name__
    return "lanes:" + json.dumps([str(name), [int(v) for v in shape], precision])


def lanes_lookup(key):
    """Lanes the tuner measured best for this (architecture, shape), or None when it was never measured."""
    ent = _get(key)
    return None if ent is None or ent[0] != "lanes" else int(ent[1])


def lanes_store(key, n):
    _put(key, "lanes", n)
