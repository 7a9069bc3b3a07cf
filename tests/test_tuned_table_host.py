"""No-GPU tests of the SHIPPED tuned table (pretorched-x_amd/tuned_gfx950.json): every key parses into the current
descriptor format, every named tile exists in this build with the operand kind its flags call for, the library's own
*_supported answers are 1 at the tuned shape AND at the shrunken shape test_gpu_tuned_table.py runs, no entry drops out of
the GPU cases except through tuned_cases.EXCLUDED, and every split is one the tile can take.  A plan build drops an entry
ptx_conv3d_config_supported refuses without a word (Plan._pick_tile); here it fails."""
import ctypes as C

import pytest

import tuned_cases as TC

NF = TC.NF


@pytest.fixture(scope="module")
def lib(ptx):
    return ptx._lib.lib()


@pytest.fixture(scope="module")
def kinds():
    return TC.split_kinds()


def _conv_names(lib):
    return {lib.ptx_conv3d_config_name(i).decode(): i
            for i in range(lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16())}


def _chain_names(lib):
    return {lib.ptx_conv3d_chain_config_name(i).decode(): i for i in range(lib.ptx_conv3d_chain_num_configs())}


def test_key_format(kinds):
    """Every key parses; conv / body: / wino: / wino4: keys carry one descriptor, chain keys (bare or behind another
    prefix) two.  An entry of another length can never match ConvDesc.key() and is dead weight."""
    assert set(kinds) <= {"conv", "chain", "alt", "body", "wino", "wino4", "lanes", "prog", "tfir"}, sorted(kinds)
    bad = {}
    for kind in ("conv", "chain", "alt", "body", "wino", "wino4"):
        for key in kinds.get(kind, {}):
            rest = key if kind == "conv" else key.split(":", 1)[1]
            want = 2 * NF if kind in ("chain", "alt") or rest.startswith("chain:") else NF
            ints = TC.key_ints(key)
            if len(ints) != want or not all(isinstance(v, int) for v in ints):
                bad[key] = (len(ints), want)
    assert not bad, "%d keys not in the current format: %s" % (len(bad), list(bad.items())[:3])
    for key, (name, n) in kinds.get("alt", {}).items():
        assert key.startswith("alt:chain:") and name in ("chain", "pair"), key
    for key, (name, n) in kinds.get("lanes", {}).items():
        assert name == "lanes" and n >= 1 and isinstance(TC.key_ints(key), list), key
    print("tuned table: %s" % {k: len(v) for k, v in sorted(kinds.items())})


def test_tiles_exist_with_the_flags_operand_kind(ptx, lib, kinds):
    from pretorched_x_amd import tuned
    conv, chain = _conv_names(lib), _chain_names(lib)
    for key, desc, tile, split in TC.conv_entries():
        assert tile in conv, "%s: this build has no tile %s" % (key, tile)
        assert tuned._tile_kind(tile) == tuned._flags_kind(desc["flags"]), (key, tile)
        assert not desc["flags"] & ptx._lib.PTX_BF16_OPERANDS, key
    for key, desc, tail, tile in TC.chain_entries():
        assert tile in chain, "%s: this build has no chained tile %s" % (key, tile)
        assert tuned._tile_kind(tile) == tuned._flags_kind(desc["flags"]) == tuned._flags_kind(tail["flags"]), (key, tile)
    for kind in ("wino", "wino4"):                     # the value names the tile the grouped conv was measured on
        for key, (tile, n) in kinds.get(kind, {}).items():
            assert tile in conv and n in (1, 2), (key, tile, n)
    for key, (shape, n) in kinds.get("body", {}).items():
        assert shape in tuned.BODY_SHAPES + ("igemm",), (key, shape)


def test_supported_at_the_tuned_and_the_shrunken_shape(lib):
    conv, chain = _conv_names(lib), _chain_names(lib)
    entries, chains = TC.conv_entries(), TC.chain_entries()
    refused = []
    for key, desc, tile, split in entries:
        for what, d in (("tuned", desc), ("shrunken", TC.shrink(desc))):
            if lib.ptx_conv3d_config_supported(C.byref(TC.fill(d)), conv[tile]) != 1:
                refused.append((what, tile, key, lib.ptx_last_error().decode()))
    for key, desc, tail, tile in chains:
        for what, (d, t) in (("tuned", (desc, tail)), ("shrunken", TC.shrink_chain(desc, tail))):
            if lib.ptx_conv3d_chain_supported(C.byref(TC.fill(d)), C.byref(TC.fill(t)), chain[tile]) != 1:
                refused.append((what, tile, key, lib.ptx_last_error().decode()))
    assert not refused, "%d refusals, e.g. %s" % (len(refused), refused[:3])
    print("supported at both shapes: %d conv entries, %d chain entries" % (len(entries), len(chains)))


def test_no_entry_drops_out_of_the_gpu_cases(kinds):
    """cases() / chain_cases() stand for every conv and chain entry of the table, except the listed exclusions."""
    assert len(TC.EXCLUDED) <= TC.MAX_EXCLUDED, "%d exclusions (cap %d)" % (len(TC.EXCLUDED), TC.MAX_EXCLUDED)
    every = set(kinds.get("conv", {})) | set(kinds.get("chain", {}))
    assert set(TC.EXCLUDED) <= every, "exclusions that name no entry: %s" % sorted(set(TC.EXCLUDED) - every)
    assert all(isinstance(r, str) and r for r in TC.EXCLUDED.values())
    assert TC.covered_keys() == every - set(TC.EXCLUDED)
    cs, ch = TC.cases(), TC.chain_cases()
    # every covered entry's shrunken problem is one of the cases, on its own tile and split
    have = {(tuple(c.desc[f] for f in TC.FIELDS), c.tile, c.split) for v in cs.values() for c in v}
    for key, desc, tile, split in TC.conv_entries():
        if key not in TC.EXCLUDED:
            assert (tuple(TC.shrink(desc)[f] for f in TC.FIELDS), tile, split) in have, key
    have = {(tuple(c.desc[f] for f in TC.FIELDS), tuple(c.tail[f] for f in TC.FIELDS), c.tile) for v in ch.values() for c in v}
    for key, desc, tail, tile in TC.chain_entries():
        if key not in TC.EXCLUDED:
            d, t = TC.shrink_chain(desc, tail)
            assert (tuple(d[f] for f in TC.FIELDS), tuple(t[f] for f in TC.FIELDS), tile) in have, key
    n_conv, n_chain = sum(len(v) for v in cs.values()), sum(len(v) for v in ch.values())
    rows = max(c.desc["N"] * c.desc["To"] * c.desc["Ho"] * c.desc["Wo"] for v in cs.values() for c in v)
    assert rows <= TC.MAX_N * TC.MAX_T * TC.MAX_H_UP2 * 256
    print("conv entries %d -> %d cases on %d tiles (largest group %d, at most %d rows, %.1f GFLOP of float64 reference); "
          "chain entries %d -> %d cases on %d tiles; exclusions %d" % (
              len(TC.conv_entries()), n_conv, len(cs), max(len(v) for v in cs.values()), rows,
              sum(TC.ref_flops(c.desc) for v in cs.values() for c in v) / 1e9,
              len(TC.chain_entries()), n_chain, len(ch), len(TC.EXCLUDED)))


def test_shrink_keeps_what_selects_code_paths():
    changed = {}
    shrunk = 0
    for key, desc, tile, split in TC.conv_entries():
        d = TC.shrink(desc)
        for f in TC.KEPT:
            if d[f] != desc[f]:
                changed[(key, f)] = (desc[f], d[f])
        assert d["N"] == min(desc["N"], TC.MAX_N) and d["To"] <= desc["To"] and d["Ho"] <= desc["Ho"], key
        for ax, k in (("T", "kT"), ("H", "kH"), ("W", "kW")):
            assert TC.extent_ok(d[ax + "i"], d[ax + "o"], d[k], d["s" + ax], d["p" + ax]), (key, ax)
            assert d[ax + "i"] <= desc[ax + "i"], (key, ax)
        shrunk += d != desc
    for key, desc, tail, tile in TC.chain_entries():
        d, t = TC.shrink_chain(desc, tail)
        for f in TC.KEPT:
            if d[f] != desc[f]:
                changed[(key, f)] = (desc[f], d[f])
        for f in set(TC.FIELDS) - {"N", "Ti", "Hi", "Wi", "To", "Ho", "Wo"}:
            if t[f] != tail[f]:
                changed[(key, "tail." + f)] = (tail[f], t[f])
        assert (t["N"], t["Ti"], t["Hi"], t["Wi"], t["To"], t["Ho"], t["Wo"]) == \
               (d["N"], d["To"], d["Ho"], d["Wo"], d["To"], d["Ho"], d["Wo"]) and t["Wo"] == tail["Wo"], key
    assert not changed, list(changed.items())[:5]
    assert shrunk >= 900                     # the shrinking is real: nearly every tuned problem is larger than its case


def test_splits(lib):
    for key, desc, tile, split in TC.conv_entries():
        assert split >= 1, key
        steps = TC.k_steps(desc, tile)
        assert split <= steps, "%s: split %d on %d k-steps of %s" % (key, split, steps, tile)
        # (a "/direct" tile runs at split 1 whatever the entry says: finalize_conv_args clamps it)
        for d in (desc, TC.shrink(desc)):
            assert (lib.ptx_conv3d_workspace_bytes(C.byref(TC.fill(d)), split) != 0) == (split > 1), key
    for key, (tile, n) in TC.split_kinds().get("chain", {}).items():
        assert n == 1, key
