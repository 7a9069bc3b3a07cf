"""Autotune and profiling, as functions of (engine, plan): every decision the tuned table (tuned.py) remembers is measured
here with HIP events on the plan's own buffers -- conv tiles and split-K, chained tiles, the body kernels against either,
chained launch vs its pair, Winograd launches vs the direct execution, conv program vs its launches, clip lanes -- and so are the per-launch times bench.py reports.
`Engine.autotune / _autotune / tune_lanes / profile_convs / profile_steps` delegate here.
"""
import ctypes as C
import json
import os
import time

import torch

from . import _lib
from ._lib import PtxError
from .steps import DwConvStep
from .steps import (AltStep, ChainStep, ConvStep, PatchConvStep, ProgramStep, StemBf16Step, StemF32Step, StemStep, StemTfirStep, _WinoExec, _dense16,
                    _r4, _stream, issued_conv_flop)
from .tuned import (BODY_SHAPES, _flags_kind, _tile_kind, alt_lookup, alt_store, body_lookup, body_store, chain_lookup,
                    chain_store, lanes_key, lanes_lookup, lanes_store, prog_lookup, prog_store, save_tuned_table, tuned_lookup,
                    tfir_lookup, tfir_store, tuned_store, wino4_lookup, wino4_store, wino_lookup, wino_store)


def _time_ms(run, iters):
    """HIP-event time of one `run()` on the current stream: one untimed launch first (warm-up, and validity: a launch the
    library refuses raises PtxError here, before anything is timed), then the mean over `iters` launches between two events."""
    run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def _launch(step):
    return lambda: step(_stream())


class _Session:
    """What the phases of one _autotune call share."""

    def __init__(self, plan, iters, verbose, only_untuned):
        self.lib, self.plan, self.iters, self.verbose, self.only_untuned = _lib.lib(), plan, iters, verbose, only_untuned
        self.log = open(os.environ["PTX_TUNE_LOG"], "w") if os.environ.get("PTX_TUNE_LOG") else None

    def note(self, log_line, line):
        if self.log is not None:
            self.log.write(log_line)
        if self.verbose and line is not None:
            print(line)


# ---------------------------------------------------------------------------------------------
# autotune
# ---------------------------------------------------------------------------------------------
def autotune(engine, model, x, iters=3, verbose=False, persist=False, only_untuned=False, plan=None):
    """Time every compiled tile configuration (x a few split-K factors) for each distinct conv
    problem of the plan with HIP events and keep the fastest.  Holds the plan's exclusive lock: the
    tuner relaunches convs into the plan's buffers."""
    own_plan = plan is not None
    if plan is None:
        engine._validate(model, x, model.arch.dims)
        with torch.cuda.device(x.device):
            plan = engine.plan_for(model, _dense16(x))
    with torch.cuda.device(x.device), plan.exclusive():
        plan = _autotune(engine, model, x, iters, verbose, persist, only_untuned, plan)
    # the clip-lanes verdict of this (architecture, shape), measured on the tuned tiles of both launch shapes -- only for
    # the engine's own full-batch plan and only when the knob is on "auto"
    if (engine._lanes == "auto" and not own_plan and not engine.use_graph and x.shape[0] >= 2 and x.shape[0] % 2 == 0
            and os.environ.get("PTX_TUNE_LANES", "1") != "0"
            and not (only_untuned and lanes_lookup(lanes_key(model, _dense16(x).shape, engine.precision_of(model))) is not None)):
        with torch.cuda.device(x.device):
            half = _dense16(_dense16(x)[:x.shape[0] // 2])
            hp = engine.plan_for(model, half)
            with hp.exclusive():
                _autotune(engine, model, half, iters, verbose, False, only_untuned, hp)
            tune_lanes(engine, model, x, verbose=verbose)
        if persist:
            save_tuned_table()
    return plan


def _autotune(engine, model, x, iters=3, verbose=False, persist=False, only_untuned=False, plan=None):
    # timed launches per candidate: 2 keeps a first-use tune under a second per network; tuning sessions that feed the
    # shipped table ask for more (PTX_TUNE_ITERS) -- many candidates differ by 1-2 %, the noise of a 2-launch average
    iters = max(iters, int(os.environ.get("PTX_TUNE_ITERS", "0")))
    with torch.cuda.device(x.device):
        if plan is None:
            plan = engine.plan_for(model, _dense16(x))
        plan.bind(model)
        plan.run_features(_dense16(x))      # make every buffer hold sane data
        t = _Session(plan, iters, verbose, only_untuned)
        _tune_conv_tiles(t)
        _tune_chain_tiles(t)
        _tune_chain_vs_pair(t)
        _tune_wino_vs_direct(t)
        _tune_stem_tfir(t)
        _tune_program_vs_launches(t)
        plan.run_features(_dense16(x))
        plan.tuned = True
        if t.log is not None:
            t.log.close()
    if persist:
        save_tuned_table()
    return plan


def admissible(name, d, kind, M, ncol, stem_macs=None):
    """(BM, BN, BK) of tile configuration `name` when the sweep times it for conv problem `d` (operand flavour `kind`, M
    output rows, `ncol` columns written), else None.  stem_macs: the algorithmic MACs of the bf16 stem, for that step only."""
    if _tile_kind(name) != kind:
        return None                          # fp16-operand / split-operand problems <-> their own tiles
    bm, bn_, bk = [int(v) for v in name.split("/")[0].split("x")]
    narrow = bn_ <= 32 and bk == 32 and bm >= 128 and not name.endswith("/dma")   # Mx16 / Mx32 tiles
    if (bk == 24) != (d.Kc == 24) and not (d.Kc == 24 and narrow):
        return None                          # BK = 24 tiles are for the kW-folded stem only
    if narrow and ncol > 32 and d.groups <= 1:
        return None
    if bk == 64 and d.Kc % 64 and kind != "x3":     # BK = 64 tiles: long, 64-aligned K only
        return None
    if name.endswith("/direct") and ncol > 32 and d.groups <= 1:   # VALU kernels: narrow outputs
        return None
    if d.groups > 1 and not name.endswith("/direct") and (d.Co // d.groups) % bn_:
        return None                          # grouped: direct tiles, or MFMA tiles inside one group
    if bn_ > 64 and ncol <= 64:
        return None
    if bn_ < 32 and ncol > 32 and name.endswith("/f16"):
        return None
    if bn_ % 48 == 0 and ncol % 48 != 0:          # 48/96-wide tiles: (2+1)D widths only
        return None
    if bm >= 128 and M < 8192:
        return None
    if stem_macs is not None and issued_conv_flop(d, (bm, bn_, bk), 2) > 3.2 * stem_macs:
        return None                          # the bf16 stem issues at most 1.6x its algorithmic MACs
    return bm, bn_, bk


def _sweep_body(t, stp, key, best_ms, kernel, tag, rival):
    """The body kernel's shapes against the best tile (`best_ms`) of the same conv / chained pair: same 2 % bar an incumbent
    defends itself with.  Stores the "body:" verdict and leaves it in stp.body; False when there was nothing to measure."""
    if not stp.body_ok or os.environ.get("PTX_CONV_BODY", "1") in ("0",) + BODY_SHAPES:
        return False
    t_best, pick, n = best_ms, -1, max(t.iters, 3)
    for sh in stp.body_ok:
        stp.body = sh
        ms = _time_ms(_launch(stp), n)
        tf = 2e-9 * stp.macs / ms
        t.note("%s\t%s/%s\t%.4f ms\t%.1f TF\n" % (stp.label, kernel, BODY_SHAPES[sh], ms, tf),
               "tune %-34s %s/%-6s %.4f ms  %.1f TF  (best %s %.4f ms)" % (stp.label, tag, BODY_SHAPES[sh], ms, tf, rival, best_ms))
        if ms < 0.98 * t_best:
            t_best, pick = ms, sh
    stp.body = pick if pick >= 0 else None
    body_store(key, pick)
    return True


def _tune_conv_tiles(t):
    """Phase 1: every distinct conv problem of the plan over the tile table x a few split-K factors, then the body kernel."""
    seen, seen_body = {}, {}
    for stp in t.plan.conv_steps:
        key = json.dumps(stp.d.key())
        if key in seen:
            stp.cfg, stp.split = seen[key]
            if key in seen_body:
                stp.body = seen_body[key]
            continue
        kind = _flags_kind(stp.d.flags)
        if t.only_untuned and tuned_lookup(key, kind) is not None and (not stp.body_ok or body_lookup(key) is not None):
            continue
        best = _best_conv_tile(t, stp, key, kind)
        stp.cfg, stp.split = best[1], best[2]
        if _sweep_body(t, stp, key, best[0], "conv_body_f32", "body", "tile"):
            seen_body[key] = stp.body
        seen[key] = (best[1], best[2])
        tuned_store(key, best[1], best[2])
        if t.verbose:
            print("tune %-34s M=%-8d N=%-5d K=%-6d -> %-20s split=%d  %.3f ms  %.1f TF" % (
                stp.label, stp.d.N * stp.d.To * stp.d.Ho * stp.d.Wo, stp.d.Co, stp.d.Kc * stp.d.kT * stp.d.kH * stp.d.kW,
                t.lib.ptx_conv3d_config_name(best[1]).decode(), best[2], best[0], 2e-9 * stp.macs / best[0]))


def _best_conv_tile(t, stp, key, kind, split_k=True):
    """(ms, tile index, split-K) of the fastest admissible tile for one conv step (ms NaN and the library's default when
    nothing admissible could be timed).  split_k=False: split 1 only (the grouped conv of a Winograd step)."""
    lib, d, best = t.lib, stp.d, None
    # PTX_TUNE_CANDIDATES="dma4/re,dma3/re": a targeted session -- only tiles whose name holds one of the
    # substrings are timed, next to the table's incumbent, which keeps its place unless beaten by 2 %
    cands = [c for c in os.environ.get("PTX_TUNE_CANDIDATES", "").split(",") if c]
    inc = tuned_lookup(key, kind) if cands else None
    inc_ms = None
    if inc is not None:
        # the incumbent is timed EXPLICITLY, up front: its split need not be among the splits the sweep below
        # tries for that tile, and without its time the 2 % rule would be skipped silently
        keep_cfg = (stp.cfg, stp.split, stp.from_table)
        stp.cfg, stp.split, stp.from_table = inc[0], inc[1], False
        try:
            inc_ms = _time_ms(_launch(stp), t.iters)
        except PtxError:
            inc = None                       # a stale entry this build refuses: nothing to defend
        stp.cfg, stp.split, stp.from_table = keep_cfg
    stp.body = None                  # the tile sweep times the implicit-GEMM path
    steps_k = d.kT * d.kH * d.kW * ((d.Kc + 31) // 32)
    M = d.N * d.To * d.Ho * d.Wo
    ncol = _r4(d.Co)                              # columns written (ldy is only the row stride)
    for cfg in range(lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16()):
        name = lib.ptx_conv3d_config_name(cfg).decode()
        if cands and not (any(c in name for c in cands) or (inc is not None and cfg == inc[0])):
            continue
        tile = admissible(name, d, kind, M, ncol, stp.macs if stp is t.plan.stem_bf16_step else None)
        if tile is None or not lib.ptx_conv3d_config_supported(C.byref(d), cfg):
            continue                         # (a tile the plan compiler would drop again; a "/ws" tile outside its rule)
        blocks =((M + tile[0] - 1) // tile[0]) * ((ncol + tile[1] - 1) // tile[1])
        splits = [1]
        if blocks < 512 and split_k and not name.endswith("/ws"):      # (a persistent tile has no split-K form)
            splits += [s for s in (2, 3, 4, 6, 8) if steps_k // s >= 4 and blocks * s <= 2048]
        for sk in splits:
            if sk > 1 and lib.ptx_conv3d_workspace_bytes(C.byref(d), sk) > t.plan.ws_bytes:
                continue
            stp.cfg, stp.split, stp.from_table = cfg, sk, False     # a refusal must surface here, not fall back
            try:
                ms = _time_ms(_launch(stp), t.iters)
            except PtxError:
                continue
            t.note("%s\tM=%d\tN=%d\tK=%d\t%s\tsplit=%d\t%.4f ms\t%.1f TF\n" % (
                stp.label, M, d.Co, d.Kc * d.kT * d.kH * d.kW, name, sk, ms, 2e-9 * stp.macs / ms), None)
            if best is None or ms < best[0]:
                best = (ms, cfg, sk)
            if inc is not None and (cfg, sk) == tuple(inc):
                inc_ms = ms
    if inc_ms is not None and best is not None and best[1] != inc[0] and best[0] > 0.98 * inc_ms:
        best = (inc_ms, inc[0], inc[1])
    if best is None:                 # nothing admissible was timed: keep the heuristic default
        sk = C.c_int(1)
        best = (float("nan"), lib.ptx_conv3d_pick_config(C.byref(d), C.byref(sk)), sk.value)
    return best


def _tune_chain_tiles(t):
    """Phase 2, chained launches: time every chained tile that holds the intermediate row, then the body kernel's chained
    form against the best of them."""
    lib, seen, seen_body = t.lib, {}, {}
    for stp in t.plan.chain_steps:
        if stp.key in seen:
            stp.cfg = seen[stp.key]
            if stp.key in seen_body:
                stp.body = seen_body[stp.key]
            continue
        if t.only_untuned and chain_lookup(stp.key) is not None and (not stp.body_ok or body_lookup(stp.key) is not None):
            continue
        best = None
        stp.body = None                  # the chained-tile sweep times the implicit-GEMM chain
        for cfg in range(lib.ptx_conv3d_chain_num_configs()):
            if not lib.ptx_conv3d_chain_supported(C.byref(stp.d), C.byref(stp.d2), cfg):
                continue
            keep, stp.cfg = stp.cfg, cfg
            try:
                ms = _time_ms(_launch(stp), t.iters)
            except PtxError:
                continue
            finally:
                stp.cfg = keep
            t.note("%s\t%s\t%.4f ms\t%.1f TF\n" % (stp.label, lib.ptx_conv3d_chain_config_name(cfg).decode(), ms,
                                                   2e-9 * stp.macs / ms), None)
            if best is None or ms < best[0]:
                best = (ms, cfg)
        if best is None:
            continue
        stp.cfg = best[1]
        if _sweep_body(t, stp, stp.key, best[0], "conv_body_chain_f32", "body-chain", "chained tile"):
            seen_body[stp.key] = stp.body
        seen[stp.key] = best[1]
        chain_store(stp.key, best[1])
        if t.verbose:
            print("tune %-34s -> %-28s %.3f ms  %.1f TF" % (stp.label, lib.ptx_conv3d_chain_config_name(best[1]).decode(),
                                                           best[0], 2e-9 * stp.macs / best[0]))


def _tune_chain_vs_pair(t):
    """Phase 3, chained launch vs the two launches it replaces: time both executions of every pair, keep the faster."""
    force = os.environ.get("PTX_CHAIN_FORCE")
    seen = {}
    for a in t.plan.alt_steps:
        if a.key in seen:
            a.use_chain = seen[a.key]
            continue
        if force in ("0", "1") or (t.only_untuned and alt_lookup(a.key) is not None):
            continue
        n = max(t.iters, 3)
        ms2 = [_time_ms(_launch(a.chain), n), _time_ms(lambda: [s_(_stream()) for s_ in a.pair], n)]
        # the chained launch has to win by a margin: timed alone in a loop it looks ~2 % better than inside the
        # forward (measured: config 2 x3, layer2 tails -- chosen at parity by the tuner, 1.2 % slower in the step)
        a.use_chain = ms2[0] < 0.97 * ms2[1]
        seen[a.key] = a.use_chain
        alt_store(a.key, a.use_chain)
        verdict = "chain" if a.use_chain else "pair"
        t.note("%s\tchain %.4f ms\tpair %.4f ms\t-> %s\n" % (a.label, ms2[0], ms2[1], verdict),
               "tune %-34s chain %.4f ms | pair %.4f ms -> %s" % (a.label, ms2[0], ms2[1], verdict))


def _tune_wino_vs_direct(t):
    """Phase 4, the Winograd forms vs the direct execution of every distinct eligible stride-1 (kT,3,3) problem.  First
    F(2x2,3x3): tune the grouped conv's tile like any conv (split 1), then time the three launches against the best direct
    execution the earlier phases left in place -- the tile or body kernel, or, where the conv opens a bottleneck tail, the
    chain-or-pair verdict with the tail's conv3 on both sides -- under the same 3 % margin as _tune_chain_vs_pair.  Then
    F(4x4,3x3) the same way (the 36-group conv's tile, the three launches) against the best execution so far, direct or
    F(2x2), under the same margin."""
    if os.environ.get("PTX_CONV_WINO", "auto") in ("0", "1", "4"):
        return
    plan, seen, seen4 = t.plan, {}, {}
    steps = plan.wino_steps + [w for w in plan.wino4_steps if w.wino is None]
    for w in steps:
        a = w.alt
        if a is not None and os.environ.get("PTX_CHAIN_FORCE") == "1":
            continue                         # the chained launch is pinned: nothing to decide for the pair's first conv
        run = _launch(a if a is not None else w)
        n = max(t.iters, 3)

        def time_form(four, g):
            """ms of the step with the F(2x2) / F(4x4) launches selected, after sweeping the grouped conv's tile."""
            gkey = json.dumps(g.d.key())
            if not (t.only_untuned and tuned_lookup(gkey, "") is not None):
                best = _best_conv_tile(t, g, gkey, "", split_k=False)
                g.cfg, g.split, g.from_table = best[1], 1, False
                tuned_store(gkey, best[1], 1)
            w.use_wino, w.use_wino4 = not four, four
            if a is not None:
                a.use_chain = False
            return _time_ms(run, n)

        # ---- F(2x2) against the direct execution
        ms_best, best_name, keep_chain = None, "direct", a.use_chain if a is not None else False
        if w.wino is not None:
            g = w.gemm
            if w.key in seen:
                w.use_wino, g.cfg = seen[w.key]
            elif not (t.only_untuned and wino_lookup(w.key) is not None):
                w.use_wino = w.use_wino4 = False
                ms_direct = _time_ms(run, n)
                ms_wino = time_form(False, g)
                w.use_wino = ms_wino < 0.97 * ms_direct
                ms_best, best_name = (ms_wino, "wino") if w.use_wino else (ms_direct, "direct")
                seen[w.key] = (w.use_wino, g.cfg)
                wino_store(w.key, w.use_wino, g.cfg)
                tile = t.lib.ptx_conv3d_config_name(g.cfg).decode()
                t.note("%s\tdirect %.4f ms\twino %.4f ms (%s)\t-> %s\n" % (w.label, ms_direct, ms_wino, tile, best_name),
                       "tune %-34s direct %.4f ms | wino %.4f ms (%s) -> %s" % (w.label, ms_direct, ms_wino, tile, best_name))
        # ---- F(4x4) against the best of the two
        if w.wino4 is not None:
            g4 = w.gemm4
            if w.key in seen4:
                w.use_wino4, g4.cfg = seen4[w.key]
                if w.use_wino4:
                    plan.wino4_weights(w, now=True)
            elif not (t.only_untuned and wino4_lookup(w.key) is not None):
                keep2 = w.use_wino
                if ms_best is None:          # the F(2x2) verdict came from the table / there is no F(2x2) form: time what runs now
                    w.use_wino4 = False
                    if a is not None and not w.use_wino:
                        a.use_chain = keep_chain
                    ms_best, best_name = _time_ms(run, n), "wino" if w.use_wino else "direct"
                plan.wino4_weights(w, now=True)
                ms_wino4 = time_form(True, g4)
                w.use_wino4 = ms_wino4 < 0.97 * ms_best
                w.use_wino = keep2 and not w.use_wino4
                seen4[w.key] = (w.use_wino4, g4.cfg)
                wino4_store(w.key, w.use_wino4, g4.cfg)
                verdict, tile = "wino4" if w.use_wino4 else best_name, t.lib.ptx_conv3d_config_name(g4.cfg).decode()
                t.note("%s\t%s %.4f ms\twino4 %.4f ms (%s)\t-> %s\n" % (w.label, best_name, ms_best, ms_wino4, tile, verdict),
                       "tune %-34s %s %.4f ms | wino4 %.4f ms (%s) -> %s" % (w.label, best_name, ms_best, ms_wino4, tile, verdict))
        if w.use_wino4:
            w.use_wino = False
        if a is not None:
            a.use_chain = False if (w.use_wino or w.use_wino4) else keep_chain


def _tune_stem_tfir(t):
    """Phase 4b, the fp32 stem's temporal fast-FIR schemes vs its direct launch: time the direct kernel and the two launches of
    every compiled scheme on the plan's own buffers, keep the fastest scheme if it beats direct by the 3 % margin of the
    Winograd phases, else direct."""
    if os.environ.get("PTX_STEM_TFIR", "auto") != "auto":
        return
    for st in t.plan.stem_tfir_steps:
        if t.only_untuned and tfir_lookup(st.key) is not None:
            continue
        run, n = _launch(st), max(t.iters, 5)
        st.use_tfir = 0
        ms_direct = _time_ms(run, n)
        best, ms_best, parts = 0, ms_direct, []
        for sid in sorted(st.tfir):
            st.use_tfir = sid
            ms = _time_ms(run, n)
            parts.append("fir%d %.4f ms" % (sid, ms))
            if ms < 0.97 * ms_direct and ms < ms_best:
                best, ms_best = sid, ms
        st.use_tfir = best
        tfir_store(st.key, best)
        verdict = "fir%d" % best if best else "direct"
        t.note("%s\tdirect %.4f ms\t%s\t-> %s\n" % (st.label, ms_direct, "\t".join(parts), verdict),
               "tune %-34s direct %.4f ms | %s -> %s" % (st.label, ms_direct, " | ".join(parts), verdict))


def _tune_program_vs_launches(t):
    """Phase 5, conv program vs the launches it replaces (PTX_PROGRAM=auto only): time both executions of every run, keep
    the faster (same margin rule); a program that loses is dissolved into its launches."""
    plan = t.plan
    if os.environ.get("PTX_PROGRAM", "0") != "auto":
        return

    def dissolve(ps):        # the launches it stood for take its place; its workspace and image are freed
        i = plan.steps.index(ps)
        plan.steps[i:i + 1] = ps.convs
        plan.program_steps.remove(ps)

    for ps in list(plan.program_steps):
        known = prog_lookup(ps.key)
        if t.only_untuned and known is not None:      # an identical run of convs was measured a moment ago: same verdict
            ps.use_program = known
            if not known:
                dissolve(ps)
            continue
        ms2 = []
        for flag in (True, False):
            ps.use_program = flag
            ms2.append(_time_ms(_launch(ps), max(t.iters, 5)))
        ps.use_program = ms2[0] < 0.97 * ms2[1]
        if ps.error() is not None:
            ps.use_program = False
        prog_store(ps.key, ps.use_program)
        if not ps.use_program:
            dissolve(ps)
        verdict = "program" if ps.use_program else "launches"
        t.note("%s\tprogram %.4f ms\tlaunches %.4f ms\t-> %s\n" % (ps.label, ms2[0], ms2[1], verdict),
               "tune %-44s program %.4f ms | %d launches %.4f ms -> %s" % (ps.label, ms2[0], len(ps.convs), ms2[1], verdict))


def tune_lanes(engine, model, x, iters=8, verbose=False):
    """Measure forward(model, x) with one and with two clip lanes (each on its own tuned plans) and record the verdict in
    the tuned table: two lanes must win by 1 % (the lanes double the activation buffers; config 2 gains 1.4-2.2 % across the
    boxes of rounds 5 and 6, which a 1.5 % bar turned into a coin flip).  Returns the lanes kept."""
    x = _dense16(x)
    key = lanes_key(model, x.shape, engine.precision_of(model))
    if engine.use_graph or x.shape[0] < 2 or x.shape[0] % 2:
        return 1
    keep = engine._lanes
    ms = {1: [], 2: []}
    try:
        for n in (1, 2):                     # plans compiled, tiles tuned, clocks up
            engine._lanes = n
            for _ in range(3):
                engine.forward(model, x)
        # interleaved rounds (1, 2, 1, 2, ...): clock / thermal drift hits both arms alike; the verdict is the MEDIAN round
        for _ in range(5):
            for n in (1, 2):
                engine._lanes = n
                torch.cuda.synchronize(x.device)
                t0 = time.perf_counter()
                for _ in range(iters):
                    engine.forward(model, x)
                torch.cuda.synchronize(x.device)
                ms[n].append(1e3 * (time.perf_counter() - t0) / iters)
    finally:
        engine._lanes = keep
    ms = {n: sorted(v)[len(v) // 2] for n, v in ms.items()}
    best = 2 if ms[2] < 0.99 * ms[1] else 1
    lanes_store(key, best)
    if verbose:
        print("tune clip lanes %s: 1 lane %.3f ms | 2 lanes %.3f ms -> %d" % (key, ms[1], ms[2], best))
    return best


# ---------------------------------------------------------------------------------------------
# profiling
# ---------------------------------------------------------------------------------------------
def profile_convs(engine, model, x, iters=5, plan=None):
    """Per-conv-launch timing with HIP events on the current stream: the launches the forward RUNS (`plan.all_convs()`:
    the active side of every chain-or-pair decision, chained launches and direct stems included), as rows of
    (label, MACs, ms, tile / kernel name, split-K).  `plan`: an already compiled (and run) plan, for models whose input
    is not one NCDHW tensor."""
    with torch.cuda.device(x.device):
        if plan is None:
            engine._validate(model, x, model.arch.dims)
            plan = engine.plan_for(model, _dense16(x))
            plan.bind(model)
            plan.run_features(_dense16(x))
        live = set(id(s) for s in plan.all_convs())
        rows = []
        for r in engine.profile_steps(plan, iters):
            if r[1] in ("conv", "stem", "chain"):
                rows.append((r[0], r[3], r[4], r[5], r[6].split if r[1] == "conv" else 1))
        if len(rows) != len(live):
            raise PtxError("profile_convs: %d timed launches for %d live conv steps" % (len(rows), len(live)))
    return rows


def profile_steps(engine, plan, iters=5, isolated=None):
    """HIP-event time of EVERY launch of a compiled (and run) plan on the current stream, convs and HBM-bound
    passes alike: rows of (label, kind, algorithmic bytes, MACs, ms, tile / kernel name).  kind is "conv" for the
    implicit-GEMM launches, "stem" for the direct stem kernels, "mem" for tagged HBM passes, "mfma" for the fused attention, "other" for the rest.

    Method (round 6).  The launches are timed INSIDE ordinary passes over the plan -- the caches and the clock / power
    state of a forward -- by a CHAIN of events, one after every launch: interval i = event i -> event i + 1, so the
    intervals of a pass sum to that pass by construction.  An event between two launches costs the stream a marker
    packet, so an instrumented pass is longer than a plain one; the same call therefore also times `iters` PLAIN passes
    (two events around all of them) and removes the difference as a constant per launch:
        overhead = (instrumented pass - plain pass) / launches,   ms_i = interval_i - overhead
    so that sum(ms_i) == the plain pass (rows are rescaled by a common factor if a clamp at 25 % of the raw interval
    was hit).  `engine.last_profile` keeps the calibration: {"plain_pass_ms", "instrumented_pass_ms", "launches",
    "overhead_us_per_launch", "raw_sum_ms", "clamped"}.  Round 5 bracketed each launch with its OWN pair of events and
    reported the raw brackets: they summed to 5.76 ms in a 5.39 ms step.

    `isolated=True` (or PTX_PROFILE_ISOLATED=1) is the round-1..4 method, every launch repeated `iters` times back to back
    on its own: it over-states the MFMA-bound launches by 5-19 % (five identical matrix-bound launches in a row pull
    the clock down)."""
    if isolated is None:
        isolated = os.environ.get("PTX_PROFILE_ISOLATED", "0") == "1"
    st = _stream()
    flat = [t for s in plan.steps for t in (s.active() if isinstance(s, (AltStep, ProgramStep, _WinoExec, StemF32Step)) else [s])]
    engine.last_profile = None
    if isolated:
        ms_of = [_time_ms(lambda stp=stp: stp(st), iters) for stp in flat]
    else:
        ms_of, engine.last_profile = _event_chain_ms(flat, st, iters)
    rows = []
    for stp, ms in zip(flat, ms_of):
        if isinstance(stp, ConvStep) and stp.body is not None:       # a direct kernel, like the stems
            rows.append((stp.label, "stem", 0, stp.macs, ms, stp.kernel))
        elif isinstance(stp, ConvStep):
            rows.append((stp.label, "conv", 0, stp.macs, ms, _lib.lib().ptx_conv3d_config_name(stp.cfg).decode(), stp))
        elif isinstance(stp, (StemStep, StemF32Step, StemTfirStep, StemBf16Step, PatchConvStep)):      # direct (patch) kernels are convs too
            rows.append((stp.label, "stem", 0, stp.macs, ms, stp.kernel))
        elif isinstance(stp, (ChainStep, ProgramStep)):     # several convs in one launch, their own tile tables
            rows.append((stp.label, "chain", 0, stp.macs, ms, stp.kernel))
        else:                                               # a tagged closure (steps._tag), or a caller's own callable
            nb, macs = getattr(stp, "hbm_bytes", 0), getattr(stp, "macs", 0)
            kind = "mem" if nb and (not macs or isinstance(stp, DwConvStep)) else "mfma" if macs else "other"       # (depthwise: streaming)
            rows.append((getattr(stp, "label", getattr(stp, "__name__", "step")), kind, nb, macs, ms, ""))
    return rows


def _event_chain_ms(flat, st, iters):
    """The event-chain method of profile_steps: (per-launch ms, calibration record)."""
    n = len(flat)
    # untimed passes first: every launch has run in this order and the clocks are back up -- the caller may have left
    # the GPU idle for seconds (bench.py's CPU leg), and the first tens of milliseconds after an idle period run at a
    # lower clock (measured: a pass 1.9 % slower than the timed steps of the same plan when only two passes preceded it)
    t_warm = time.perf_counter()
    for k in range(64):
        for stp in flat:
            stp(st)
        if k >= 3 and (k & 3) == 3:
            torch.cuda.synchronize()
            if time.perf_counter() - t_warm > 0.25:
                break
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(n + 1)] for _ in range(iters)]
    pa, pb = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    pc, pd = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def plain(e0, e1, k):
        e0.record()
        for _ in range(k):
            for stp in flat:
                stp(st)
        e1.record()
    half = max(1, iters // 2)
    plain(pa, pb, half)                 # plain passes on BOTH sides of the instrumented ones (clock drift)
    for it in range(iters):
        ev[it][0].record()
        for i, stp in enumerate(flat):
            stp(st)
            ev[it][i + 1].record()
    plain(pc, pd, half)
    torch.cuda.synchronize()
    plain_ms = (pa.elapsed_time(pb) + pc.elapsed_time(pd)) / (2 * half)
    raw = [sum(ev[it][i].elapsed_time(ev[it][i + 1]) for it in range(iters)) / iters for i in range(n)]
    inst_ms = sum(ev[it][0].elapsed_time(ev[it][n]) for it in range(iters)) / iters
    over = max(0.0, (inst_ms - plain_ms) / max(n, 1))
    ms_of = [max(r - over, 0.25 * r) for r in raw]
    clamped = sum(1 for r in raw if r - over < 0.25 * r)
    tot = sum(ms_of)
    if tot > 0 and (clamped or inst_ms < plain_ms):
        ms_of = [m * plain_ms / tot for m in ms_of]
    return ms_of, {"method": "event chain inside ordinary passes, constant per-launch marker overhead removed",
                   "iters": iters, "launches": n, "plain_pass_ms": plain_ms, "instrumented_pass_ms": inst_ms,
                   "raw_sum_ms": sum(raw), "overhead_us_per_launch": 1e3 * over, "clamped": clamped}
