"""No-GPU tests of the fp32 stem as a fast FIR along time (include/ptx_amd_tfir.h, csrc/conv_stem_tfir_f32.hip): the scheme
tables, the `supported` rule and its refusals, the sizes, header / bindings / exports, and the plan compiler's step on dry plans."""
import ctypes as C
import re

import numpy as np

SCHEMES = {1: (2, 8), 2: (4, 13), 3: (4, 10)}       # id -> (m, P)
KT = 7


def _tables(lib, sid):
    m, P = C.c_int32(), C.c_int32()
    assert lib.ptx_stem_tfir_scheme(sid, C.byref(m), C.byref(P), None, None, None) == 0
    m, P = m.value, P.value
    at, g, bt = (C.c_float * (m * P))(), (C.c_float * (P * KT))(), (C.c_float * (P * (m + KT - 1)))()
    assert lib.ptx_stem_tfir_scheme(sid, None, None, at, g, bt) == 0
    f = lambda a, r, c: np.array(list(a), dtype=np.float32).reshape(r, c).astype(np.float64)
    return m, P, f(at, m, P), f(g, P, KT), f(bt, P, m + KT - 1)


def _stem_desc(L, N=8, T=16, H=224, W=224, Co=64, s=2):
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, 3, 0
    d.To, d.Ho, d.Wo, d.Co, d.ldy = T, (H + 6 - 7) // s + 1, (W + 6 - 7) // s + 1, Co, (Co + 3) // 4 * 4
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = 7, 7, 7, 1, s, s, 3, 3, 3
    d.Kc, d.Co_pad, d.flags = 24, (Co + 127) // 128 * 128, L.PTX_EPI_RELU
    return d, (3 * T * H * W, T * H * W, H * W)


def test_scheme_tables_are_exact_bilinear_forms(ptx):
    """sum_j AT[o][j] G[j][k] BT[j][i] == [i == o + k] to 1e-6 in float64 from the fp32 tables, m and P as documented, the
    entries the fp32 roundings of small rationals, and the committed tables are what scripts/gen_tfir_tables.py derives."""
    import importlib.util
    import os
    lib = ptx._lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_tfir_tables", os.path.join(root, "scripts", "gen_tfir_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for sid, (m_want, P_want) in SCHEMES.items():
        m, P, at, g, bt = _tables(lib, sid)
        assert (m, P) == (m_want, P_want)
        got = np.einsum("oj,jk,ji->oki", at, g, bt)
        want = np.zeros_like(got)
        for o in range(m):
            for k in range(KT):
                want[o, k, o + k] = 1.0
        assert np.abs(got - want).max() <= 1e-6, (sid, np.abs(got - want).max())
        gm, gP, gat, gg, gbt = gen.scheme(sid)
        assert (gm, gP) == (m, P)
        for mine, theirs in ((at, gat), (g, gg), (bt, gbt)):
            exact = np.array([[np.float32(np.float32(v.numerator) / np.float32(v.denominator)) for v in row] for row in theirs])
            assert np.array_equal(mine.astype(np.float32), exact), sid
    # products per 16 output frames: 64 / 52 / 40 against the direct kernel's 100
    assert [-(-16 // m) * P for m, P in SCHEMES.values()] == [64, 52, 40]
    assert lib.ptx_stem_tfir_scheme(0, None, None, None, None, None) == 2 and lib.ptx_stem_tfir_scheme(4, None, None, None, None, None) == 2


def test_supported_rule_sizes_and_refusals(ptx):
    """The direct stem's rule plus sT == 1, kT == 7, a scheme 1..3, V and every operand below 2 GiB; the sizes."""
    L = ptx._lib
    lib = L.lib()
    d, st = _stem_desc(L)
    for sid, (m, P) in SCHEMES.items():
        assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(d), *st, sid) == 1
        groups = -(-16 // m)
        assert lib.ptx_stem_tfir_f32_workspace_bytes(C.byref(d), sid) == 4 * 8 * 3 * groups * P * 224 * 224
        assert lib.ptx_stem_tfir_f32_weight_elems(C.byref(d), sid) == P * 7 * 2 * 11 * 2 * 64
        assert lib.ptx_stem_tfir_f32_weight_elems(C.byref(d), sid) * 7 == lib.ptx_stem_f32_weight_elems(C.byref(d)) * P
    assert lib.ptx_stem_tfir_f32_workspace_bytes(C.byref(d), 2) == 250 * 1000 * 1000 + 478592       # config 2: V = 250 MB
    for bad in (0, 4, -1):
        assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(d), *st, bad) == 0
        assert lib.ptx_stem_tfir_f32_workspace_bytes(C.byref(d), bad) == 0 and lib.ptx_stem_tfir_f32_weight_elems(C.byref(d), bad) == 0
    # a width with a padded pitch: V rows keep the pitch; To % m != 0: a last partial group
    dp, stp = _stem_desc(L, N=1, T=5, H=18, W=22, Co=40, s=1)
    dp.ldx = 24
    stp = (3 * 5 * 18 * 24, 5 * 18 * 24, 18 * 24)
    assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(dp), *stp, 2) == 1
    assert lib.ptx_stem_tfir_f32_workspace_bytes(C.byref(dp), 2) == 4 * 3 * 2 * 13 * 18 * 24
    assert lib.ptx_stem_tfir_f32_workspace_bytes(C.byref(dp), 1) == 4 * 3 * 3 * 8 * 18 * 24
    # refusals: what the direct kernel refuses ...
    assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(d), st[0], st[1], st[2] + 2, 2) == 0       # frame stride not 16-byte
    # ... a frame-strided view is a stride, as there
    d2, _ = _stem_desc(L, T=8)
    assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(d2), 3 * 16 * 224 * 224, 16 * 224 * 224, 2 * 224 * 224, 2) == 1
    # I3D's stride-2 stem, the (1,7,7) stems, a 5-tap filter, a residual epilogue
    for edit in (dict(sT=2, To=8), dict(kT=1, pT=0), dict(kT=5, pT=2), dict(flags=L.PTX_EPI_RELU | L.PTX_EPI_RES_ADD)):
        de, _ = _stem_desc(L)
        for k, v in edit.items():
            setattr(de, k, v)
        assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(de), *st, 2) == 0, edit
        null = C.c_void_p(0)
        buf = (C.c_float * 16)()
        p = C.cast(buf, C.c_void_p)
        assert lib.ptx_stem_tfir_in_f32(C.byref(de), 2, p, *st, p, null) == 2
        assert lib.ptx_conv_stem_tfir_f32_fwd(C.byref(de), 2, p, p, p, p, null) == 2
    # V at or above 2 GiB while x and y stay below it (8 clips of 128 frames, 8 output channels): scheme 1's V is 4x the clip
    # (2.47 GB, refused), scheme 3's 2.5x (1.54 GB, taken)
    big, stb = _stem_desc(L, T=128, Co=8)
    assert lib.ptx_conv_stem_f32_supported(C.byref(big), *stb) == 1
    assert lib.ptx_stem_tfir_f32_workspace_bytes(C.byref(big), 1) >= 2 ** 31 > lib.ptx_stem_tfir_f32_workspace_bytes(C.byref(big), 3)
    assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(big), *stb, 1) == 0
    assert lib.ptx_conv_stem_tfir_f32_supported(C.byref(big), *stb, 3) == 1
    # null / misaligned pointers are PTX_ERR_INVALID
    assert lib.ptx_conv_stem_tfir_f32_fwd(C.byref(d), 2, None, None, None, None, None) == 1
    assert lib.ptx_stem_tfir_in_f32(C.byref(d), 2, C.c_void_p(8), *st, C.c_void_p(16), None) == 1


def test_header_bindings_and_exports_agree(ptx):
    """The seven calls live in include/ptx_amd_tfir.h: that header, _lib.SIGNATURES_TFIR and the library's exports name the same
    functions, and ptx_amd.h's own census is untouched."""
    L = ptx._lib
    text = open(L.TFIR_HEADER_PATH).read()
    declared = L.header_symbols(L.TFIR_HEADER_PATH)
    assert declared == sorted(L.SIGNATURES_TFIR) and len(declared) == 7
    assert not set(declared) & set(L.SIGNATURES) and not set(declared) & set(L.header_symbols()) and not set(declared) & set(L.SIGNATURES_WINO4)
    assert '#include "ptx_amd.h"' in text
    lib = L.lib()
    for name in declared:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (L.SIGNATURES_TFIR[name][0], list(L.SIGNATURES_TFIR[name][1]))
        # the header's parameter count is the binding's
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
        assert len(decl.split(",")) == len(L.SIGNATURES_TFIR[name][1]), name
    integ = open(L.HEADER_PATH.replace("include/ptx_amd.h", "INTEGRATION.md")).read()
    assert "ptx_amd_tfir.h" in integ and all(n in integ for n in declared)


def test_dry_plan_default_unchanged_and_verdict_switches(ptx, monkeypatch):
    """Config 2 on a dry plan: without a verdict the stem is the direct launch (the plan's launches are what they were); a stored
    "tfir:" verdict switches it to [input transform, forward]; PTX_STEM_TFIR=0 compiles no form, =3 forces scheme 3; stems the
    library refuses ((1,7,7) stems, I3D's stride-2 stem) carry none; decoded uint8 frames share the clip's forms and key."""
    import torch
    from pretorched_x_amd import tuned
    from pretorched_x_amd.steps import StemF32Step, StemTfirStep, TFIR_SCHEMES
    monkeypatch.delenv("PTX_STEM_TFIR", raising=False)
    keep = tuned.tuned_snapshot()
    try:
        assert not any(k.startswith("tfir:") for k in keep)        # the shipped table carries no verdict: measured at run time
        m = ptx.resnet3d50(num_classes=339, pretrained=None)
        shape = (8, 3, 16, 224, 224)
        plan = m.engine().dry_plan(m, shape)
        st = plan.steps[0]
        assert isinstance(st, StemF32Step) and plan.stem_tfir_steps == [st] and st.use_tfir == 0 and st.active() == [st]
        assert sorted(st.tfir) == list(TFIR_SCHEMES) == [1, 2] and tuned.tfir_lookup(st.key) is None
        n_convs, macs = len(plan.all_convs()), sum(s.macs for s in plan.all_convs())
        monkeypatch.setenv("PTX_STEM_TFIR", "0")
        plan0 = m.engine().dry_plan(m, shape)
        assert plan0.steps[0].tfir is None and plan0.stem_tfir_steps == [] and len(plan0.steps) == len(plan.steps)
        assert [type(s).__name__ for s in plan0.steps] == [type(s).__name__ for s in plan.steps]
        assert plan.wino_bytes >= plan0.wino_bytes and plan.wino_bytes >= 4 * 8 * 3 * 8 * 8 * 224 * 224
        monkeypatch.delenv("PTX_STEM_TFIR")
        for sid, (mm, P) in ((2, (4, 13)), (1, (2, 8))):
            tuned.tfir_store(st.key, sid)
            assert tuned.tfir_lookup(st.key) == sid
            plan2 = m.engine().dry_plan(m, shape)
            s2 = plan2.steps[0]
            assert isinstance(s2, StemF32Step) and s2.use_tfir == sid and len(plan2.steps) == len(plan.steps)
            pre, fwd = s2.active()
            assert isinstance(fwd, StemTfirStep) and (fwd.scheme, fwd.m, fwd.P) == (sid, mm, P) and fwd.kernel == "conv_stem_tfir_f32"
            assert pre.label == "tfir%d_in" % sid and fwd.label == "conv1.tfir%d" % sid and fwd.macs == st.macs
            v_bytes = 4 * 8 * 3 * -(-16 // mm) * P * 224 * 224
            assert pre.hbm_bytes == 4 * 8 * 3 * 16 * 224 * 224 + v_bytes and not getattr(pre, "macs", 0)
            # issued MFMA work: all P products of every group, against the direct kernel's pruned 100 per 16 frames
            assert abs(fwd.issued_flop() / st.issued_flop() - (-(-16 // mm) * P) / 100.0) < 1e-9
            assert len(plan2.all_convs()) == n_convs and sum(s.macs for s in plan2.all_convs()) == macs
            assert plan2.all_convs()[0] is fwd
        tuned.tfir_store(st.key, 0)                                  # measured, direct stays
        assert tuned.tfir_lookup(st.key) == 0 and m.engine().dry_plan(m, shape).steps[0].use_tfir == 0
        tuned.tfir_store(st.key, 3)                                  # a verdict for a scheme this build does not time: direct
        assert m.engine().dry_plan(m, shape).steps[0].use_tfir == 0
        monkeypatch.setenv("PTX_STEM_TFIR", "3")
        s3 = m.engine().dry_plan(m, shape).steps[0]
        assert s3.use_tfir == 3 and sorted(s3.tfir) == [3] and s3.active()[1].P == 10
        monkeypatch.delenv("PTX_STEM_TFIR")
        # the 4-clip plan of the clip lanes has a key of its own
        half = m.engine().dry_plan(m, (4,) + shape[1:]).steps[0]
        assert half.key != st.key and half.use_tfir == 0
        # stems outside the rule keep the single direct launch
        r2 = ptx.r2plus1d18(num_classes=174)
        for s in r2.engine().dry_plan(r2, (2, 3, 8, 64, 64)).steps:
            assert not isinstance(s, StemF32Step) or s.tfir is None
        from pretorched_x_amd import engine
        norm = ptx._lib.NormDesc.make([0.4, 0.4, 0.4], [0.2, 0.2, 0.2], "RGB", [0, 1])
        planu = engine.Plan(m.engine(), m, (2, 3, 8, 64, 64), torch.device("meta"), norm)
        su = [s for s in planu.steps if isinstance(s, StemF32Step)][0]
        sc = m.engine().dry_plan(m, (2, 3, 8, 64, 64)).steps[0]
        assert su.src is not None and sc.src is None and sorted(su.tfir) == sorted(sc.tfir) == [1, 2] and su.key == sc.key
    finally:
        tuned.tuned_replace(keep)
