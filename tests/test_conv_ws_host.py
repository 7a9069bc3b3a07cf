"""Host-side tests of the persistent weight-stationary tiles ("/ws", csrc/conv_ws_kernel.h; no GPU): the eligibility rule of
ptx_conv3d_config_supported with one case per refusal, the PTX_CONV_WS switch, and the tile table's invariants."""
import ctypes as C

import pytest


def _names(lib):
    return [lib.ptx_conv3d_config_name(i).decode() for i in range(lib.ptx_conv3d_num_configs() + lib.ptx_conv3d_num_configs_bf16())]


def _ws(lib):
    return [i for i, n in enumerate(_names(lib)) if n.endswith("/ws")]


def _desc(L, N=1, T=2, H=7, W=9, Ci=64, Co=64, flags=1):
    d = L.ConvDesc()
    d.N, d.Ti, d.Hi, d.Wi, d.Ci, d.ldx = N, T, H, W, Ci, Ci
    d.To, d.Ho, d.Wo, d.Co, d.ldy = T, H, W, Co, (Co + 3) // 4 * 4
    d.kT, d.kH, d.kW, d.sT, d.sH, d.sW, d.pT, d.pH, d.pW = 1, 1, 1, 1, 1, 1, 0, 0, 0
    d.Kc, d.Co_pad, d.flags, d.ldr = Ci, (Co + 127) // 128 * 128, flags, (Co + 3) // 4 * 4
    return d


def _tile(name):
    bm, bn, bk = (int(v) for v in name.split("/")[0].split("x"))
    return bm, bn, bk


def _lds(name, K):
    """Bytes of LDS one worker needs: filter slice [BN][K], a ring of two [BM][K] row tiles, four parking slices
    [MT][BN / 2 + 4] of the row-major epilogue."""
    bm, bn, _ = _tile(name)
    mt = int(name.split("/m")[1].split("/")[0])
    return 4 * (K * (bn + 2 * bm) + 4 * mt * (bn // 2 + 4))


def test_ws_tiles_exist_and_table_invariants(ptx):
    lib = ptx._lib.lib()
    names = _names(lib)
    ws = _ws(lib)
    assert ws, "no /ws tile in this build"
    assert len(set(names)) == len(names)                                       # names are unique
    n0 = lib.ptx_conv3d_num_configs()
    assert all(n.endswith("/bf16") for n in names[n0:]) and not any(n.endswith("/bf16") for n in names[:n0])   # bf16 closes the table
    assert max(ws) < n0
    # after the last fp32 tile: nothing but /ws tiles between the first of them and the bf16 block
    assert ws == list(range(min(ws), n0))
    from pretorched_x_amd.tuned import _tile_kind
    from pretorched_x_amd.tuner import admissible
    d = _desc(ptx._lib, N=8, T=4, H=56, W=56, Ci=256, Co=64)
    for i in ws:
        bm, bn, bk = _tile(names[i])                                           # "BMxBNxBK/..." as the tuner parses it
        assert bk == 32 and bm in (32, 64) and bn in (64, 128)
        assert _tile_kind(names[i]) == ""                                      # an fp32 tile
        assert (admissible(names[i], d, "", 8 * 4 * 56 * 56, 64) is not None) == (bn == 64)


def test_ws_eligibility_one_case_per_refusal(ptx):
    L, lib = ptx._lib, ptx._lib.lib()
    names = _names(lib)

    def ok(cfg, **edits):
        shape = {k: edits.pop(k) for k in list(edits) if k in ("N", "T", "H", "W", "Ci", "Co", "flags")}
        d = _desc(L, **shape)
        for k, v in edits.items():
            setattr(d, k, v)
        return bool(lib.ptx_conv3d_config_supported(C.byref(d), cfg))

    for cfg in _ws(lib):
        name = names[cfg]
        bm, bn, bk = _tile(name)
        assert ok(cfg) and ok(cfg, flags=0) and ok(cfg, flags=L.PTX_EPI_RELU | L.PTX_EPI_RES_ADD)
        assert ok(cfg, Co=100, ldy=112) and ok(cfg, ldx=72)
        assert not ok(cfg, kT=3, kH=3, kW=3, pT=1, pH=1, pW=1)                  # a 3x3x3 filter
        assert not ok(cfg, sH=2, sW=2, Ho=4, Wo=5)                              # stride 2
        assert not ok(cfg, groups=2)                                            # groups
        assert not ok(cfg, x2_C=32, x2_ld=32, x2_T=2, x2_H=7, x2_W=9, x2_sT=1, x2_sH=1, x2_sW=1)   # a second source
        assert not ok(cfg, flags=L.PTX_EPI_RELU | L.PTX_EPI_RES_PADA, res_C=32, res_T=2, res_H=7, res_W=9, res_sT=1, res_sH=1,
                      res_sW=1, ldr=32)                                         # RES_PADA
        assert not ok(cfg, flags=L.PTX_F16X3_OPERANDS) and not ok(cfg, flags=L.PTX_F16_OPERANDS)
        assert not ok(cfg, Ci=48)                                               # Kc not a multiple of BK
        assert not ok(cfg, Ci=48, ldx=48, Kc=64)                                # rows shorter than the filter's K
        # the largest K whose filter slice, ring and parking area fit the 160 KiB of a CU; one chunk more is refused
        kmax = max(k for k in range(bk, 1024 + bk, bk) if _lds(name, k) <= 160 * 1024)
        assert kmax >= 256 and ok(cfg, Ci=kmax) and not ok(cfg, Ci=kmax + bk)
        # every operand below 2 GiB: 2^22 rows x 128 floats = 2 GiB exactly
        assert ok(cfg, N=1, T=1, H=2048, W=2047, Ci=64, ldx=128) and not ok(cfg, N=1, T=1, H=2048, W=2048, Ci=64, ldx=128)
        assert ok(cfg, N=1, T=1, H=2048, W=2047, Co=64, ldy=128) and not ok(cfg, N=1, T=1, H=2048, W=2048, Co=64, ldy=128)
        assert not ok(cfg, N=1, T=1, H=2048, W=2048, Co=64, flags=L.PTX_EPI_RES_ADD, ldr=128)
    # split-K is not a property of the descriptor: a /ws tile launched with split_k > 1 runs the generic tile of its shape
    # (tests/test_gpu_conv_ws.py); the tuner only times tiles that support the problem
    big = [i for i in _ws(lib) if _tile(names[i])[:2] == (32, 64)]
    assert big and ok(big[0], Ci=256)                                           # layer1.{1,2}.conv1 / layer2.0.conv1: K = 256


def test_ws_switch_turns_every_ws_tile_off(ptx, monkeypatch):
    L, lib = ptx._lib, ptx._lib.lib()
    d = _desc(L)
    assert all(lib.ptx_conv3d_config_supported(C.byref(d), i) for i in _ws(lib))
    monkeypatch.setenv("PTX_CONV_WS", "0")
    assert not any(lib.ptx_conv3d_config_supported(C.byref(d), i) for i in _ws(lib))
    generic = _names(lib).index("64x64x32/2x2/m32/dma/re")
    assert lib.ptx_conv3d_config_supported(C.byref(d), generic)                 # nothing else is switched
    monkeypatch.setenv("PTX_CONV_WS", "1")
    assert all(lib.ptx_conv3d_config_supported(C.byref(d), i) for i in _ws(lib))


@pytest.mark.parametrize("shape", [(8, 4, 56, 56, 64, 64), (8, 4, 56, 56, 256, 64), (8, 4, 56, 56, 64, 256), (8, 4, 28, 28, 128, 512),
                                   (1, 1, 7, 5, 64, 64), (8, 4, 28, 28, 512, 128), (2, 2, 7, 7, 2048, 512)])
def test_pick_config_never_returns_a_ws_tile(ptx, shape):
    L, lib = ptx._lib, ptx._lib.lib()
    N, T, H, W, Ci, Co = shape
    ws = set(_ws(lib))
    for flags in (0, L.PTX_EPI_RELU, L.PTX_EPI_RELU | L.PTX_EPI_RES_ADD):
        sk = C.c_int(0)
        assert lib.ptx_conv3d_pick_config(C.byref(_desc(L, N, T, H, W, Ci, Co, flags)), C.byref(sk)) not in ws
