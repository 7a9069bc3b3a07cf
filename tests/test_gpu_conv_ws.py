"""The persistent weight-stationary tiles ("/ws", csrc/conv_ws_kernel.h) on the GPU, through tests/conv_cases.py's runner:
every /ws tile against the float64 reference at the runner's fp32 bar (2e-4 of max(1, max|want|)), the output and the input
columns [Kc, ldx) pre-filled with NaN, the sentinel in [round_up(Co, 4), ldy) intact (the runner's layout contract).

Shapes are the smallest at which the kernel can go wrong: M = 3 BM + 9 or + 11 rows (four row tiles, the last ragged) with
PTX_WS_WORKERS=2 (two tiles per worker: both ring buffers, the store-under-load overlap), =5 (a worker without a tile), =1
(one worker walks all four) and unset; M = 5 (less than one tile); K from one chunk to the largest the tile supports; Co of
one, several and a ragged number of column blocks.  The walk order is fixed, so every worker count gives the same bits, as do
two consecutive launches; and the k-order is the generic BK = 32 tile's, so the bits are those of "/dma/re" too."""
import ctypes as C
import itertools

import pytest
import torch

import conv_cases as CC
import tuned_cases as TC

pytestmark = pytest.mark.gpu

RELU, RES_ADD = 1, 2
TILES = ["32x64x32/2x2/m16/dma/ws"]          # (64x64, 64x128 and 32x128 were built, measured and dropped: DESIGN.md 3.42)


def _desc(N, T, H, W, Ci, Co, flags):
    d = dict.fromkeys(TC.FIELDS, 0)
    d.update(N=N, Ti=T, Hi=H, Wi=W, Ci=Ci, ldx=Ci + 8, To=T, Ho=H, Wo=W, Co=Co, ldy=Co + 12, kT=1, kH=1, kW=1, sT=1, sH=1, sW=1,
             Kc=Ci, Co_pad=(Co + 127) // 128 * 128, flags=flags, ldr=(Co + 3) // 4 * 4 if flags & RES_ADD else 0)
    return d


def _ragged(bm):
    """(N, T, H, W) with M = 7 W = 3 BM + r, 0 < r < BM: four row tiles, the last ragged."""
    w = (3 * bm + 5 + 6) // 7
    assert 3 * bm < 7 * w < 4 * bm
    return 1, 1, 7, w


def _ks(ptx, tile):
    """{BK, 64, 256, the largest supported} that this tile supports."""
    lib = ptx._lib.lib()
    cfg = CC.tile_index(lib, tile)
    ok = [k for k in range(32, 1056, 32) if lib.ptx_conv3d_config_supported(C.byref(TC.fill(_desc(1, 1, 7, 15, k, 64, 0))), cfg)]
    assert ok and ok == list(range(32, ok[-1] + 32, 32)), ok
    return sorted({k for k in (32, 64, 256, ok[-1]) if k in ok})


def _run(ptx, d, tile, seed, workers, monkeypatch):
    if workers is None:
        monkeypatch.delenv("PTX_WS_WORKERS", raising=False)
    else:
        monkeypatch.setenv("PTX_WS_WORKERS", str(workers))
    assert ptx._lib.lib().ptx_conv3d_config_supported(C.byref(TC.fill(d)), CC.tile_index(ptx._lib.lib(), tile)) == 1
    (got, want, bar), = CC.run_conv(ptx, d, tile, 1, seed=seed)
    r = CC.error_over_bar(got, want, bar)
    print("ws %s K=%d Co=%d flags=%d M=%d workers=%s: error / bar = %.3g" % (
        tile, d["Ci"], d["Co"], d["flags"], d["N"] * d["To"] * d["Ho"] * d["Wo"], workers, r))
    assert r <= 1.0, (tile, d, workers, r)
    return got


def _tiles(ptx):
    lib = ptx._lib.lib()
    names = [lib.ptx_conv3d_config_name(i).decode() for i in range(lib.ptx_conv3d_num_configs())]
    ws = [n for n in names if n.endswith("/ws")]
    assert sorted(ws) == sorted(TILES), ws           # a tile this file does not list would go untested
    return ws


@pytest.mark.parametrize("tile", TILES)
def test_ws_tile_vs_float64(ptx, tile, monkeypatch):
    assert tile in _tiles(ptx)
    bm = int(tile.split("x")[0])
    ks = _ks(ptx, tile)
    assert ks[0] == 32 and 256 in ks and ks[-1] > 256
    shape = _ragged(bm)
    for n, (k, co, flags) in enumerate(itertools.product(ks, (64, 256, 100), (0, RELU, RELU | RES_ADD))):
        _run(ptx, _desc(*shape, k, co, flags), tile, 100 + n, 2, monkeypatch)
    # a worker with no tile; one worker for all four tiles; the default grid; less than one tile
    for n, (k, workers) in enumerate(itertools.product(ks, (5, 1, None))):
        _run(ptx, _desc(*shape, k, 100, RELU | RES_ADD), tile, 200 + n, workers, monkeypatch)
    for n, (k, workers) in enumerate(itertools.product(ks, (2, None))):
        _run(ptx, _desc(1, 1, 1, 5, k, 100, RELU | RES_ADD), tile, 300 + n, workers, monkeypatch)


def test_some_ws_tile_covers_k256(ptx):
    """layer1.{1,2}.conv1 and layer2.0.conv1 of the 3-D ResNet-50 have K = 256."""
    assert any(256 in _ks(ptx, t) for t in _tiles(ptx))


@pytest.mark.parametrize("tile", TILES)
def test_ws_bits_do_not_depend_on_workers_or_launch(ptx, tile, monkeypatch):
    assert tile in _tiles(ptx)
    bm = int(tile.split("x")[0])
    generic = tile.replace("/ws", "/re")
    for n, (k, co) in enumerate(itertools.product(_ks(ptx, tile), (256, 100))):
        d = _desc(*_ragged(bm), k, co, RELU | RES_ADD)
        base = _run(ptx, d, tile, 400 + n, 1, monkeypatch)
        for workers in (1, 2, 5, None):              # (workers = 1 again: two consecutive launches)
            assert torch.equal(_run(ptx, d, tile, 400 + n, workers, monkeypatch), base), (tile, k, co, workers)
        # the same k-order as the generic BK = 32 tile of the same MFMA shape: the same bits
        (got, _, _), = CC.run_conv(ptx, d, generic, 1, seed=400 + n)
        assert torch.equal(got, base), (tile, generic, k, co)


def test_ws_tile_with_split_or_switch_off_runs_the_generic_tile(ptx, monkeypatch):
    """A /ws index outside its eligibility (split-K > 1 here, which no descriptor carries; or PTX_CONV_WS=0) is served by the
    generic row-major tile of the same shape: same result, no refusal -- the sweeps that launch every fp32 tile on every
    problem (tests/test_gpu_kernels.py) rely on it."""
    tile = _tiles(ptx)[0]
    bm = int(tile.split("x")[0])
    d = _desc(*_ragged(bm), 128, 100, RELU | RES_ADD)
    base = _run(ptx, d, tile, 500, 2, monkeypatch)
    (got, want, bar), = CC.run_conv(ptx, d, tile, 2, seed=500)
    assert CC.error_over_bar(got, want, bar) <= 1.0
    monkeypatch.setenv("PTX_CONV_WS", "0")
    (got, want, bar), = CC.run_conv(ptx, d, tile, 1, seed=500)
    assert torch.equal(got, base)
