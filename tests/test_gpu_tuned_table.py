"""Every verdict of the SHIPPED tuned table on the GPU: the table's tile, at the table's split, on the table's problem
shrunk to a few rows (tests/tuned_cases.py), against a float64 CPU reference composed from the descriptor's flags
(tests/conv_cases.py).  The kernel tests cover the tile axis and the geometry axis one at a time; the table ships their
combinations -- 98 tiles x splits 1..8 x 21 flag words over pointwise, strided, temporal, grouped and dual-source problems
-- and the tuner measures time, not correctness.  One test per tile runs all of that tile's cases.

Bars are the project's own: fp32 tiles 2e-4 of max(1, max|want|) (close() of test_gpu_kernels.py), split-operand tiles
2e-5, fp16-operand / fused generator-stage cases the bars of _fused_stage_case (2e-4; 2e-3 for half outputs), chained
tiles test_conv_chain's 2e-5.  The wino:, wino4:, body: and lanes: verdicts get the host checks only."""
import pytest

import conv_cases as CC
import tuned_cases as TC

pytestmark = pytest.mark.gpu

CASES = TC.cases()
CHAIN_CASES = TC.chain_cases()
MUTATE = None          # "no_residual" | "drop_tap": falsify the reference (an uncommitted edit shows the tests have teeth)


def _seed(i, tile):
    return 9000 + 16 * i + 4096 * (sum(tile.encode()) % 97)


def _judge(tile, results):
    """results: [(case, [(got, want, bar)])].  Prints the worst error over bar of the tile, asserts every case."""
    worst, bad = 0.0, []
    for case, outs in results:
        for got, want, bar in outs:
            r = CC.error_over_bar(got, want, bar)
            worst = max(worst, r)
            if not r <= 1.0:
                bad.append((r, case.key, getattr(case, "split", 1)))
    kind = TC.operand_kind(results[0][0].desc["flags"])
    print("tuned-table %s %s: %d cases, worst error / bar = %.3g" % (kind, tile, len(results), worst))
    assert not bad, "%d of %d cases of %s miss their bar (error / bar, key, split): %s" % (len(bad), len(results), tile, sorted(bad)[-3:])


@pytest.mark.parametrize("tile", list(CASES))
def test_tuned_conv_tile(ptx, tile):
    _judge(tile, [(c, CC.run_conv(ptx, c.desc, c.tile, c.split, seed=_seed(i, tile), mutate=MUTATE))
                  for i, c in enumerate(CASES[tile])])


@pytest.mark.parametrize("tile", list(CHAIN_CASES))
def test_tuned_chain_tile(ptx, tile):
    _judge(tile, [(c, CC.run_chain(ptx, c.desc, c.tail, c.tile, seed=_seed(i, tile), mutate=MUTATE))
                  for i, c in enumerate(CHAIN_CASES[tile])])
