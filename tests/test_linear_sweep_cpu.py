"""The checker of tests/test_gpu_linear_sweep.py, tried on the CPU: torch's fp32 product stands in for the HIP result.  Every
row of the sweep's table passes both modes, every integer case keeps its partial sums below 2^24, and in integer mode the
checker flags each of these corruptions of the stand-in at every row: one k row dropped, one counted twice, the K % 16
tail dropped (the last 16 k where K % 16 == 0), one 16 x 16 edge tile zeroed, the bias added twice.  No row is exempt.

Rows of more than R_MAX rows run here with R_MAX + R % 16 rows (the two 2^20 + 3 shapes and the 2^22 + 5 one, whose x
alone is 8.6 GB): what the checker does is the same for every R.  Their 2^24 condition is asserted for the full R from
the value ranges instead."""
import pytest
import torch

import test_gpu_linear_sweep as S

R_MAX = 1 << 13
ROWS = [r.scaled(R_MAX) for r in S.TABLE]


def _standin(ops):
    return S.cpu_products(ops)


def _check(row, ops, outs, mode):
    stats = S.new_stats(row, 1)
    S.check_outputs(stats, ops, outs, _standin(ops) if mode == "gauss" else None)
    for s in stats.values():
        s.assert_exact() if mode == "int" else s.assert_rounding()


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in S.TABLE])
def test_standin_passes_both_modes(row):
    for mode in ("int", "gauss"):
        for draw in range(2 if mode == "int" else 1):
            ops = S.make_operands(row, mode, draw, torch.device("cpu"))
            _check(row, ops, _standin(ops), mode)


@pytest.mark.parametrize("row", S.TABLE, ids=[r.id for r in S.TABLE])
def test_integer_rows_are_exact_at_full_size(row):
    """sum_k |a_k| |b_k| from the value ranges: |x|, |dy| <= vmax, |w| <= 2, |b| <= 5."""
    assert "int" in row.modes
    assert row.I * row.vmax * 2 + 5 < 2 ** 24 and row.O * row.vmax * 2 < 2 ** 24
    assert row.R * row.vmax * row.vmax < 2 ** 24


def _factors(ops, name):
    """The output as L @ M over its contraction index: L [m][K], M [K][n]."""
    x, w, dy = ops["x"], ops["w"], ops["dy"]
    return {"y": (x, w.t()), "dx": (dy, w), "dw": (dy.t(), x), "db": (dy.t(), torch.ones(dy.shape[0], 1))}[name]


def _corruptions(ops, name, good):
    """(what, corrupted copy of `good`) for one output tensor."""
    Lm, Mm = _factors(ops, name)
    K = Lm.shape[1]
    weight = Lm.abs().sum(0) * Mm.abs().sum(1)
    assert float(weight.max()) > 0, "no k row contributes"
    k = int(weight.argmax())
    delta = (Lm[:, k:k + 1] @ Mm[k:k + 1, :]).reshape(good.shape)
    yield "one k row dropped", good - delta
    yield "one k row counted twice", good + delta
    t0 = K - (K % 16 or min(K, 16))
    yield "K % 16 tail dropped", good - (Lm[:, t0:] @ Mm[t0:, :]).reshape(good.shape)
    tile = good.clone()
    if tile.dim() == 2:  # the last, possibly partial, 16 x 16 tile
        tile[(tile.shape[0] - 1) // 16 * 16:, (tile.shape[1] - 1) // 16 * 16:] = 0
    else:
        tile[(tile.shape[0] - 1) // 16 * 16:] = 0
    yield "edge tile zeroed", tile
    if name == "y":
        yield "bias added twice", good + ops["b"]


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in S.TABLE])
def test_corrupted_standin_is_flagged(row):
    """Both integer draws.  A corruption that changes nothing (zeroing a tile whose true values are all zero: the index
    pattern's products cancel over whole periods) is no corruption; each one must be real, and flagged, in a draw."""
    flagged = {}
    for draw in (0, 1):
        ops = S.make_operands(row, "int", draw, torch.device("cpu"))
        good = _standin(ops)
        for name in ("y", "dx", "dw", "db"):
            for what, bad in _corruptions(ops, name, good[name]):
                flagged.setdefault((name, what), 0)
                if torch.equal(bad, good[name]):
                    continue
                outs = dict(good)
                outs[name] = bad
                with pytest.raises(AssertionError):
                    _check(row, ops, outs, "int")
                    pytest.fail(f"{row.id} {name}: '{what}' passed the checker", pytrace=False)
                flagged[(name, what)] += 1
    assert all(flagged.values()), f"{row.id}: never a real corruption: {[k for k, v in flagged.items() if not v]}"


@pytest.mark.parametrize("row", S.TABLE, ids=[r.id for r in S.TABLE])
def test_rows_meet_the_plan_they_name(row):
    """Without a device the library plans for 256 CUs, the MI355X's count: the table's split counts hold there."""
    from fullsubnet_amd import _lib
    S.check_plan(_lib.lib(), row)
