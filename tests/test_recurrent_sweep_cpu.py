"""The table and the checker of tests/test_gpu_recurrent_sweep.py, tried on the CPU with stand-ins for the device.  Rows run
scaled down (N capped at 48, T at 12; the T = 1 / 2 rows keep their length): what the checker does is the same for every N.

* torch's fp32 run of the written-out recurrence as the "device" passes every row (its ratio to itself is 1).
* An fp32 emulation of lstm_cell.h's gate formulas (rcp(1 + exp2(-x log2 e)), 1 - 2 rcp(1 + exp2(2 x log2 e)), derivatives from
  the saved activations; torch's exp2 and division) is held to torch's fp32: <= 1.9 x on hidden outputs and <= 1.4 x on gradients
  for wide inputs at T >= 9, as the issue measured; with a narrow input it is NOT within SHARP (4.8 x on y, 4.7 x on gradients at
  T <= 2: 1 - 2 rcp(..) cancels near 0) and is held to an absolute bound there (test_cell_emulation_against_torch_fp32).
* Deliberately wrong stand-ins FAIL the checker: the last step's term missing from dW_hh; dW_hh summed over T instead of T - 1
  products (shifted by one step); one 16-row tile's cell state not reset between two calls; the f and g blocks swapped in db
  only; one K chunk of 16 input columns dropped from dW_ih; dx of the last row tile scaled by (1 + 2e-6) (on the gain-2 rows whose
  dx is held to torch's fp32; elsewhere the yardstick is of that size and the checker lets it through); b_hn's gradient copied
  from b_in's (GRU).
* UNCAUGHT, stated and not tested: one hidden element off by 4 ULP at t = T - 1.  No accuracy rule with a margin of 4 separates
  it: torch's own fp32 hidden sequence has a largest error of 1 - 2 ULP of its largest elements at T = 1 (two activations and a
  product) and more later, so the mutated element stands at 2.5 - 5 ULP against an allowance of 4 - 8; per-step and per-tile
  Frobenius ratios do not move for one element of >= 1024; measured on the T = 1 rows, the mutated tensor's largest error is
  0.4 - 1.1 x the largest error of the fp32 runs it is compared with.  A per-element bound derived from the formats is wider
  still ((K + 2) 2^-24 |W| |x| on the pre-activation alone).  The exact rule of the carried-state rows (state == last step)
  is a rule of its own and no detector of this mutation: a kernel 4 ULP off puts the same bits into both.
* The table: ids unique, every path name present, every kernel family with its T = 1, 2 and 190 rows.
"""
import pytest
import torch

import test_gpu_recurrent_sweep as S

ROWS = [r.scaled() for r in S.TABLE]
IDS = [r.id for r in S.TABLE]
LSTM_TRAIN = [(r, i) for r, i in zip(ROWS, IDS) if r.entry == "layer_train"]
GRU_TRAIN = [(r, i) for r, i in zip(ROWS, IDS) if r.entry == "gru_train"]
LSTM_INFER = [(r, i) for r, i in zip(ROWS, IDS) if r.entry == "layer"]


def _check(row, ops, outs, ref64=None, cpu32=None, emu32=None):
    stats = {}
    S.check_outputs(stats, row, ops, outs, cpu32, ref64, emu32)
    S.assert_stats(row, stats, log=lambda s: None)
    return stats


def _flagged(row, ops, outs, what, **kw):
    with pytest.raises(AssertionError):
        _check(row, ops, outs, **kw)
        pytest.fail(f"{row.id}: '{what}' passed the checker", pytrace=False)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_torch_fp32_passes(row):
    for draw in range(S.draws_for(row, row.N())):
        ops = S.make_operands(row, row.N(), draw)
        _check(row, ops, S.reference(row, ops, torch.float32))


U = 2.0 ** -24
EMU_WORST = {}


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_cell_emulation_against_torch_fp32(row):
    """lstm_cell.h's formulas in CPU fp32 against torch's own sigmoid / tanh and autograd, both held to fp64: the evidence
    behind SHARP and behind yardstick_of.  Relative Frobenius error of the whole tensor, emulation / torch:
      wide input, T >= 9                     <= 1.9 on hidden outputs, <= 1.4 on gradients (the issue's figures; seen 1.41 / 1.27)
      every other output held to torch       <= SHARP (seen: wide T <= 2 2.48 / 1.52, narrow T >= 9 gradients 1.89)
      outputs held to the emulation (narrow) no ratio holds (seen 4.82 hidden, 4.65 gradients at T <= 2; 2.82 hidden at T >= 9):
        the absolute term is bounded instead.  A step evaluates five activations, each within three roundings of 2^-24
        absolute (|sigma|, |tanh| <= 1), and they enter h through factors <= 1: the rms error of a hidden output is held to
        15 x 2^-24 (seen 3.7e-7 = 6 x 2^-24); a gradient is linear in the activations' derivatives, of magnitude >= 1/4 where it
        matters: relative Frobenius error held to 60 x 2^-24 (seen 1.4e-6)."""
    ops = S.make_operands(row, row.N(), 0)
    ref = S.reference(row, ops, torch.float64)
    cpu = S.reference(row, ops, torch.float32)
    emu = S.reference(row, ops, torch.float32, act="cell")
    for k, r in ref.items():
        ec, ee, nr = float((cpu[k].double() - r).norm()), float((emu[k].double() - r).norm()), float(r.norm())
        hidden = k in S.HIDDEN
        if nr == 0 or ec == 0:
            assert ee == 0, f"{k}: the emulation is off where torch's fp32 is exact"
            continue
        ratio = ee / ec
        w = EMU_WORST.setdefault((S.yardstick_of(row, k), "hidden" if hidden else "gradient"), [0.0, ""])
        if ratio > w[0]:
            w[0], w[1] = ratio, f"{row.id} {k}"
        if S.yardstick_of(row, k) == "cell":
            if hidden:
                assert ee / r.numel() ** 0.5 <= 15 * U, f"{k}: rms error {ee / r.numel() ** 0.5:.3e} of the emulation beyond 15 x 2^-24"
            else:
                assert ee / nr <= 60 * U, f"{k}: relative error {ee / nr:.3e} of the emulation beyond 60 x 2^-24"
        elif row.I > S.NARROW and row.T >= 9:
            assert ratio <= (1.9 if hidden else 1.4), f"{k}: the emulation at {ratio:.2f} x torch's fp32"
        else:
            assert ratio <= S.SHARP, f"{k}: the emulation at {ratio:.2f} x torch's fp32"
    print("[rsweep-emu] worst so far: " + "; ".join(f"{k}: {v[0]:.2f} x ({v[1]})" for k, v in EMU_WORST.items()))


def _lstm_train_case(row):
    ops = S.make_operands(row, row.N(), 0)
    ref64 = S.reference(row, ops, torch.float64)
    good = S.reference(row, ops, torch.float32, probe=True)
    dg = good.pop("dgates")
    return ops, ref64, good, dg


@pytest.mark.parametrize("row", [r for r, _ in LSTM_TRAIN], ids=[i for _, i in LSTM_TRAIN])
def test_wrong_lstm_gradients_are_flagged(row):
    ops, ref64, good, dg = _lstm_train_case(row)
    T, N, H, I = row.T, row.N(), row.H, row.I
    kw = dict(ref64=ref64, cpu32={k: v for k, v in good.items()})
    _check(row, ops, good, **kw)
    y = good["y"]
    if T >= 2:
        bad = dict(good)
        bad["dw_hh"] = good["dw_hh"] - dg[T - 1].t() @ y[T - 2]
        _flagged(row, ops, bad, "the last step's term missing from dW_hh", **kw)
        bad = dict(good)
        bad["dw_hh"] = torch.einsum("tng,tnh->gh", dg, y)
        _flagged(row, ops, bad, "dW_hh over T products, shifted by one step", **kw)
    bad = dict(good)
    db = good["db"].view(4, H).clone()
    db[[1, 2]] = db[[2, 1]]
    bad["db"] = db.reshape(-1)
    _flagged(row, ops, bad, "f and g blocks swapped in db", **kw)
    bad = dict(good)
    k0 = (I - 1) // 16 * 16
    bad["dw_ih"] = good["dw_ih"].clone()
    bad["dw_ih"][:, k0:k0 + 16] -= torch.einsum("tng,tni->gi", dg, ops["x"])[:, k0:k0 + 16]
    _flagged(row, ops, bad, "one K chunk of 16 input columns dropped from dW_ih", **kw)
    # NOT flagged, and not tried, where the yardstick itself is of that size: with saturating gates torch's own fp32 dx is 2.4e-6
    # of fp64, and dx of a narrow T <= 2 row is held to the cell emulation (yardstick_of).  A statistic for COHERENT error (the
    # projection of a tile's error on its reference) would see it there; the checker has none.
    if row.gain == 2.0 and S.yardstick_of(row, "dx") == "torch":
        bad = dict(good)
        bad["dx"] = good["dx"].clone()
        bad["dx"][:, N - 16:] *= (1 + 2e-6)
        _flagged(row, ops, bad, "dx of the last row tile scaled by 1 + 2e-6", **kw)


@pytest.mark.parametrize("row", [r for r, _ in GRU_TRAIN], ids=[i for _, i in GRU_TRAIN])
def test_wrong_gru_bias_gradient_is_flagged(row):
    ops = S.make_operands(row, row.N(), 0)
    good = S.reference(row, ops, torch.float32)
    bad = dict(good)
    bad["db_hh"] = good["db_hh"].clone()
    bad["db_hh"][2 * row.H:] = good["db_ih"][2 * row.H:]
    _flagged(row, ops, bad, "b_hn's gradient copied from b_in's")


@pytest.mark.parametrize("row", [r for r, _ in LSTM_INFER], ids=[i for _, i in LSTM_INFER])
def test_wrong_hidden_sequences_are_flagged(row):
    ops = S.make_operands(row, row.N(), 0)
    ref64 = S.reference(row, ops, torch.float64)
    good = S.reference(row, ops, torch.float32)
    kw = dict(ref64=ref64, cpu32=good)
    N, H = row.N(), row.H
    # the last 16-row tile starts from the cell state the previous call left there
    x, w = ops["x"], ops["layers"][0]
    z = torch.zeros(N, H)
    _, _, c_fin = S.lstm_layer(x, *w, z, z)
    c0 = torch.zeros(N, H)
    c0[N - 16:] = c_fin[N - 16:]
    bad = dict(y=S.lstm_layer(x, *w, z, c0)[0])
    _flagged(row, ops, bad, "one tile's cell state not reset between two calls", **kw)


STATE = [(r, i) for r, i in zip(ROWS, IDS) if r.entry in ("layer_state", "gru_state")]


@pytest.mark.parametrize("row", [r for r, _ in STATE], ids=[i for _, i in STATE])
def test_state_that_is_not_the_last_step_is_flagged(row):
    """The checker's exact rule on the carried-state rows: the h state handed on equals the last step of the hidden sequence
    bit for bit.  One ULP on one element of either breaks it."""
    ops = S.make_operands(row, row.N(), 0)
    good = S.reference(row, ops, torch.float32)
    _check(row, ops, good)
    for k in ("h_fin", "y"):
        bad = dict(good)
        bad[k] = good[k].clone()
        v = bad[k].view(-1)[-1:].view(torch.int32)
        v += 1
        _flagged(row, ops, bad, f"{k} one ULP off the other")


def test_table():
    assert len(set(IDS)) == len(IDS), "row ids are not unique"
    paths = {r.path for r in S.TABLE}
    assert not set(S.PATHS) - paths, f"paths without a row: {sorted(set(S.PATHS) - paths)}"
    for fam in S.FAMILIES:
        have = {r.T for r in S.TABLE if r.family == fam}
        assert {1, 2, 190} <= have, f"kernel family {fam}: rows of T = {sorted(have)}, needs 1, 2 and 190"
    assert {r.family for r in S.TABLE} <= set(S.FAMILIES) | {"rec_gx", "train_group_bptt"}
    for fam in S.FAMILIES:
        assert any(r.gain == 6.0 for r in S.TABLE if r.family == fam), f"kernel family {fam}: no row with saturating gates"
    assert all(r.T in (1, 2, 9, 190, 4095, 4096) for r in S.TABLE)
