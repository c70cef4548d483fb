"""The table and the checker of tests/test_gpu_multi_sweep.py, tried without a device.  Rows run scaled down (every stack
capped at one whole cluster of 64 rows plus its partial cluster's residue, T at 12): what the checker does is the same for every N.

* The table, for 256 CUs and for 304 (cap = 38, not a multiple of 8): ids unique, every named row present, the Python mirror of
  the plan rule gives each row the plan it was written for, every stack a multiple of 16 rows, at most 8 stacks; `linear-map`
  has clusters % 8 != 0 and `one-stack-cap` exactly cap clusters; `threshold-lo`'s first three stacks share one shape (the
  weight-set equality needs them).
* torch's fp32 run of the written-out recurrence as the "device" passes every stack of every row.
* Deliberately wrong stand-ins FAIL the checker (all on `partial-each`, whose stacks end in a partial cluster, and
  `threshold-lo`): a stack whose boundary cluster (its first 64 rows) was computed with the previous stack's b_ih1 + b_hh1; the
  same with the previous stack's W_hh1; one 16-row tile of the partial last cluster holding a copy of the stack's first tile;
  one step's output of one cluster written one step early; two stacks of equal shape with their outputs exchanged.  A tile of a
  partial cluster that is STORED at the last step lands behind the tensor: the accuracy rule cannot see it, S.Out's guard does
  (tried here on a CPU S.Out).
* UNCAUGHT, stated and not tested:
  - a missing tile stored at a step BEFORE the last.  [T][N][H] has no room between steps: the 16 rows behind step t's last row
    are step t + 1's first rows, which cluster 0 of the same set writes one step later.  If the rightful store comes second the
    stray one leaves no trace in any output; only when it comes second (a race the kernel does not order) does the rule see it.
    The sweep pins the code that decides it instead: tile_ok is one expression for every step, and the last step's stray store
    has nothing behind it but the guard.
  - of a one-tile set's three missing tiles, the LAST alone stored at the last step: it starts 2 x 16 x 384 elements behind the
    tensor, beyond GUARD = 1024.  (All three share one predicate; the first lands inside the guard.)
  - one hidden element off by 4 ULP, for the reason tests/test_recurrent_sweep_cpu.py gives: the rule has a margin of 4.
* The host entries that answer without a device: fsn_lstm2_multi_workspace_bytes is 0 for every refused argument and the largest
  per-stack fsn_lstm2_fwd_workspace_bytes on the fallback; fsn_lstm2_multi_is_persistent is 0 without a device.
"""
import ctypes

import pytest
import torch

import test_gpu_multi_sweep as M
import test_gpu_recurrent_sweep as S

ROWS = [r.scaled() for r in M.TABLE]
IDS = [r.id for r in M.TABLE]
BY_NAME = dict(zip(IDS, ROWS))


def _case(row):
    rows = row.stack_rows()
    return rows, [M.stack_case(r, k) for k, r in enumerate(rows)]


def _check(r, cs, y):
    return M.check_stack(r, cs[0], cs[1:], y, log=None)


def _flagged(r, cs, y, what):
    with pytest.raises(AssertionError):
        _check(r, cs, y)
        pytest.fail(f"{r.id}: '{what}' passed the checker", pytrace=False)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_torch_fp32_passes(row):
    for r, cs in zip(*_case(row)):
        whole, block = _check(r, cs, cs[2]["y"])
        if S.yardstick_of(r, "y") == "torch":
            assert whole == 1.0 and block == 1.0  # its ratio to itself


@pytest.mark.parametrize("c", [256, 304])
def test_table(c):
    assert len(set(IDS)) == len(IDS), "row ids are not unique"
    assert set(IDS) == set(M.NAMES), f"rows {sorted(set(IDS) ^ set(M.NAMES))} named but not in the table, or the reverse"
    cap, lo = M.cap_of(c), M.lo_of(c)
    assert 4 * lo >= 3 * cap > 4 * (lo - 1)
    for row in M.TABLE:
        ns = row.Ns(c)
        assert 1 <= len(ns) <= 8, f"{row.id}: {len(ns)} stacks"
        assert all(n >= 16 and n % 16 == 0 for n in ns), f"{row.id}: rows {ns}"
        assert M.plan_rule(c, row.shapes(c), row.T) == row.wants_persistent(c), f"{row.id} on {c} CUs: not the plan it was written for"
        assert len(row.stack_rows(c)) == len(ns)
    by = {r.id: r for r in M.TABLE}
    cl = lambda name: sum((n + 63) // 64 for n in by[name].Ns(c))
    assert cl("one-stack-cap") == cap and cl("threshold-lo") == lo and cl("below-lo") == lo - 1 and cl("above-cap") == cap + 1
    assert lo <= cl("linear-map") <= cap and cl("linear-map") % 8 != 0
    assert all(n % 64 == 0 for name in ("threshold-lo", "below-lo", "above-cap") for n in by[name].Ns(c))
    assert [n % 64 for n in by["partial-each"].Ns(c)] == [16, 32, 48, 16] and lo <= cl("partial-each") <= cap
    assert by["tile-sets-first"].Ns(c)[:7] == [16] * 7 and len(by["tile-sets-first"].Ns(c)) == 8 and cl("tile-sets-first") == cap
    assert by["tile-set-last"].Ns(c)[-1] == 16 and by["tile-set-last"].Ns(c)[0] % 64 == 32
    assert by["model-48k"].Ns(c) == [640, 800, 192, 128]
    assert [r.I for r in by["narrow-wide"].stack_rows(c)] == [1, 16, 17, 257]
    t = by["threshold-lo"].stack_rows(c)
    assert t[0].N() == t[1].N() == t[2].N(), "the weight-set equality needs three stacks of one shape"
    for a, b in (("T4", 4), ("T3", 3), ("T33", 33)):
        assert by[a].T == b
    assert by["T4"].Ns(c) == by["T3"].Ns(c) == by["h320-as-384"].Ns(c) == by["mixed-hidden"].Ns(c) == by["threshold-lo"].Ns(c)
    assert by["T33"].Ns(c) == by["gain6"].Ns(c) == by["partial-each"].Ns(c) and by["gain6"].gain == 6.0
    if c == 256:  # the device the rows are written for: both mappings are taken, and the model's own layout is persistent
        assert cl("one-stack-cap") % 8 == 0 and cl("threshold-lo") % 8 == 0 and cl("tile-set-last") % 8 != 0
        assert by["model-48k"].wants_persistent(c)


def test_the_plan_rule_at_its_edges():
    c = 256
    assert [M.plan_rule(c, [(64 * k, 384, 384)], 9) for k in (23, 24, 32, 33)] == [False, True, True, False]
    assert M.plan_rule(c, [(64 * 23 + 16, 384, 384)], 9), "a partial cluster counts as one"
    assert not M.plan_rule(c, [(64 * 24, 384, 384)], 3) and M.plan_rule(c, [(64 * 24, 384, 384)], 4)
    assert not M.plan_rule(c, [(64 * 12, 384, 384), (64 * 12, 320, 320)], 9)
    assert not M.plan_rule(c, [(64 * 3, 384, 384)] * 9, 9) and M.plan_rule(c, [(64 * 3, 384, 384)] * 8, 9)
    assert not M.plan_rule(0, [(64 * 24, 384, 384)], 9)


def _layer1(r, ops, rows, bias_from=None, whh_from=None):
    """fp32 hseq1 of rows [rows] of a stack, layer 1 taking b_ih + b_hh / W_hh from another stack's operands."""
    (wi0, wh0, bi0, bh0), (wi1, wh1, bi1, bh1) = ops["layers"]
    x = ops["x"][:, rows]
    z = torch.zeros(x.shape[1], r.H)
    y0, _, _ = S.lstm_layer(x, wi0, wh0, bi0, bh0, z, z)
    if bias_from is not None:
        bi1, bh1 = bias_from["layers"][1][2], bias_from["layers"][1][3]
    if whh_from is not None:
        wh1 = whh_from["layers"][1][1]
    return S.lstm_layer(y0, wi1, wh1, bi1, bh1, z, z)[0]


@pytest.mark.parametrize("name", ["partial-each", "threshold-lo", "gain6"])
def test_a_neighbours_weight_set_at_the_boundary_cluster_is_flagged(name):
    rows, cases = _case(BY_NAME[name])
    for k in range(1, len(rows)):
        r, cs, prev = rows[k], cases[k], cases[k - 1][0]
        first = slice(0, 64)
        good = cs[2]["y"]
        assert torch.allclose(_layer1(r, cs[0], first), good[:, first], atol=1e-5), "the stand-in's own recurrence is not the reference's"
        bad = good.clone()
        bad[:, first] = _layer1(r, cs[0], first, bias_from=prev)
        _flagged(r, cs, bad, "the first cluster with the previous stack's b_ih1 + b_hh1")
        bad = good.clone()
        bad[:, first] = _layer1(r, cs[0], first, whh_from=prev)
        _flagged(r, cs, bad, "the first cluster with the previous stack's W_hh1")


@pytest.mark.parametrize("name", ["partial-each", "gain6", "tile-set-last"])
def test_a_wrong_tile_or_step_is_flagged(name):
    rows, cases = _case(BY_NAME[name])
    for r, cs in zip(rows, cases):
        N, good = r.N(), cs[2]["y"]
        if N % 64 and N > 64:
            bad = good.clone()
            bad[:, N - 16:] = good[:, :16]
            _flagged(r, cs, bad, "the last tile of the partial cluster holds a copy of the first tile")
        for t in (1, r.T - 1):
            bad = good.clone()
            bad[t - 1, :min(N, 64)] = good[t, :min(N, 64)]
            _flagged(r, cs, bad, f"step {t} of the first cluster written at step {t - 1}")


def test_exchanged_outputs_of_equal_shapes_are_flagged():
    rows, cases = _case(BY_NAME["threshold-lo"])
    assert rows[0].N() == rows[1].N()
    _flagged(rows[0], cases[0], cases[1][2]["y"], "stack 0 holds stack 1's output")
    _flagged(rows[1], cases[1], cases[0][2]["y"], "stack 1 holds stack 0's output")


def test_a_stored_missing_tile_at_the_last_step_hits_the_guard():
    """Residue 16: the cluster's second tile does not exist; stored at step T - 1 it lies behind the tensor."""
    row = BY_NAME["partial-each"]
    r, cs = row.stack_rows()[0], M.stack_case(row.stack_rows()[0], 0)
    assert r.N() % 64 == 16
    y = cs[2]["y"]
    o = S.Out(torch.device("cpu"), (r.T, r.N(), r.H1))
    o.f[:y.numel()] = y.reshape(-1)
    assert torch.equal(o.take("hseq1"), y)
    o.f[y.numel():y.numel() + S.GUARD] = y[-1, :16].reshape(-1)[:S.GUARD]
    with pytest.raises(AssertionError, match="outside its declared region"):
        o.take("hseq1")


def _stacks(shapes):
    from fullsubnet_amd import _lib
    arr = (_lib.Lstm2Stack * max(len(shapes), 1))()
    for q, (N, I, ldx, H0, H1) in zip(arr, shapes):
        q.N, q.I, q.ldx, q.H0, q.H1 = N, I, ldx, H0, H1
    return arr


def test_host_queries_without_a_device():
    """test_host_cpu.py's pattern: the size and plan queries answer from the shapes alone."""
    from fullsubnet_amd import _lib
    L = _lib.lib()
    ok = (16, 62, 64, 384, 384)
    q = lambda shapes, T=9, n=None: L.fsn_lstm2_multi_workspace_bytes(len(shapes) if n is None else n, ctypes.byref(_stacks(shapes)), T)
    assert q([ok, ok]) > 0
    assert q([ok], n=0) == 0 and b"stacks" in L.fsn_last_error()
    assert q([ok] * 9) == 0
    assert L.fsn_lstm2_multi_workspace_bytes(2, None, 9) == 0
    assert q([ok, (24, 62, 64, 384, 384)]) == 0
    assert q([ok, (16, 62, 64, 384, 100)]) == 0
    assert q([(16, 62, 62, 384, 384), ok]) == 0
    assert q([ok], T=0) == 0
    # the fallback (T = 3 is one on every device): one stack's workspace at a time, the largest
    shapes = [(640, 62, 64, 384, 384), (800, 68, 80, 384, 384), (192, 100, 112, 320, 320), (128, 180, 192, 384, 384)]
    per = [L.fsn_lstm2_fwd_workspace_bytes(3, N, I, H0, H1) for N, I, _, H0, H1 in shapes]
    assert min(per) > 0 and q(shapes, T=3) == max(per)
    assert L.fsn_lstm2_multi_is_persistent(4, ctypes.byref(_stacks(shapes)), 3) == 0
    assert L.fsn_lstm2_multi_is_persistent(4, ctypes.byref(_stacks(shapes)), 9) == 0  # a stack at H = 320
    assert L.fsn_lstm2_multi_is_persistent(0, ctypes.byref(_stacks(shapes)), 9) == 0
    assert L.fsn_lstm2_multi_is_persistent(2, None, 9) == 0
    if not torch.cuda.is_available():
        for row in M.TABLE:
            rows = row.stack_rows()
            arr = _stacks([(r.N(), r.I, r.ldx, r.H, r.H1) for r in rows])
            assert L.fsn_lstm2_multi_is_persistent(len(rows), ctypes.byref(arr), row.T) == 0, f"{row.id}: persistent without a device"
            per = [L.fsn_lstm2_fwd_workspace_bytes(row.T, r.N(), r.I, r.H, r.H1) for r in rows]
            assert L.fsn_lstm2_multi_workspace_bytes(len(rows), ctypes.byref(arr), row.T) == max(per)
