"""The checkers of tests/test_gpu_amp_sweep.py, tried on the CPU with torch stand-ins for the device.  The stand-in that is
the emulation in fp32 (torch's fp32 product of the 16-bit operands, tensor.to(type) for the conversion) passes everything;
each wrong stand-in must fail the assertion named for it:

  a K tail of 16 rows dropped from a product   the hard bound (Gaussians) and the equality (integers), every row, both types
  round toward zero instead of nearest-even     the to16 table, both types
  ties rounded away from zero                   the to16 table, both types (the table holds every tie of a few binades)
  fp16 subnormals flushed to zero               the to16 table under f16
  W_hh left unrounded                           check_one_step (2a) at T 1, 2, 3, 9, both types
  round toward zero instead of nearest-even     the same; and check_saved16 on the decoded gate slots
  h_{t-1} taken from step t - 2                 check_one_step at T >= 3; a stale step of y in check_recurrence (2b)
  one 16-row tile swapped                       check_one_step and check_recurrence; a step 4.5 x off alone: its own block
  rows beside the launch from rounded operands  check_one_step on g16-left
  dx rounded where the path leaves it, and back check_backward_t1 and check_recurrence at T = 1
  a gate slot of another unit quad, a wrong h_t check_saved16
All of them go through the device test's own checkers (check_one_step, check_recurrence, check_saved16) on shrunken paths
(48 cluster rows + 16 beside them, the table's T).

It also measures what the yardstick rules rest on: one fp32 step summed as ONE chain per element against the blocked sums of
a CPU GEMM (check_one_step); the two fp32 runs of the emulation against each other, whole tensors and tile by tile
(yardstick_of, assert_recurrence).  And it asserts that every path name occurs, that every kernel family has a T = 1, a
T = 2 and a T >= 9 row, and the three loss scales.

Rows run here with at most K_MAX + K % 32 rows of K: what the checker does is the same for every K.  Their 2^24 condition
is asserted for the full K from the value ranges, and every row's plan (form and split count at 256 CUs, which the
library assumes without a device) through the same query the device test uses."""
import pytest
import torch

import test_gpu_amp_sweep as S

K_MAX = 256
ROWS = [r.scaled(K_MAX) for r in S.TABLE]
IDS = [r.id for r in S.TABLE]
CPU = torch.device("cpu")


def _operands(row, mode, draw, ar):
    A, B = S.make_operands(row.M, row.Nc, row.K, mode, draw, ar, CPU, representable=row.kind != "tn")
    return (A, B) if row.kind != "tn" else (S.r16(A, ar), S.r16(B, ar))  # gemm_tn rounds on load


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_standin_passes_both_modes(row):
    for ar in S.ARITHS:
        for mode, draws in (("int", 2), ("gauss", 1)):
            for draw in range(draws):
                A, B = _operands(row, mode, draw, ar)
                S.check_product(row.id, row.K, 1, S.cpu_product(A, B), A, B, mode)


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_dropped_k_tail_is_flagged(row):
    """The product without its last 16 k rows (what a reduction that forgets the K % 32 tail returns at K % 32 == 16)."""
    for ar in S.ARITHS:
        for mode, what in (("int", "differ from the fp64 product"), ("gauss", "bound")):
            A, B = _operands(row, mode, 1, ar)
            bad = S.cpu_product(A[:-16], B[:-16])
            assert not torch.equal(bad, S.cpu_product(A, B))
            with pytest.raises(AssertionError, match=what):
                S.check_product(row.id, row.K, 1, bad, A, B, mode)


@pytest.mark.parametrize("G,I", S.DX16, ids=[f"G{g}-I{i}" for g, i in S.DX16])
def test_dx16_standin_and_dropped_tail(G, I):
    rows = 48
    for ar in S.ARITHS:
        for mode, what in (("int", "differ from the fp64 product"), ("gauss", "bound")):
            W, Dt = S.make_operands(I, rows, G, mode, 1, ar, CPU)
            S.check_product("dx16", G, 1, S.cpu_product(Dt, W), Dt, W, mode)
            with pytest.raises(AssertionError, match=what):
                S.check_product("dx16", G, 1, S.cpu_product(Dt[:-16], W[:-16]), Dt, W, mode)


def test_integer_rows_are_exact_at_full_size():
    """sum_k |a_k| |b_k| <= K x 2 x 3 from the value ranges, for every row, the dx products and the boundary walk's window."""
    for row in S.TABLE:
        assert row.K * 2 * 3 < 2 ** 24, row.id
    assert all(G * 2 * 3 < 2 ** 24 for G, _ in S.DX16) and (1 << 17) * 2 * 3 < 2 ** 24


def test_table_names_every_path():
    kinds = {(r.kind, r.form, r.wide) for r in S.TABLE}
    assert {("tn16h", 1, 1), ("tn16h", 2, 1), ("tn16h", 1, 0), ("tn16n", 1, 1), ("tn", None, 1)} <= kinds
    assert any(r.kind == "tn16h" and r.K % 32 == 16 and r.form == f for r in S.TABLE for f in (1, 2))
    assert {r.layout for r in S.TN16H} == {"plain", "saved", "offset"}
    assert (1536, 384) in S.CLASSES and (192, 192) in S.CLASSES
    assert {r.Nc for r in S.TN16N} == {1, 17, 20, 31, 32} and {r.M for r in S.TN16N} == {384, 1536}
    assert {r.K for r in S.TN16N} >= {2048, 2064}
    paths = {r.path for r in S.LSTM2_PLAN}
    assert paths >= {"g16-full", "g16-left", "g16-in16-off", "fwd-group16-bwd-by-layer", "hook-0", "hook-2", "hook-3"}
    assert {1, 2} <= {r.T for r in S.LSTM2_PLAN if r.path == "g16-full"}


@pytest.mark.parametrize("row", S.TABLE, ids=IDS)
def test_rows_meet_the_plan_they_name(row):
    """Without a device the library plans for 256 CUs, the MI355X's count: the table's forms and split counts hold there."""
    from fullsubnet_amd import _lib
    L = _lib.lib()
    try:
        if not row.wide:
            L.fsn_debug_tn16h_wide(0)
        form, splits = S.check_plan(L, row)
        assert form and splits >= 1, f"{row.id}: no plan"
    finally:
        L.fsn_debug_tn16h_wide(1)


@pytest.mark.parametrize("M,Nc", S.CLASSES)
def test_plan_boundaries_exist(M, Nc):
    from fullsubnet_amd import _lib
    changes = S.plan_changes(_lib.lib(), M, Nc, 1 << 17, S.BOUNDARIES)
    assert len(changes) == S.BOUNDARIES and changes[0][1] == (0, 0)
    first = min(r.K for r in S.TN16H if (r.M, r.Nc) == (M, Nc))
    assert changes[0][0] == first, f"{M} x {Nc}: the smallest K with a plan is {changes[0][0]}, the table starts at {first}"


# ---- to16 -----------------------------------------------------------------------------------------------------------------

def _magnitude_down(src, ar):
    """Round toward zero: the nearest-even result, one step back where it went away from zero."""
    dt = S.ARITHS[ar][1]
    near = src.to(dt)
    bits = near.view(torch.int16).clone()
    away = (near.float().abs() > src.abs()) & ~torch.isnan(src)  # (an overflow to inf included)
    bits[away] -= 1  # sign-magnitude: one less in either sign is one step toward zero
    return bits


def _ties_away(src, ar):
    dt = S.ARITHS[ar][1]
    near = src.to(dt)
    bits = near.view(torch.int16).clone()
    down = (near.float().abs() < src.abs()) & torch.isfinite(src)
    up = bits + 1  # the neighbour away from zero
    tie = down & ((up.view(dt).float().abs().double() - src.abs().double()) == (src.abs().double() - near.float().abs().double()))
    bits[tie] += 1
    return bits


def _flush_f16_subnormals(src, ar):
    bits = src.to(torch.float16).view(torch.int16).clone()
    sub = (src.abs() < 2.0 ** -14)
    bits[sub] &= -0x8000  # keep the sign
    return bits


def test_to16_standin_passes():
    table = S.to16_table()
    assert table.numel() % 4 == 0 and bool(torch.isnan(table).any()) and bool(torch.isinf(table).any())
    for ar in S.ARITHS:
        S.assert_to16(table, table.to(S.ARITHS[ar][1]).view(torch.int16), ar)
    # a NaN is compared as a NaN only: another payload passes, a number does not
    nan = torch.tensor([float("nan")] * 4)
    for ar in S.ARITHS:
        S.assert_to16(nan, torch.full((4,), S.NAN16[ar] | 1, dtype=torch.int16), ar)
        with pytest.raises(AssertionError, match="to16"):
            S.assert_to16(nan, torch.zeros(4, dtype=torch.int16), ar)


@pytest.mark.parametrize("ar", list(S.ARITHS))
@pytest.mark.parametrize("wrong", [_magnitude_down, _ties_away], ids=["toward-zero", "ties-away"])
def test_to16_wrong_rounding_is_flagged(wrong, ar):
    table = S.to16_table()
    bad = wrong(table, ar)
    n = S.to16_mismatches(table, bad, ar).numel()
    assert n > 100, f"{wrong.__name__} {ar}: only {n} elements of the table tell it from nearest-even"
    with pytest.raises(AssertionError, match="to16"):
        S.assert_to16(table, bad, ar)
    for i in S.to16_mismatches(table, bad, ar)[:64].tolist():  # every 4-element call that holds one of them fails too
        q = i // 4 * 4
        with pytest.raises(AssertionError, match="to16"):
            S.assert_to16(table[q:q + 4], bad[q:q + 4], ar)


def test_to16_flushed_subnormals_are_flagged():
    table = S.to16_table()
    with pytest.raises(AssertionError, match="to16 f16"):
        S.assert_to16(table, _flush_f16_subnormals(table, "f16"), "f16")
    small = table[(table.abs() < 2.0 ** -126) & (table != 0)]
    assert small.numel() >= 256  # bf16's subnormals: fp32's own
    flushed = small.to(torch.bfloat16).view(torch.int16) & -0x8000
    assert S.to16_mismatches(small, flushed, "bf16").numel() > 100


# ---- the one step of the two-layer check ---------------------------------------------------------------------------------------

def _step_case(N=64, I=12, seed=5):
    g = torch.Generator().manual_seed(seed)
    H = 384
    a = 2.0 / H ** 0.5
    w = [(torch.rand(sh, generator=g) * 2 - 1) * a for sh in ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,))]
    x = torch.randn(N, I, generator=g)
    h = torch.tanh(torch.randn(N, H, generator=g)) * 0.3
    c = torch.randn(N, H, generator=g) * 0.3
    return x, h, c, w


def _err(got, ref):
    e = (got.double() - ref).abs()
    return float(e.pow(2).sum().sqrt()), float(e.max())


def test_one_step_yardsticks_and_the_chain_term():
    """The rule of check_one_step rests on this: one fp32 step with ONE chain of K = I + 384 terms per element (the fp32 step
    kernels) against the blocked sums of a CPU GEMM, both against fp64: the chain is the less accurate legitimate fp32 run, by
    1.2 - 3 x in Frobenius norm on the gates; both are far below the effect of a 16-bit rounding of the operands."""
    ident = lambda t: t
    x, h, c, w = _step_case()
    ref = S.one_step(x, h, c, w, torch.float64, "torch", ident)
    blocked = S.one_step(x, h, c, w, torch.float32, "cell", ident)
    chain = S.one_step(x, h, c, w, torch.float32, "cell", ident, chain=True)
    for k, name in enumerate(("gates", "c", "h")):
        fb, mb = _err(blocked[k], ref[k])
        fc, mc = _err(chain[k], ref[k])
        print(f"one step {name}: chain / blocked Frobenius {fc / fb:.2f} x, max {mc / mb:.2f} x")
        assert 1.1 * fb < fc < 4 * fb, (name, fc / fb)
    for ar in S.ARITHS:  # the arithmetic itself: 100 x and more above either fp32 run
        rounded = S.one_step(x, h, c, w, torch.float64, "torch", lambda t: S.r16(t.float(), ar))
        assert _err(rounded[0], ref[0])[0] > 100 * _err(chain[0], ref[0])[0]


@pytest.mark.parametrize("ar", list(S.ARITHS))
def test_one_step_flags_an_unrounded_operand(ar):
    """W_hh left unrounded, and round toward zero instead of nearest-even, on a stand-in for the device (the rounded one step in
    fp32): the Frobenius statistic against the rounded fp64 one step exceeds SHARP x the yardstick's; the right stand-in passes."""
    x, h, c, w = _step_case()
    rnd = lambda t: S.r16(t.float(), ar)
    ref = S.one_step(x, h, c, w, torch.float64, "torch", rnd)
    yard = S.one_step(x, h, c, w, torch.float32, "cell", rnd)
    good = S.one_step(x, h, c, w, torch.float32, "torch", rnd)
    w_raw = [w[0], w[1] + 0, w[2], w[3]]

    def unrounded_whh(t):
        return t if t.shape == w[1].shape else rnd(t)

    def toward_zero(t):
        bits = _magnitude_down(t.float().contiguous().view(-1), ar)
        return bits.view(S.ARITHS[ar][1]).float().view(t.shape)

    for k in range(3):
        fy = _err(yard[k], ref[k])[0]
        assert _err(good[k], ref[k])[0] <= S.SHARP * fy
    for wrong in (unrounded_whh, toward_zero):
        bad = S.one_step(x, h, c, w_raw, torch.float32, "cell", wrong)
        assert _err(bad[0], ref[0])[0] > S.SHARP * _err(yard[0], ref[0])[0], wrong.__name__


# ---- the device checkers of the two-layer entries on CPU stand-ins -------------------------------------------------------------

def _standin_forward(path, ar, ops, wrong=None):
    """What check_one_step reads of a forward call - hseq0 / hseq1 and the save buffers gates [T][N][4H] | c [T][N][H] - from
    the path's recurrence in CPU fp32 (torch's activations), or from a deliberately wrong one."""
    main = path.N - path.left
    ident = lambda t: t
    rnd = (lambda t: S.r16(t.float(), ar)) if path.fwd_rounded else ident
    if wrong == "toward-zero" and path.fwd_rounded:
        rnd = lambda t: _magnitude_down(t.float().contiguous().view(-1), ar).view(S.ARITHS[ar][1]).float().view(t.shape)
    fw, inp = {}, ops["x"]
    for k, w in enumerate(ops["layers"]):
        ww = list(w)
        rm = rnd
        if wrong == "whh-unrounded":
            rm = lambda t, w1=w[1]: t if t.shape == w1.shape else rnd(t)
        zero = torch.zeros(path.N, 384)
        hs, cs, gs = [], [], []
        for t in range(path.T):
            hp, cp = (hs[-1], cs[-1]) if t else (zero, zero)
            if wrong == "stale-h" and t >= 2:
                hp = hs[-2]
            parts = [S.one_step(inp[t, :main], hp[:main], cp[:main], ww, torch.float32, "torch", rm)]
            if path.left:
                parts.append(S.one_step(inp[t, main:], hp[main:], cp[main:], ww, torch.float32, "torch",
                                        rnd if wrong == "left-rounded" else ident))
            g, c, h = (torch.cat([pt[j] for pt in parts]) for j in range(3))
            gs.append(g), cs.append(c), hs.append(h)
        inp = torch.stack(hs)
        if wrong == "tile-swap" and k == 1:
            inp = inp.clone()
            inp[-1, :16], inp[-1, 16:32] = inp[-1, 16:32].clone(), inp[-1, :16].clone()
        fw[f"hseq{k}"] = inp
        fw[f"s{k}"] = torch.cat([torch.stack(gs).reshape(-1), torch.stack(cs).reshape(-1)])
    return fw


CPU_PATHS = [p.scaled() for p in S.PATHS]
CPU_IDS = [p.id for p in S.PATHS]


@pytest.mark.parametrize("path", CPU_PATHS, ids=CPU_IDS)
def test_one_step_checker_passes_the_right_standin(path):
    quiet = lambda *_: None
    for ar in S.ARITHS:
        ops = path.operands()
        S.check_one_step(path, ar, ops, _standin_forward(path, ar, ops), log=quiet)


@pytest.mark.parametrize("ar", list(S.ARITHS))
@pytest.mark.parametrize("wrong", ["whh-unrounded", "toward-zero", "stale-h", "tile-swap", "left-rounded"])
def test_one_step_checker_flags(wrong, ar):
    """Through check_one_step itself (per-step and per-tile blocks, max statistic, the split of the rows beside the launch):
    W_hh unrounded and round toward zero fail at every T (1, 2, 3, 9 are run); h_{t-1} taken from step t - 2 and one swapped
    16-row tile fail at T >= 3 in a block of their own step / tile; rounded operands on the rows beside the launch fail on g16-left."""
    quiet = lambda *_: None
    name = "g16-left" if wrong == "left-rounded" else "g16-full"
    paths = [p for p in CPU_PATHS if p.path == name and (p.T >= 3 or wrong not in ("stale-h", "tile-swap"))]
    assert paths and (wrong in ("stale-h", "tile-swap", "left-rounded") or {1, 2, 9} <= {p.T for p in paths})
    for path in paths:
        ops = path.operands()
        with pytest.raises(AssertionError, match="Frobenius error|max error"):
            S.check_one_step(path, ar, ops, _standin_forward(path, ar, ops, wrong), log=quiet)
            pytest.fail(f"{path.id} {ar}: '{wrong}' passed check_one_step", pytrace=False)


def _recurrence_paths():
    return [p for p in CPU_PATHS if p.path in ("g16-full", "g16-left", "g16-in16-off", "fwd-group16-bwd-by-layer", "saturated")]


@pytest.mark.parametrize("path", _recurrence_paths(), ids=lambda p: p.id)
def test_recurrence_checker_passes_the_emulation_in_fp32(path):
    """2b with the stand-in that is the emulation in fp32 (for each output the run its rule names), and the two fp32 runs
    measured against each other (printed).  At these 48 - 64 rows the ratio is no statistic: an fp32 run is as far from the fp64
    emulation as the handful of its operands that fell on the other side of a 16-bit boundary (1 in about 5000; layer 1 rounds
    the hidden state of layer 0 even at T = 1) - a run with none of them sits 100 x below a run with three.  The device rows
    have 1536 rows and more, where both runs have hundreds."""
    quiet = lambda *_: None
    for ar in S.ARITHS:
        ops = path.operands()
        rounding = path.rounding()
        runs = {a: S.emulated_path(path, ar, ops, torch.float32, a, rounding) for a in ("torch", "cell")}
        got = {k: runs[S.R.yardstick_of(path.row, k)][k] for k in runs["torch"]}
        stats = S.check_recurrence(path, ar, ops, got, rounding, log=quiet)
        for k, s in stats.items():
            a = s.acc["all"]
            if a[1] > 0 and a[6] > 0:
                ratio = (a[6] / a[1]) ** 0.5
                print(f"{path.id} {ar} {k}: fp32 cell run / fp32 torch run {ratio:.2f} x")


def _matched(path, ar, ops, rounding):
    """For every output the fp32 run of the emulation that its rule names: the stand-in that passes 2b exactly."""
    runs = {a: S.emulated_path(path, ar, ops, torch.float32, a, rounding) for a in ("torch", "cell")}
    return {k: runs[S.R.yardstick_of(path.row, k)][k] for k in runs["torch"]}


@pytest.mark.parametrize("ar", list(S.ARITHS))
def test_recurrence_checker_flags(ar):
    """dx rounded where the path leaves it unrounded and the reverse, at T = 1 (the one-step backward); a stale h_{t-1} and a
    swapped 16-row tile at T = 9, in the block of their own."""
    quiet = lambda *_: None
    t1 = next(p for p in CPU_PATHS if p.path == "g16-full" and p.T == 1)
    ops = t1.operands()
    for in16 in (False, True):
        rounding = dict(fwd=True, bwd16=True, in16=in16)
        good = _matched(t1, ar, ops, rounding)
        bad = dict(good, dx=_matched(t1, ar, ops, dict(rounding, in16=not in16))["dx"])
        with pytest.raises(AssertionError, match="dx"):
            S.check_recurrence(t1, ar, ops, bad, rounding, log=quiet)
        assert bool((good["dw_hh0"] == 0).all()) and bool((good["dw_hh1"] == 0).all())
    t9 = next(p for p in CPU_PATHS if p.path == "g16-full" and p.T == 9)
    ops = t9.operands()
    rounding = t9.rounding()
    good = _matched(t9, ar, ops, rounding)
    for name in ("y", "dx"):
        bad = dict(good)
        v = good[name].clone()
        v[4, :16], v[4, 16:32] = good[name][4, 16:32], good[name][4, :16]
        bad[name] = v
        with pytest.raises(AssertionError, match=rf"{name}.*(Frobenius error|max error)"):
            S.check_recurrence(t9, ar, ops, bad, rounding, log=quiet)
        # the per-step block on its own: step 4 alone 4.5 x as far from fp64 as the yardstick, the whole tensor 2.3 x
        ref = S.emulated_path(t9, ar, ops, torch.float64, "torch", rounding)[name]
        v = good[name].clone()
        v[4] = (ref[4] + 4.5 * (good[name][4].double() - ref[4])).float()
        with pytest.raises(AssertionError, match=rf"{name} \[step 4\]|max error"):
            S.check_recurrence(t9, ar, ops, dict(good, **{name: v}), rounding, log=quiet)
    bad = dict(good)
    v = good["y"].clone()
    v[5] = good["y"][4]  # a stale step
    bad["y"] = v
    with pytest.raises(AssertionError, match=r"y.*(Frobenius error|max error)"):
        S.check_recurrence(t9, ar, ops, bad, rounding, log=quiet)


def test_every_family_has_its_lengths_and_every_path_its_row():
    names = {p.path for p in S.PATHS}
    assert names == set(S.PATH_NAMES)
    assert {n for fam in S.FAMILIES.values() for n in fam} | {"g16-in16-off"} == names
    for fam, members in S.FAMILIES.items():
        ts = {p.T for p in S.PATHS if p.path in members}
        assert 1 in ts and 2 in ts and max(ts) >= 9, f"{fam}: T of its rows {sorted(ts)}"
    assert {p.dy_scale for p in S.PATHS if p.path == "scale"} == {1.0, 64.0, 2.0 ** 14}


def test_two_fp32_runs_differ_tile_by_tile():
    """What assert_recurrence's tile rule rests on, without a device: the two legitimate fp32 runs of the emulation (torch's
    activations, lstm_cell.h's formulas) at T 2, 256 rows.  Whole tensors within SHARP x of each other under f16; the SAME
    16-row tile more than SHARP x apart on a hidden output under both types (seen: up to 28 x under f16, 1400 x under bf16)."""
    path = S.Path("g16-full", 2, 256, 20, 32, g16_fwd=1, g16_bptt=1)
    rounding = dict(fwd=True, bwd16=True, in16=False)
    for ar in S.ARITHS:
        ops = path.operands()
        ref = S.emulated_path(path, ar, ops, torch.float64, "torch", rounding)
        a = S.emulated_path(path, ar, ops, torch.float32, "torch", rounding)
        b = S.emulated_path(path, ar, ops, torch.float32, "cell", rounding)
        worst = 0.0
        for k in ("y0", "y", "dx"):
            ea, eb = a[k].double() - ref[k], b[k].double() - ref[k]
            whole = float(eb.norm() / ea.norm())
            r = [float(eb[:, n:n + 16].norm() / ea[:, n:n + 16].norm().clamp_min(1e-300)) for n in range(0, path.N, 16)]
            spread = max(max(r), 1 / min(r))
            print(f"{ar} {k}: cell run / torch run whole {whole:.2f} x, per tile {min(r):.2f} .. {max(r):.2f} x")
            worst = max(worst, spread)
            if ar == "f16":
                assert 1 / S.SHARP < whole < S.SHARP, (k, whole)
        assert worst > S.SHARP, (ar, worst)


@pytest.mark.parametrize("ar", list(S.ARITHS))
def test_saved16_checker(ar):
    """decode_saved16 / check_saved16 on a stand-in that writes the slots as the header describes; it flags gates stored
    rounded toward zero, a gate slot of another unit quad, and an h_t that is not the rounded hidden sequence."""
    quiet = lambda *_: None
    path = next(p for p in CPU_PATHS if p.path == "g16-left" and p.T == 2)
    ops = path.operands()
    fw = _standin_forward(path, ar, ops)
    T, N, H, dt = path.T, path.N, 384, S.ARITHS[ar][1]

    def slots(round_gates=lambda t: t.to(dt), shift=0, h_of=lambda h: h.to(dt)):
        out = {"hseq0": fw["hseq0"], "hseq1": fw["hseq1"]}
        for k in range(2):
            sv = fw[f"s{k}"]
            gates = sv[:T * N * 4 * H].view(T, N, 4, H // 4, 4).permute(0, 1, 3, 2, 4)  # [quad][gate][unit]
            g16 = round_gates(gates.reshape(T, N, 4 * H)).view(torch.int16).roll(16 * shift, -1)
            h16 = h_of(fw[f"hseq{k}"]).view(torch.int16)
            slot = torch.cat([g16, h16, torch.zeros(T, N, 3 * H, dtype=torch.int16)], -1)
            out[f"s{k}"] = torch.cat([slot.reshape(-1).view(torch.float32), sv[T * N * 4 * H:]])
        return out

    S.check_saved16(path, ar, ops, slots(), log=quiet)
    toward_zero = lambda t: _magnitude_down(t.contiguous().view(-1), ar).view(dt).view(t.shape)
    for bad in (slots(round_gates=toward_zero), slots(shift=1), slots(h_of=lambda h: (h * (1 + 2.0 ** -6)).to(dt))):
        with pytest.raises(AssertionError, match="saved 16-bit value|16-bit h_t"):
            S.check_saved16(path, ar, ops, bad, log=quiet)


@pytest.mark.parametrize("ar", list(S.ARITHS))
def test_backward_t1_checker(ar):
    """check_backward_t1 on the T = 1 stand-in: its own fp32 run passes; dx rounded where the path leaves it unrounded, and the
    reverse, fails on dx; a non-zero dw_hh fails."""
    quiet = lambda *_: None
    path = next(p for p in CPU_PATHS if p.path == "g16-full" and p.T == 1)
    ops = path.operands()
    fw = _standin_forward(path, ar, ops)
    for in16 in (False, True):
        rounding = dict(fwd=True, bwd16=True, in16=in16)
        good = S.backward_t1(path, ar, ops, fw, rounding, torch.float32, CPU)
        S.check_backward_t1(path, ar, ops, fw, good, rounding, log=quiet)
        bad = dict(good, dx=S.backward_t1(path, ar, ops, fw, dict(rounding, in16=not in16), torch.float32, CPU)["dx"])
        with pytest.raises(AssertionError, match="dx"):
            S.check_backward_t1(path, ar, ops, fw, bad, rounding, log=quiet)
        with pytest.raises(AssertionError, match="dw_hh0"):
            S.check_backward_t1(path, ar, ops, fw, dict(good, dw_hh0=good["dw_hh0"] + 1e-30), rounding, log=quiet)
