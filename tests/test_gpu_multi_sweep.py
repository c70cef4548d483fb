"""fsn_lstm2_forward_multi - up to eight two-layer H = 384 stacks as ONE launch of lstm2_group_multi_kernel - held to an fp64
recurrence over a sweep of its plans.  Needs an MI355X:
python -m pytest tests/test_gpu_multi_sweep.py -m gpu -s

The entry is called through fullsubnet_amd._lib directly with an array of _lib.Lstm2Stack, so that ldx, the workspace, the
stack order and the operands are the test's to choose.  TABLE has one named MRow per line; a row is a list of stacks (rows per
stack as a function of the CU count `c`: cap = c // 8 clusters of 64 rows, lo = ceil(3 cap / 4)), input widths from
(62, 68, 100, 180) and T = 9 unless the row says otherwise.  What the path adds over the single-stack group kernel is what
the rows are there for: the set lookup and the per-set rebasing of the flag groups, both workgroup-to-slot mappings, a partial
last cluster in every set (tiles that load a valid tile's rows and store nothing in the MIDDLE of the launch), one-tile sets,
n = 8 sets, the two thresholds of the host rule and its fallback.

Per stack everything test_gpu_recurrent_sweep.py (S) has is reused unchanged: an S.Row(entry="lstm2") with n_fixed,
S.make_operands (seeded per stack: two stacks of one shape do not share operands), S.reference, S.check_outputs, S.assert_stats,
S.yardstick_of, S.Out, S._padded, SENTINEL, GUARD, SHARP.  The rule is theirs: for each stack's hseq1 the relative Frobenius
error and max|err| / max|ref| against the torch fp64 recurrence, for the whole tensor, per step and per 16-row tile, each at
most SHARP = 4 x the same statistic of the CPU fp32 run that yardstick_of picks (torch's fp32; the fp32 emulation of
lstm_cell.h's formulas for at most 48 input columns).  Statistics are kept PER STACK and never pooled: a wrong 16-row stack
must not hide behind a 1500-row one.  Weights uniform +- gain / sqrt(H), gain 2 (6 on `gain6`).

Every row: the plan (fsn_lstm2_multi_is_persistent == plan_rule, the rule of include/fsn_hip.h written out in Python, == what
the row was written for); the launch count (persistent rows: fsn_debug_persist_stats shows launches + 1, waits unchanged,
unreported 0); fallback rows: each stack bit-identical to fsn_lstm2_forward for that stack alone; every hseq1 behind the NaN
sentinel with GUARD elements, guard intact, every declared element written and finite; the workspace exactly
fsn_lstm2_multi_workspace_bytes and 0xFF-filled; two calls in a row the same bits; ldx = round_up(I, 16) + 16 the same bits;
a clean stream status.  Zero-padded units (`h320-as-384`) are exactly 0.0.

Persistent rows, one launch each, exact:
1. stack order: the stacks reversed, and rotated by one, give every stack the same bits (the order only changes cluster0, the
   workgroup sets and the carve addresses);
2. tile position (`partial-each`): the inputs of the first 16-row tile and of the last tile (in the partial cluster) of every
   stack exchanged: the two output tiles come back exchanged bit for bit, every other tile unchanged;
3. weight sets (`threshold-lo`): three stacks of one shape on the SAME x, the first with its own weights, the other two with the
   same weights: the two are bit-identical, the first differs and is held to its own fp64 reference.

Refusals (test_multi_refusals): n = 0, n = 9, N = 24, H1 = 100, ldx = I = 62, hseq1 == NULL, a workspace one byte short
(FSN_ERR_WORKSPACE, on the fallback and on the persistent plan); the outputs' sentinels untouched.

Read on the way (csrc/lstm_group_kernels.hip, csrc/fsn_api_layers.hip), confirmed by the rows:
* a.flags is rebased by cluster0 and the cluster index is set-local, so group_body's fl0 / fl1 = a.flags + cluster * 2 GFS land on
  the launch's flag group cluster0 + cluster; a.status stays the launch's one word behind ALL flag groups
  (flags + clusters * 2 GFS), which is also the word fsn_launch_poison_if reads per stack.
* tile_ok / my_tile compare the set-local cluster * 64 + wave * 16 with the set's own Nrows; gx_tiles = N / 16 is the real tile
  count of the set and a missing tile reads tile `cluster * 4 + 0`, which exists whenever the cluster does.
* lstm2_multi_carve takes the 3 n recurrent matrices first (n x 3 x 4 H H floats = 14.2 MB at n = 8), then per stack W_ih0, the
  biases, gx and hseq0: no gx lies between two recurrent matrices, the largest offset from the lowest pointer is
  (3 n - 1) 4 H H = 13.6 M elements, far inside both the 32-bit offsets and the launcher's 0x1fffffff bound.
* The rule has a third condition the header did not name: T >= 4 (rows `T4` / `T3`); the header says so now.

Not covered: the 2 GB bound on T N 384 4 bytes of one stack's hidden sequence (lstm2_multi_clusters and the launcher both refuse
it; N is bounded by 64 cap = 2048 rows on the persistent plan, so T would have to exceed 682 and the fp64 reference minutes).
A device with fewer than 64 CUs (cap < 8: `tile-sets-first` has no room for its eighth stack).

Fixed on the way: nothing in the kernels or the host rule.  Every row passed on its first run, the three equalities included; the one
finding is the header's silence about T >= 4.

Seen on an MI355X (256 CUs: cap 32, lo 24), all 16 rows and the refusals, 10.3 s for the module (references 0.1 - 1.2 s per row, T33
keeps T = 33), every plan and launch-count assertion holding, all three equalities bit for bit.  Worst relative-Frobenius ratio hip /
yardstick over the row's stacks, whole tensor / worst block (the worst block is step 0 of an I = 62 / 68 stack throughout: one cell
update, where lstm_cell.h's tanh formula alone - the fp32 emulation - stands at 2 x torch's fp32):
threshold-lo 3.00 / 3.47; below-lo (stack by stack) 2.17 / 3.14; T4 3.17 / 3.49; T3 (stack by stack) 2.59 / 3.19; h320-as-384
3.09 / 3.76; mixed-hidden (stack by stack) 2.17 / 3.14; narrow-wide 2.20 / 2.28 (I = 1, 16, 17 held to the cell emulation); one-stack-
cap 2.68 / 2.91; above-cap (stack by stack) 2.19 / 3.19; linear-map 3.01 / 3.49; partial-each 2.99 / 3.48; gain6 1.59 / 1.69;
T33 2.90 / 3.48; tile-sets-first 2.95 / 3.47; tile-set-last 3.00 / 3.49; model-48k 3.01 / 3.49 (largest max-error ratio 3.86 x,
its 640-row stack).
"""
import ctypes
import math
import time

import pytest
import torch

import test_gpu_recurrent_sweep as S

pytestmark = pytest.mark.gpu

CUS = S.CUS
WIDTHS = (62, 68, 100, 180)
H = 384
GSETS = 8  # stacks per call at most
FSN_ERR_ARG, FSN_ERR_WORKSPACE = -1, -2


def cap_of(c):
    return c // 8


def lo_of(c):
    return -(-3 * cap_of(c) // 4)


def plan_rule(c, stacks, T):
    """include/fsn_hip.h on fsn_lstm2_forward_multi: one persistent launch when every stack has H0 = H1 = 384, T >= 4 and the
    stacks together fill 3/4 .. 1 x CUs / 8 clusters of 64 rows.  stacks: [(N, H0, H1)]."""
    cap = c // 8
    if cap < 1 or not 1 <= len(stacks) <= GSETS or T < 4:
        return False
    if any(h0 != 384 or h1 != 384 or n < 16 or n % 16 for n, h0, h1 in stacks):
        return False
    clusters = sum((n + 63) // 64 for n, _, _ in stacks)
    return 3 * cap <= 4 * clusters and clusters <= cap


def split(k, n):
    """k clusters over n stacks: n - 1 equal ones, the last takes what is left."""
    a = k // n
    return [a] * (n - 1) + [k - a * (n - 1)]


def _threshold(c):
    return [64 * p for p in split(lo_of(c), 4)]


def _below(c):
    n = _threshold(c)
    return n[:3] + [n[3] - 64]


def _partial(c):
    return [64 * (p - 1) + r for p, r in zip(split(lo_of(c), 4), (16, 32, 48, 16))]


def _linear(c):
    k = max(k for k in range(lo_of(c), cap_of(c) + 1) if k % 8)
    return [64 * p for p in split(k, 3)]


class MRow:
    """One line of the sweep.  stacks: CU count -> rows per stack; persistent: the plan the row was written for (a function of
    the CU count where the layout is the model's and not the device's); hreal / hidden: {stack: 320} - that stack's units
    320 .. 383 all-zero in every matrix and bias / that stack at H0 = H1 = 320."""

    def __init__(self, name, stacks, T=9, widths=WIDTHS, gain=2.0, persistent=True, hreal=None, hidden=None, n_cap=False):
        self.name, self.stacks, self.T, self.widths, self.gain = name, stacks, T, widths, gain
        self.persistent, self.hreal, self.hidden, self.n_cap = persistent, hreal or {}, hidden or {}, n_cap

    @property
    def id(self):
        return self.name

    def Ns(self, c=CUS):
        ns = list(self.stacks(c))
        if self.n_cap:  # the CPU self-test: one whole cluster at most, the partial cluster's residue kept
            ns = [min(n, 64 + n % 64 if n % 64 else 64) for n in ns]
        return ns

    def wants_persistent(self, c=CUS):
        return self.persistent(c) if callable(self.persistent) else self.persistent

    def hidden_of(self, k):
        return self.hidden.get(k, H)

    def shapes(self, c=CUS):
        return [(n, self.hidden_of(k), self.hidden_of(k)) for k, n in enumerate(self.Ns(c))]

    def stack_rows(self, c=CUS):
        """One S.Row per stack."""
        out = []
        for k, n in enumerate(self.Ns(c)):
            I = self.widths[k % len(self.widths)]
            r = S.Row(f"{self.name}/stack{k}", "multi", "lstm2", self.T, None, I, S.ru16(I), self.hidden_of(k), gain=self.gain,
                      Hreal=self.hreal.get(k))
            r.n_fixed = n
            out.append(r)
        return out

    def scaled(self, t_max=12):
        return MRow(self.name, self.stacks, min(self.T, t_max), self.widths, self.gain, self.persistent, self.hreal, self.hidden,
                    n_cap=True)


TABLE = [
    MRow("threshold-lo", _threshold),                                       # the lower threshold, inclusive; all N % 64 == 0
    MRow("below-lo", _below, persistent=False),                             # one cluster fewer: stack by stack
    MRow("T4", _threshold, T=4),                                            # the shortest persistent length
    MRow("T3", _threshold, T=3, persistent=False),
    MRow("h320-as-384", _threshold, hreal={1: 320}),                        # padded units exactly 0.0 in that stack
    MRow("mixed-hidden", _threshold, hidden={1: 320}, persistent=False),    # one H = 320 stack: the whole call falls back
    MRow("narrow-wide", _threshold, widths=(1, 16, 17, 257)),               # Ipad = 16 / 16 / 32 / 272 projection GEMMs
    MRow("one-stack-cap", lambda c: [64 * cap_of(c)], widths=(100,)),       # clusters == cap; the XCD mapping on 256 CUs
    MRow("above-cap", lambda c: [64 * p for p in split(cap_of(c) + 1, 4)], persistent=False),
    MRow("linear-map", _linear),                                            # clusters % 8 != 0: the linear slot mapping
    MRow("partial-each", _partial),                                         # N % 64 = 16, 32, 48, 16: first, middle, last set
    MRow("gain6", _partial, gain=6.0),                                      # saturating gates
    MRow("T33", _partial, T=33),                                            # more steps than any buffer depth or parity
    MRow("tile-sets-first", lambda c: [16] * 7 + [64 * (cap_of(c) - 7)]),   # one-tile clusters, n = 8 = GSETS
    MRow("tile-set-last", lambda c: [64 * (lo_of(c) - 1) + 32, 16]),        # a one-tile set as the final cluster
    MRow("model-48k", lambda c: [S.ru16(32 * u) for u in (20, 25, 6, 4)],   # Improved FullSubNet's sections at 48 kHz, B = 32
         persistent=lambda c: lo_of(c) <= 28 <= cap_of(c)),
]
NAMES = ("one-stack-cap", "threshold-lo", "below-lo", "above-cap", "linear-map", "partial-each", "tile-sets-first", "tile-set-last",
         "model-48k", "T4", "T3", "T33", "narrow-wide", "gain6", "h320-as-384", "mixed-hidden")


# ---- operands and references, per stack --------------------------------------------------------------------------------

def stack_operands(r, k, variant=0):
    """S.make_operands for stack k (a seed of its own per stack and variant); a zero-padded stack has BOTH layers' units beyond
    Hreal zero - S.make_operands pads layer 0 only - so that they are exactly 0.0 in hseq1."""
    ops = S.make_operands(r, r.N(), 101 * (k + 1) + 10007 * variant)
    if r.Hreal < r.H:
        for t in ops["layers"][1]:
            t.view(4, r.H1, -1)[:, r.Hreal:] = 0
        ops["layers"][1][1][:, r.Hreal:] = 0
    return ops


_REFS = {}  # (stack shape, seed) -> (ops, fp64, torch fp32, cell fp32): the threshold-lo family shares most of its stacks


def stack_case(r, k, variant=0, x=None):
    key = (r.T, r.N(), r.I, r.H, r.H1, r.Hreal, r.gain, k, variant)
    if key not in _REFS:
        ops = stack_operands(r, k, variant)
        if x is not None:
            ops["x"] = x
        refs = tuple(S.reference(r, ops, dt, act=act) for dt, act in
                     ((torch.float64, "torch"), (torch.float32, "torch"), (torch.float32, "cell")))
        while len(_REFS) >= 8:
            _REFS.pop(next(iter(_REFS)))
        _REFS[key] = (ops,) + refs
    return _REFS[key]


def check_stack(r, ops, refs, y, log=print):
    """One stack's hseq1 (a CPU tensor) under the recurrent sweep's rule; returns its worst hip / yardstick Frobenius ratio
    (whole tensor, and over the blocks)."""
    stats = {}
    S.check_outputs(stats, r, ops, {"y": y}, cpu32=refs[1], ref64=refs[0], emu32=refs[2])
    S.assert_stats(r, stats, log=(lambda s: log(s.replace("[rsweep]", "[msweep]"))) if log else (lambda s: None))
    s, col = stats["y"], 1 if S.yardstick_of(r, "y") == "torch" else 6
    ratio = lambda a: math.sqrt(a[0] / a[col]) if a[col] > 0 else (0.0 if a[0] == 0 else float("inf"))
    return ratio(s.acc["all"]), max(ratio(a) for a in s.acc.values())


# ---- the device side ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return fullsubnet_amd


class Stacks:
    """The stacks of one call on the device.  run(): fsn_lstm2_forward_multi on them in `order`, every hseq1 behind its
    sentinel, the workspace exactly the query's size and 0xFF-filled; returns the hseq1 tensors (device) in the table's order."""

    def __init__(self, fsn, rows, ops):
        self.lib, self.L, self.rows = fsn._lib, fsn._lib.lib(), rows
        self.dev = torch.device("cuda:0")
        self.x = [o["x"].to(self.dev) for o in ops]
        self.w = [[p.to(self.dev).contiguous() for lp in o["layers"] for p in lp] for o in ops]
        self.st = self.lib.stream_ptr(self.dev)
        self.T = rows[0].T

    def fill(self, order, ldx_extra, xs, outs):
        arr = (self.lib.Lstm2Stack * max(len(order), 1))()
        keep = []
        for q, k in zip(arr, order):
            r = self.rows[k]
            ldx = r.ldx + ldx_extra
            x = S._padded(self.x[k] if xs is None else xs[k], ldx)
            keep.append(x)
            q.x, q.ldx = x.data_ptr(), ldx
            for name, t in zip(("w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1"), self.w[k]):
                setattr(q, name, self.lib.dev_ptr(t, name).value)
            q.N, q.I, q.H0, q.H1 = r.N(), r.I, r.H, r.H1
            q.hseq1 = outs[k].f.data_ptr() if outs else None
        return arr, keep

    def outs(self):
        return [S.Out(self.dev, (self.T, r.N(), r.H1)) for r in self.rows]

    def run(self, order=None, ldx_extra=0, xs=None):
        order = list(range(len(self.rows))) if order is None else order
        outs = self.outs()
        arr, keep = self.fill(order, ldx_extra, xs, outs)
        n = len(order)
        ws = self.lib.workspace(self.L.fsn_lstm2_multi_workspace_bytes(n, ctypes.byref(arr), self.T), self.dev).fill_(0xFF)
        self.lib.check(self.L.fsn_lstm2_forward_multi(n, ctypes.byref(arr), self.T, ws.data_ptr(), ws.numel(), self.st))
        got = [o.take(f"hseq1 of stack {k}") for k, o in enumerate(outs)]
        self.lib.check_canaries()
        del keep
        return got

    def is_persistent(self):
        arr, _ = self.fill(list(range(len(self.rows))), 0, None, None)
        return self.L.fsn_lstm2_multi_is_persistent(len(self.rows), ctypes.byref(arr), self.T)

    def alone(self, k):
        """fsn_lstm2_forward for stack k on the same operands."""
        r, p = self.rows[k], self.lib.dev_ptr
        y = S.Out(self.dev, (self.T, r.N(), r.H1))
        ws = self.lib.workspace(self.L.fsn_lstm2_fwd_workspace_bytes(self.T, r.N(), r.I, r.H, r.H1), self.dev).fill_(0xFF)
        x = S._padded(self.x[k], r.ldx)
        self.lib.check(self.L.fsn_lstm2_forward(p(x), r.ldx, *[p(t) for t in self.w[k]], self.T, r.N(), r.I, r.H, r.H1, p(y.f),
                                                ws.data_ptr(), ws.numel(), self.st))
        return y.take(f"hseq1 of stack {k} alone")


def _same(a, b, what):
    for k, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), f"stack {k}: {what}: not bit-identical"


@pytest.mark.parametrize("row", TABLE, ids=[r.id for r in TABLE])
def test_multi_sweep(fsn, row):
    t0 = time.time()
    lib = fsn._lib
    c = torch.cuda.get_device_properties(0).multi_processor_count
    assert c >= 64, f"{c} CUs: the table needs cap = CUs / 8 >= 8"
    rows = row.stack_rows(c)
    n = len(rows)
    assert 1 <= n <= GSETS and all(r.N() % 16 == 0 and r.N() >= 16 for r in rows)
    cases = [stack_case(r, k) for k, r in enumerate(rows)]
    t_ref = time.time() - t0
    d = Stacks(fsn, rows, [cs[0] for cs in cases])
    # the plan
    want = plan_rule(c, row.shapes(c), row.T)
    assert want == row.wants_persistent(c), f"{row.id}: written for persistent = {row.wants_persistent(c)}, the rule on {c} CUs says {want}"
    plan = d.is_persistent()
    assert plan == int(want), f"{row.id}: fsn_lstm2_multi_is_persistent = {plan}, the header's rule says {int(want)}"
    # the call and its launch count
    before = lib.persist_stats()
    got = d.run()
    after = lib.persist_stats()
    if want:
        assert (after[0] - before[0], after[1] - before[1], after[2]) == (1, 0, 0), \
            f"{row.id}: persistent launches / waits / unreported {before} -> {after}, expected one launch more and nothing else"
    else:
        b1 = lib.persist_stats()
        alone = [d.alone(k) for k in range(n)]
        a1 = lib.persist_stats()
        _same(got, alone, "the fallback against fsn_lstm2_forward for that stack alone")
        assert (after[0] - before[0], after[2]) == (a1[0] - b1[0], 0), f"{row.id}: the fallback's persistent launches {before} -> {after}"
    _same(d.run(), got, "two calls in a row")
    _same(d.run(ldx_extra=16), got, "ldx = round_up(I, 16) + 16")
    if want:
        _same(d.run(order=list(reversed(range(n)))), got, "the stacks in reversed order")
        if n > 2:  # (with two stacks the rotation IS the reversal)
            _same(d.run(order=list(range(1, n)) + [0]), got, "the stacks rotated by one")
        if row.name == "partial-each":
            xs = []
            for x in d.x:
                x2 = x.clone()
                x2[:, :16], x2[:, -16:] = x[:, -16:], x[:, :16]
                xs.append(x2)
            sw = d.run(xs=xs)
            for k, (u, v) in enumerate(zip(sw, got)):
                assert torch.equal(u[:, :16], v[:, -16:]) and torch.equal(u[:, -16:], v[:, :16]), \
                    f"stack {k}: first and last 16-row tile exchanged on the input: the output tiles are not the exchanged bits"
                assert torch.equal(u[:, 16:-16], v[:, 16:-16]), f"stack {k}: exchanging the first and last tile changed another tile"
    assert lib.stream_status(d.dev, synchronize=True) == (0, 0), "the stream carries a timeout record"
    host = [g.cpu() for g in got]
    worst = []
    for k, (r, cs, y) in enumerate(zip(rows, cases, host)):
        if r.Hreal < r.H:
            assert bool((y[..., r.Hreal:] == 0).all()), f"stack {k}: zero-padded units are not exactly 0.0 in hseq1"
        worst.append(check_stack(r, cs[0], cs[1:], y))
    if want and row.name == "threshold-lo":
        _weight_sets(fsn, row, rows, cases, got)
    print(f"[msweep] {row.id}: stacks N {[r.N() for r in rows]} I {[r.I for r in rows]} T {row.T} persistent {int(want)}: worst hip / "
          f"yardstick whole {max(w[0] for w in worst):.2f} x, block {max(w[1] for w in worst):.2f} x; references {t_ref:.1f} s, "
          f"row {time.time() - t0:.1f} s")


def _weight_sets(fsn, row, rows, cases, got):
    """Equality 3: stacks 0, 1, 2 (one shape) on stack 1's x; stack 0 with weights of its own, stacks 1 and 2 with stack 1's."""
    assert rows[0].N() == rows[1].N() == rows[2].N()
    r = rows[1]
    ops1 = cases[1][0]
    own = stack_case(r, 1, variant=1, x=ops1["x"])
    d = Stacks(fsn, [r, r, r] + rows[3:], [own[0], ops1, ops1] + [cs[0] for cs in cases[3:]])
    out = d.run()
    assert torch.equal(out[1], out[2]), "two stacks with the same weights and x: not bit-identical"
    assert torch.equal(out[1], got[1]), "stack 1: its bits depend on its neighbour's weights and x"
    assert not torch.equal(out[0], out[1]), "two stacks with different weights on the same x gave the same bits"
    _same(out[3:], got[3:], "the stacks behind the exchanged ones")
    check_stack(r, own[0], own[1:], out[0].cpu())
    assert fsn._lib.stream_status(d.dev, synchronize=True) == (0, 0)


# ---- refusals -------------------------------------------------------------------------------------------------------------

def _untouched(outs, what):
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert bool((o.buf == S.SENTINEL).all()), f"{what}: the refused call wrote to hseq1 of stack {k}"


def test_multi_refusals(fsn):
    lib, L = fsn._lib, fsn._lib.lib()
    T = 4
    small = MRow("refusals", lambda c: [16, 32, 16, 48, 16, 16, 32, 16, 16], T=T)  # nine stacks: n = 9 has its array
    rows = small.stack_rows()
    d = Stacks(fsn, rows, [stack_operands(r, k) for k, r in enumerate(rows)])
    ws = lib.workspace(64 << 20, d.dev)  # more than any of these calls could ask for: a refusal is never the workspace's

    def refused(n, edit, what, rc_want=FSN_ERR_ARG, nbytes=None, query_zero=True):
        outs = d.outs()
        arr, keep = d.fill(list(range(min(max(n, 1), 9))), 0, None, outs)
        edit(arr)
        if query_zero:
            assert L.fsn_lstm2_multi_workspace_bytes(n, ctypes.byref(arr), T) == 0, f"{what}: the workspace query accepted it"
        rc = L.fsn_lstm2_forward_multi(n, ctypes.byref(arr), T, ws.data_ptr(), ws.numel() if nbytes is None else nbytes, d.st)
        assert rc == rc_want, f"{what}: returned {rc}, expected {rc_want}"
        _untouched(outs, what)

    refused(0, lambda a: None, "n = 0")
    refused(9, lambda a: None, "n = 9")
    refused(2, lambda a: setattr(a[1], "N", 24), "N = 24")
    refused(2, lambda a: setattr(a[1], "H1", 100), "H1 = 100")
    assert rows[0].I == 62
    refused(2, lambda a: setattr(a[0], "ldx", 62), "ldx = I = 62")
    refused(2, lambda a: setattr(a[1], "hseq1", None), "hseq1 == NULL", query_zero=False)
    arr, keep = d.fill([0, 1], 0, None, d.outs())
    need = L.fsn_lstm2_multi_workspace_bytes(2, ctypes.byref(arr), T)
    assert 0 < need <= ws.numel()
    refused(2, lambda a: None, "a workspace one byte short (stack by stack)", FSN_ERR_WORKSPACE, need - 1, query_zero=False)
    # ... and on the persistent plan
    c = torch.cuda.get_device_properties(0).multi_processor_count
    big = MRow("refusals-persistent", _threshold, T=T)
    rows = big.stack_rows(c)
    d = Stacks(fsn, rows, [stack_operands(r, k) for k, r in enumerate(rows)])
    assert d.is_persistent() == 1
    outs = d.outs()
    arr, keep = d.fill(list(range(len(rows))), 0, None, outs)
    need = L.fsn_lstm2_multi_workspace_bytes(len(rows), ctypes.byref(arr), T)
    ws = lib.workspace(need, d.dev)
    before = lib.persist_stats()[0]
    rc = L.fsn_lstm2_forward_multi(len(rows), ctypes.byref(arr), T, ws.data_ptr(), need - 1, d.st)
    assert rc == FSN_ERR_WORKSPACE, f"a workspace one byte short (persistent): returned {rc}"
    assert lib.persist_stats()[0] == before
    _untouched(outs, "a workspace one byte short (persistent)")
    assert lib.stream_status(d.dev, synchronize=True) == (0, 0)
