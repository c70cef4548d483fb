"""The fused inference call held to an fp64 model on every plan its host code can take.  Needs an MI355X:
python -m pytest tests/test_gpu_core_sweep.py -m gpu -s

fsn_fullsubnet_forward, fsn_fullsubnet_forward_rows and fsn_fullsubnet_fullband (csrc/fsn_api_fullsubnet.hip: core_dims, run_core,
run_recurrence, core_chunks) pick their kernels from the shape alone: the per-step wavefront, the group kernel with one or two
clusters per workgroup set, the step regime without it, the persistent pair at 1 - 5 row tiles per workgroup with or without
left-over tiles, the fused output layer, lstm_rec_in / lstm_rec_x or the lstm_rec<XIN> fallback, whole rounds with a padded
tile, several rounds, batch chunking.  TABLE has one Row per line, named after the path it is there for; the entries are called
through fullsubnet_amd._lib directly, so the workspace, the guards and the row range are the test's to choose.

The plan is asserted FIRST, as literals written for 256 CUs and 32 group slots (the MI355X; another CU count fails the test
with that message): fsn_debug_core_call_plan reports the CoreDims of every core call the row makes (each chunk of
fsn_debug_core_chunks for `forward`, the row slice for `rows`) - tiles, row tiles per workgroup, workgroups, left-over tiles,
clusters and tiles beside the group launch, the split of run_recurrence's step rows, chain, fused output layer, lstm_rec_x,
input chunks.  After the call fsn_debug_core_last_launches must name exactly the launchers that plan implies (launches_of: the
kernels that RAN, not only the plan that was predicted) and fsn_debug_persist_stats must have grown by the plan's persistent
launches (chain + group, per core call).  A row whose plan does not hold on the device fails.

Reference: the model written out on the CPU in fp64 - oracle/fullsubnet_oracle.py for the padding, the norms and freq_unfold,
lstm_layer of tests/test_gpu_recurrent_sweep.py for the four LSTM layers; it agrees with O.fullsubnet_forward(dtype=float64) to
1e-14 (tests/test_core_sweep_cpu.py).  Inputs: |N(0, 1)| + 0.05 magnitudes, O.make_params(gain, mask_gain=24).  The model has no
cross-utterance term, so a batch is k distinct base utterances repeated, b -> base[b % k], and EVERY row of the batch is held to
fp64 at the cost of k utterances: k the smallest odd number >= 3 with ceil(B / k) <= 16.  Two asserted conditions make a mix-up of
rows visible: no two copies of one utterance lie a whole number of 16-row tiles apart inside one core call ((j k F) % 16 != 0 for
0 < j < B / k), and no chunk offset is a multiple of k.  `fullband` rows use B distinct utterances.

Yardstick, computed in the same run: the same model in fp32 on the CPU.  The mask is a hidden output behind a 32-column input
(the yardstick_of rule of the recurrent sweep), so it is held to the run with lstm_cell.h's activation formulas (act="cell");
fb_output to the run with torch's activations.  The ratio of the two fp32 runs is printed with every figure.  Statistics
against fp64: the relative Frobenius error and max|err| / max|ref|.  Asserted, stat_hip <= SHARP x stat_yardstick with SHARP = 4:
both statistics of the whole tensor; the Frobenius one per frame, per region of the plan (main / left-over rows, cluster / aux
rows, cu / small-step rows) of every core call, per chunk; and per 16-row tile of every core call's local rows against 4 x the
yardstick's WORST tile of that call (the precedent of the 16-bit sweep).  tests/test_core_sweep_cpu.py runs this checker on the
CPU with torch's fp32 and with deliberately wrong stand-ins.

In every row besides: outputs behind the NaN sentinel with GUARD elements that must survive, every declared element written;
the workspace exactly the queried size and filled with 0xFF; two calls bit-identical; the stream status clean.  A row range
aligned to utterances is bit-equal to `forward` on those utterances where `forward` does not chunk
(test_aligned_row_range_equals_forward).

What `forward` cannot reach: the cost model of core_chunks splits 17 / 33 / 49 utterances as 9 + 8 / 32 + 1 / 48 + 1 and
core_chunk splits everything above 64, so the general whole-round plans (137 x 2, 177 x 3, 197 x 4), RT 5 and the multi-round
plans are reached through `rows` only - over the whole batch where the issue names a batch size.

Fixed on the way: with a device at hand fsn_debug_core_chunks gave 17 utterances as [8, 9] - the remainder search of
core_chunks_search puts the round size it picked before what is left - where its contract and
tests/test_host_cpu.py::test_batches_are_covered_exactly_by_the_chunks_they_run_as (which passes without a device, where the group
kernel's plans do not exist) say largest first.  The remainder's calls are now sorted: [9, 8].  Nothing computes differently
within a call; utterance 8 of such a batch now runs in the first call.

Seen on an MI355X (256 CUs), all 91 rows and the three bit-equality cases, 8 s, every plan, launch-trace and persistent-launch
assertion holding as first written; no row above the margin, no bug found (the wholly padded tile, den_stride under row ranges,
RT 5 and the seven-round RT 1 plan - the candidates by reading - are all inside 1.7 x).  Worst hip / yardstick ratio of the
relative Frobenius error per output and path (max-error ratio in brackets where it is the larger):
mask - wavefront 1.30 x (1.86 x on range-across-boundary), at F = 65 1.56 x (1.88 x); group kernel, one cluster per set 1.46 x
(1.71 x); two per set 1.46 x (1.55 x); step regime without the group kernel 1.66 x (1.77 x); one tile per workgroup 1.67 x, at
F = 65 and look-ahead 3 1.78 x (2.57 x, the largest of the module); one tile + left-over tiles 1.67 x; whole rounds with the
padded tile 1.48 x; RT 2 - 4 on lstm_rec_in / lstm_rec_x 1.50 x (1.56 x), with the lstm_rec<XIN> fallback 1.52 x (1.60 x); RT 5
1.46 x (1.62 x); several rounds 1.42 x at RT 3, 1.61 x (1.68 x) at seven rounds of RT 1, 1.48 x at RT 4 + 8; chunked forward 1.47 x
(1.73 x), 1.65 x at 16 input columns; row ranges off 0 1.19 - 1.61 x under both norms.  Worst 16-row tile against the yardstick's
worst tile: 2.37 x (rt3-rounds, look-ahead 3), 2.12 x (rt1-first at 16 input columns), else <= 1.8 x.  The cell emulation
itself stands at 1.07 - 2.1 x torch's fp32 on the mask from 6 steps on, at 2.98 x in the single-step rows and 5.21 x in the
single-step row with 2 input columns (the tanh term of the recurrent sweep's yardstick_of); the device is 1.04 - 1.13 x the
emulation there.
fb_output (against torch's fp32) - chain kernel at H = 512: 1.61 - 1.92 x (2.03 x at 64 utterances) over its three shapes; at
H = 384 1.60 - 1.79 x; wavefront fallback 1.54 x (2.36 x) at 65 utterances, 1.38 - 1.50 x at H = 256.
"""
import ctypes
import functools
import math
import time

import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O
from test_gpu_recurrent_sweep import ACTS, GUARD, SENTINEL, SHARP, Out, lstm_layer  # noqa: F401 (ACTS: the `act` names of lstm_layer;
#                                                                    GUARD / SENTINEL: what Out puts behind every output)

pytestmark = pytest.mark.gpu

CUS = 256    # the literals of TABLE are written for the MI355X: 256 CUs ...
SLOTS = 32   # ... and one group-kernel workgroup set per eight of them
NORMS = {"offline": "offline_laplace_norm", "cumulative": "cumulative_laplace_norm"}


def ru16(n):
    return (n + 15) // 16 * 16


# ---- expected plans ---------------------------------------------------------------------------------------------------

def P(tiles, rt, main, left, grp=0, aux=0, cu=None, st=None):
    """The literal part of one core call's expected plan.  tiles: 16-row tiles (padding tiles of whole rounds included); rt /
    main / left: row tiles per workgroup, workgroups and left-over tiles of the persistent pair (main = 0: no persistent part,
    all tiles `left`); grp / aux: clusters of the group kernel and tiles beside it; cu / st: tiles on lstm_step_cu / lstm_step
    inside run_recurrence (default: the left-over tiles beside a persistent part go to lstm_step)."""
    regime = "group" if grp else "wavefront" if main == 0 and left < 96 else "persistent"
    if cu is None:
        cu, st = (0, left) if regime == "persistent" and main > 0 else (0, 0)
    assert regime != "persistent" or main > 0 or cu + st == left
    return dict(tiles=tiles, npad=16 * tiles, rt=rt, main_wgs=main, left_tiles=left, grp_clusters=grp, grp_aux_tiles=aux,
                cu_tiles=cu, aux_tiles=st, fc_fused=int(main > 0 and rt >= 2), l1x=int(main > 0 and 2 <= rt <= 4), regime=regime)


def G(tiles, clusters, aux):  # the group kernel: `clusters` of 64 rows + `aux` tiles beside them
    assert 4 * clusters + aux == tiles
    return P(tiles, 1, 0, tiles, grp=clusters, aux=aux)


def S(tiles, cu, st):  # the step regime without the group kernel: lstm_step_cu on `cu` tiles, lstm_step on `st` beside it
    return P(tiles, 1, 0, tiles, cu=cu, st=st)


# one core call of b whole utterances at F = 257 (what a chunk of `forward` runs), with / without the group kernel's shape
CALL = {1: P(17, 1, 0, 17), 2: P(33, 1, 0, 33), 5: P(81, 1, 0, 81), 6: G(97, 24, 1), 8: G(129, 32, 1), 9: G(145, 32, 17),
        16: G(257, 64, 1), 32: P(514, 2, 256, 2), 48: P(771, 3, 256, 3), 64: P(1028, 4, 256, 4)}
CALL_NOGRP = {**CALL, 6: S(97, 96, 1), 7: S(113, 112, 1), 8: S(129, 128, 1), 16: P(257, 1, 256, 1)}


class Row:
    """One line of the sweep.  entry "forward": B utterances, `chunks` the expected core calls (default: one), each with the
    plan CALL[b] unless `plan` gives them; "rows": N sub-band rows from global row `begin` of a batch of `batch` utterances
    (default: the utterances the range touches), plan a P; "fullband": B distinct utterances."""

    def __init__(self, path, entry, B=None, N=None, begin=0, batch=None, plan=None, chunks=None, nb=15, T=4, la=2, F=257, Hf=512,
                 norm="offline", gain=2.0, k=None):
        self.path, self.entry, self.nb, self.T, self.la, self.F, self.Hf, self.norm, self.gain = path, entry, nb, T, la, F, Hf, norm, gain
        self.begin, self.N = begin, N
        if entry == "rows":
            self.B = batch or -(-(begin + N) // F)
            self.plans = [plan]
        else:
            self.B = B
            self.chunks = chunks or [B]
            assert sum(self.chunks) == B
            table = CALL if ru16(2 * nb + 2) == 32 else CALL_NOGRP
            self.plans = [None] if entry == "fullband" else [plan] if plan else [table.get(b) for b in self.chunks]
        self.k = B if entry == "fullband" else k or base_count(self.B)  # k given: where a chunk offset would be a multiple of it

    @property
    def Tp(self):
        return self.T + self.la

    @property
    def id(self):
        what = f"N{self.N}" + (f"@{self.begin}of{self.B}" if self.begin or self.B * self.F != self.N else "") if self.entry == "rows" \
            else f"B{self.B}"
        return f"{self.path}-{self.entry}-{what}-T{self.T}+{self.la}" + (f"-nb{self.nb}" if self.nb != 15 else "") + \
            (f"-F{self.F}" if self.F != 257 else "") + (f"-Hf{self.Hf}" if self.Hf != 512 else "") + \
            ("-cum" if self.norm == "cumulative" else "") + (f"-g{self.gain:g}" if self.gain != 2.0 else "")

    def cfg(self, lib):
        return lib.Cfg(self.F, self.la, self.nb, self.Hf, 384, lib.NORM_TYPES[NORMS[self.norm]], 0)

    def calls(self, chunks=None):
        """(first utterance, utterances, first local row r0, rows n, first GLOBAL row) of every core call."""
        if self.entry == "rows":
            b_lo = self.begin // self.F
            Bs = (self.begin + self.N - 1) // self.F - b_lo + 1
            return [(b_lo, Bs, self.begin - b_lo * self.F, self.N, self.begin)]
        out, b0 = [], 0
        for b in (self.chunks if chunks is None else chunks):
            out.append((b0, b, 0, b * self.F, b0 * self.F))
            b0 += b
        return out


def base_count(B):
    """Distinct base utterances of a batch of B: the smallest odd k >= 3 with ceil(B / k) <= 16."""
    k = 3
    while -(-B // k) > 16:
        k += 2
    return k


def check_duplication(row, calls):
    """The two conditions under which b -> base[b % k] cannot hide a mix-up of rows (module docstring)."""
    k, F = row.k, row.F
    for j in range(1, -(-row.B // k)):
        assert (j * k * F) % 16 != 0, f"{row.id}: copies {j} periods apart lie a whole number of row tiles apart"
    for b_lo, _, _, _, _ in calls[1:]:
        assert b_lo % k != 0, f"{row.id}: the core call at utterance {b_lo} starts at a multiple of k = {k}"


def _table():
    rows = []
    add = rows.append
    R = lambda path, **kw: add(Row(path, "rows", **kw))      # noqa: E731
    W = lambda path, B, **kw: add(Row(path, "forward", B=B, **kw))  # noqa: E731 (whole utterances)
    FB = lambda path, B, **kw: add(Row(path, "fullband", B=B, **kw))  # noqa: E731
    # ---- the two-layer wavefront of per-step launches: fewer than 96 row tiles ----
    W("wavefront", 1)
    W("wavefront", 5)
    R("wavefront-last", N=1520, plan=P(95, 1, 0, 95))
    W("wavefront", 1, T=1, la=0)
    W("wavefront", 2, norm="cumulative", T=5)
    W("wavefront", 5, la=3, gain=6.0)
    W("wavefront-F65", 4, F=65, plan=P(17, 1, 0, 17))
    # ---- the group kernel, one cluster per workgroup set: 96 - 159 tiles ----
    R("group1-first-noaux", N=1536, plan=G(96, 24, 0))
    W("group1", 6)
    W("group1", 9)
    R("group1-last", N=2544, plan=G(159, 32, 31))
    W("group1", 6, T=1, la=0)
    W("group1", 6, norm="cumulative", T=5, gain=6.0)
    W("group1", 9, la=3)
    W("group1-F161", 10, F=161, plan=G(101, 25, 1))
    # ---- the step regime without the group kernel (another input width): lstm_step_cu + lstm_step beside it ----
    W("step-nogroup", 6, nb=7)
    W("step-nogroup", 8, nb=7, norm="cumulative", T=5)
    W("step-nogroup-k64", 7, nb=31)
    W("step-nogroup-k2", 6, nb=0, T=1, la=0)
    # ---- persistent, one tile per workgroup, no left-over: projection GEMM, lstm_rec<XIN> at RT 1, no fused output layer ----
    R("rt1-first", N=2545, plan=P(160, 1, 160, 0))
    R("rt1-last", N=3568, plan=P(223, 1, 223, 0))
    R("rt1-first", N=2545, nb=7, plan=P(160, 1, 160, 0))
    R("rt1-last", N=3568, nb=7, plan=P(223, 1, 223, 0), norm="cumulative", T=5)
    R("rt1-F65", N=40 * 65, F=65, plan=P(163, 1, 163, 0), la=3)
    # ---- the group kernel, two clusters per workgroup set: 224 - 264 tiles ----
    R("group2-first", N=3569, plan=G(224, 56, 0))
    W("group2", 16)
    R("group2-last", N=4224, plan=G(264, 64, 8))
    W("group2", 16, T=1, la=0)
    W("group2", 16, norm="cumulative", T=5)
    R("group2-first", N=3569, gain=6.0, la=3, plan=G(224, 56, 0))
    # ---- one tile per workgroup on every CU + left-over tiles ----
    R("rt1-left9", N=4225, plan=P(265, 1, 256, 9))
    R("rt1-left16", N=4352, plan=P(272, 1, 256, 16))
    W("rt1-left1", 16, nb=7)
    R("rt1-left9", N=4225, norm="cumulative", T=5, gain=6.0, plan=P(265, 1, 256, 9))
    R("rt1-left16", N=4352, T=1, la=0, plan=P(272, 1, 256, 16))
    # ---- whole rounds with a wholly padded tile: 273 tiles run as 137 x 2 = 274, rows 4368 .. 4383 are all padding ----
    R("rounds-padded-tile", N=4353, plan=P(274, 2, 137, 0))
    R("rounds-padded-tile", N=4353, norm="cumulative", T=5, plan=P(274, 2, 137, 0))
    # ---- RT 2 / 3 / 4: lstm_rec_in + lstm_rec_x with the fused output layer ----
    R("rt2-rounds", N=17 * 257, plan=P(274, 2, 137, 0))  # 17 utterances whole (`forward` runs them as 8 + 9)
    W("rt2-left2", 32)
    R("rt3-rounds", N=33 * 257, plan=P(531, 3, 177, 0))  # 33 whole (`forward`: 32 + 1)
    W("rt3-left3", 48)
    R("rt4-rounds", N=49 * 257, plan=P(788, 4, 197, 0))  # 49 whole (`forward`: 48 + 1)
    W("rt4-left4", 64)
    R("rt2-left16", N=8448, plan=P(528, 2, 256, 16))
    R("rt4-left16-nochain", N=16640, plan=P(1040, 4, 256, 16))  # 65 utterances: the full-band stage is off the chain
    R("rt2-rounds", N=17 * 257, T=1, la=0, plan=P(274, 2, 137, 0))
    R("rt2-rounds", N=17 * 257, norm="cumulative", T=5, gain=6.0, plan=P(274, 2, 137, 0))
    R("rt3-rounds", N=33 * 257, la=3, plan=P(531, 3, 177, 0))
    R("rt2-F161", N=28 * 161, F=161, plan=P(282, 2, 141, 0))
    # ... at 16 input columns lstm_rec_in refuses and layer 0 falls back to lstm_rec<XIN>
    R("rt2-xin-fallback", N=17 * 257, nb=7, plan=P(274, 2, 137, 0))
    R("rt3-xin-fallback", N=33 * 257, nb=7, plan=P(531, 3, 177, 0))
    R("rt4-xin-fallback", N=49 * 257, nb=7, plan=P(788, 4, 197, 0), norm="cumulative")
    # ---- RT 5: no lstm_rec_x - the layer-1 GEMM + lstm_rec with the fused output layer ----
    R("rt5-rounds", N=16641, plan=P(1045, 5, 209, 0))
    R("rt5-left1", N=20481, plan=P(1281, 5, 256, 1))
    R("rt5-rounds", N=16641, norm="cumulative", T=5, plan=P(1045, 5, 209, 0))
    # ---- several rounds ----
    R("rounds-rt3", N=20737, plan=P(1299, 3, 433, 0))
    R("rounds-rt1x7", N=25000, plan=P(1563, 1, 1563, 0))
    R("rounds-rt4-left8", N=32896, plan=P(2056, 4, 512, 8))
    # ---- chunked forward ----
    W("chunked", 10, chunks=[8, 2])
    W("chunked", 17, chunks=[9, 8], k=5)  # largest first (fixed on the way); k = 3 would put the second call at a multiple of k
    W("chunked", 24, chunks=[16, 8])
    W("chunked", 33, chunks=[32, 1])
    W("chunked", 40, chunks=[32, 8])
    W("chunked", 49, chunks=[48, 1], norm="cumulative")
    W("chunked", 72, chunks=[64, 8])
    W("chunked", 104, chunks=[64, 32, 8])
    W("chunked", 128, chunks=[64, 64], T=4)
    W("chunked", 17, chunks=[16, 1], nb=7)
    # ---- row ranges that do not start at 0 (the cumulative divisors are indexed by GLOBAL row with den_stride) ----
    for norm in ("offline", "cumulative"):
        R("range-inside-utterance", N=100, begin=257 + 5, batch=3, norm=norm, plan=P(7, 1, 0, 7))
        R("range-across-boundary", N=354, begin=257 + 200, batch=4, norm=norm, plan=P(23, 1, 0, 23))
        R("range-group", N=1536, begin=100, batch=8, norm=norm, plan=G(96, 24, 0))
        R("range-rt1-left9", N=4230, begin=300, batch=20, norm=norm, plan=P(265, 1, 256, 9))
        R("range-rt2-rounds", N=4500, begin=300, batch=20, norm=norm, plan=P(282, 2, 141, 0))
    # ---- the full-band stage on its own output: the chain's three shapes, its other width, the wavefront fallback ----
    for B in (1, 16, 17, 32, 33, 64, 65):
        FB("fullband-chain" if B <= 64 else "fullband-wavefront", B)
    FB("fullband-chain-h384", 17, Hf=384, norm="cumulative")
    FB("fullband-chain-h384", 64, Hf=384, F=161)
    FB("fullband-wavefront-h256", 16, Hf=256)
    FB("fullband-wavefront-h256", 33, Hf=256, F=161, norm="cumulative", T=5)
    FB("fullband-chain", 33, norm="cumulative", T=1, la=0)
    FB("fullband-chain", 16, F=161, la=3, gain=6.0)
    return rows


TABLE = _table()
PATHS = ("wavefront", "wavefront-last", "wavefront-F65", "group1-F161", "rt1-F65", "rt2-F161", "group1-first-noaux", "group1", "group1-last", "step-nogroup", "step-nogroup-k64",
         "step-nogroup-k2", "rt1-first", "rt1-last", "group2-first", "group2", "group2-last", "rt1-left9", "rt1-left16", "rt1-left1",
         "rounds-padded-tile", "rt2-rounds", "rt2-left2", "rt3-rounds", "rt3-left3", "rt4-rounds", "rt4-left4", "rt2-left16",
         "rt4-left16-nochain", "rt2-xin-fallback", "rt3-xin-fallback", "rt4-xin-fallback", "rt5-rounds", "rt5-left1", "rounds-rt3",
         "rounds-rt1x7", "rounds-rt4-left8", "chunked", "range-inside-utterance", "range-across-boundary", "range-group",
         "range-rt1-left9", "range-rt2-rounds", "fullband-chain", "fullband-chain-h384", "fullband-wavefront", "fullband-wavefront-h256")


def fb_chain_expected(row, utterances):
    """The full-band pair runs on the chain kernel at H = 512 / 384 up to 64 rows (and 4095 steps, never reached here)."""
    return int(row.Hf in (384, 512) and utterances <= 64)


def expected_plan(row, plan, utterances, n):
    """All fields of fsn_debug_core_call_plan for one core call of `utterances` utterances and n sub-band rows."""
    want = {k: v for k, v in (plan or {}).items() if k != "regime"}
    want.update(rows=n, fb_chain=fb_chain_expected(row, utterances), npad_fb=ru16(utterances), kin_chunks=ru16(2 * row.nb + 2) // 16)
    return want


def launches_of(row, plan, utterances):
    """The launchers one core call on `plan` goes through (run_core, csrc/fsn_api_fullsubnet.hip, read as rules of the plan's
    literals): what fsn_debug_core_last_launches must report."""
    ran = {"fb_chain" if fb_chain_expected(row, utterances) else "lstm_wavefront2"}
    if row.entry == "fullband":
        return ran
    if plan["regime"] == "wavefront":
        return ran | {"gemm_sb_proj", "lstm_wavefront2", "gemm_sb_out"}
    if plan["regime"] == "group":
        return ran | {"lstm2_group"} | ({"gemm_sb_proj", "lstm_wavefront2", "gemm_sb_out"} if plan["grp_aux_tiles"] else set())
    main, rt, left = plan["main_wgs"], plan["rt"], plan["left_tiles"]
    if left:
        ran |= {"gemm_sb_proj"} | ({"lstm_step_cu"} if plan["cu_tiles"] else set()) | ({"lstm_step"} if plan["aux_tiles"] else set())
    if main:  # layer 0: lstm_rec_in at 2 - 4 row tiles and 32 input columns, else lstm_rec<XIN>
        ran |= {"lstm_rec_in"} if 2 <= rt <= 4 and ru16(2 * row.nb + 2) == 32 else {"lstm_rec"}
    if plan["l1x"]:  # layer 1 forms its projection itself; only the left-over rows get a GEMM
        ran |= {"lstm_rec_x"} | ({"gemm_sb_l1"} if left else set())
    else:
        ran |= {"gemm_sb_l1"} | ({"lstm_rec"} if main else set())
    if not plan["fc_fused"] or left:
        ran |= {"gemm_sb_out"}
    return ran


def regions_of(plan, n):
    """(label, first local row, end) of the parts of one core call's n rows that different kernels process."""
    if plan["regime"] == "group":
        cut, names = 64 * plan["grp_clusters"], ("cluster rows", "aux rows")
    elif plan["main_wgs"] > 0:
        cut, names = 16 * plan["main_wgs"] * plan["rt"], ("main rows", "left-over rows")
    elif plan["regime"] == "persistent":
        cut, names = 16 * plan["cu_tiles"], ("cu-step rows", "small-step rows")
    else:
        return []
    return [(nm, lo, hi) for nm, lo, hi in ((names[0], 0, min(cut, n)), (names[1], min(cut, n), n)) if hi > lo]


# ---- the reference ----------------------------------------------------------------------------------------------------

def _seq(x, params, prefix, dtype, act, relu):
    """nn.LSTM(2 layers) + nn.Linear on x [N, I, T] -> [N, out, T]."""
    td = torch.float64 if dtype == np.float64 else torch.float32
    o = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype).transpose(2, 0, 1)))  # [T, N, I]
    for k in range(2):
        g = lambda n: torch.from_numpy(np.asarray(params[f"{prefix}.sequence_model.{n}_l{k}"], dtype=dtype))  # noqa: E731
        z = torch.zeros(o.shape[1], g("weight_hh").shape[1], dtype=td)
        o, _, _ = lstm_layer(o, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"), z, z, act=act)
    w = torch.from_numpy(np.asarray(params[f"{prefix}.fc_output_layer.weight"], dtype=dtype))
    b = torch.from_numpy(np.asarray(params[f"{prefix}.fc_output_layer.bias"], dtype=dtype))
    o = o @ w.t() + b
    return (torch.relu(o) if relu else o).numpy().transpose(1, 2, 0)


def fullband_stage(mag, params, la, norm, dtype, act):
    """mag [B, 1, F, T] -> (padded input [B, 1, F, Tp], fb_output [B, 1, F, Tp]): model.py:85-95."""
    x = np.pad(np.asarray(mag, dtype=dtype), [(0, 0), (0, 0), (0, 0), (0, la)])
    B, _, F, Tp = x.shape
    fb = _seq(O.NORMS[NORMS[norm]](x, dtype=dtype).reshape(B, F, Tp), params, "fb_model", dtype, act, True)
    return x, fb.reshape(B, 1, F, Tp)


def subband_units(x, fb, nb, unfold=O.freq_unfold):
    """The sub-band units before their norm, [B, F, 2 nb + 2, Tp] (model.py:110): 2 nb + 1 noisy bins + the full-band output."""
    B, _, F, Tp = x.shape
    return np.concatenate([unfold(x, nb).reshape(B, F, 2 * nb + 1, Tp), O.freq_unfold(fb, 0).reshape(B, F, 1, Tp)], axis=2)


def subband_input(x, fb, nb, norm, dtype):
    """The normalised sub-band input [B F, 2 nb + 2, Tp] (model.py:110-125)."""
    B, _, F, Tp = x.shape
    return np.ascontiguousarray(O.NORMS[NORMS[norm]](subband_units(x, fb, nb), dtype=dtype)).reshape(B * F, 2 * nb + 2, Tp)


def subband_stage(sb_in, params, la, dtype, act):
    """[N, 2 nb + 2, Tp] -> mask rows [N, 2, T] (the look-ahead frames dropped)."""
    return _seq(sb_in, params, "sb_model", dtype, act, False)[..., la:]


def model(mag, params, la, nb, norm, dtype, act, fb_only=False):
    """(mask rows [B F, 2, T] or None, fb_output [B, F, Tp]) of the model written out in `dtype`."""
    x, fb = fullband_stage(mag, params, la, norm, dtype, act)
    m = None if fb_only else subband_stage(subband_input(x, fb, nb, norm, dtype), params, la, dtype, act)
    return m, fb[:, 0]


def rows_to_mask(rows, B):
    """[B F, 2, T] -> the entry's layout [B, 2, F, T]."""
    return rows.reshape(B, -1, 2, rows.shape[-1]).transpose(0, 2, 1, 3)


def make_inputs(F, nb, Hf, T, gain, k):
    params = O.make_params(seed=3, num_freqs=F, fb_hidden=Hf, sb_num_neighbors=nb, gain=gain, mask_gain=24.0)
    rng = np.random.default_rng(1000 * T + 10 * F + k)
    return params, (np.abs(rng.standard_normal((k, 1, F, T))) + 0.05).astype(np.float32)


class Ref:
    """k base utterances through the fp64 model and the two fp32 yardsticks; arrays are read-only (shared between rows)."""

    def __init__(self, F, nb, Hf, la, T, norm, gain, k, fb_only):
        self.params, self.mag = make_inputs(F, nb, Hf, T, gain, k)
        run = lambda dtype, act: model(self.mag, self.params, la, nb, norm, dtype, act, fb_only)  # noqa: E731
        self.mask64, self.fb64 = run(np.float64, "torch")
        self.mask_t32, self.fb_t32 = run(np.float32, "torch")
        self.mask_c32, self.fb_c32 = (None, None) if fb_only else run(np.float32, "cell")
        self.F, self.k = F, k
        for a in (self.mag, self.mask64, self.fb64, self.mask_t32, self.fb_t32, self.mask_c32, self.fb_c32):
            if a is not None:
                a.setflags(write=False)

    def rows(self, which, begin, n):
        """Global rows [begin, begin + n) of a batch built as b -> base[b % k]: [n, 2, T]."""
        g = np.arange(begin, begin + n)
        return getattr(self, which)[(g // self.F % self.k) * self.F + g % self.F]


@functools.lru_cache(maxsize=None)
def reference(F, nb, Hf, la, T, norm, gain, k, fb_only=False):
    return Ref(F, nb, Hf, la, T, norm, gain, k, fb_only)


def reference_of(row):
    return reference(row.F, row.nb, row.Hf, row.la, row.T, row.norm, row.gain, row.k, row.entry == "fullband")


# ---- the checker ------------------------------------------------------------------------------------------------------

def _ss(a):
    return float((a * a).sum())


def frob(a, r):
    return math.sqrt(_ss(a - r) / _ss(r)) if _ss(r) > 0 else (0.0 if _ss(a - r) == 0 else float("inf"))


def maxrel(a, r):
    return float(np.abs(a - r).max() / np.abs(r).max())


def check_tensor(name, got, yard, ref, calls=(), log=print, tile=16, who="the fp32 cell emulation", max_rule=True):
    """got / yard / ref [rows, ..., frames] (fp64 `ref`).  calls: (label, first row, end, regions) of the core calls, regions
    (label, first row, end) relative to the call.  Asserts the rules of the module docstring and returns the whole tensor's
    (Frobenius ratio, max ratio, worst tile ratio).  max_rule=False (the CPU self-test only) leaves out the whole
    tensor's max-error rule."""
    got = np.where(np.isfinite(got), got, np.inf).astype(np.float64)
    yard = yard.astype(np.float64)

    def hold(label, g, y, r, both=False):
        fg, fy = frob(g, r), frob(y, r)
        assert fg <= SHARP * fy, (f"{name} [{label}]: Frobenius error {fg:.3e} of the device against {fy:.3e} of {who} on the CPU "
                                  f"({fg / fy if fy > 0 else float('inf'):.2f} x, allowed {SHARP:g} x)")
        if both:
            mg, my = maxrel(g, r), maxrel(y, r)
            assert mg <= SHARP * my, (f"{name} [{label}]: max error {mg:.3e} of the device against {my:.3e} of {who} on the CPU "
                                      f"({mg / my if my > 0 else float('inf'):.2f} x, allowed {SHARP:g} x; max |ref| {np.abs(r).max():.3e})")

    worst_tile = 0.0
    for label, lo, hi, regions in calls or [("all rows", 0, ref.shape[0], [])]:
        g, y, r = got[lo:hi], yard[lo:hi], ref[lo:hi]
        starts = range(0, hi - lo, tile)  # the narrowest rule first: its message names the rows
        y_worst = max(frob(y[s:s + tile], r[s:s + tile]) for s in starts)
        for s in starts:
            fg = frob(g[s:s + tile], r[s:s + tile])
            worst_tile = max(worst_tile, fg / y_worst if y_worst > 0 else float("inf"))
            where = "".join(f" of the {rl}" for rl, a, b in regions if a <= s < b)
            assert fg <= SHARP * y_worst, (f"{name} [{label}: rows {s} .. {min(s + tile, hi - lo) - 1}{where}]: Frobenius error {fg:.3e} "
                                           f"of the device against {y_worst:.3e}, the WORST {tile}-row tile of {who} on the CPU "
                                           f"({fg / y_worst if y_worst > 0 else float('inf'):.2f} x, allowed {SHARP:g} x)")
        for rl, a, b in regions:
            hold(f"{label}: {rl} {a} .. {b - 1}", g[a:b], y[a:b], r[a:b])
        if len(calls) > 1:
            hold(label, g, y, r)
    for t in range(ref.shape[-1]):
        hold(f"frame {t}", got[..., t], yard[..., t], ref[..., t])
    hold("whole tensor", got, yard, ref, both=max_rule)
    fy, my = frob(yard, ref), maxrel(yard, ref)
    rf, rm = frob(got, ref) / fy if fy > 0 else float("nan"), maxrel(got, ref) / my if my > 0 else float("nan")
    log(f"[csweep] {name}: frob hip {frob(got, ref):.3e} yardstick {fy:.3e} ({rf:.2f} x) max hip {maxrel(got, ref):.3e} yardstick "
        f"{my:.3e} ({rm:.2f} x) worst tile {worst_tile:.2f} x of the yardstick's worst")
    return rf, rm, worst_tile


def check_row(row, ref, got, call_list, log=print, max_rule=True):
    """got: the entry's output brought to rows, [n, 2, T] for the row's global rows (fullband: [B, F, Tp]).  call_list:
    (calls(), plan) pairs of the core calls."""
    if row.entry == "fullband":
        two = frob(ref.fb_t32, ref.fb64)
        log(f"[csweep] {row.id}: fb_output yardstick torch's fp32 {two:.3e}")
        return {"fb_output": check_tensor(f"{row.id} fb_output", got, ref.fb_t32, ref.fb64, log=log, who="torch's fp32")}
    begin = call_list[0][0][4]
    n = sum(c[3] for c, _ in call_list)
    r64, c32, t32 = (ref.rows(w, begin, n) for w in ("mask64", "mask_c32", "mask_t32"))
    log(f"[csweep] {row.id}: mask yardsticks cell {frob(c32, r64):.3e} / torch {frob(t32, r64):.3e} = "
        f"{frob(c32, r64) / frob(t32, r64):.2f} x, max |mask| {np.abs(r64).max():.2f}")
    calls = [(f"core call {i} ({c[1]} utterances)", c[4] - begin, c[4] - begin + c[3], regions_of(p, c[3])) for i, (c, p) in enumerate(call_list)]
    return {"mask": check_tensor(f"{row.id} mask", got, c32, r64, calls, log=log, max_rule=max_rule)}


# ---- the device side ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return fullsubnet_amd


_PACKED = {}


def packed_weights(lib, row, cfg, params, dev):
    key = (row.F, row.nb, row.Hf, row.gain)
    if key not in _PACKED:
        tensors = [torch.from_numpy(np.ascontiguousarray(params[k], dtype=np.float32)).to(dev) for k in lib.STATE_KEYS]
        prm = lib.Params(*[lib.dev_ptr(t, k) for t, k in zip(tensors, lib.STATE_KEYS)])
        packed = torch.empty(lib.lib().fsn_fullsubnet_packed_bytes(ctypes.byref(cfg)), dtype=torch.uint8, device=dev)
        lib.check(lib.lib().fsn_fullsubnet_pack(ctypes.byref(cfg), ctypes.byref(prm), packed.data_ptr(), packed.numel(), lib.stream_ptr(dev)))
        torch.cuda.synchronize()
        _PACKED[key] = packed
    return _PACKED[key]


def run_entry(lib, row, cfg, packed, mag):
    """One call of the row's entry: output behind the sentinel, workspace exact and poisoned.  Returns (output in the entry's
    layout on the device, launch trace, persistent launches added)."""
    L, dev, c = lib.lib(), mag.device, ctypes.byref(cfg)
    st = lib.stream_ptr(dev)
    B, T = row.B, row.T
    if row.entry == "rows":
        nbytes = L.fsn_fullsubnet_rows_workspace_bytes(c, B, T, row.begin, row.begin + row.N)
        out = Out(dev, (row.N, 2, T))
    else:
        nbytes = L.fsn_fullsubnet_workspace_bytes(c, B, T)
        out = Out(dev, (B, 2, row.F, T) if row.entry == "forward" else (B, row.F, row.Tp))
    ws = lib.workspace(nbytes, dev).fill_(0xFF)
    before = lib.persist_stats()[0]
    if row.entry == "rows":
        rc = L.fsn_fullsubnet_forward_rows(c, packed.data_ptr(), lib.dev_ptr(mag), B, T, row.begin, row.begin + row.N, lib.dev_ptr(out.f),
                                           ws.data_ptr(), ws.numel(), st)
    else:
        f = L.fsn_fullsubnet_forward if row.entry == "forward" else L.fsn_fullsubnet_fullband
        rc = f(c, packed.data_ptr(), lib.dev_ptr(mag), B, T, lib.dev_ptr(out.f), ws.data_ptr(), ws.numel(), st)
    ran = lib.core_last_launches()  # before any other entry of the library clears it
    lib.check(rc)
    added = lib.persist_stats()[0] - before
    return out.take(f"{row.id} output"), ran, added


def plan_and_calls(lib, row, cfg):
    """Assert the plan of every core call of the row; returns [(call, plan)]."""
    L, c = lib.lib(), ctypes.byref(cfg)
    if row.entry == "forward":
        sizes = (ctypes.c_int * 80)()
        n = L.fsn_debug_core_chunks(c, row.B, sizes, 80)
        chunks = list(sizes[:n])
        assert sum(chunks) == row.B, f"{row.id}: chunks {chunks} do not add up to {row.B}"
        assert chunks == row.chunks, f"{row.id}: runs as core calls of {chunks} utterances, the row was written for {row.chunks}"
    calls = row.calls()
    for call, plan in zip(calls, row.plans):
        b_lo, Bs, r0, n, _ = call
        got = lib.core_call_plan(cfg, row.B, row.T, row.begin, row.begin + row.N) if row.entry == "rows" else lib.core_call_plan(cfg, Bs, row.T)
        assert plan is not None or row.entry == "fullband", f"{row.id}: no expected plan written for a core call of {Bs} utterances"
        want = expected_plan(row, plan, Bs, n)
        if row.entry == "fullband":
            got, want = ({k: d[k] for k in ("fb_chain", "npad_fb")} for d in (got, want))
        assert got == want, f"{row.id}: the core call of {Bs} utterances / {n} rows has the plan\n{got}, the row was written for\n{want}"
    return list(zip(calls, row.plans))


@pytest.mark.parametrize("row", TABLE, ids=[r.id for r in TABLE])
def test_core_sweep(fsn, row):
    t0 = time.time()
    lib = fsn._lib
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == CUS, f"the plans of this table are literals for {CUS} CUs, the device has {cus}"
    cfg = row.cfg(lib)
    call_list = plan_and_calls(lib, row, cfg)
    check_duplication(row, [c for c, _ in call_list])
    ref = reference_of(row)
    mag = torch.from_numpy(ref.mag[np.arange(row.B) % row.k]).to(dev).contiguous()
    packed = packed_weights(lib, row, cfg, ref.params, dev)
    try:
        got, ran, added = run_entry(lib, row, cfg, packed, mag)
        torch.cuda.synchronize()
    except RuntimeError as e:  # a launch or the device failed: nothing more may run on it in this session
        pytest.exit(f"{row.id}: the device call failed, stopping the sweep: {e}", returncode=3)
    want_ran = set().union(*(launches_of(row, p, c[1]) for c, p in call_list))
    assert ran == want_ran, f"{row.id}: the call went through {sorted(ran)}, the plan implies {sorted(want_ran)}"
    want_added = sum(fb_chain_expected(row, c[1]) + (0 if row.entry == "fullband" else int(p["grp_clusters"] > 0)) for c, p in call_list)
    assert added == want_added, f"{row.id}: {added} persistent launches, the plan says {want_added}"
    again, _, _ = run_entry(lib, row, cfg, packed, mag)
    assert torch.equal(got, again), f"{row.id}: two calls in a row are not bit-identical"
    assert lib.stream_status(dev) == (0, 0), "the stream carries a timeout record"
    lib.check_canaries()
    host = got.cpu().numpy()
    if row.entry == "forward":
        host = np.ascontiguousarray(host.transpose(0, 2, 1, 3)).reshape(row.B * row.F, 2, row.T)
    del got, again
    check_row(row, ref, host, call_list)
    print(f"[csweep] {row.id}: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("batch,lo,hi", [(5, 1, 4), (9, 2, 8), (34, 1, 33)])
def test_aligned_row_range_equals_forward(fsn, batch, lo, hi):
    """A row range aligned to utterances is exactly fsn_fullsubnet_forward on those utterances (one core call: the wavefront at
    3 utterances, the group kernel at 6, the persistent pair at 32), bit for bit."""
    lib = fsn._lib
    dev = torch.device("cuda:0")
    whole = Row("aligned", "rows", N=(hi - lo) * 257, begin=lo * 257, batch=batch, plan=None)
    part = Row("aligned", "forward", B=hi - lo)
    cfg = whole.cfg(lib)
    sizes = (ctypes.c_int * 80)()
    assert lib.lib().fsn_debug_core_chunks(ctypes.byref(cfg), hi - lo, sizes, 80) == 1, "forward chunks this batch: not comparable"
    assert lib.core_call_plan(cfg, batch, 4, lo * 257, hi * 257) == lib.core_call_plan(cfg, hi - lo, 4)
    ref = reference(257, 15, 512, 2, 4, "offline", 2.0, 3)
    mag = torch.from_numpy(ref.mag[np.arange(batch) % 3]).to(dev).contiguous()
    packed = packed_weights(lib, whole, cfg, ref.params, dev)
    rows, _, _ = run_entry(lib, whole, cfg, packed, mag)
    fwd, _, _ = run_entry(lib, part, cfg, packed, mag[lo:hi].contiguous())
    assert torch.equal(rows, fwd.permute(0, 2, 1, 3).reshape(-1, 2, 4)), "the aligned row range differs from forward on its utterances"
