"""The LSTM / GRU layer entries and their BPTT held to an fp64 recurrence over a sweep of paths.  Needs an MI355X:
python -m pytest tests/test_gpu_recurrent_sweep.py -m gpu -s

Every recurrence outside the fused inference call runs through fsn_lstm_layer_forward[_fc | _state], fsn_lstm_layer_backward,
fsn_lstm2_forward[_train], fsn_lstm2_backward[_phase], fsn_gru_layer_forward[_state], fsn_gru_layer_backward and
fsn_gru2_forward, whose host side picks a code path from the shape alone.  TABLE has one Row per line, named after the path it
is there for; the entries are called through fullsubnet_amd._lib directly so that ldx, lddx, save == NULL, dx == NULL and the
phase form are the test's to choose.  The plan is asserted first, through the library's own queries and the launch counter of
fsn_debug_persist_stats (the kernels whose workgroups wait for each other - chain, group, their BPTT - report their launches
there; lstm_rec_in / lstm_rec_x have independent workgroups and do not, their rows are pinned through
fsn_lstm_layer_fc_supported / fsn_lstm_layer_plan_rows / fsn_gru_layer_is_persistent).  Row counts that depend on the CU count are
functions of it (`c`); a row whose asserted plan does not hold on the device fails.

Reference: the recurrence written out in torch fp64 on the CPU (gates i, f, g, o / r, z, n; h0 = c0 = 0 or the carried state),
gradients by autograd of sum(y * dy).  Operands are fp32 values: seeded Gaussians for x and dy, uniform weights and biases
+- gain / sqrt(H) (gain 2; gain 6 - saturating gates - on one row per kernel family).

Yardstick: for every output tensor two statistics against fp64, the relative Frobenius error and max|err| / max|ref|, taken for
the HIP result and, in the same run, for torch's CPU fp32 execution of the same written-out recurrence and autograd.
Assertion: stat_hip <= SHARP x stat_torch32, SHARP = 4 (the margin of test_gpu_linear_sweep.py).  One stated exception,
chosen by the rule yardstick_of(row, output) and printed with every figure and in every message: the hidden outputs of rows
with at most 48 input columns, and their gradients at T <= 2, are held to 4 x the statistic of the fp32 emulation of
lstm_cell.h's gate formulas instead (act="cell", a reference-side run).  The term: tanh as 1 - 2 rcp(1 + exp2(..)) carries
an absolute error of a few 2^-24 where torch's tanh keeps a relative one; a narrow input keeps pre-activations, g and h small,
and the emulation alone is then 4.8 x torch's fp32 on y and 4.7 x on gradients at T <= 2, 2.8 x on y at T >= 9 (1.4 x / 1.3 x
with a wide input at T >= 9, the issue's case; tests/test_recurrent_sweep_cpu.py asserts all of this).
Beside the whole tensor the
Frobenius statistic is taken per step and per 16-row tile of every [T][N][.] output and per gate block of every gate-major
gradient (a wrong tile or step hides in a whole-tensor norm); tests/test_recurrent_sweep_cpu.py runs this checker on the CPU
with torch's fp32 and deliberately wrong stand-ins.

In every row besides: outputs behind a NaN sentinel with a guard of 1024 elements (intact outside the declared region, finite
inside, dx columns I .. lddx - 1 and out0 columns N .. ldo - 1 untouched); workspaces exactly their query's size and filled with
0xFF; save buffers exactly fsn_*_save_bytes; two calls in a row bit-identical; dx == NULL gives the same weight gradients;
another ldx / lddx gives the same bits where the path takes any stride; fsn_lstm2_backward_phase 1, 4, 2 equal phase 7; hidden
units with all-zero weights (H = 320 run as 384) are exactly 0.0 in hseq and in their gradient rows; the stream status is clean.

Not covered: the chain BPTT's own step limit (fsn_fb_chain_bptt_max_steps, 16 382).  No row runs past it (a 16-row fp64 autograd
of that length takes minutes) and no query exposes it: fsn_lstm2_train_is_persistent is already 0 from 4096 steps on because of
the FORWARD chain, whose limit (4095 / 4096) is what the chain-last-length / chain-first-fallback / train-chain-length rows pin.

Fixed on the way: train-group-left0 T190 N1536 I20 (fsn_lstm2_forward_train + fsn_lstm2_backward, group pair) failed with the
relative Frobenius error of dw_hh0 at 2.32e-6 against 4.38e-7 of the yardstick (5.3 x), dw_ih1 2.31e-6 against 3.58e-7 (6.5 x),
dw_hh1 2.24e-6 against 3.56e-7 (6.3 x).  These are the [4H][H] weight-gradient products over K = T N = 291 840 rows:
fsn_launch_gemm_tn split K sixteen ways (one workgroup per CU), one fp32 chain of 18 240 rows per split.  It now forms a
product whose splits would exceed 4096 rows in K segments of 2048 rows per split, summed in a fixed order (gemm_tn_kernels.hip);
after: dw_hh0 1.01e-6 (2.6 x torch's fp32), dw_ih1 7.8e-7 (2.2 x), dw_hh1 7.7e-7 (2.2 x); the row's y 3.5 x, dx 2.5 x unchanged.

Seen on an MI355X, all 88 rows, 154 s, every plan assertion holding (also under FSN_WS_CANARY=1 before the K-segment fix):
worst relative-Frobenius ratio hip / torch's fp32 per output and its row: y 5.6 x (group-lstm2-T2-N4096-I12); out0 1.4 x
(fc-o1-rt2-layer_fc-T9-N8192-I384); out1 1.3 x (fc-o2-rt3); dx 3.1 x (train-group-bptt-only-lstm2_train-T9-N1536-I12); dw_ih
2.2 x (train-layer-layer_train-T9-N1104-I257); db 1.9 x (train-layer-layer_train-T9-N1104-I257); dw_hh 2.2 x (train-layer-
layer_train-T9-N1104-I257); y0 4.9 x (train-group-bptt-only-lstm2_train-T2-N1536-I12); dw_ih0 2.7 x (train-group-bptt-only-
lstm2_train-T9-N1536-I12); dw_hh0 3.2 x (train-group-bptt-only-lstm2_train-T9-N1536-I12); db0 3.4 x (train-group-bptt-only-
lstm2_train-T9-N1536-I12); dw_ih1 3.0 x (train-chain-length-lstm2_train-T2-N16-I16); dw_hh1 5.4 x (train-chain-length-
lstm2_train-T2-N16-I16); db1 1.9 x (train-chain-lstm2_train-T2-N64-I33); db_ih 1.4 x (gru-train-gru_train-T2-N48-I32); db_hh
1.3 x (gru-train-gru_train-T2-N48-I32); h_fin 2.3 x (state-lstm-layer_state-T9-N48-I20); c_fin 1.6 x (state-lstm-
layer_state-T9-N48-I20).  Every ratio above 4 is on a row that yardstick_of holds to the cell emulation.  These figures are
from the run that asserted against the larger of the two fp32 statistics; the run under the rule above (torch alone, the
emulation alone where the rule says so) and test_gru2_forward_refuses_off_the_chain have not been on the device yet.
"""
import ctypes
import math
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0DEAD  # a quiet NaN with a recognisable payload
GUARD = 1024  # elements allocated (and checked) behind every output
POOL_ELEMS = 256  # draws are repeated until every output tensor has contributed this many elements
SHARP = 4.0
CUS = 256  # the MI355X's CU count: ids and the CPU self-test are written for it

LSTM_ENTRIES = ("layer", "layer_fc", "lstm2", "layer_train", "lstm2_train", "layer_state")
GRU_ENTRIES = ("gru_layer", "gru2", "gru_train", "gru_state")
TRAIN_ENTRIES = ("layer_train", "lstm2_train", "gru_train")


def ru16(n):
    return (n + 15) // 16 * 16


class Row:
    """One line of the sweep.  tiles: 16-row tiles, an int or a function of the CU count.  launches: True = the entry must
    add persistent launches (fsn_debug_persist_stats), False = none, None = not a property of this path.  queries: (name of a
    plan query, function (row, N) -> arguments, expected value or function of the CU count)."""

    def __init__(self, path, family, entry, T, tiles, I, ldx, H, H1=None, O=None, gain=2.0, Hreal=None, ldo_extra=0,
                 launches=None, queries=(), alt_ldx=True):
        self.path, self.family, self.entry, self.T, self.tiles, self.I, self.ldx, self.H = path, family, entry, T, tiles, I, ldx, H
        self.H1 = H if H1 is None else H1
        self.O, self.gain, self.Hreal, self.ldo_extra = O, gain, Hreal or H, ldo_extra
        if launches is None and family in ("step", "gru_step", "rec_gx"):  # step by step: no launch of the waiting kernels
            launches = False
        self.launches, self.queries, self.alt_ldx = launches, queries, alt_ldx
        self.cell = "gru" if entry in GRU_ENTRIES else "lstm"
        self.n_fixed = None

    def N(self, cus=CUS):
        if self.n_fixed is not None:
            return self.n_fixed
        return 16 * (self.tiles(cus) if callable(self.tiles) else self.tiles)

    @property
    def id(self):
        return f"{self.path}-{self.entry}-T{self.T}-N{self.N()}-I{self.I}-ld{self.ldx}-H{self.H}" + \
            (f"x{self.H1}" if self.H1 != self.H else "") + (f"-O{self.O}" if self.O else "") + \
            (f"-g{self.gain:g}" if self.gain != 2.0 else "")

    def scaled(self, n_max=48, t_max=12):
        """The same row with fewer rows and steps (the CPU self-test of the checker); T = 1 / 2 are kept."""
        r = Row(self.path, self.family, self.entry, min(self.T, t_max), None, self.I, self.ldx, self.H, self.H1, self.O,
                self.gain, self.Hreal, self.ldo_extra)
        r.n_fixed = min(self.N(), n_max)
        return r


def _q_fc(expected):
    return ("fsn_lstm_layer_fc_supported", lambda r, N: (r.T, N, 384, 384, 384, 1), expected)


def _q_rows(expected):  # fsn_lstm_layer_plan_rows(N, H): N itself = no cheaper padded plan; expected: function of (N, c)
    return ("fsn_lstm_layer_plan_rows", lambda r, N: (N, r.H), expected)


def _q_l2(expected):
    return ("fsn_lstm2_forward_is_persistent", lambda r, N: (r.T, N, r.I, r.ldx, r.H, r.H1), expected)


def _q_train(expected):
    return ("fsn_lstm2_train_is_persistent", lambda r, N: (r.T, N, r.I, r.H), expected)


def _q_gru(expected):
    return ("fsn_gru_layer_is_persistent", lambda r, N: (r.T, N, r.I, r.ldx, r.H), expected)


def _q_gru2(expected):
    return ("fsn_gru2_forward_supported", lambda r, N: (r.T, N, r.H), expected)


def _table():
    rows = []
    add = rows.append
    # ---- one LSTM layer, inference (save == NULL) ----
    # step by step: H != 384, or fewer than CUs / 4 row tiles
    add(Row("step-h64", "step", "layer", 1, 1, 20, 32, 64))
    add(Row("step-h64", "step", "layer", 2, 3, 5, 16, 64))
    add(Row("step-h64", "step", "layer", 9, 69, 20, 32, 64, gain=6.0))
    add(Row("step-h320pad", "step", "layer", 9, 3, 33, 48, 384, Hreal=320, queries=(_q_fc(0),)))
    add(Row("step-h512", "step", "layer", 190, 1, 257, 272, 512))
    add(Row("step-h512", "step", "layer", 2, 69, 40, 48, 512))
    # lstm_rec_in_kernel: narrow input, projection inside; one tile per workgroup from CUs / 4 tiles on
    add(Row("rec-narrow-1chunk", "rec_in", "layer", 190, lambda c: c // 4, 12, 32, 384, queries=(_q_fc(0),)))
    add(Row("rec-narrow-1chunk", "rec_in", "layer", 1, lambda c: c // 4, 16, 16, 384))
    add(Row("rec-narrow-2chunk", "rec_in", "layer", 2, lambda c: c, 20, 48, 384))
    add(Row("rec-narrow-2chunk", "rec_in", "layer", 9, lambda c: c // 2, 32, 32, 384, gain=6.0))
    for rt in (2, 3, 4):  # whole rounds, nothing left over (fsn_lstm_layer_fc_supported answers exactly that for a stacked layer)
        add(Row(f"rec-rt{rt}", "rec_in", "layer", 2, lambda c, rt=rt: rt * c, 20, 32, 384, queries=(_q_fc(1), _q_rows(lambda N, c: N))))
    add(Row("rec-left1", "rec_in", "layer", 9, lambda c: 2 * c + 1, 12, 16, 384, queries=(_q_fc(0), _q_rows(lambda N, c: N))))
    add(Row("rec-left17-rounds", "rec_in", "layer", 2, lambda c: 2 * c + 17, 20, 32, 384, queries=(_q_fc(0),)))
    add(Row("rec-rounds", "rec_in", "layer", 2, lambda c: 8 * c + 3, 12, 16, 384, queries=(_q_fc(0),)))
    # 448 tiles on 256 CUs: 224 workgroups x 2 tiles instead of 256 x 1 + 192 left over
    add(Row("rec-fewer-wgs", "rec_in", "layer", 2, lambda c: c + 3 * c // 4, 12, 16, 384, queries=(_q_fc(1), _q_rows(lambda N, c: N))))
    add(Row("rec-fewer-wgs-pad", "rec_gx", "layer", 1, lambda c: c + 3 * c // 4 - 1, 12, 16, 384,
            queries=(_q_rows(lambda N, c: N + 16),)))
    # lstm_rec_x_kernel: the layer above an equally wide one, I = H = ldx
    add(Row("rec-stacked", "rec_x", "layer", 190, lambda c: c + 102, 384, 384, 384, queries=(_q_fc(1),), alt_ldx=False))
    add(Row("rec-stacked", "rec_x", "layer", 1, lambda c: 3 * c, 384, 384, 384, queries=(_q_fc(1),), alt_ldx=False))
    add(Row("rec-stacked", "rec_x", "layer", 2, lambda c: 4 * c, 384, 384, 384, queries=(_q_fc(1),), alt_ldx=False, gain=6.0))
    add(Row("rec-stacked-left7", "rec_x", "layer", 2, lambda c: 3 * c + 7, 384, 384, 384, queries=(_q_fc(0),), alt_ldx=False))
    add(Row("rec-stacked-h320pad", "rec_x", "layer", 2, lambda c: 2 * c, 384, 384, 384, Hreal=320, alt_ldx=False))
    # near-misses: projection GEMM + run_recurrence
    add(Row("miss-I33", "rec_gx", "layer", 2, lambda c: 2 * c, 33, 48, 384))
    add(Row("miss-I48", "rec_gx", "layer", 1, lambda c: c // 4, 48, 48, 384))
    add(Row("miss-I48", "rec_gx", "layer", 190, lambda c: c // 4, 40, 48, 384))
    add(Row("miss-ldx", "rec_gx", "layer", 9, lambda c: 2 * c, 384, 400, 384, gain=6.0,
            queries=(("fsn_lstm_layer_fc_supported", lambda r, N: (r.T, N, 384, 400, 384, 1), 0),)))
    # ---- the last layer + nn.Linear(H, O) ----
    add(Row("fc-o1-rt2", "rec_x", "layer_fc", 9, lambda c: 2 * c, 384, 384, 384, O=1, queries=(_q_fc(1),), alt_ldx=False))
    add(Row("fc-o2-rt3-ldo", "rec_x", "layer_fc", 2, lambda c: 3 * c, 384, 384, 384, O=2, ldo_extra=16, queries=(_q_fc(1),), alt_ldx=False))
    add(Row("fc-o2-rt4", "rec_x", "layer_fc", 1, lambda c: 4 * c, 384, 384, 384, O=2, queries=(_q_fc(1),), alt_ldx=False))
    # ---- two stacked layers, inference ----
    add(Row("chain-h384", "chain", "lstm2", 190, 1, 20, 32, 384, launches=True, queries=(_q_l2(1),)))
    add(Row("chain-h384", "chain", "lstm2", 1, 3, 257, 272, 384, launches=True, queries=(_q_l2(1),)))
    add(Row("chain-h512", "chain", "lstm2", 2, 4, 257, 272, 512, launches=True, queries=(_q_l2(1),)))
    add(Row("chain-h512", "chain", "lstm2", 9, 3, 33, 48, 512, launches=True, queries=(_q_l2(1),), gain=6.0))
    add(Row("chain-last-length", "chain", "lstm2", 4095, 1, 16, 16, 512, launches=True, queries=(_q_l2(1),), alt_ldx=False))
    add(Row("chain-first-fallback", "wavefront", "lstm2", 4096, 1, 16, 16, 512, launches=False, queries=(_q_l2(0),), alt_ldx=False))
    # lowest / highest cluster counts of both ranges (one cluster of 64 rows per eight CUs, or two on nearly every set)
    for k, (tiles, ld) in enumerate(((96, 32), (lambda c: c // 2, 16), (lambda c: 7 * c // 8, 32), (lambda c: c, 16))):
        add(Row("group", "group", "lstm2", 2 if k else 190, tiles, 20 if ld == 32 else 12, ld, 384, launches=True,
                queries=(_q_l2(1),), alt_ldx=False))
    add(Row("group", "group", "lstm2", 1, 100, 32, 32, 384, launches=True, queries=(_q_l2(1),), alt_ldx=False, gain=6.0))
    add(Row("wavefront-h0-h1", "wavefront", "lstm2", 9, 2, 20, 32, 128, H1=64, launches=False, queries=(_q_l2(0),)))
    add(Row("wavefront-80rows", "wavefront", "lstm2", 190, 5, 20, 32, 384, launches=False, queries=(_q_l2(0),)))
    add(Row("wavefront-ldx48", "wavefront", "lstm2", 1, 96, 20, 48, 384, launches=False, queries=(_q_l2(0),), alt_ldx=False))
    add(Row("wavefront-ldx48", "wavefront", "lstm2", 2, 1, 20, 48, 512, H1=384, launches=False, queries=(_q_l2(0),), gain=6.0))
    # ---- training pairs: one layer (the per-step kernels and bptt_step) ----
    add(Row("train-layer", "train_step", "layer_train", 1, 1, 1, 16, 64, launches=False))
    add(Row("train-layer", "train_step", "layer_train", 2, 3, 32, 32, 384, launches=False))
    add(Row("train-layer", "train_step", "layer_train", 9, 69, 257, 272, 512, launches=False))
    add(Row("train-layer", "train_step", "layer_train", 190, 1, 32, 48, 384, launches=False, gain=6.0))
    add(Row("train-layer-h320pad", "train_step", "layer_train", 9, 3, 20, 32, 384, Hreal=320, launches=False))
    # ---- training pairs: two layers ----
    # group pair: 0, 1, 8 left-over tiles beside whole 64-row clusters (at most CUs / 8 of them)
    for T, tiles, left, I in ((190, 96, 0, 20), (1, 97, 1, 17), (2, lambda c: c // 2 + 8, 8, 32), (9, 96, 0, 32)):
        add(Row(f"train-group-left{left}", "train_group", "lstm2_train", T, tiles, I, 32, 384, launches=True,
                queries=(_q_train(1),), gain=6.0 if T == 9 else 2.0, alt_ldx=False))  # the group forward: x rows of exactly 32
    add(Row("train-group-left9-fallback", "train_step", "lstm2_train", 2, lambda c: c // 2 + 9, 20, 32, 384, launches=False,
            queries=(_q_train(0),)))
    add(Row("train-group-bptt-only", "train_group_bptt", "lstm2_train", 2, 96, 12, 16, 384, launches=True, queries=(_q_train(0),)))
    add(Row("train-group-bptt-only", "train_group_bptt", "lstm2_train", 1, 100, 64, 64, 384, launches=True, queries=(_q_train(0),)))
    add(Row("train-group-bptt-only", "train_group_bptt", "lstm2_train", 9, 96, 12, 16, 384, launches=True, queries=(_q_train(0),)))
    add(Row("train-chain", "train_chain", "lstm2_train", 190, 1, 257, 272, 512, launches=True, queries=(_q_train(1),)))
    add(Row("train-chain", "train_chain", "lstm2_train", 1, 4, 257, 272, 512, launches=True, queries=(_q_train(1),)))
    add(Row("train-chain", "train_chain", "lstm2_train", 2, 4, 33, 48, 512, launches=True, queries=(_q_train(1),), gain=6.0))
    add(Row("train-chain-bptt-only", "train_chain", "lstm2_train", 9, 5, 257, 272, 512, launches=True, queries=(_q_train(0),)))
    add(Row("train-96rows-by-layer", "train_step", "lstm2_train", 9, 6, 257, 272, 512, launches=False, queries=(_q_train(0),)))
    add(Row("train-chain-length", "train_chain", "lstm2_train", 2, 1, 16, 16, 512, launches=True,
            queries=(_q_train(1), ("fsn_lstm2_train_is_persistent", lambda r, N: (4095, N, r.I, r.H), 1),
                     ("fsn_lstm2_train_is_persistent", lambda r, N: (4096, N, r.I, r.H), 0))))
    # ---- GRU ----
    add(Row("gru-step", "gru_step", "gru_layer", 1, 1, 20, 32, 128, queries=(_q_gru(0),)))
    add(Row("gru-step", "gru_step", "gru_layer", 2, 3, 257, 272, 512, queries=(_q_gru(0),)))
    add(Row("gru-step", "gru_step", "gru_layer", 190, 1, 33, 48, 384, queries=(_q_gru(0),), gain=6.0))
    add(Row("gru-rec-narrow", "gru_rec", "gru_layer", 190, lambda c: c + c // 8, 12, 16, 384, queries=(_q_gru(1),)))
    add(Row("gru-rec-narrow-left", "gru_rec", "gru_layer", 1, lambda c: 2 * c + 3, 20, 48, 384, queries=(_q_gru(1),)))
    add(Row("gru-rec-stacked", "gru_rec", "gru_layer", 2, lambda c: 3 * c, 384, 384, 384, queries=(_q_gru(1),), alt_ldx=False))
    add(Row("gru-rec-stacked-left", "gru_rec", "gru_layer", 9, lambda c: 2 * c + 5, 384, 384, 384, queries=(_q_gru(1),), alt_ldx=False,
            gain=6.0))
    add(Row("gru-rec-miss", "gru_step", "gru_layer", 2, lambda c: c, 12, 16, 384, queries=(_q_gru(0),)))
    add(Row("gru2-chain", "gru_chain", "gru2", 190, 1, 257, 272, 512, launches=True, queries=(_q_gru2(1),)))
    add(Row("gru2-chain", "gru_chain", "gru2", 1, 4, 20, 32, 384, launches=True, queries=(_q_gru2(1),)))
    add(Row("gru2-chain", "gru_chain", "gru2", 2, 3, 33, 48, 384, launches=True, queries=(_q_gru2(1),), gain=6.0))
    add(Row("gru2-off-chain", "gru_step", "gru_layer", 9, 5, 20, 32, 512, queries=(_q_gru(0), _q_gru2(0))))
    add(Row("gru-train", "gru_train", "gru_train", 1, 1, 1, 16, 128, launches=False))
    add(Row("gru-train", "gru_train", "gru_train", 2, 3, 32, 32, 384, launches=False))
    add(Row("gru-train", "gru_train", "gru_train", 9, 69, 257, 272, 512, launches=False, gain=6.0))
    add(Row("gru-train", "gru_train", "gru_train", 190, 1, 20, 32, 384, launches=False))
    # ---- carried state: T steps in chunks of 1 + 5 + the rest from a non-zero state ----
    add(Row("state-lstm", "state", "layer_state", 9, 3, 20, 32, 384, launches=False))
    add(Row("state-lstm", "state", "layer_state", 190, 1, 257, 272, 512, launches=False))
    add(Row("state-lstm", "state", "layer_state", 1, 1, 20, 32, 64, launches=False))
    add(Row("state-lstm", "state", "layer_state", 2, 2, 20, 32, 64, launches=False, gain=6.0))
    add(Row("state-gru", "gru_state", "gru_state", 9, 3, 20, 32, 384, launches=False))
    add(Row("state-gru", "gru_state", "gru_state", 190, 1, 257, 272, 512, launches=False))
    add(Row("state-gru", "gru_state", "gru_state", 1, 1, 20, 32, 128, launches=False))
    add(Row("state-gru", "gru_state", "gru_state", 2, 2, 20, 32, 128, launches=False, gain=6.0))
    return rows


TABLE = _table()
# every family has a T = 1, a T = 2 and a T = 190 row (tests/test_recurrent_sweep_cpu.py asserts it); rec_gx and
# train_group_bptt are the near-miss / BPTT-only variants of families that have theirs
FAMILIES = ("step", "rec_in", "rec_x", "chain", "group", "wavefront", "train_step", "train_group", "train_chain", "gru_step",
            "gru_rec", "gru_chain", "gru_train", "state", "gru_state")
PATHS = ("step-h64", "step-h320pad", "step-h512", "rec-narrow-1chunk", "rec-narrow-2chunk", "rec-rt2", "rec-rt3", "rec-rt4",
         "rec-left1", "rec-left17-rounds", "rec-rounds", "rec-fewer-wgs", "rec-stacked", "rec-stacked-left7", "miss-I33", "miss-I48",
         "miss-ldx", "fc-o1-rt2", "fc-o2-rt3-ldo", "fc-o2-rt4", "chain-h384", "chain-h512", "chain-last-length", "chain-first-fallback",
         "group", "wavefront-h0-h1", "wavefront-80rows", "wavefront-ldx48", "train-layer", "train-group-left0", "train-group-left1",
         "train-group-left8", "train-group-left9-fallback", "train-group-bptt-only", "train-chain", "train-chain-bptt-only",
         "train-96rows-by-layer", "gru-step", "gru-rec-narrow", "gru-rec-stacked", "gru2-chain", "gru2-off-chain", "gru-train",
         "state-lstm", "state-gru")


# ---- operands and the reference ---------------------------------------------------------------------------------------

def _layer_dims(row):
    """(input width, hidden width, declared-nonzero hidden units) per layer."""
    if row.entry in ("lstm2", "lstm2_train", "gru2"):
        return [(row.I, row.H, row.Hreal), (row.H, row.H1, row.H1)]
    return [(row.I, row.H, row.Hreal)]


def make_operands(row, N, draw, device="cpu"):
    """fp32 operands on the CPU: x [T][N][I], dy [T][N][H_last], per layer w_ih / w_hh / b_ih / b_hh (uniform +- gain / sqrt(H);
    hidden units beyond Hreal all zero, as a zero-padded smaller layer), fc_w / fc_b, the carried state h0 / c0."""
    g = torch.Generator().manual_seed(7919 * draw + 31 * row.T + N + 17 * row.I + row.H)
    G = 3 if row.cell == "gru" else 4
    ops = dict(x=torch.randn(row.T, N, row.I, generator=g))
    layers = []
    prev_real = row.I
    for I, H, Hreal in _layer_dims(row):
        a = row.gain / math.sqrt(H)
        p = [(torch.rand(s, generator=g) * 2 - 1) * a for s in ((G * H, I), (G * H, H), (G * H,), (G * H,))]
        if Hreal < H:
            for t in p:
                t.view(G, H, -1)[:, Hreal:] = 0
            p[1][:, Hreal:] = 0
        p[0][:, prev_real:] = 0
        prev_real = Hreal
        layers.append(p)
    ops["layers"] = layers
    Hl = _layer_dims(row)[-1][1]
    ops["dy"] = torch.randn(row.T, N, Hl, generator=g)
    if len(layers) == 1 and row.Hreal < row.H:  # nothing downstream reads a zero-padded unit: its gradient is zero
        ops["dy"][..., row.Hreal:] = 0
    if row.O:
        a = 1.0 / math.sqrt(row.H)
        ops["fc_w"] = (torch.rand(row.O, row.H, generator=g) * 2 - 1) * a
        ops["fc_b"] = (torch.rand(row.O, generator=g) * 2 - 1) * a
    if row.entry in ("layer_state", "gru_state"):
        ops["h0"] = torch.tanh(torch.randn(N, row.H, generator=g))
        ops["c0"] = torch.randn(N, row.H, generator=g)
    return ops


class _SigFast(torch.autograd.Function):
    """lstm_cell.h: rcp(1 + exp2(-x log2 e)); derivative from the saved activation."""

    @staticmethod
    def forward(ctx, x):
        y = 1.0 / (1.0 + torch.exp2(x * x.new_tensor(-1.4426950408889634)))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return g * (y * (1.0 - y))


class _TanhFast(torch.autograd.Function):
    """lstm_cell.h: 1 - 2 rcp(1 + exp2(2 x log2 e)); derivative from the saved activation."""

    @staticmethod
    def forward(ctx, x):
        y = 1.0 - 2.0 / (1.0 + torch.exp2(x * x.new_tensor(2.8853900817779268)))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return g * (1.0 - y * y)


ACTS = {"torch": (torch.sigmoid, torch.tanh), "cell": (_SigFast.apply, _TanhFast.apply)}


def lstm_layer(x, w_ih, w_hh, b_ih, b_hh, h, c, act="torch", probe=None):
    """nn.LSTM's recurrence, gates i, f, g, o.  probe [T][N][4H] (zeros that require grad): added to the pre-activations, its
    gradient is the gate gradient."""
    sig, tanh = ACTS[act]
    b = b_ih + b_hh
    ys = []
    for t in range(x.shape[0]):
        a = x[t] @ w_ih.t() + b + h @ w_hh.t()
        if probe is not None:
            a = a + probe[t]
        i, f, g, o = a.chunk(4, -1)
        c = sig(f) * c + sig(i) * tanh(g)
        h = sig(o) * tanh(c)
        ys.append(h)
    return torch.stack(ys), h, c


def gru_layer(x, w_ih, w_hh, b_ih, b_hh, h, act="torch"):
    """nn.GRU's recurrence, gates r, z, n: n = tanh(W_in x + b_in + r (W_hn h + b_hn)), h = (1 - z) n + z h."""
    sig, tanh = ACTS[act]
    ys = []
    for t in range(x.shape[0]):
        gh = h @ w_hh.t() + b_hh
        xr, xz, xn = (x[t] @ w_ih.t() + b_ih).chunk(3, -1)
        hr, hz, hn = gh.chunk(3, -1)
        r, z = sig(xr + hr), sig(xz + hz)
        n = tanh(xn + r * hn)
        h = (1 - z) * n + z * h
        ys.append(h)
    return torch.stack(ys), h


def reference(row, ops, dtype, act="torch", probe=False):
    """Every output of the row's entry in `dtype` on the CPU.  probe: also "dgates" (single LSTM layer, training)."""
    with torch.set_grad_enabled(row.entry in TRAIN_ENTRIES):
        return _reference(row, ops, dtype, act, probe)


def _reference(row, ops, dtype, act, probe):
    train = row.entry in TRAIN_ENTRIES
    x = ops["x"].to(dtype).requires_grad_(train)
    layers = [[p.to(dtype).requires_grad_(train) for p in lp] for lp in ops["layers"]]
    N = x.shape[1]
    out = {}
    pr = torch.zeros(row.T, N, 4 * row.H, dtype=dtype, requires_grad=True) if probe else None
    if row.cell == "lstm":
        h = ops["h0"].to(dtype) if "h0" in ops else torch.zeros(N, row.H, dtype=dtype)
        c = ops["c0"].to(dtype) if "c0" in ops else torch.zeros(N, row.H, dtype=dtype)
        y, h, c = lstm_layer(x, *layers[0], h, c, act, pr)
        if len(layers) == 2:
            out["y0"] = y
            z = torch.zeros(N, row.H1, dtype=dtype)
            y, _, _ = lstm_layer(y, *layers[1], z, z, act)
        if row.entry == "layer_state":
            out["h_fin"], out["c_fin"] = h, c
    else:
        h = ops["h0"].to(dtype) if "h0" in ops else torch.zeros(N, row.H, dtype=dtype)
        y, h = gru_layer(x, *layers[0], h, act)
        if len(layers) == 2:
            y, _ = gru_layer(y, *layers[1], torch.zeros(N, row.H1, dtype=dtype), act)
        if row.entry == "gru_state":
            out["h_fin"] = h
    if row.entry == "layer_fc":
        o = y @ ops["fc_w"].to(dtype).t() + ops["fc_b"].to(dtype)
        for k in range(row.O):
            out[f"out{k}"] = o[..., k]
    else:
        out["y"] = y
    if row.entry not in ("lstm2_train",):
        out.pop("y0", None)
    if train:
        wanted = [x] + [p for lp in layers for p in lp] + ([pr] if probe else [])
        grads = torch.autograd.grad((y * ops["dy"].to(dtype)).sum(), wanted)
        out["dx"] = grads[0]
        for k, lp in enumerate(layers):
            g = grads[1 + 4 * k:5 + 4 * k]
            s = str(k) if len(layers) == 2 else ""
            out["dw_ih" + s], out["dw_hh" + s] = g[0], g[1]
            if row.cell == "lstm":
                out["db" + s] = g[2]
            else:
                out["db_ih" + s], out["db_hh" + s] = g[2], g[3]
        if probe:
            out["dgates"] = grads[-1]
    return {k: v.detach() for k, v in out.items()}


# ---- the checker ------------------------------------------------------------------------------------------------------

def _blocks(name, t, row):
    """(label, view) of the blocks whose Frobenius error is held beside the whole tensor's: steps and 16-row tiles of a
    [T][N][.] tensor, row tiles of a [T][N] or [N][H] one, gate blocks of a gate-major gradient."""
    G = 3 if row.cell == "gru" else 4
    if t.dim() == 3:
        for s in range(t.shape[0]):
            yield f"step {s}", t[s]
        for n in range(0, t.shape[1], 16):
            yield f"rows {n}..", t[:, n:n + 16]
    elif name.startswith("out") or name.endswith("_fin"):
        for n in range(0, t.shape[-2 if name.endswith("_fin") else -1], 16):
            yield f"rows {n}..", (t[n:n + 16] if name.endswith("_fin") else t[:, n:n + 16])
    elif name.startswith("d"):
        for k in range(G):
            yield f"gate {k}", t.view(G, t.shape[0] // G, -1)[k]
        if t.dim() == 2 and name.startswith("dw_ih"):
            for k in range(0, t.shape[1], 16):
                yield f"columns {k}..", t[:, k:k + 16]


HIDDEN = ("y", "y0", "out0", "out1", "h_fin", "c_fin")
NARROW = 48  # input columns up to which a row's activations stay small (see yardstick_of)


def yardstick_of(row, name):
    """Which CPU fp32 run an output is held to: "torch" (the written-out recurrence with torch.sigmoid / torch.tanh) unless
    the cancellation of the cell's tanh applies, then "cell" (the same recurrence with lstm_cell.h's formulas).
    tanh as 1 - 2 rcp(1 + exp2(2 x log2 e)) carries an ABSOLUTE error of a few 2^-24 whatever its value, torch's tanh a RELATIVE
    one.  With at most NARROW input columns and weights of 2 / sqrt(H) the pre-activations stay below ~0.5, g = tanh(.) and h
    around 0.1 - 0.2: there the absolute term is 3 - 5 x torch's whole error on every hidden output, at every T (the CPU module
    measures it).  Gradients feel it only while nothing else has accumulated, T <= 2.  Wide inputs (pre-activations of order
    1) and all gradients from T = 9 on are held to torch's fp32 alone."""
    if row.I <= NARROW and (name in HIDDEN or row.T <= 2):
        return "cell"
    return "torch"


class Stat:
    """Errors of one output tensor against fp64, of the device ("hip") and of torch's CPU fp32 ("cpu"), pooled over draws:
    sums of squares and maxima for the whole tensor and for each block."""

    def __init__(self, name):
        self.name, self.n = name, 0
        self.acc = {}  # label -> [ss_hip, ss_cpu, ss_ref, max_hip, max_cpu, max_ref, ss_emu, max_emu]

    def add(self, row, got, cpu, ref, emu=None):
        self.n += ref.numel()
        g, c = got.double(), cpu.double()
        e = c if emu is None else emu.double()
        g = torch.where(torch.isfinite(g), g, torch.full_like(g, float("inf")))
        views = [("all", g, c, ref, e)] + [(lb, gv, cv, rv, ev) for (lb, gv), (_, cv), (_, rv), (_, ev) in
                                           zip(*(_blocks(self.name, t, row) for t in (g, c, ref, e)))]
        for lb, gv, cv, rv, ev in views:
            if lb != "all" and rv.numel() < POOL_ELEMS:  # too few elements for a statistic of its own
                continue
            a = self.acc.setdefault(lb, [0.0] * 8)
            eh, ec, ee = (gv - rv), (cv - rv), (ev - rv)
            a[0] += float((eh * eh).sum())
            a[1] += float((ec * ec).sum())
            a[2] += float((rv * rv).sum())
            a[3] = max(a[3], float(eh.abs().max()))
            a[4] = max(a[4], float(ec.abs().max()))
            a[5] = max(a[5], float(rv.abs().max()))
            a[6] += float((ee * ee).sum())
            a[7] = max(a[7], float(ee.abs().max()))

    def frob(self, key, label="all"):
        a = self.acc[label]
        return math.sqrt(a[0 if key == "hip" else 1] / a[2]) if a[2] > 0 else (0.0 if a[0 if key == "hip" else 1] == 0 else float("inf"))

    def maxrel(self, key, label="all"):
        a = self.acc[label]
        return a[3 if key == "hip" else 4] / a[5] if a[5] > 0 else (0.0 if a[3 if key == "hip" else 4] == 0 else float("inf"))

    def ratios(self):
        """(frobenius ratio, max ratio) hip / cpu of the whole tensor (for the report)."""
        f, m = self.frob("cpu"), self.maxrel("cpu")
        return (self.frob("hip") / f if f > 0 else float("nan")), (self.maxrel("hip") / m if m > 0 else float("nan"))

    def worst_block(self):
        worst = ("all", 0.0)
        for lb, a in self.acc.items():
            if a[1] > 0 and math.sqrt(a[0] / a[1]) > worst[1]:
                worst = (lb, math.sqrt(a[0] / a[1]))
        return worst

    def assert_sharp(self, yard="torch"):
        """hip <= SHARP x yardstick for both statistics of the whole tensor and the Frobenius one of every block; yard:
        "torch" or "cell" (yardstick_of).  A block the fp64 reference holds at exactly zero (zero-padded units) must be
        exactly zero on both sides."""
        who = "torch's fp32" if yard == "torch" else "the fp32 cell emulation"
        acc = {lb: ([a[0], a[1], a[2], a[3], a[4], a[5]] if yard == "torch" else [a[0], a[6], a[2], a[3], a[7], a[5]])
               for lb, a in self.acc.items()}
        for lb, a in acc.items():
            assert a[0] <= SHARP * SHARP * a[1], \
                (f"{self.name} [{lb}]: Frobenius error {math.sqrt(a[0] / max(a[2], 1e-300)):.3e} of the device against "
                 f"{math.sqrt(a[1] / max(a[2], 1e-300)):.3e} of {who} on the CPU ({math.sqrt(a[0] / a[1]) if a[1] > 0 else float('inf'):.2f} x, "
                 f"allowed {SHARP:g} x)")
        a = acc["all"]
        assert a[3] <= SHARP * a[4], (f"{self.name}: max error {a[3]:.3e} of the device against {a[4]:.3e} of {who} on the "
                                      f"CPU ({a[3] / a[4] if a[4] > 0 else float('inf'):.2f} x, allowed {SHARP:g} x; max |ref| {a[5]:.3e})")
        # the error of the LAST step alone (a [T][N][.] tensor): both statistics
        last = [lb for lb in self.acc if lb.startswith("step ")]
        if last:
            a = acc[last[-1]]
            assert a[3] <= SHARP * a[4], (f"{self.name} [{last[-1]}]: max error {a[3]:.3e} of the device against {a[4]:.3e} of "
                                          f"{who} on the CPU")


def check_outputs(stats, row, ops, outs, cpu32=None, ref64=None, emu32=None):
    """Accumulate into `stats` (name -> Stat) the comparison of outs (name -> CPU fp32 tensor, declared regions only) with the
    fp64 recurrence of `ops`; the yardstick cpu32 is torch's fp32 run of the same recurrence."""
    ref64 = reference(row, ops, torch.float64) if ref64 is None else ref64
    cpu32 = reference(row, ops, torch.float32) if cpu32 is None else cpu32
    emu32 = reference(row, ops, torch.float32, act="cell") if emu32 is None else emu32
    assert set(outs) == set(ref64), f"outputs {sorted(outs)} against the reference's {sorted(ref64)}"
    if "h_fin" in outs:  # exact, whatever the rounding: the state handed to the next chunk IS the last step's hidden state
        assert torch.equal(outs["h_fin"], outs["y"][-1]), "the carried h state is not the last step of the hidden sequence, bit for bit"
    for k, v in outs.items():
        assert v.shape == ref64[k].shape, f"{k}: shape {tuple(v.shape)} against {tuple(ref64[k].shape)}"
        stats.setdefault(k, Stat(k)).add(row, v, cpu32[k], ref64[k], emu32[k])
    return ref64


def draws_for(row, N):
    G = 3 if row.cell == "gru" else 4
    smallest = min(G * row.H1, N * row.H1, row.T * N)
    return max(1, -(-POOL_ELEMS // smallest))


def assert_stats(row, stats, log=print):
    for s in stats.values():
        rf, rm = s.ratios()
        lb, wb = s.worst_block()
        log(f"[rsweep] {row.id} {s.name} [{yardstick_of(row, s.name)}]: n {s.n} emu {math.sqrt(s.acc['all'][6] / max(s.acc['all'][2], 1e-300)):.3e} frob hip {s.frob('hip'):.3e} cpu {s.frob('cpu'):.3e} ({rf:.2f} x) max hip "
            f"{s.maxrel('hip'):.3e} cpu {s.maxrel('cpu'):.3e} ({rm:.2f} x) worst block {lb} {wb:.2f} x")
    for s in stats.values():
        s.assert_sharp(yardstick_of(row, s.name))


# ---- the device side ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return fullsubnet_amd


class Out:
    """An output of `shape` (the last dimension strided by ld >= shape[-1]) behind the sentinel."""

    def __init__(self, dev, shape, ld=None):
        self.shape, self.ld = tuple(shape), ld or shape[-1]
        self.n = math.prod(self.shape[:-1]) * self.ld
        self.buf = torch.full((self.n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)

    @property
    def f(self):
        return self.buf.view(torch.float32)

    def take(self, what):
        assert bool((self.buf[self.n:] == SENTINEL).all()), f"{what}: written outside its declared region"
        full = self.buf[:self.n].view(*self.shape[:-1], self.ld)
        if self.ld > self.shape[-1]:
            assert bool((full[..., self.shape[-1]:] == SENTINEL).all()), f"{what}: columns beyond the declared ones written"
        v = full.view(torch.float32)[..., :self.shape[-1]]
        assert bool(torch.isfinite(v).all()), f"{what}: not every declared element was written"
        return v.contiguous()


def _padded(t, ld):
    if ld == t.shape[-1]:
        return t.contiguous()
    out = torch.zeros(t.shape[:-1] + (ld,), dtype=t.dtype, device=t.device)
    out[..., :t.shape[-1]] = t
    return out


class Device:
    """The row's entry on device operands: outputs behind sentinels, workspaces and save buffers exact and poisoned."""

    def __init__(self, fsn, row, N, ops):
        self.lib, self.L, self.row, self.N = fsn._lib, fsn._lib.lib(), row, N
        self.dev = torch.device("cuda:0")
        self.x = ops["x"].to(self.dev)
        self.dy = ops["dy"].to(self.dev)
        self.w = [[p.to(self.dev).contiguous() for p in lp] for lp in ops["layers"]]
        self.extra = {k: ops[k].to(self.dev).contiguous() for k in ("fc_w", "fc_b", "h0", "c0") if k in ops}
        self.st = self.lib.stream_ptr(self.dev)

    def ws(self, nbytes):
        return self.lib.workspace(nbytes, self.dev).fill_(0xFF)  # 0xFFFFFFFF is a NaN; guarded under FSN_WS_CANARY

    def wp(self, k=None):
        p = self.lib.dev_ptr
        return [p(t) for lp in (self.w if k is None else [self.w[k]]) for t in lp]

    def run(self, ldx, lddx=None, want_dx=True, phases=(7,)):
        r, L, p, T, N = self.row, self.L, self.lib.dev_ptr, self.row.T, self.N
        I, H, H1 = r.I, r.H, r.H1
        x = _padded(self.x, ldx)
        ck = self.lib.check
        out = {}
        if r.entry in ("layer", "gru_layer"):
            q, f = (L.fsn_lstm_layer_fwd_workspace_bytes, L.fsn_lstm_layer_forward) if r.cell == "lstm" else \
                (L.fsn_gru_layer_fwd_workspace_bytes, L.fsn_gru_layer_forward)
            ws, y = self.ws(q(T, N, I, H)), Out(self.dev, (T, N, H))
            ck(f(p(x), ldx, *self.wp(), T, N, I, H, p(y.f), None, 0, ws.data_ptr(), ws.numel(), self.st))
            out["y"] = y.take("hseq")
        elif r.entry == "layer_fc":
            ldo = N + r.ldo_extra
            ws = self.ws(L.fsn_lstm_layer_fc_workspace_bytes(T, N, I, H))
            o = [Out(self.dev, (T, N), ldo) for _ in range(r.O)]
            ck(L.fsn_lstm_layer_forward_fc(p(x), ldx, *self.wp(), T, N, I, H, p(self.extra["fc_w"]), p(self.extra["fc_b"]), r.O,
                                           p(o[0].f), p(o[1].f) if r.O > 1 else None, ldo, ws.data_ptr(), ws.numel(), self.st))
            for k in range(r.O):
                out[f"out{k}"] = o[k].take(f"out{k}")
        elif r.entry == "lstm2":
            ws, y = self.ws(L.fsn_lstm2_fwd_workspace_bytes(T, N, I, H, H1)), Out(self.dev, (T, N, H1))
            ck(L.fsn_lstm2_forward(p(x), ldx, *self.wp(), T, N, I, H, H1, p(y.f), ws.data_ptr(), ws.numel(), self.st))
            out["y"] = y.take("hseq1")
        elif r.entry == "gru2":
            ws, y = self.ws(L.fsn_gru2_fwd_workspace_bytes(T, N, I, H)), Out(self.dev, (T, N, H))
            ck(L.fsn_gru2_forward(p(x), ldx, *self.wp(), T, N, I, H, p(y.f), ws.data_ptr(), ws.numel(), self.st))
            out["y"] = y.take("hseq1")
        elif r.entry in ("layer_train", "gru_train"):
            lstm = r.cell == "lstm"
            G = 4 if lstm else 3
            nsave = (L.fsn_lstm_layer_save_bytes if lstm else L.fsn_gru_layer_save_bytes)(T, N, H)
            save = self.ws(nsave)
            ws, y = self.ws((L.fsn_lstm_layer_fwd_workspace_bytes if lstm else L.fsn_gru_layer_fwd_workspace_bytes)(T, N, I, H)), \
                Out(self.dev, (T, N, H))
            ck((L.fsn_lstm_layer_forward if lstm else L.fsn_gru_layer_forward)(
                p(x), ldx, *self.wp(), T, N, I, H, p(y.f), save.data_ptr(), save.numel(), ws.data_ptr(), ws.numel(), self.st))
            out["y"] = y.take("hseq")
            hseq = y.f[:T * N * H]
            ws = self.ws((L.fsn_lstm_layer_bwd_workspace_bytes if lstm else L.fsn_gru_layer_bwd_workspace_bytes)(T, N, I, H))
            dx = Out(self.dev, (T, N, I), lddx) if want_dx else None
            dwi, dwh = Out(self.dev, (G * H, I)), Out(self.dev, (G * H, H))
            dbs = [Out(self.dev, (G * H,)) for _ in range(1 if lstm else 2)]
            ck((L.fsn_lstm_layer_backward if lstm else L.fsn_gru_layer_backward)(
                p(self.dy), p(x), ldx, p(self.w[0][0]), p(self.w[0][1]), T, N, I, H, p(hseq), save.data_ptr(),
                p(dx.f) if want_dx else None, lddx, p(dwi.f), p(dwh.f), *[p(b.f) for b in dbs], ws.data_ptr(), ws.numel(), self.st))
            if want_dx:
                out["dx"] = dx.take("dx")
            out["dw_ih"], out["dw_hh"] = dwi.take("dw_ih"), dwh.take("dw_hh")
            if lstm:
                out["db"] = dbs[0].take("db")
            else:
                out["db_ih"], out["db_hh"] = dbs[0].take("db_ih"), dbs[1].take("db_hh")
        elif r.entry == "lstm2_train":
            nsave = L.fsn_lstm_layer_save_bytes(T, N, H)
            s0, s1 = self.ws(nsave), self.ws(nsave)
            ws = self.ws(L.fsn_lstm2_train_workspace_bytes(T, N, I, H, 0))
            y0, y1 = Out(self.dev, (T, N, H)), Out(self.dev, (T, N, H))
            ck(L.fsn_lstm2_forward_train(p(x), ldx, *self.wp(), T, N, I, H, p(y0.f), p(y1.f), s0.data_ptr(), s1.data_ptr(), nsave,
                                         ws.data_ptr(), ws.numel(), 0, self.st))
            out["y0"], out["y"] = y0.take("hseq0"), y1.take("hseq1")
            ws = self.ws(L.fsn_lstm2_bwd_workspace_bytes(T, N, I, H, 0))
            dx = Out(self.dev, (T, N, I), lddx) if want_dx else None
            g = dict(dw_ih0=Out(self.dev, (4 * H, I)), dw_hh0=Out(self.dev, (4 * H, H)), db0=Out(self.dev, (4 * H,)),
                     dw_ih1=Out(self.dev, (4 * H, H)), dw_hh1=Out(self.dev, (4 * H, H)), db1=Out(self.dev, (4 * H,)))
            args = [p(self.dy), p(x), ldx, p(self.w[0][0]), p(self.w[0][1]), p(self.w[1][0]), p(self.w[1][1]), T, N, I, H,
                    p(y0.f[:T * N * H]), p(y1.f[:T * N * H]), s0.data_ptr(), s1.data_ptr(), p(dx.f) if want_dx else None, lddx] + \
                   [p(v.f) for v in g.values()] + [ws.data_ptr(), ws.numel(), 0]
            if phases == (7,):
                ck(L.fsn_lstm2_backward(*args, self.st))
            else:
                for ph in phases:
                    ck(L.fsn_lstm2_backward_phase(*args, ph, self.st))
            if want_dx:
                out["dx"] = dx.take("dx")
            for k, v in g.items():
                out[k] = v.take(k)
        else:  # the state entries: 1 + 5 + the rest steps from the carried state
            lstm = r.cell == "lstm"
            y = Out(self.dev, (T, N, H))
            hs = Out(self.dev, (N, H))
            hs.f[:N * H] = self.extra["h0"].reshape(-1)
            cs = Out(self.dev, (N, H))
            cs.f[:N * H] = self.extra["c0"].reshape(-1)
            if lstm:
                pk = self.ws(L.fsn_lstm_layer_packed_bytes(I, H))
                ck(L.fsn_lstm_layer_pack(*self.wp(), I, H, pk.data_ptr(), pk.numel(), self.st))
            t0 = 0
            for k in (1, 5, T):
                k = min(k, T - t0)
                if k <= 0:
                    break
                xk = x[t0:t0 + k].contiguous()
                yk = ctypes.c_void_p(y.f.data_ptr() + 4 * t0 * N * H)
                if lstm:
                    ws = self.ws(L.fsn_lstm_layer_state_workspace_bytes(k, N, H))
                    ck(L.fsn_lstm_layer_forward_state(p(xk), ldx, pk.data_ptr(), k, N, I, H, yk, p(hs.f), p(cs.f), ws.data_ptr(),
                                                      ws.numel(), self.st))
                else:
                    ws = self.ws(L.fsn_gru_layer_fwd_workspace_bytes(k, N, I, H))
                    ck(L.fsn_gru_layer_forward_state(p(xk), ldx, *self.wp(), k, N, I, H, yk, p(hs.f), ws.data_ptr(), ws.numel(),
                                                     self.st))
                t0 += k
            out["y"], out["h_fin"] = y.take("hseq"), hs.take("h_state")
            if lstm:
                out["c_fin"] = cs.take("c_state")
        self.lib.check_canaries()
        return out


def check_plan(L, row, N, cus):
    for name, args, expected in row.queries:
        want = expected(N, cus) if callable(expected) else expected
        got = getattr(L, name)(*args(row, N))
        assert got == want, f"{row.id}: {name}{args(row, N)} = {got}, the row was written for {want}"


def _same(a, b, what):
    for k in a:
        if k in b:
            assert torch.equal(a[k], b[k]), f"{k}: {what}: not bit-identical"


def run_draw(fsn, row, N, draw, stats, first):
    ops = make_operands(row, N, draw)
    d = Device(fsn, row, N, ops)
    train = row.entry in TRAIN_ENTRIES
    lddx = ru16(row.I) + 4 if train else None
    before = fsn._lib.persist_stats()[0]
    got = d.run(row.ldx, lddx)
    added = fsn._lib.persist_stats()[0] - before
    if row.launches is not None:
        assert (added > 0) == row.launches, f"{row.id}: {added} persistent launches, the row expects {'some' if row.launches else 'none'}"
    if first:
        _same(d.run(row.ldx, lddx), got, "two calls in a row")
        if row.alt_ldx:
            _same(d.run(row.ldx + 16, None if lddx is None else row.I), got, "another ldx / lddx")
        if train:
            _same(d.run(row.ldx, lddx, want_dx=False), got, "dx == NULL")
        if row.entry == "lstm2_train":
            _same(d.run(row.ldx, lddx, phases=(1, 4, 2)), got, "phases 1, 4, 2 against 7")
    assert fsn._lib.stream_status(d.dev) == (0, 0), "the stream carries a timeout record"
    host = {k: v.cpu() for k, v in got.items()}
    if row.Hreal < row.H:  # zero-padded units: exactly zero, in the hidden sequence and in their gradient rows
        G = 4
        for k, v in host.items():
            if k in ("y", "y0") and not (row.entry == "lstm2_train" and k == "y"):
                assert bool((v[..., row.Hreal:] == 0).all()), f"{k}: zero-padded units are not exactly 0.0"
            if k in ("dw_ih", "dw_hh", "db", "dw_ih0", "dw_hh0", "db0"):
                assert bool((v.view(G, row.H, -1)[:, row.Hreal:] == 0).all()), f"{k}: gradient rows of zero-padded units are not exactly 0.0"
            if k == "dw_hh":
                assert bool((v[:, row.Hreal:] == 0).all()), "dw_hh: gradient columns of zero-padded units are not exactly 0.0"
    if row.cell == "gru" and train:  # the two bias gradients differ in the n block only
        assert torch.equal(host["db_ih"][:2 * row.H], host["db_hh"][:2 * row.H]), "db_ih / db_hh differ outside the n block"
        assert not torch.equal(host["db_ih"][2 * row.H:], host["db_hh"][2 * row.H:]), "db_ih / db_hh equal in the n block"
    del d
    check_outputs(stats, row, ops, host)


@pytest.mark.parametrize("row", TABLE, ids=[r.id for r in TABLE])
def test_recurrent_sweep(fsn, row):
    t0 = time.time()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = row.N(cus)
    check_plan(fsn._lib.lib(), row, N, cus)
    stats = {}
    for draw in range(draws_for(row, N)):
        run_draw(fsn, row, N, draw, stats, draw == 0)
    assert_stats(row, stats)
    print(f"[rsweep] {row.id}: {time.time() - t0:.1f} s")


def test_gru2_forward_refuses_off_the_chain(fsn):
    """fsn_gru2_forward has no generic path: off the chain (80 rows) it returns an error and writes nothing."""
    L, lib = fsn._lib.lib(), fsn._lib
    row = Row("gru2-off-chain", "gru_step", "gru2", 2, 5, 20, 32, 512)
    N = row.N()
    assert L.fsn_gru2_forward_supported(row.T, N, row.H) == 0
    d = Device(fsn, row, N, make_operands(row, N, 0))
    y = Out(d.dev, (row.T, N, row.H))
    ws = d.ws(max(L.fsn_gru2_fwd_workspace_bytes(row.T, N, row.I, row.H), 256))
    rc = L.fsn_gru2_forward(lib.dev_ptr(_padded(d.x, row.ldx)), row.ldx, *d.wp(), row.T, N, row.I, row.H, lib.dev_ptr(y.f),
                            ws.data_ptr(), ws.numel(), d.st)
    assert rc != 0, "fsn_gru2_forward accepted a shape off the chain"
    torch.cuda.synchronize()
    assert bool((y.buf == SENTINEL).all()), "the refused call wrote to its output"
