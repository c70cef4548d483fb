"""The 16-bit training arithmetic's conversion and product kernels held to an exact emulation over a sweep.  Needs an MI355X:
python -m pytest tests/test_gpu_amp_sweep.py -m gpu -s

Every shipped configuration trains under use_amp: to16_kernel, gemm_tn16h (192 x 192 and 192 x 384 tiles), gemm_tn16n,
gemm_dx16 and the `arith` forms of gemm_tn form every weight gradient and layer 0's dx of the sub-band pair.  They are
called here through the fsn_debug_* entries (the internal launchers unchanged behind size checks) with operands GIVEN in 16
bits, so no rounding of an fp32 intermediate can fall on the other side of a 16-bit boundary: the emulation of each product is
the fp64 product of the very same 16-bit values.  The design is that of tests/test_gpu_linear_sweep.py, whose Stat does
the comparing; tests/test_amp_sweep_cpu.py runs this module's checkers on the CPU against correct and corrupted stand-ins.

to16      bit-exact against tensor.to(torch.float16 / torch.bfloat16) viewed as int16 (NaN compared as NaN only) on
          `to16_table`: Gaussians at scales 2^-30 .. 2^20, every exact tie of both types in a few binades, fp16's subnormal
          range with its ties, +-65504 / +-65520 and beyond, the fp32 values around bf16's overflow, +-0, +-inf, NaN, and
          fp32 subnormals (bf16 keeps fp32's exponent range: they are its subnormals).  n = 4 and one n past a whole grid
          pass (2048 x 256 x 4 + 4).
products  two kinds of operands, as in the linear sweep:
          * integers (A in {-2 .. 2}, B in {0 .. 3}: exact in both types), an index pattern and a hash.  The test asserts
            sum_k |a_k| |b_k| < 2^24 on the reference; the result must EQUAL the fp64 product.  Tolerance 0, derived.
          * Gaussians rounded to the type beforehand.  hard: |C - C_64| <= (K + S + 2) 2^-24 (|A|^T |B|)_ij per element, S
            the K splits from fsn_debug_tn16_plan / fsn_debug_tn_plan (1 for dx); sharp: the rms over elements of
            err_ij / (|A|^T |B|)_ij at most SHARP = 4 x that of torch's CPU fp32 product of the same operands.
          gemm_tn with `arith` takes fp32 operands that are NOT representable; its reference is r(A)^T r(B) in fp64 and its
          yardstick the CPU fp32 product of r(A), r(B).
In every row: both arithmetics; outputs behind a NaN sentinel with a 1024-element guard (and dx's columns I .. lddx - 1) that
must survive; workspace of exactly the queried size filled with 0xFF; two calls in a row give the same bits.  TN16H names
every (M, Nc) class the planner distinguishes at 256 CUs with the form and split count each K was written for, asserted
through the query: another device or a changed plan rule fails there instead of quietly testing another path.
test_tn16h_plan_boundaries walks K in steps of 16 through the query, and at the first K on either side of the first
BOUNDARIES changes of plan of every class runs the product where there is a plan and requires a refusal that writes
nothing where there is none.

The two-layer entries (fsn_lstm2_forward_train, fsn_lstm2_backward, fsn_lstm2_backward_phase under f16, bf16 and + s16) run
on PATHS, one row per path that tests/test_gpu_amp.py's single shape does not reach (H = 384, written for 256 CUs; a row
whose plan, fsn_debug_lstm2_plan16, does not hold on the device fails).  What each path does, and what the emulation takes:
  g16-full                  both directions on lstm_group16_kernels.hip, every product from rounded operands.  T 1: no tn16h,
                            dw_hh by memset; T 2 at 1536 rows: K = 1536 has no tn16h plan, gemm_tn rounds fp32 buffers on load
  g16-left                  the same, and 16 / 128 rows beside the launch on the fp32 step kernels: their recurrence products
                            take UNROUNDED operands in both directions, their gate gradients are rounded for the products
  g16-in16-off              I 12 / ldx 16 and I 64 / ldx 64: the forward layer by layer in fp32 (nothing rounded), the BPTT on
                            the 16-bit kernel, dx a plain fp32 GEMM of unrounded gate gradients
  fwd-group16-bwd-by-layer  56 clusters: the forward on lstm2_group_kernel<.., F16> (rounded), the backward layer by layer in fp32
  hook-0 / -2 / -3          fsn_debug_g16_kernels: the fp32-era group kernels under the arithmetic; the large products from fp32
                            buffers; dx and dW_ih0 from fp32 gate gradients
  h320pad, saturated        Hreal 320 (layer 0's padded units: h, g, c exactly 0.0, i / f / o exactly 0.5, their gradient rows
                            and the dw_hh0 / dw_ih1 columns they multiply exactly 0.0; layer 1 has no padded unit); gain 6 on
                            g16-full and g16-left
  scale                     dy at 1, 64 and 2^14 on g16-full T 2 (the loss scale: gate gradients from fp16's subnormals to 10^4)
Where the table leaves the issue's, and why: "left 8" is N 2176 (32 clusters + 8 tiles), not N 1664 - at 256 CUs 1664 rows are 26
whole clusters and nothing is left; N 1552 T 4 is kept though K = 4656 has no tn16h plan (a plan needs every K split non-empty:
fsn_debug_tn16_plan), its K tail is covered by part 1's tail rows; I 32 runs at T 2 and on hook-0 T 9, I 20 elsewhere (both take
the same 32-column kernels); + s16 runs on every row but scale, the left-over rows included; the boundary walk visits the first
BOUNDARIES = 4 plan changes of each class up to K = 2^17 - the changes recur with K without end, each visit is both sides.
2a, forward (check_one_step): under fp32 saves the device's own gates, c_t, h_t of EVERY step of both layers against the one
step formed in fp64 from the device's h_{t-1}, c_{t-1} (layer 1: the device's hseq0) with the operands rounded as the path
rounds them - no rounding can flip, the state is the device's.  Yardstick: the same one step in CPU fp32 with lstm_cell.h's
formulas; stat_hip <= 4 x for the relative Frobenius error and max |err| / max |ref|, whole tensor, per step, per 16-row
tile, every gate a tensor of its own.  The rule for the yardstick's sums is check_one_step's docstring.
2a under + s16 (check_saved16): the 16-bit gates and h_t decoded from the save slots (row stride 2G, h_t at + G) within half
a 16-bit ulp + 4 x the yardstick of the fp64 one step, h_t equal to the rounded hidden sequence bit for bit.
2b (check_recurrence): y0, y, dx and the six gradients of the whole recurrence against the autograd of emulated_path - the
recurrence with every product rounded as Path.rounding says the path rounds it - in fp64.  Yardstick: the CPU fp32 run of the
same emulation, with torch's activations or lstm_cell.h's formulas by the recurrent sweep's rule yardstick_of (row, output);
4 x for the whole tensor, per step, per gate / column block, and per 16-row tile by assert_recurrence's rule.  The T = 1 rows
are the one-step backward (dg1, dh0 = r(dg1) r(W_ih1), dg0, dx, the six gradients; dw_hh exactly 0.0), formed by the same
autograd from the inputs, not from the device's saves: its one rounding of hseq0 into layer 1 can flip.  Printed with every
output: the fp32 mode's distance from the emulation.
2c, bit for bit: two calls in a row (forward with its saves, backward); dx == NULL; lddx; phases 1, 4, 2 and 8, 1, 2 | 16, 4
against 7; + s16 leaves hseq0 / hseq1 unchanged, and changes NOTHING where one direction is not on the 16-bit kernels; the
hooks change only the outputs their products feed; the persistent-launch counter moves exactly where the plan has
clusters; the stream status stays clean.  LSTM2_PLAN asserts further plans without running a kernel.
2a, backward at T = 1 (check_backward_t1): the same outputs against the backward written out by hand from the device's saves,
held to its CPU fp32 run at 4 x (g16-full and hook-0).
Not in this module: 2b under + s16 (the emulation does not round the saved gates).

Fixed on the way (each failed here first):
  * fsn_gemm_tn16h_supported accepted fsn_tn_plan's square plan, which counts K in 16 rows; the launcher re-splits in chunks
    of 32 and refuses when the split count changes.  lstm2_backward_phases asked the query for K = (T - 1) N only, while
    dW_ih1 sums T N rows.  fsn_lstm2_backward failed with "gemm_tn16h: no plan" at e.g. T 4 N 1552 and T 2 N 2064 under both
    arithmetics (test_backward_where_tn16h_has_no_plan).  One rule now serves launcher, query and plan, for both K.
  * gemm_tn's reduction added the K % 16 tail rows from UNROUNDED fp32 operands under a 16-bit arithmetic:
    tn-arith M 1536 Nc 384 K 2069 f16 stood at 8.44 u rms against 0.14 u of the CPU product (60 x); after: 0.071 u (0.5 x).
  * FSN_ARITH_SAVES16 reached the 16-bit BPTT launch whatever the forward had done: with I 12 or I 64 the forward runs layer
    by layer and saves fp32 gates, which that launch decoded as 16-bit ones (train_arith_of asks for + s16 by default).
    The plan now puts the flag in force only where both directions run the 16-bit kernels; elsewhere + s16 is bit-equal
    to fp32 saves in every output (asserted on g16-in16-off, fwd-group16-bwd-by-layer and hook-0), and the fp32-saves run of
    those rows meets 2b (I 12 / I 64: dx at most 1.5 x, gradients at most 1.7 x).  No "before" figure: the old behaviour was read, not run.

Seen on an MI355X (the module: 40 s, 149 tests, of which test_lstm2_paths 31 s), worst hip / yardstick ratio per output and its row:
  part 1, sharp rms   tn16h 1.2 x (square-1-tail16 M 192 N 192 K 32784 bf16), tn16n 1.5 x (M 384 N 31 K 8240 bf16), gemm_tn
                      arith 0.9 x (M 1536 N 384 K 2069 bf16), dx16 2.4 x (G 1920 I 31 bf16: one chain of K = 1920).  Hard bound: at
                      most 0.004 of it (dx16 G 384).  Every integer row equals fp64; to16 is bit-exact in both types, fp16 and
                      bf16 subnormals included; every refusal beside a plan boundary wrote nothing.
  2a, Frobenius       gates i, f, o 1.23 x (saturated T 3 N 1536 bf16), g 1.30 x, c 1.28 x, h 1.11 x (g16-full T 9 bf16)
  2a, max             gates 2.4 x (g: fwd-group16-bwd-by-layer T 2 N 3584 bf16), c 2.1 x, h 1.4 x; worst block 1.41 x (g, step 1)
  2a + s16            every decoded gate and h_t within the bound (worst element at 1.000 of it: a value on a tie)
  2a, T = 1 backward  dx and every gradient 1.00 - 1.12 x in both statistics (worst: dw_ih0, hook-0 T 1 bf16); dw_hh exactly 0.0
  2b, Frobenius       dw_ih0 2.4 x, dw_hh0 2.6 x, db0 2.6 x, dw_ih1 2.7 x, dw_hh1 2.8 x, db1 2.9 x (all g16-left T 3 N 2176 bf16),
                      dx 2.6 x (g16-left T 4 N 1552 bf16), y0 2.6 x, y 3.1 x (g16-in16-off T 3 I 64 f16: the fp32 forward's
                      chain sums); g16-full rows 1.0 - 1.3 x on every output (T 9 f16: dx 1.07 x, dw_hh1 1.29 x)
  fp32 mode           its distance from the emulation, relative Frobenius: gradients 3e-4 .. 9e-4 under f16, 2e-3 .. 7e-3 under
                      bf16 (e.g. g16-full T 2 N 1536 f16: dw_ih0 4.3e-4 against a yardstick of 1.0e-4; T 9: dx 4.4e-4 against
                      2.2e-4).  4 x the yardstick lies below that distance on 172 of the 180 (row, type, output) of the T <= 2
                      rows - they hold the arithmetic (the other 8 miss by at most 4 %) - and on 190 of 208 from T = 3 on; the
                      rest, T 9 foremost (dx: 8.9e-4 allowed against 4.4e-4), hold structure only.
"""
import ctypes
import time

import pytest
import torch

import test_gpu_recurrent_sweep as R
from test_gpu_linear_sweep import GUARD, SENTINEL, SHARP, Stat, _int_block

pytestmark = pytest.mark.gpu

ARITHS = {"f16": (2, torch.float16), "bf16": (3, torch.bfloat16)}
SAVES16 = 0x100
NAN16 = {"f16": 0x7E00, "bf16": 0x7FC0}  # a quiet NaN of each type: what surrounds an operand embedded in a larger buffer
ERR_ARG = -1
BOUNDARIES = 4  # plan changes per class that test_tn16h_plan_boundaries visits


def r16(t, ar):
    """t rounded to the arithmetic's type (nearest even), as fp32."""
    return t.to(ARITHS[ar][1]).float()


def ru4(n):
    return (n + 3) // 4 * 4


# ---- to16 ---------------------------------------------------------------------------------------------------------------

def to16_table():
    """fp32 inputs of the conversion (CPU tensor, a multiple of 4 long); see the module docstring."""
    g = torch.Generator().manual_seed(16)
    parts = [torch.randn(512, generator=g) * 2.0 ** e for e in range(-30, 21)]
    k = torch.arange(1024, dtype=torch.float64)
    for e in (-14, -1, 0, 7, 15):  # every tie of fp16 (10 fraction bits) in the binade [2^e, 2^(e+1))
        parts.append(((1024 + k + 0.5) * 2.0 ** (e - 10)).float())
    k7 = torch.arange(128, dtype=torch.float64)
    for e in (-126, -20, 0, 15, 16, 100, 127):  # ... and of bf16 (7 fraction bits)
        parts.append(((128 + k7 + 0.5) * 2.0 ** (e - 7)).float())
    # fp16's subnormal range: its values k 2^-24, its ties, and Gaussians across it; the smallest normal's neighbours
    parts += [(k * 2.0 ** -24).float(), ((k + 0.5) * 2.0 ** -24).float(), torch.randn(1024, generator=g) * 2.0 ** -17,
              torch.randn(1024, generator=g) * 2.0 ** -24]
    big = torch.tensor([65504.0, 65519.996, 65520.0, 65520.004, 65536.0, 1e5, 3.3895313892515355e38, 3.3961775292304601e38,
                        3.3961777e38, 3.4e38, 3.4028234663852886e38, float("inf"), 0.0, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23),
                        2.0 ** -24, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12)], dtype=torch.float64).float()
    parts += [big, torch.nextafter(big, torch.zeros_like(big)), torch.nextafter(big, torch.full_like(big, float("inf")))]
    # fp32 subnormals (bf16's own subnormals and ties between them)
    parts.append((torch.arange(1, 257, dtype=torch.float64) * 2.0 ** -134).float())
    parts.append(torch.tensor([2.0 ** -149, 2.0 ** -134, 2.0 ** -133, 3 * 2.0 ** -135, 2.0 ** -127, 2.0 ** -126], dtype=torch.float64).float())
    parts.append(torch.tensor([float("nan")] * 4))
    v = torch.cat(parts)
    v = torch.cat([v, -v])
    return torch.cat([v, torch.zeros(-v.numel() % 4)])


def to16_mismatches(src, got16, ar):
    """Elements where got16 (int16) is not tensor.to(type) of src bit for bit; a NaN only has to be a NaN."""
    dt = ARITHS[ar][1]
    want = src.to(dt)
    nan = torch.isnan(src)
    bad = (got16 != want.view(torch.int16)) & ~nan
    bad |= nan & ~torch.isnan(got16.view(dt))
    return bad.nonzero().flatten()


def assert_to16(src, got16, ar):
    bad = to16_mismatches(src, got16, ar)
    if bad.numel():
        i = int(bad[0])
        want = int(src[i:i + 1].to(ARITHS[ar][1]).view(torch.int16)) & 0xFFFF
        raise AssertionError(f"to16 {ar}: {bad.numel()} of {src.numel()} elements differ; first at {i}: {float(src[i])!r} -> "
                             f"0x{int(got16[i]) & 0xFFFF:04x}, expected 0x{want:04x}")


# ---- products: rows -----------------------------------------------------------------------------------------------------

class Row:
    """One product C [M][Nc] = A^T B over K rows.  kind: tn16h / tn16n / tn.  form, splits: what fsn_debug_tn16_plan must say
    (tn16h / tn16n; None: not asserted), wide = 0: through fsn_debug_tn16h_wide(0)."""

    def __init__(self, kind, path, M, Nc, K, form=None, splits=None, wide=1, layout="plain"):
        self.kind, self.path, self.M, self.Nc, self.K = kind, path, M, Nc, K
        self.form, self.splits, self.wide, self.layout = form, splits, wide, layout

    @property
    def id(self):
        return f"{self.kind}-{self.path}-M{self.M}-N{self.Nc}-K{self.K}"

    def scaled(self, k_max):
        """The same row with fewer k rows (the CPU self-test of the checker); K % 32 is kept."""
        if self.K <= k_max:
            return self
        return Row(self.kind, self.path, self.M, self.Nc, k_max + self.K % 32, None, None, self.wide, self.layout)


def _tn16h_rows():
    rows = []
    # (M, Nc) classes at 256 CUs: tiles = (M / 192) (Nc / 192) must divide 32 (whole K splits per XCD); the 192 x 384 form
    # halves the tiles and doubles the splits where Nc % 384 == 0, from a larger K on.  `first`: the smallest K with a plan.
    #   class            M     Nc   first  its form, splits      a K on the wide form (32-row chunks) and its splits
    classes = (("ship", 1536, 384, 2048, 1, 16, 4000, 32),     # the sub-band pair's dW_hh / dW_ih1
               ("square-1", 192, 192, 32768, 1, 256, None, 0),  # the smallest shape: one tile, 256 splits, never wide
               ("square-2", 384, 192, 16384, 1, 128, None, 0),  # Nc % 384 != 0: never wide
               ("wide-1", 192, 384, 16384, 1, 128, 32672, 256),  # one wide tile
               ("tiles-32", 1536, 768, 1024, 1, 8, 1952, 16),   # the most tiles a plan takes
               ("wide-only", 1536, 1536, 928, 2, 8, None, 0))   # 64 square tiles have no plan: the 192 x 384 form alone
    for name, M, Nc, first, form, s, kw, sw in classes:
        rows.append(Row("tn16h", f"{name}-first", M, Nc, first, form, s))
        rows.append(Row("tn16h", f"{name}-tail16", M, Nc, first + 16, form, s))  # K % 32 == 16: tail rows in the reduction
        if kw:
            rows.append(Row("tn16h", f"{name}-wide", M, Nc, kw + 16, 2, sw))  # K % 32 == 16 on the wide form
            rows.append(Row("tn16h", f"{name}-wide-forced-square", M, Nc, kw + 16, 1, sw // 2, wide=0))
    # every tail length's ends, the shorter-last-split case and the layouts of the training step, at the shipped class
    rows.append(Row("tn16h", "ship-tail1", 1536, 384, 2049, 1, 16))
    rows.append(Row("tn16h", "ship-tail31", 1536, 384, 2079, 1, 16))
    rows.append(Row("tn16h", "ship-uneven-tail16", 1536, 384, 4368, 1, 16))   # 136 chunks over 16 splits of 9: the last one takes 1
    rows.append(Row("tn16h", "ship-T3-N1536", 1536, 384, 3072, 1, 16))
    rows.append(Row("tn16h", "ship-h16-saved", 1536, 384, 3072, 1, 16, layout="saved"))    # B at + G in rows of 2 G (the save slots)
    rows.append(Row("tn16h", "ship-h16-saved-wide", 1536, 384, 4016, 2, 32, layout="saved"))
    rows.append(Row("tn16h", "ship-offset", 1536, 384, 3072, 1, 16, layout="offset"))      # A starts N x G elements into its buffer
    rows.append(Row("tn16h", "ship-offset-wide", 1536, 384, 4016, 2, 32, layout="offset"))
    return rows


def _tn16n_rows():
    rows = []
    # K32 = 2048 is the lower bound; 8240 = 257 chunks + 16 tail rows.  Splits: one workgroup per CU or what the workspace of
    # an [M][Nc + 1] product holds of [M][32] partials
    splits = {(384, 1): (16, 16, 16), (384, 17): (64, 64, 129), (384, 20): (64, 64, 129), (384, 31): (64, 64, 129),
              (384, 32): (64, 64, 129), (1536, 1): (5, 5, 5), (1536, 17): (32, 32, 43), (1536, 20): (32, 32, 52),
              (1536, 31): (64, 64, 52), (1536, 32): (64, 64, 52)}
    for (M, Nc), ss in splits.items():
        for K, s in zip((2048, 2064, 8240), ss):
            rows.append(Row("tn16n", "narrow", M, Nc, K, 1, s))
    return rows


def _tn_rows():
    rows = []
    for Nc in (384, 20):
        # 1536: T 2 at 1536 rows, where tn16h has no plan and the products round fp32 buffers on load; 2069: a K % 16 tail
        for K in (1536, 2069):
            rows.append(Row("tn", "arith", 1536, Nc, K))
    return rows


TN16H, TN16N, TN = _tn16h_rows(), _tn16n_rows(), _tn_rows()
TABLE = TN16H + TN16N + TN
DX16 = [(G, I) for G in (384, 1536, 1920) for I in (1, 17, 31, 32)]
DX16_ROWS = (16, 48, 1552)


# ---- products: operands and the checker -----------------------------------------------------------------------------------

def make_operands(M, Nc, K, mode, draw, ar, device, representable=True):
    """A [K][M], B [K][Nc] as fp32 holding values of the 16-bit type (representable) or plain fp32 Gaussians."""
    if mode == "int":
        kind = "pattern" if draw == 0 else "hash"
        return _int_block(kind, 1, 0, K, M, -2, 2, device), _int_block(kind, 0, 0, K, Nc, 0, 3, device)
    g = torch.Generator(device=device).manual_seed(1000 * draw + K + 7 * M + 13 * Nc)
    A = torch.randn(K, M, generator=g, device=device)
    B = torch.randn(K, Nc, generator=g, device=device)
    return (r16(A, ar), r16(B, ar)) if representable else (A, B)


def reference(A, B):
    """(A^T B, |A|^T |B|) in fp64, on the operands' device, returned on the CPU."""
    a, b = A.double(), B.double()
    return (a.t() @ b).cpu(), (a.abs().t() @ b.abs()).cpu()


def cpu_product(A, B):
    """torch's own fp32 CPU product: the implementation whose error the sharp bound is measured against."""
    return A.cpu().t() @ B.cpu()


def check_product(name, K, splits, got, A, B, mode):
    """Compare got [M][Nc] (CPU fp32) with the fp64 product of A [K][M], B [K][Nc]; returns the Stat (asserted)."""
    stat = Stat(name, K + splits + 2)
    ref, ref_abs = reference(A, B)
    stat.add(got, ref, ref_abs, cpu_product(A, B) if mode == "gauss" else None)
    if mode == "int":
        stat.assert_exact()
    else:
        stat.assert_rounding()
    return stat


def tn16_plan(L, narrow, M, Nc, K):
    s, f = ctypes.c_int(0), ctypes.c_int(0)
    assert L.fsn_debug_tn16_plan(narrow, M, Nc, K, ctypes.byref(s), ctypes.byref(f)) == 0
    return f.value, s.value


def check_plan(L, row):
    """(form, splits) of the row's product; asserted against what the row was written for (256 CUs)."""
    if row.kind == "tn":
        s, bound = ctypes.c_int(0), ctypes.c_long(0)
        assert L.fsn_debug_tn_plan(row.M, row.Nc, row.K, 2, ctypes.byref(s), ctypes.byref(bound)) == 0
        assert 1 <= s.value <= bound.value
        return 1, s.value
    form, s = tn16_plan(L, 1 if row.kind == "tn16n" else 0, row.M, row.Nc, row.K)
    if row.form is not None:
        assert (form, s) == (row.form, row.splits), f"{row.id}: form {form} with {s} K splits, the row expects {row.form} with {row.splits}"
    return form, s


# ---- the device side ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    return fullsubnet_amd


def _sentinel(n, dev):
    return torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _as16(t, ar):
    """fp32 tensor of representable values -> its 16-bit image (int16)."""
    return t.to(ARITHS[ar][1]).view(torch.int16)


def _embed(t16, ld, col0, rows_before, ar):
    """t16 [K][n] inside a NaN-filled [rows_before + K][ld] buffer at column col0; returns (buffer, view of its first element)."""
    K, n = t16.shape
    fill = NAN16[ar] - (1 << 16) if NAN16[ar] >= 1 << 15 else NAN16[ar]
    buf = torch.full((rows_before + K, ld), fill, dtype=torch.int16, device=t16.device)
    buf[rows_before:, col0:col0 + n] = t16
    return buf, buf[rows_before:, col0:]


def launch_tn(fsn, row, ar, A, B, ldb=None, layout="plain", expect=0):
    """One call of the row's entry on A [K][M], B [K][Nc] (fp32 on the device).  Returns C [M][Nc] (device), or None after a
    refusal (expect = ERR_ARG), in which case nothing may have been written."""
    lib, L = fsn._lib, fsn._lib.lib()
    M, Nc, K = row.M, row.Nc, row.K
    dev = A.device
    nbytes = L.fsn_debug_gemm_tn_workspace_bytes(M, Nc, K)
    ws = lib.workspace(nbytes, dev).fill_(0xFF)
    buf = _sentinel(M * Nc, dev)
    C = buf.view(torch.float32)
    keep = []
    if row.kind == "tn":
        a, b, lda, ldb = A.contiguous(), B.contiguous(), M, Nc
        fn = L.fsn_debug_gemm_tn
    else:
        a16, b16 = _as16(A, ar), _as16(B, ar)
        lda, ldb = M, (ldb or Nc)
        if row.kind == "tn16n":  # rows of 32 columns, those beyond Nc zero
            ldb = 32
            b = torch.zeros((K, 32), dtype=torch.int16, device=dev)
            b[:, :Nc] = b16
        elif layout == "saved":  # the save slots: a row of 4H fp32 gates = 2 G 16-bit words, h_t in its second half
            hold, b = _embed(b16, 2 * M, M, 0, ar)
            keep.append(hold)
            ldb = 2 * M
        else:
            b = b16.contiguous()
        if layout == "offset":  # an operand that starts N x G elements into its buffer
            hold, a = _embed(a16, M, 0, K // 2, ar)
            keep.append(hold)
        else:
            a = a16.contiguous()
        fn = L.fsn_debug_gemm_tn16n if row.kind == "tn16n" else L.fsn_debug_gemm_tn16h
    rc = fn(_ptr(a), lda, _ptr(b), ldb, _ptr(C), Nc, M, Nc, K, ws.data_ptr(), ws.numel(), ARITHS[ar][0], lib.stream_ptr(dev))
    if expect != 0:
        assert rc == expect, f"{row.id} {ar}: returned {rc}, expected the refusal {expect}"
        assert bool((buf == SENTINEL).all()), f"{row.id} {ar}: refused, yet C was written"
        assert bool((ws == 0xFF).all()), f"{row.id} {ar}: refused, yet the workspace was written"
        return None
    lib.check(rc)
    assert bool((buf[M * Nc:] == SENTINEL).all()), f"{row.id} {ar}: C written outside its declared region"
    C = C[:M * Nc].view(M, Nc)
    assert bool(torch.isfinite(C).all()), f"{row.id} {ar}: not every declared element was written"
    return C


def run_row(fsn, row, ar, splits):
    dev = torch.device("cuda:0")
    out = []
    for mode, draws in (("int", 2), ("gauss", 1)):
        for draw in range(draws):
            A, B = make_operands(row.M, row.Nc, row.K, mode, draw, ar, dev, representable=row.kind != "tn")
            C = launch_tn(fsn, row, ar, A, B, layout=row.layout)
            assert torch.equal(launch_tn(fsn, row, ar, A, B, layout=row.layout), C), f"{row.id} {ar}: two calls in a row differ"
            if row.layout != "plain":  # the embedded operand gives the bits of the compact one
                assert torch.equal(launch_tn(fsn, row, ar, A, B), C), f"{row.id} {ar}: layout {row.layout} against the compact operands"
            if row.kind == "tn":  # rounded on load: the reference and the yardstick take the rounded operands
                A, B = r16(A, ar), r16(B, ar)
            stat = check_product(f"{row.id} {ar} {mode}", row.K, splits, C.cpu(), A, B, mode)
            if mode == "gauss":
                out.append(stat)
    return out


def _print(stat, splits):
    ratio = stat.rms("hip") / stat.rms("cpu") if stat.rms("cpu") > 0 else float("nan")
    print(f"[amp-sweep] {stat.name}: S {splits} hard {stat.hard:.4f} rms hip {stat.rms('hip'):.4f} u cpu {stat.rms('cpu'):.4f} u "
          f"({ratio:.2f} x)")


@pytest.mark.parametrize("row", TABLE, ids=[r.id for r in TABLE])
def test_products(fsn, row):
    t0 = time.time()
    L = fsn._lib.lib()
    try:
        if not row.wide:
            L.fsn_debug_tn16h_wide(0)
        _, splits = check_plan(L, row)
        for ar in ARITHS:
            for stat in run_row(fsn, row, ar, splits):
                _print(stat, splits)
    finally:
        L.fsn_debug_tn16h_wide(1)
    torch.cuda.synchronize()
    print(f"[amp-sweep] {row.id}: {time.time() - t0:.1f} s")


def plan_changes(L, M, Nc, k_end, count):
    """The first `count` K (multiples of 16 up to k_end) at which the tn16h plan of (M, Nc) differs from that of K - 16."""
    out, prev = [], (0, 0)
    for K in range(16, k_end, 16):
        p = tn16_plan(L, 0, M, Nc, K)
        if p != prev:
            out.append((K, prev, p))
            prev = p
            if len(out) == count:
                break
    return out


CLASSES = sorted({(r.M, r.Nc) for r in TN16H})


@pytest.mark.parametrize("M,Nc", CLASSES, ids=[f"M{m}-N{n}" for m, n in CLASSES])
def test_tn16h_plan_boundaries(fsn, M, Nc):
    """Both sides of the first plan changes of the class, integer operands (hash draw), both arithmetics: with a plan the
    product equals fp64, without one the entry refuses and writes nothing."""
    L = fsn._lib.lib()
    dev = torch.device("cuda:0")
    changes = plan_changes(L, M, Nc, 1 << 17, BOUNDARIES)
    assert len(changes) == BOUNDARIES and changes[0][1] == (0, 0), f"plan changes of {M} x {Nc}: {changes}"
    for K, before, after in changes:
        for k, (form, s) in ((K - 16, before), (K, after)):
            if k < 16:
                continue
            row = Row("tn16h", "boundary", M, Nc, k, form, s)
            for ar in ARITHS:
                A, B = make_operands(M, Nc, k, "int", 1, ar, dev)
                C = launch_tn(fsn, row, ar, A, B, expect=0 if form else ERR_ARG)
                if form:
                    check_product(f"{row.id} {ar}", k, s, C.cpu(), A, B, "int")
        print(f"[amp-sweep] tn16h {M} x {Nc}: K {K - 16} {before} | K {K} {after}")


@pytest.mark.parametrize("G,I", DX16, ids=[f"G{g}-I{i}" for g, i in DX16])
def test_gemm_dx16(fsn, G, I):
    """dx [rows][lddx] = dg16 [rows][G] W [G][I]: K = G, one chain (S = 1); columns I .. lddx - 1 stay untouched."""
    lib, L = fsn._lib, fsn._lib.lib()
    dev = torch.device("cuda:0")
    for ar in ARITHS:
        for rows in DX16_ROWS:
            for mode, draws in (("int", 2), ("gauss", 1)):
                for draw in range(draws):
                    Wt, Dt = make_operands(I, rows, G, mode, draw, ar, dev)  # [G][I], [G][rows]: dx^T = W^T-side product
                    W, dg = Wt.contiguous(), Dt.t().contiguous()
                    dg16 = _as16(dg, ar).contiguous()
                    first = None
                    for lddx in (ru4(I), 36):
                        for rep in range(2):
                            wf = torch.full((G * 32,), -1, dtype=torch.int16, device=dev)
                            buf = _sentinel(rows * lddx, dev)
                            dx = buf.view(torch.float32)
                            lib.check(L.fsn_debug_gemm_dx16(_ptr(dg16), G, _ptr(W), _ptr(wf), wf.numel() * 2, _ptr(dx), lddx, rows, G, I,
                                                            ARITHS[ar][0], lib.stream_ptr(dev)))
                            what = f"dx16 G{G} I{I} rows{rows} lddx{lddx} {ar} {mode}"
                            assert bool((buf[rows * lddx:] == SENTINEL).all()), f"{what}: written outside its declared region"
                            body = buf[:rows * lddx].view(rows, lddx)
                            assert bool((body[:, I:] == SENTINEL).all()), f"{what}: columns beyond I written"
                            got = dx[:rows * lddx].view(rows, lddx)[:, :I]
                            assert bool(torch.isfinite(got).all()), f"{what}: not every declared element was written"
                            if first is None:
                                first = got.clone()
                            assert torch.equal(got, first), f"{what}: differs from the first call (lddx {ru4(I)})"
                    stat = check_product(f"dx16 G{G} I{I} rows{rows} {ar} {mode}", G, 1, first.cpu(), dg.t(), W, mode)
                    if mode == "gauss" and rows == DX16_ROWS[-1]:
                        _print(stat, 1)


TO16_COUNTS = (4, 2048 * 256 * 4 + 4)


@pytest.mark.parametrize("ar", list(ARITHS))
def test_to16(fsn, ar):
    lib, L = fsn._lib, fsn._lib.lib()
    dev = torch.device("cuda:0")
    table = to16_table().to(dev)

    def convert(src):
        n = src.numel()
        buf = _sentinel((n + 1) // 2, dev)
        lib.check(L.fsn_debug_to16(_ptr(src), _ptr(buf), n, ARITHS[ar][0], lib.stream_ptr(dev)))
        assert bool((buf[n // 2:] == SENTINEL).all()), f"to16 {ar} n {n}: written outside its declared region"
        return buf[:n // 2].view(torch.int16).clone()

    # one n past a whole grid pass: the table repeated, its last four elements once more at the very end
    big = table.repeat(-(-TO16_COUNTS[1] // table.numel()))[:TO16_COUNTS[1]].contiguous()
    got = convert(big)
    assert torch.equal(convert(big), got), f"to16 {ar}: two calls in a row differ"
    assert_to16(big.cpu(), got.cpu(), ar)
    for i in range(0, table.numel(), 4 * 997):  # n = 4: quadruples from all over the table, the NaNs and the specials included
        quad = table[i:i + 4].contiguous()
        assert_to16(quad.cpu(), convert(quad).cpu(), ar)
    specials = torch.tensor([65520.0, -0.0, float("nan"), float("-inf")], device=dev)
    assert_to16(specials.cpu(), convert(specials).cpu(), ar)


# ---- the plan of the two-layer training entries -----------------------------------------------------------------------------

PLAN_FIELDS = ("fwd16", "bwd16", "g16_fwd", "g16_bptt", "tn16h", "tn16h_form", "in16", "h16_saved", "left", "clusters",
               "fwd_left", "fwd_clusters", "saves16")


class PlanRow:
    """One path of fsn_lstm2_forward_train / fsn_lstm2_backward under the 16-bit arithmetic (H = 384, 256 CUs) and the plan
    it was written for; hook: the fsn_debug_g16_kernels value it runs under."""

    def __init__(self, path, T, N, I, ldx, hook=1, s16=False, **want):
        self.path, self.T, self.N, self.I, self.ldx, self.hook, self.s16, self.want = path, T, N, I, ldx, hook, s16, want

    @property
    def id(self):
        return f"{self.path}-T{self.T}-N{self.N}-I{self.I}" + ("-s16" if self.s16 else "")


def _plan_rows():
    g16 = dict(fwd16=1, bwd16=1, g16_fwd=1, g16_bptt=1)
    full = dict(g16, left=0, fwd_left=0)
    rows = [
        # T 1: no tn16h, dw_hh by memset.  T 2 at 1536 rows: K = 1536 has no tn16h plan, the products round fp32 buffers on load
        PlanRow("g16-full", 1, 1536, 20, 32, **full, clusters=24, fwd_clusters=24, tn16h=0, tn16h_form=0, in16=0, h16_saved=0),
        PlanRow("g16-full", 2, 1536, 20, 32, **full, clusters=24, tn16h=0, in16=0, h16_saved=0),
        PlanRow("g16-full", 2, 1536, 20, 32, s16=True, **full, clusters=24, tn16h=0, in16=0, h16_saved=0),
        PlanRow("g16-full", 3, 1536, 32, 32, **full, clusters=24, tn16h=1, tn16h_form=1, in16=1, h16_saved=0),
        PlanRow("g16-full", 3, 1536, 32, 32, s16=True, **full, clusters=24, tn16h=1, tn16h_form=1, in16=1, h16_saved=1),
        PlanRow("g16-full", 2, 2048, 20, 32, **full, clusters=32, fwd_clusters=32, tn16h=1, tn16h_form=1, in16=1),
        PlanRow("g16-full", 2, 2048, 20, 32, s16=True, **full, clusters=32, tn16h=1, in16=1, h16_saved=1),
        PlanRow("g16-full", 9, 1536, 20, 32, **full, clusters=24, tn16h=1, tn16h_form=2, in16=1, h16_saved=0),
        # left-over rows beside the launch: fp32 step by step, both directions; never h16_saved.  (T - 1) N = 1552 and 4656 have
        # no tn16h plan (a plan needs every K split non-empty); 2176 rows = 32 clusters + 8 tiles, K = 4352 and 6528 have one
        PlanRow("g16-left", 2, 1552, 20, 32, **g16, left=16, fwd_left=16, clusters=24, tn16h=0, in16=0),
        PlanRow("g16-left", 4, 1552, 20, 32, **g16, left=16, fwd_left=16, clusters=24, tn16h=0, in16=0),
        PlanRow("g16-left", 3, 2176, 20, 32, **g16, left=128, fwd_left=128, clusters=32, tn16h=1, tn16h_form=1, in16=1),
        PlanRow("g16-left", 3, 2176, 20, 32, s16=True, **g16, left=128, clusters=32, tn16h=1, in16=1, h16_saved=0),
        # dW_hh's K = (T - 1) N = 2064 has a plan, dW_ih1's K = T N = 4128 has none: no tn16h (see ONE_PLAN below)
        PlanRow("g16-left-one-plan", 2, 2064, 20, 32, **g16, left=16, clusters=32, tn16h=0, in16=0),
        # ldx != 32: no group forward (layer by layer, fp32); the BPTT still on the 16-bit kernel, dx an fp32 GEMM
        PlanRow("g16-in16-off", 3, 1536, 12, 16, fwd16=0, g16_fwd=0, fwd_clusters=0, bwd16=1, g16_bptt=1, tn16h=1, in16=0),
        PlanRow("g16-in16-off", 3, 1536, 64, 64, fwd16=0, g16_fwd=0, fwd_clusters=0, bwd16=1, g16_bptt=1, tn16h=1, in16=0),
        # 56 clusters: the forward on lstm2_group_kernel<.., F16>, the backward layer by layer in fp32
        PlanRow("fwd-group16-bwd-by-layer", 2, 3584, 20, 32, fwd16=1, g16_fwd=0, fwd_clusters=56, bwd16=0, g16_bptt=0, clusters=0,
                tn16h=0, in16=0, h16_saved=0),
        PlanRow("hook-0", 3, 1536, 20, 32, hook=0, fwd16=1, bwd16=1, g16_fwd=0, g16_bptt=0, tn16h=0, in16=0, clusters=24),
        PlanRow("hook-2", 3, 1536, 20, 32, hook=2, **g16, tn16h=0, tn16h_form=0, in16=0, clusters=24),
        PlanRow("hook-3", 3, 1536, 20, 32, hook=3, **g16, tn16h=1, tn16h_form=1, in16=0, clusters=24),
    ]
    return rows


LSTM2_PLAN = _plan_rows()


def lstm2_plan16(L, T, N, I, ldx, H, arith):
    out = (ctypes.c_int * len(PLAN_FIELDS))()
    n = L.fsn_debug_lstm2_plan16(T, N, I, ldx, H, arith, out, len(PLAN_FIELDS))
    assert n == len(PLAN_FIELDS), f"fsn_debug_lstm2_plan16 returned {n}"
    return dict(zip(PLAN_FIELDS, out))


@pytest.mark.parametrize("row", LSTM2_PLAN, ids=[r.id for r in LSTM2_PLAN])
def test_lstm2_plan16(fsn, row):
    L = fsn._lib.lib()
    torch.zeros(1, device="cuda:0")  # the plan asks the current device for its CU count and the kernels' occupancy
    try:
        L.fsn_debug_g16_kernels(row.hook)
        for ar, (code, _) in ARITHS.items():
            plan = lstm2_plan16(L, row.T, row.N, row.I, row.ldx, 384, code | (SAVES16 if row.s16 else 0))
            diff = {k: (plan[k], v) for k, v in row.want.items() if plan[k] != v}
            assert not diff, f"{row.id} {ar}: plan {plan} differs from what the row expects in (got, expected) {diff}"
        plan = lstm2_plan16(L, row.T, row.N, row.I, row.ldx, 384, 0)  # fp32: nothing 16-bit, the same clusters
        assert not any(plan[k] for k in PLAN_FIELDS[:8]), f"{row.id}: fp32 plan {plan}"
    finally:
        L.fsn_debug_g16_kernels(1)


ONE_PLAN = (2, 2064, 20)  # T, N, I: of the two K of the large weight-gradient products only (T - 1) N has a tn16h plan
NO_PLAN_32 = (4, 1552, 20)  # neither K has one, but fsn_tn_plan's 16-row count had a square plan for both


def test_tn16h_needs_a_plan_for_both_k(fsn):
    """The plan takes tn16h only where BOTH K of the large products have a plan, over every (T, N) of a window around the
    shipped shapes; ONE_PLAN is in it and is a shape where they differ."""
    L = fsn._lib.lib()
    torch.zeros(1, device="cuda:0")
    differ = []
    for N in range(1536, 2192, 16):
        for T in range(2, 13):
            plan = lstm2_plan16(L, T, N, 20, 32, 384, ARITHS["f16"][0])
            a, b = tn16_plan(L, 0, 1536, 384, (T - 1) * N)[0], tn16_plan(L, 0, 1536, 384, T * N)[0]
            if plan["g16_bptt"]:
                assert plan["tn16h"] == int(bool(a and b)), f"T {T} N {N}: tn16h {plan['tn16h']} with forms {a} (dW_hh) and {b} (dW_ih1)"
            if bool(a) != bool(b):
                differ.append((T, N))
    assert ONE_PLAN[:2] in differ, f"shapes where the two K differ: {differ}"


@pytest.mark.parametrize("shape", [ONE_PLAN, NO_PLAN_32], ids=["one-plan", "no-plan-32"])
@pytest.mark.parametrize("ar", list(ARITHS))
def test_backward_where_tn16h_has_no_plan(fsn, ar, shape):
    """Fixed on the way: lstm2_backward_phases chose tn16h from fsn_gemm_tn16h_supported of K = (T - 1) N alone.  That query
    accepted fsn_tn_plan's square plan as it stood, while the launcher re-splits K in chunks of 32 rows and refuses when
    the split count changes (NO_PLAN_32), and dW_ih1 sums K = T N rows, which may have no plan where (T - 1) N has one
    (ONE_PLAN): fsn_lstm2_backward failed with "gemm_tn16h: no plan" under both arithmetics.  The query now is the
    launcher's rule and the plan asks it for both K; these shapes run on the products that round the fp32 buffers on load -
    the path fsn_debug_g16_kernels(2) forces: the same bits in every output."""
    from fullsubnet_amd.train import Lstm2Function
    T, N, I = shape
    H, L = 384, fsn._lib.lib()
    g = torch.Generator().manual_seed(21)
    x = torch.randn(T, N, I, generator=g)
    shapes = ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,), (4 * H, H), (4 * H, H), (4 * H,), (4 * H,))
    w = [(torch.rand(s_, generator=g) * 2 - 1) * 2 / H ** 0.5 for s_ in shapes]
    dy = torch.randn(T, N, H, generator=g) * 64.0

    def run():
        xd = x.cuda().requires_grad_(True)
        wd = [t.cuda().requires_grad_(True) for t in w]
        y = Lstm2Function.apply(xd, *wd, ar)
        (y * dy.cuda()).sum().backward()
        torch.cuda.synchronize()
        return [y.detach().cpu(), xd.grad.cpu()] + [t.grad.cpu() for t in wd]

    got = run()
    assert all(bool(torch.isfinite(t).all()) for t in got)
    try:
        L.fsn_debug_g16_kernels(2)
        forced = run()
    finally:
        L.fsn_debug_g16_kernels(1)
    names = ["y", "dx", "dw_ih0", "dw_hh0", "db_ih0", "db_hh0", "dw_ih1", "dw_hh1", "db_ih1", "db_hh1"]
    for name, a, b in zip(names, got, forced):
        assert torch.equal(a, b), f"{ar} {name}: differs from the products forced onto the fp32 buffers"
    fsn._lib.stream_status(torch.device("cuda:0"))


# ---- the two-layer entries under f16 / bf16 / + s16: one step from the device's own state, and identities ---------------------

class Path:
    """One row of the two-layer sweep: a recurrent-sweep Row (operands, blocks) + what the path does.  fwd_rounded: the forward
    launch rounds the operands of its products (False: layer by layer in fp32); left: rows beside the launch, whose
    recurrence products are fp32 in both directions; hook: the fsn_debug_g16_kernels value; plan: fields asserted on the device."""

    def __init__(self, path, T, N, I, ldx, fwd_rounded=True, left=0, hook=1, gain=2.0, Hreal=None, s16=True, dy_scale=1.0, **plan):
        self.row = R.Row(path, "train_group", "lstm2_train", T, N // 16, I, ldx, 384, gain=gain, Hreal=Hreal, alt_ldx=False)
        self.path, self.T, self.N, self.I, self.ldx = path, T, N, I, ldx
        self.fwd_rounded, self.left, self.hook, self.s16, self.plan = fwd_rounded, left, hook, s16, plan
        self.dy_scale = dy_scale

    def operands(self, draw=0):
        ops = R.make_operands(self.row, self.N, draw)
        ops["dy"] = ops["dy"] * self.dy_scale
        return ops

    def scaled(self, n_main=48):
        """The same path with n_main cluster rows (+ 16 beside them where the path has such rows): the CPU self-test."""
        left = 16 if self.left else 0
        p = Path(self.path, self.T, n_main + left, self.I, self.ldx, self.fwd_rounded, left, self.hook, self.row.gain,
                 self.row.Hreal if self.row.Hreal != 384 else None, self.s16, self.dy_scale, **self.plan)
        return p

    def rounding(self, plan=None):
        """What the path rounds, from its plan fields (the device's, or the row's own on the CPU): bwd16 - the backward launch
        runs in the 16-bit arithmetic (its recurrence products and dh0 round their operands on cluster rows, every
        weight-gradient product rounds both operands on ALL rows); in16 - dx is a 16-bit-operand product (all rows)."""
        plan = plan or self.plan
        bwd16 = bool(plan.get("bwd16", plan.get("g16_bptt", 0)))
        return dict(fwd=self.fwd_rounded, bwd16=bwd16, in16=bool(plan.get("in16", 0)))

    @property
    def id(self):
        r = self.row
        return f"{self.path}-T{self.T}-N{self.N}-I{self.I}" + (f"-g{r.gain:g}" if r.gain != 2.0 else "") + \
            (f"-h{r.Hreal}" if r.Hreal != r.H else "") + (f"-dy{self.dy_scale:g}" if self.dy_scale != 1.0 else "")


def _paths():
    g16 = dict(g16_fwd=1, g16_bptt=1)
    return [
        Path("g16-full", 1, 1536, 20, 32, **g16, tn16h=0, in16=0, left=0),
        Path("g16-full", 2, 1536, 32, 32, **g16, tn16h=0, in16=0),
        Path("g16-full", 3, 1536, 20, 32, **g16, tn16h=1, in16=1),
        Path("g16-full", 9, 1536, 20, 32, **g16, tn16h=1, tn16h_form=2, in16=1),
        Path("g16-full", 2, 2048, 20, 32, **g16, tn16h=1, in16=1, clusters=32),
        Path("g16-left", 2, 1552, 20, 32, left=16, **g16, tn16h=0),
        Path("g16-left", 4, 1552, 20, 32, left=16, **g16, tn16h=0),
        Path("g16-left", 3, 2176, 20, 32, left=128, **g16, tn16h=1, in16=1),
        Path("g16-in16-off", 3, 1536, 12, 16, fwd_rounded=False, fwd16=0, g16_bptt=1, tn16h=1, in16=0),
        Path("g16-in16-off", 3, 1536, 64, 64, fwd_rounded=False, fwd16=0, g16_bptt=1, tn16h=1, in16=0),
        Path("fwd-group16-bwd-by-layer", 2, 3584, 20, 32, fwd16=1, g16_fwd=0, bwd16=0, fwd_clusters=56),
        Path("hook-0", 3, 1536, 20, 32, hook=0, fwd16=1, bwd16=1, g16_fwd=0, g16_bptt=0),
        Path("hook-0", 1, 1536, 20, 32, hook=0, s16=False, fwd16=1, bwd16=1, g16_fwd=0, g16_bptt=0),
        Path("hook-0", 9, 1536, 32, 32, hook=0, s16=False, fwd16=1, bwd16=1, g16_fwd=0, g16_bptt=0),
        Path("hook-2", 3, 1536, 20, 32, hook=2, **g16, tn16h=0, in16=0),
        Path("hook-3", 3, 1536, 20, 32, hook=3, **g16, tn16h=1, in16=0),
        Path("h320pad", 2, 1536, 20, 32, Hreal=320, **g16),
        Path("saturated", 3, 1536, 20, 32, gain=6.0, **g16, tn16h=1),
        Path("saturated", 3, 2176, 20, 32, gain=6.0, left=128, **g16, tn16h=1),
        # the loss scale: dy of order 1 (the smallest gate gradients in fp16's subnormal range), 64, 2^14 (towards 65504)
        Path("scale", 2, 2048, 20, 32, dy_scale=1.0, s16=False, **g16, tn16h=1, in16=1),
        Path("scale", 2, 2048, 20, 32, dy_scale=64.0, s16=False, **g16, tn16h=1, in16=1),
        Path("scale", 2, 2048, 20, 32, dy_scale=2.0 ** 14, s16=False, **g16, tn16h=1, in16=1),
    ]


PATHS = _paths()
# kernel families of the two-layer entries under a 16-bit arithmetic and the paths that run them; each has a T = 1, a T = 2 and
# a T >= 9 row between its paths (tests/test_amp_sweep_cpu.py asserts it)
FAMILIES = {"g16 (lstm_group16_kernels.hip, both directions)": ("g16-full", "g16-left", "hook-2", "hook-3", "h320pad", "saturated", "scale"),
            "group kernels with arith (lstm2_group_kernel / lstm2_group_bptt_kernel<F16 / BF16>)": ("hook-0", "fwd-group16-bwd-by-layer")}
PATH_NAMES = ("g16-full", "g16-left", "g16-in16-off", "fwd-group16-bwd-by-layer", "hook-0", "hook-2", "hook-3", "h320pad", "saturated",
              "scale")
GRADS = ("dw_ih0", "dw_hh0", "db0", "dw_ih1", "dw_hh1", "db1")


class Lstm2:
    """fsn_lstm2_forward_train / fsn_lstm2_backward[_phase] of a Path under `arith` on device operands: outputs behind
    sentinels, save buffers and workspaces exactly their queries' size and filled with 0xFF."""

    def __init__(self, fsn, path, ops, arith):
        self.lib, self.L, self.p, self.arith = fsn._lib, fsn._lib.lib(), path, arith
        self.dev = torch.device("cuda:0")
        self.x = R._padded(ops["x"].to(self.dev), path.ldx)
        self.dy = ops["dy"].to(self.dev).contiguous()
        self.w = [[t.to(self.dev).contiguous() for t in lp] for lp in ops["layers"]]
        self.st = self.lib.stream_ptr(self.dev)

    def ws(self, nbytes):
        return self.lib.workspace(nbytes, self.dev).fill_(0xFF)

    def forward(self):
        L, p, q = self.L, self.lib.dev_ptr, self.p
        T, N, I, H = q.T, q.N, q.I, 384
        nsave = L.fsn_lstm_layer_save_bytes(T, N, H)
        fw = dict(s0=self.ws(nsave), s1=self.ws(nsave), y0=R.Out(self.dev, (T, N, H)), y1=R.Out(self.dev, (T, N, H)))
        ws = self.ws(L.fsn_lstm2_train_workspace_bytes(T, N, I, H, self.arith))
        self.lib.check(L.fsn_lstm2_forward_train(p(self.x), q.ldx, *[p(t) for lp in self.w for t in lp], T, N, I, H, p(fw["y0"].f),
                                                 p(fw["y1"].f), fw["s0"].data_ptr(), fw["s1"].data_ptr(), nsave, ws.data_ptr(),
                                                 ws.numel(), self.arith, self.st))
        fw["hseq0"], fw["hseq1"] = fw["y0"].take("hseq0"), fw["y1"].take("hseq1")
        self.lib.check_canaries()
        return fw

    def backward(self, fw, lddx, want_dx=True, phases=(7,)):
        L, p, q = self.L, self.lib.dev_ptr, self.p
        T, N, I, H = q.T, q.N, q.I, 384
        ws = self.ws(L.fsn_lstm2_bwd_workspace_bytes(T, N, I, H, self.arith))
        dx = R.Out(self.dev, (T, N, I), lddx) if want_dx else None
        g = dict(dw_ih0=R.Out(self.dev, (4 * H, I)), dw_hh0=R.Out(self.dev, (4 * H, H)), db0=R.Out(self.dev, (4 * H,)),
                 dw_ih1=R.Out(self.dev, (4 * H, H)), dw_hh1=R.Out(self.dev, (4 * H, H)), db1=R.Out(self.dev, (4 * H,)))
        args = [p(self.dy), p(self.x), q.ldx, p(self.w[0][0]), p(self.w[0][1]), p(self.w[1][0]), p(self.w[1][1]), T, N, I, H,
                p(fw["y0"].f[:T * N * H]), p(fw["y1"].f[:T * N * H]), fw["s0"].data_ptr(), fw["s1"].data_ptr(),
                p(dx.f) if want_dx else None, lddx] + [p(v.f) for v in g.values()] + [ws.data_ptr(), ws.numel(), self.arith]
        if phases == (7,):
            self.lib.check(L.fsn_lstm2_backward(*args, self.st))
        else:
            for ph in phases:
                self.lib.check(L.fsn_lstm2_backward_phase(*args, ph, self.st))
        out = {k: v.take(k) for k, v in g.items()}
        if want_dx:
            out["dx"] = dx.take("dx")
        self.lib.check_canaries()
        return out


def chain_product(acc, a, w):
    """acc + a w^T formed as ONE sequential chain per element, k ascending: what a matrix-instruction loop over K with a single
    accumulator does (the fp32 step kernels and the NN GEMM), against the blocked sum of a CPU GEMM."""
    wt = w.t().contiguous()
    for k in range(a.shape[1]):
        acc = acc.addcmul_(a[:, k:k + 1], wt[k:k + 1])
    return acc


def one_step(inp, h_prev, c_prev, w, dtype, act, rnd, chain=False):
    """One LSTM step from a given state in `dtype`: the activated gates [N][4H] (i, f, g, o), c_t, h_t.  rnd: the rounding of
    the products' operands (identity for an fp32 path); chain: sums as chain_product forms them."""
    sig, tanh = R.ACTS[act]
    w_ih, w_hh, b_ih, b_hh = (t.to(dtype) for t in w)
    if chain:
        a = (b_ih + b_hh).expand(inp.shape[0], -1).clone()
        a = chain_product(chain_product(a, rnd(inp).to(dtype), rnd(w_ih).to(dtype)), rnd(h_prev).to(dtype), rnd(w_hh).to(dtype))
    else:
        a = rnd(inp).to(dtype) @ rnd(w_ih).to(dtype).t() + rnd(h_prev).to(dtype) @ rnd(w_hh).to(dtype).t() + (b_ih + b_hh)
    i, f, g, o = a.chunk(4, -1)
    i, f, g, o = sig(i), sig(f), tanh(g), sig(o)
    c = f * c_prev.to(dtype) + i * g
    return torch.cat([i, f, g, o], -1), c, o * tanh(c)


def one_step_outputs(path, ar, layers, x, hseq, gates, cseq, dtype, act, device, chain=False):
    """The one-step results of every step of both layers from the DEVICE's own h_{t-1}, c_{t-1} (and hseq0 as layer 1's
    input): name -> [T][N][.] in `dtype` on `device`.  Cluster rows take rounded operands where the forward runs in the 16-bit
    arithmetic, the rows beside the launch never."""
    main = path.N - path.left
    ident = lambda t: t
    rnd = (lambda t: t.to(ARITHS[ar][1]).float()) if path.fwd_rounded else ident
    out = {}
    for layer in range(2):
        inp = (x if layer == 0 else hseq[0]).to(device)
        w = [t.to(device) for t in layers[layer]]
        h, c = hseq[layer].to(device), cseq[layer].to(device)
        zero = torch.zeros_like(h[0])
        res = []
        for t in range(path.T):
            hp, cp = (h[t - 1], c[t - 1]) if t else (zero, zero)
            parts = [one_step(inp[t, :main], hp[:main], cp[:main], w, dtype, act, rnd, chain and not path.fwd_rounded)]
            if path.left:
                parts.append(one_step(inp[t, main:], hp[main:], cp[main:], w, dtype, act, ident, chain))
            res.append([torch.cat([pt[k] for pt in parts]) for k in range(3)])
        G = torch.stack([r[0] for r in res])
        for k, name in enumerate("ifgo"):
            out[f"gate_{name}{layer}"] = G[..., k * 384:(k + 1) * 384]
        out[f"c{layer}"], out[f"h{layer}"] = torch.stack([r[1] for r in res]), torch.stack([r[2] for r in res])
    return out


def check_one_step(path, ar, ops, fw, log=print):
    """2a, forward: device gates, c_t, h_t of every step against the fp64 one step; yardstick: the same one step in CPU fp32 with
    lstm_cell.h's formulas.  stat_hip <= SHARP x yardstick: relative Frobenius and max, whole tensor, per step, per 16-row tile
    (every gate is a tensor of its own).  Rule for the yardstick's sums, by rows: rows that the 16-bit launch computes - a CPU
    GEMM (blocked sums); rows that run on the fp32 step kernels (all rows of a layer-by-layer forward, the rows beside a
    launch) - chain_product, one sequential chain per element like those kernels' single accumulator.  The term is reproduced
    on the CPU alone (tests/test_amp_sweep_cpu.py asserts that the chain is the less accurate of the two legitimate fp32 runs:
    1.2 - 1.5 x in Frobenius norm at 64 rows with fused adds; 1.5 x on a sigmoid gate, 2.2 x on g, max 2.6 - 3.3 x with
    separate multiply and add at 1536 rows).  On the device the I 12 row stood at Frobenius 1.4 / 2.0 x and max 3.9 / 4.7 x
    (gate g of layer 0: 1.28e-6 against 2.75e-7) of the blocked yardstick - the one miss before this rule; with it no ratio
    of such rows is above 1.3 x."""
    T, N, H = path.T, path.N, 384
    x = ops["x"]
    hseq = [fw["hseq0"], fw["hseq1"]]
    saves = [fw[k].view(torch.float32) for k in ("s0", "s1")]
    gates = [s[:T * N * 4 * H].view(T, N, 4 * H) for s in saves]
    cseq = [s[T * N * 4 * H:T * N * 5 * H].view(T, N, H) for s in saves]
    dev = hseq[0].device
    ref = one_step_outputs(path, ar, ops["layers"], x, hseq, gates, cseq, torch.float64, "torch", dev)
    yard = one_step_outputs(path, ar, ops["layers"], x, hseq, gates, cseq, torch.float32, "cell", torch.device("cpu"), chain=True)
    got = {}
    for layer in range(2):
        for k, name in enumerate("ifgo"):
            got[f"gate_{name}{layer}"] = gates[layer][..., k * H:(k + 1) * H]
        got[f"c{layer}"], got[f"h{layer}"] = cseq[layer], hseq[layer]
    stats = {}
    for k in ref:
        s = stats[k] = R.Stat(k)
        s.add(path.row, got[k].cpu(), yard[k], ref[k].cpu())
        rf, rm = s.ratios()
        lb, wb = s.worst_block()
        log(f"[amp-sweep] 2a {path.id} {ar} {k}: frob hip {s.frob('hip'):.3e} yard {s.frob('cpu'):.3e} ({rf:.2f} x) max hip "
            f"{s.maxrel('hip'):.3e} yard {s.maxrel('cpu'):.3e} ({rm:.2f} x) worst block {lb} {wb:.2f} x")
    for s in stats.values():
        s.assert_sharp("torch")
    return stats


class PathProduct(torch.autograd.Function):
    """y = x w^T as a path forms it.  Forward: rows below `main` from rounded operands where f_main, the rows beside the launch
    never.  Backward: dx = dy w from rounded operands on the cluster rows where dx_main and on the other rows where dx_left;
    dw = dy^T x from rounded operands on ALL rows where dw_round."""

    @staticmethod
    def forward(ctx, x, w, dt, main, f_main, dx_main, dx_left, dw_round):
        ctx.save_for_backward(x, w)
        ctx.cfg = (dt, main, dx_main, dx_left, dw_round)
        r = lambda t, on: t.to(dt).to(t.dtype) if on else t
        y = r(x[:main], f_main) @ r(w, f_main).t()
        return y if main >= x.shape[0] else torch.cat([y, x[main:] @ w.t()])

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dt, main, dx_main, dx_left, dw_round = ctx.cfg
        r = lambda t, on: t.to(dt).to(t.dtype) if on else t
        dx = r(dy[:main], dx_main) @ r(w, dx_main)
        if main < x.shape[0]:
            dx = torch.cat([dx, r(dy[main:], dx_left) @ r(w, dx_left)])
        return dx, r(dy, dw_round).t() @ r(x, dw_round), None, None, None, None, None, None


def emulated_path(path, ar, ops, dtype, act, rounding, device="cpu"):
    """The two-layer entries as `path` computes them (Path.rounding), in `dtype` with the activations `act`, gradients by
    autograd of sum(y * dy): name -> tensor, the names of the recurrent sweep's reference."""
    dt = ARITHS[ar][1]
    main = path.N - path.left
    sig, tanh = R.ACTS[act]
    f, b16, in16 = rounding["fwd"], rounding["bwd16"], rounding["in16"]
    x = ops["x"].to(device=device, dtype=dtype).requires_grad_(True)
    layers = [[t.to(device=device, dtype=dtype).requires_grad_(True) for t in lp] for lp in ops["layers"]]
    inp, seqs = x, []
    for k, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
        h = torch.zeros(path.N, 384, dtype=dtype, device=device)
        c = torch.zeros_like(h)
        ys = []
        for t in range(path.T):
            dxf = (in16, in16) if k == 0 else (b16, False)  # layer 0's dx: one product for all rows; dh0: inside the launch
            a = PathProduct.apply(inp[t], w_ih, dt, main, f, dxf[0], dxf[1], b16) + \
                PathProduct.apply(h, w_hh, dt, main, f, b16, False, b16) + (b_ih + b_hh)
            i, fg, g, o = a.chunk(4, -1)
            c = sig(fg) * c + sig(i) * tanh(g)
            h = sig(o) * tanh(c)
            ys.append(h)
        inp = torch.stack(ys)
        seqs.append(inp)
    grads = torch.autograd.grad((seqs[1] * ops["dy"].to(device=device, dtype=dtype)).sum(), [x] + [t for lp in layers for t in lp])
    out = dict(y0=seqs[0], y=seqs[1], dx=grads[0])
    for k in range(2):
        out[f"dw_ih{k}"], out[f"dw_hh{k}"], out[f"db{k}"] = grads[1 + 4 * k], grads[2 + 4 * k], grads[3 + 4 * k]
    return {k: v.detach().cpu() for k, v in out.items()}


def check_recurrence(path, ar, ops, got, rounding, ref_device="cpu", f32mode=None, log=print):
    """2b: every output of the whole recurrence against the emulation's autograd in fp64.  Yardsticks: the CPU fp32 runs of the
    SAME emulation with torch's activations and with lstm_cell.h's formulas; which one holds an output is the recurrent
    sweep's rule yardstick_of(row, output) (narrow inputs: hidden outputs, and gradients at T <= 2, to the cell formulas;
    tests/test_amp_sweep_cpu.py measures the two runs against each other under both arithmetics).  stat_hip <= 4 x, whole
    tensor, per step, per gate block, and per 16-row tile by the rule of assert_recurrence.  Printed with every output: the distance of the fp32 mode from the
    emulation.  Rows with T <= 2 also hold the arithmetic (4 x the yardstick lies below that distance); from T = 3 on a hidden
    state that differs in its last bit moves some operands by a whole 16-bit ulp and the rows hold structure only."""
    ref = emulated_path(path, ar, ops, torch.float64, "torch", rounding, ref_device)
    t32 = emulated_path(path, ar, ops, torch.float32, "torch", rounding)
    c32 = emulated_path(path, ar, ops, torch.float32, "cell", rounding)
    stats = {}
    for k, v in got.items():
        s = stats[k] = R.Stat(k)
        s.add(path.row, v, t32[k], ref[k], c32[k])
        yard = R.yardstick_of(path.row, k)
        a = s.acc["all"]
        fy = (a[1] if yard == "torch" else a[6]) ** 0.5
        dist = ""
        if f32mode is not None:
            dist = f" fp32 mode at {float((f32mode[k].double() - ref[k]).norm() / ref[k].norm().clamp_min(1e-300)):.2e}"
        log(f"[amp-sweep] 2b {path.id} {ar} {k} [{yard}]: frob hip {s.frob('hip'):.3e} yard {fy / max(a[2], 1e-300) ** 0.5:.3e} "
            f"({a[0] ** 0.5 / fy if fy > 0 else float('nan'):.2f} x) other fp32 run {(a[6] if yard == 'torch' else a[1]) ** 0.5 / max(a[2], 1e-300) ** 0.5:.3e}"
            f" worst block {s.worst_block()[0]}{dist}")
    for k, s in stats.items():
        assert_recurrence(s, R.yardstick_of(path.row, k))
    return stats


def assert_recurrence(stat, yard):
    """The recurrent sweep's assert_sharp (hip <= SHARP x yardstick: Frobenius and max of the whole tensor, Frobenius of every
    step, gate and column block, max of the last step) with ONE other rule, for the 16-row tiles: a tile's relative Frobenius
    error is held to SHARP x that of the yardstick's WORST tile, not of the same tile.  The reason is a reference-side term
    that tests/test_amp_sweep_cpu.py reproduces without a device: what separates an fp32 run from the fp64 emulation is the
    operands that fall on the other side of a 16-bit boundary, about 1 in 5000, and a tile of 16 rows holds none or a few of
    them - between the two fp32 CPU runs of the emulation the same tile differs by up to 28 x under f16 and 1400 x under bf16
    (whole tensors: 2 - 3 x), so no implementation meets 4 x tile by tile.  A wrong tile is wrong by its own size, 10^3 and
    more times the worst tile of the yardstick."""
    tiles = {lb: a for lb, a in stat.acc.items() if lb.startswith("rows ")}
    rest = R.Stat(stat.name)
    rest.acc = {lb: a for lb, a in stat.acc.items() if lb not in tiles}
    rest.assert_sharp(yard)
    j = 1 if yard == "torch" else 6
    worst = max((a[j] / a[2] for a in tiles.values() if a[2] > 0), default=0.0)
    for lb, a in tiles.items():
        rel = a[0] / a[2] if a[2] > 0 else (0.0 if a[0] == 0 else float("inf"))
        assert rel <= SHARP * SHARP * worst, \
            (f"{stat.name} [{lb}]: Frobenius error {rel ** 0.5:.3e} of the device against {worst ** 0.5:.3e} of the yardstick's worst "
             f"16-row tile ({(rel / worst) ** 0.5 if worst > 0 else float('inf'):.2f} x, allowed {SHARP:g} x)")


def backward_t1(path, ar, ops, fw, rounding, dtype, device):
    """The T = 1 backward written out by hand from the DEVICE's saves (activated gates, c_1 of both layers, hseq0) in `dtype`:
    dg1 from dy, dh0 = r(dg1) r(W_ih1), dg0, dx = r(dg0) r(W_ih0) (unrounded without in16), dW_ih = r(dg)^T r(input), db = the
    column sums of the unrounded dg, dw_hh = 0.  r = identity where the backward is not in the 16-bit arithmetic; the rows
    beside the launch form dh0 from unrounded operands."""
    N, H, main = path.N, 384, path.N - path.left
    dt = ARITHS[ar][1]
    r = (lambda t: t.to(dt).to(dtype)) if rounding["bwd16"] else (lambda t: t)
    rx = r if rounding["in16"] else (lambda t: t)
    to = lambda t: t.to(device=device, dtype=dtype)

    def dgates(save, dh):
        sv = save.view(torch.float32)
        i, f, g, o = to(sv[:N * 4 * H].view(N, 4 * H)).chunk(4, -1)
        tc = torch.tanh(to(sv[N * 4 * H:N * 5 * H].view(N, H)))
        dc = dh * o * (1 - tc * tc)
        return torch.cat([dc * g * i * (1 - i), torch.zeros_like(dc), dc * i * (1 - g * g), dh * tc * o * (1 - o)], -1)

    w_ih0, w_ih1 = to(ops["layers"][0][0]), to(ops["layers"][1][0])
    dg1 = dgates(fw["s1"], to(ops["dy"][0]))
    dh0 = r(dg1[:main]) @ r(w_ih1)
    if path.left:
        dh0 = torch.cat([dh0, dg1[main:] @ w_ih1])
    dg0 = dgates(fw["s0"], dh0)
    zero = torch.zeros(4 * H, H, dtype=dtype)
    out = dict(dx=(rx(dg0) @ rx(w_ih0))[None], dw_ih0=r(dg0).t() @ r(to(ops["x"][0])), db0=dg0.sum(0),
               dw_ih1=r(dg1).t() @ r(to(fw["hseq0"][0])), db1=dg1.sum(0), dw_hh0=zero, dw_hh1=zero)
    return {k: v.cpu() for k, v in out.items()}


def check_backward_t1(path, ar, ops, fw, got, rounding, log=print):
    """2a, backward at T = 1: the device's dx and six gradients against backward_t1 in fp64; yardstick: its CPU fp32 run;
    4 x by assert_recurrence; dw_hh exactly 0.0."""
    ref = backward_t1(path, ar, ops, fw, rounding, torch.float64, fw["hseq0"].device)
    yard = backward_t1(path, ar, ops, fw, rounding, torch.float32, torch.device("cpu"))
    for k in ref:
        if k.startswith("dw_hh"):
            assert bool((got[k] == 0).all()), f"T = 1: {k} is not exactly 0.0"
            continue
        s = R.Stat(k)
        s.add(path.row, got[k], yard[k], ref[k])
        rf, rm = s.ratios()
        log(f"[amp-sweep] 2a-bwd {path.id} {ar} {k}: frob hip {s.frob('hip'):.3e} yard {s.frob('cpu'):.3e} ({rf:.2f} x) max ({rm:.2f} x)")
        assert_recurrence(s, "torch")


def half_ulp16(v, ar):
    """Half the spacing of the 16-bit type at |v| (fp16's subnormal spacing below 2^-14)."""
    e = torch.frexp(v.abs().double().clamp_min(1e-300))[1] - 1  # floor(log2 |v|)
    frac, emin = (10, -14) if ar == "f16" else (7, -126)
    return torch.pow(2.0, (e.clamp_min(emin) - frac - 1).double())


def decode_saved16(save, T, N, ar):
    """Under FSN_ARITH_SAVES16 a cluster row's save slot (4H fp32 = 8H 16-bit words) holds the activated gates as [unit quad 96]
    [gate 4][4 units] in its first half and h_t in the first H words of its second half: (gates [T][N][4][H], h [T][N][H]) as fp32."""
    H = 384
    slot = save.view(torch.int16)[:T * N * 8 * H].view(T, N, 8 * H)
    dt = ARITHS[ar][1]
    gates = slot[..., :4 * H].reshape(T, N, H // 4, 4, 4).permute(0, 1, 3, 2, 4).reshape(T, N, 4, H)
    return gates.contiguous().view(dt).float(), slot[..., 4 * H:5 * H].contiguous().view(dt).float()


def check_saved16(path, ar, ops, fw16, log=print):
    """2a under + s16: the 16-bit gates and h_t decoded from the save slots of the cluster rows (the rows beside the launch keep
    the fp32 layout) against the fp64 one step from the device's own state.  A saved value is r(v') of a v' within the yardstick
    of the fp64 v, so |saved - v| <= half a 16-bit ulp at |v| (+ one fp32 ulp for a v' across a binade) + SHARP x the
    yardstick's largest error on that tensor: derived, per element."""
    T, N, H = path.T, path.N, 384
    main = N - path.left
    hseq = [fw16["hseq0"], fw16["hseq1"]]
    saves = [fw16[k].view(torch.float32) for k in ("s0", "s1")]
    cseq = [sv[T * N * 4 * H:T * N * 5 * H].view(T, N, H) for sv in saves]
    dev = hseq[0].device
    ref = one_step_outputs(path, ar, ops["layers"], ops["x"], hseq, None, cseq, torch.float64, "torch", dev)
    yard = one_step_outputs(path, ar, ops["layers"], ops["x"], hseq, None, cseq, torch.float32, "cell", torch.device("cpu"), chain=True)
    for layer in range(2):
        gates, h16 = decode_saved16(fw16[f"s{layer}"], T, N, ar)
        for name, got in [(f"gate_{g}{layer}", gates[:, :, k]) for k, g in enumerate("ifgo")] + [(f"h{layer}", h16)]:
            v = ref[name][:, :main].cpu()
            slack = SHARP * float((yard[name][:, :main].double() - v).abs().max())
            err = (got[:, :main].cpu().double() - v).abs()
            bound = half_ulp16(v, ar) * (1 + 2.0 ** -20) + slack
            worst = float((err / bound).max())
            log(f"[amp-sweep] 2a+s16 {path.id} {ar} {name}: worst |saved - v| at {worst:.3f} of half a 16-bit ulp + {SHARP:g} x {slack / SHARP:.2e}")
            assert worst <= 1.0, f"{name}: a saved 16-bit value lies {worst:.2f} x the bound from the fp64 one step"
        assert torch.equal(h16[:, :main], hseq[layer][:, :main].to(ARITHS[ar][1]).float()), \
            f"h{layer}: the 16-bit h_t in the save slots is not the rounded hidden sequence"


def _same(a, b, what, keys=None):
    for k in (keys or a):
        if k in a and k in b:
            assert torch.equal(a[k], b[k]), f"{k}: {what}: not bit-identical"


def _plan_of(L, path, arith):
    plan = lstm2_plan16(L, path.T, path.N, path.I, path.ldx, 384, arith)
    want = dict(path.plan)
    want.setdefault("left", path.left if plan["clusters"] else 0)
    diff = {k: (plan[k], v) for k, v in want.items() if plan[k] != v}
    assert not diff, f"{path.id}: plan {plan} differs from what the row expects in (got, expected) {diff}"
    return plan


@pytest.mark.parametrize("ar", list(ARITHS))
@pytest.mark.parametrize("path", PATHS, ids=[p.id for p in PATHS])
def test_lstm2_paths(fsn, path, ar):
    """Every path of the two-layer entries: its plan, the one-step check of the forward (2a), and the identities (2c)."""
    t0 = time.time()
    lib, L = fsn._lib, fsn._lib.lib()
    torch.zeros(1, device="cuda:0")
    code = ARITHS[ar][0]
    ops = path.operands()
    lddx = R.ru16(path.I) + 4
    try:
        L.fsn_debug_g16_kernels(1)
        d32 = Lstm2(fsn, path, ops, 0)  # the fp32 mode of the same entries: how far the arithmetic moves every output
        fw32 = d32.forward()
        f32mode = {k: v.cpu() for k, v in d32.backward(fw32, lddx).items()}
        f32mode["y0"], f32mode["y"] = fw32["hseq0"].cpu(), fw32["hseq1"].cpu()
        del d32, fw32
        L.fsn_debug_g16_kernels(path.hook)
        plan = _plan_of(L, path, code)
        d = Lstm2(fsn, path, ops, code)
        before = lib.persist_stats()[0]
        fw = d.forward()
        launched = lib.persist_stats()[0] - before
        assert (launched > 0) == (plan["fwd_clusters"] > 0), f"{path.id}: {launched} persistent launches in the forward, plan {plan}"
        check_one_step(path, ar, ops, fw)
        again = d.forward()
        _same(fw, again, "two forward calls in a row", ("hseq0", "hseq1"))
        assert torch.equal(fw["s0"], again["s0"]) and torch.equal(fw["s1"], again["s1"]), "save buffers: two forward calls differ"
        if path.row.Hreal < 384:  # zero-padded units of layer 0: h exactly 0.0, g and c exactly 0.0, i / f / o exactly 0.5
            Hr, H, T, N = path.row.Hreal, 384, path.T, path.N
            assert bool((fw["hseq0"][..., Hr:] == 0).all()), "hseq0: zero-padded units are not exactly 0.0"
            sv = fw["s0"].view(torch.float32)
            gates = sv[:T * N * 4 * H].view(T, N, 4, H)[..., Hr:]
            assert bool((gates[:, :, 2] == 0).all()) and bool((gates[:, :, [0, 1, 3]] == 0.5).all()), "saved gates of zero-padded units"
            assert bool((sv[T * N * 4 * H:T * N * 5 * H].view(T, N, H)[..., Hr:] == 0).all()), "saved cell state of zero-padded units"
        before = lib.persist_stats()[0]
        g = d.backward(fw, lddx)
        launched = lib.persist_stats()[0] - before
        assert (launched > 0) == (plan["clusters"] > 0), f"{path.id}: {launched} persistent launches in the backward, plan {plan}"
        _same(d.backward(fw, lddx), g, "two backward calls in a row")
        _same(d.backward(fw, lddx, want_dx=False), g, "dx == NULL", GRADS)
        _same(d.backward(fw, path.I if path.I % 4 == 0 else R.ru16(path.I)), g, "another lddx")
        _same(d.backward(fw, lddx, phases=(1, 4, 2)), g, "phases 1, 4, 2 against 7")
        if plan["clusters"]:
            _same(d.backward(fw, lddx, phases=(8, 1, 2 | 16, 4)), g, "phases 8, 1, 2 | 16, 4 against 7")
        if path.row.Hreal < 384:
            for k in ("dw_ih0", "dw_hh0", "db0"):
                assert bool((g[k].view(4, 384, -1)[:, path.row.Hreal:] == 0).all()), f"{k}: gradient rows of zero-padded units are not 0.0"
            for k in ("dw_hh0", "dw_ih1"):  # ... and the columns that multiply their (zero) hidden state
                assert bool((g[k][:, path.row.Hreal:] == 0).all()), f"{k}: gradient columns of zero-padded units are not 0.0"
        if path.T == 1:
            assert bool((g["dw_hh0"] == 0).all()) and bool((g["dw_hh1"] == 0).all()), "T = 1: dw_hh is not exactly 0.0"
        got = {k: v.cpu() for k, v in g.items()}
        got["y0"], got["y"] = fw["hseq0"].cpu(), fw["hseq1"].cpu()
        check_recurrence(path, ar, ops, got, path.rounding(plan), ref_device="cuda:0", f32mode=f32mode)
        if path.T == 1:
            check_backward_t1(path, ar, ops, fw, got, path.rounding(plan))
        if path.s16:  # 16-bit saves: the same hidden sequences bit for bit, and the backward's identities on its own saves
            p16 = lstm2_plan16(L, path.T, path.N, path.I, path.ldx, 384, code | SAVES16)
            assert p16["saves16"] == int(bool(plan["g16_fwd"] and plan["g16_bptt"])), f"{path.id}: +s16 plan {p16}"
            assert p16["h16_saved"] == int(bool(p16["saves16"] and plan["tn16h"] and not path.left)), f"{path.id}: +s16 plan {p16}"
            assert {k: v for k, v in p16.items() if k not in ("saves16", "h16_saved")} == \
                {k: v for k, v in plan.items() if k not in ("saves16", "h16_saved")}, f"{path.id}: +s16 changes the plan: {p16}"
            d16 = Lstm2(fsn, path, ops, code | SAVES16)
            fw16 = d16.forward()
            _same(fw16, fw, "hseq under 16-bit saves against fp32 saves", ("hseq0", "hseq1"))
            g16 = d16.backward(fw16, lddx)
            if p16["saves16"]:
                check_saved16(path, ar, ops, fw16)
            if not p16["saves16"]:  # one direction is not on the 16-bit kernels: the flag changes nothing at all
                assert torch.equal(fw16["s0"], fw["s0"]) and torch.equal(fw16["s1"], fw["s1"]), "+s16 where it does not apply: saves differ"
                _same(g16, g, "+s16 where it does not apply")
            _same(d16.backward(fw16, lddx), g16, "+s16: two backward calls in a row")
            _same(d16.backward(fw16, lddx, phases=(8, 1, 2 | 16, 4)), g16, "+s16: phases 8, 1, 2 | 16, 4 against 7")
            _same(d16.backward(fw16, lddx, want_dx=False), g16, "+s16: dx == NULL", GRADS)
        assert lib.stream_status(d.dev) == (0, 0), "the stream carries a timeout record"
    finally:
        L.fsn_debug_g16_kernels(1)
    print(f"[amp-sweep] {path.id} {ar}: {time.time() - t0:.1f} s")


def test_hooks_change_only_what_their_products_feed(fsn):
    """hook-2 (the large products round the fp32 buffers on load instead of reading 16-bit copies) and hook-3 (dx and dW_ih0 from
    the fp32 gate gradients) against the default, T 3, N 1536, f16: the forward and every output the hook's products do not feed
    keep their bits.  hook-2 feeds dw_ih1, dw_hh1, dw_hh0 (and, in16 going with tn16h, dx and dw_ih0); hook-3 feeds dx, dw_ih0."""
    L = fsn._lib.lib()
    path = next(p for p in PATHS if p.path == "hook-2")
    ops = path.operands()
    lddx, code = R.ru16(path.I) + 4, ARITHS["f16"][0]

    def run(hook):
        try:
            L.fsn_debug_g16_kernels(hook)
            d = Lstm2(fsn, path, ops, code)
            fw = d.forward()
            return fw, d.backward(fw, lddx)
        finally:
            L.fsn_debug_g16_kernels(1)

    fw1, g1 = run(1)
    for hook, fed in ((2, ("dw_ih1", "dw_hh1", "dw_hh0", "dx", "dw_ih0")), (3, ("dx", "dw_ih0"))):
        fw, g = run(hook)
        _same(fw, fw1, f"hook {hook}: the forward", ("hseq0", "hseq1"))
        _same(g, g1, f"hook {hook}: an output its products do not feed", [k for k in g1 if k not in fed])
