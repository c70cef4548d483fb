"""The glue of a training step (train_glue_kernels.hip), the MSE loss and the fused clip + Adam (optim_kernels.hip) held to
fp64 references over a sweep of shapes.  Needs an MI355X:  python -m pytest tests/test_gpu_train_glue_sweep.py -m gpu -s

The whole-model test sees these kernels through four LSTM layers, at T <= 9 frames, with padded sizes rounded to 16.  TABLE
below has one row per code path of the 24 kernels, named after the path it is there for: the 64-frame chunk carry of
tr_fb_cum_den_kernel, a second x-block of tr_fb_colsum_kernel, the lane stride of tr_rowsum_kernel, several 32-frame tiles,
the eight-segment scans beyond one element per segment, the t >= 256 / f >= 256 strides of the per-utterance reductions,
uneven drop_band groups, every padded size and leading dimension, more than 65535 target rows.  The C entries are called
through fullsubnet_amd._lib directly, so that (Bp, Fp, Rp), ld_fb, ld_dfb and ld are the test's to choose.

References
* forward of the glue: numpy at float64, built from oracle/fullsubnet_oracle.py in the order of fullsubnet/model.py:85-135
  (pad, norm of the full-band input, unfold ++ fb_out, norm of the unfolded tensor - formed explicitly here, which makes
  the kernel's analytic window multiplicity a tested claim -, drop_band);
* backward of the sub-band input: torch.float64 autograd on the CPU through `torch_sequence`, a plain torch transcription
  of the same sequence (tests/test_train_glue_sweep_cpu.py holds it to the numpy oracle at 1e-12), gradient with respect
  to fb_out, times fb_out > 0 (the entry returns the gradient through the ReLU of the full-band output layer);
* MSE and Adam: float64 transcriptions in numpy of torch.nn.MSELoss and of clip_grad_norm_ + torch.optim.Adam without
  weight decay (coefficient max_norm / (norm + 1e-6) clamped to 1; lerp; mul / addcmul; sqrt(v) / sqrt(bc2) + eps; both bias
  corrections from the step count), held to torch itself by the CPU module.

Assertions (the checkers - Stat, check_exact - are tried on the CPU by tests/test_train_glue_sweep_cpu.py, with the fp32
evaluation as a stand-in that must pass and eleven wrong stand-ins that must not)
* data movement is exact: mag_tm, mask_out, mask_grad, rows <-> pieces and every promised zero (rows >= R and columns
  >= 2 nb + 2 of sb_in, beyond (B, F) of x_tm / mag_tm / d_fb, look-ahead frames and columns >= 2 of dy: exactly +0).  Outputs
  are allocated GUARD elements larger than declared and pre-filled with the NaN sentinel 0x7FC0DEAD, which must survive
  outside; padding of fb_out_tm and of dx holds the same sentinel and must not be read.
* arithmetic outputs, hard:  |hip - ref64| <= k 2^-24 S per element, S = the sum of the absolute values of the terms the
  element is made of, k = the fp32 roundings on the longest path of the kernel's own sequence.  Adam's g, m, v, p alone:
  k (2^-24 S + 2^-149), the smallest fp32 step (gradients of 1e-30 have squares below the fp32 range).  The build has no
  fast-math and -ffp-contract=off: division and sqrtf are correctly rounded.
    den      k = 2   (float)(fp64 sum / count) + eps                                         S = den
    x_tm     k = 3   den, one division                                                       S = |x / den|
    sb_in    k = 3   the same                                                                S = |raw / den|
    d_fb     k = 7   dx / den (3) + mean term: sb_in (3) den (2) cast (1) = 6, + the sum (1) S = |dx / den| + sum |dx y| / den / count
                     (cumulative: sum over this and all later frames of sum_c |dx y| / den_t / (C (t + 1)))
    target   k = 8   with an expf of 1 ULP - PRINTED ONLY: the ROCm install carries no device-library document that states
                     expf's error, so the sharp rule alone governs the target
    mse      k = 3   fl(x - y) squared (2) + cast (1); gradient: fl(x - y), (float)(2 / n), product    S = |x - y| terms, which is
                     within the |x| + |y| the difference is formed from
    scale    k = 1
    norm     k = 3   g / scale (2), cast of sqrt of the fp64 sum (1)                          S = norm
    g        k = 8   unscale (2), coefficient = fl(max_norm / fl(norm + 1e-6)) (3 + 2), product (1)   S = |g coef|
    m        k = 12  g (8), g - m, (float)(1 - b1), product, sum                              S = |m| + (1 - b1) (|g| + |m|)
    v        k = 20  g^2 (16 + 1), (float)(1 - b2), product, sum                              S = v'
    p        k = 30  m (12) + denominator (v / 2 + sqrt, cast of sqrt(bc2), division, + eps = 14) + division, cast of
                     lr / bc1, product (3) + the sum (1)                                      S = |p| + lr / bc1 S_m / denom
* arithmetic outputs, sharp: the root mean square over elements of err / S is at most SHARP = 4 times the same statistic of
  the CPU fp32 evaluation (torch on the CPU at float32, same sequence; torch.optim.Adam + clip_grad_norm_ themselves for
  Adam) against the same fp64 result.  Every row repeats its draws until its smallest multi-element output has pooled
  POOL_ELEMS elements (glue_draws, mse_draws, target_draws) and fails if one falls short; the outputs of one element per
  call or utterance (offline den, loss, total norm) are held to the rule by the rows *-pool, which repeat a small shape.
* every row: the workspace is exactly the queried size and pre-filled with 0xFF; two calls in a row give the same bits;
  rows with pads = "all" give the same bits for every (Bp, Fp, Rp) in {(B, F, R), (ru16, ru16, ru16), (B + 3, F + 5, ru64(R))},
  ld_fb in {F, F + 7}, ld_dfb in {F, F + 9}; ld of the mask gradient in {2, 3, 16} everywhere.

Defect found by writing this module (by reading; the row `target-65792-rows` is there for it): fsn_train_cirm_target put
the row index on grid.y, so B Fs > 65535 rows (256 utterances of 257 bins) was a launch the runtime refuses.  The kernel
now strides over the rows; every other shape launches the same grid and computes the same bits.

With -s every row prints, per output, `hard` (worst err / bound, must be <= 1) and the two rms figures of the sharp rule in
units of 2^-24.
"""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -149
SENTINEL = 0x7FC0DEAD  # a quiet NaN with a recognisable payload
GUARD = 1024           # elements allocated (and checked) behind every output
POOL_ELEMS = 256       # the sharp statistic is asserted from this many pooled elements on
SHARP = 4.0
OFF, CUM = "offline", "cumulative"
NORM_ID = {OFF: 0, CUM: 1}  # FSN_NORM_OFFLINE_LAPLACE / FSN_NORM_CUMULATIVE_LAPLACE
EPS = float(O.EPSILON)
K = dict(den=2, x_tm=3, sb_in=3, d_fb=7, target=8, loss=3, grad=3, scale=1, norm=3, g=8, m=12, v=20, p=30)
NO_HARD = ("target",)  # expf's error is not documented in the install: sharp rule only (the hard ratio is printed)


def ru(n, m):
    return (n + m - 1) // m * m


# ---- the table --------------------------------------------------------------------------------------------------------

class Dims:
    """fsn_train_dims and what tr_dims derives from it."""

    def __init__(self, B, F, T, la, nb, groups, norm):
        self.B, self.F, self.T, self.la, self.nb, self.groups, self.norm = B, F, T, la, nb, groups, norm
        self.g = groups if (B > 1 and groups > 1) else 1
        self.Tp = T + la
        self.Fd = F - F % self.g
        self.Fs = self.Fd // self.g if self.g > 1 else F
        self.R = B * self.Fs
        self.C = 2 * nb + 2


class Row:
    def __init__(self, kind, path, **kw):
        self.kind, self.path, self.kw = kind, path, kw
        self.__dict__.update(kw)

    @property
    def id(self):
        return self.path


def G(path, B, F, T, la, nb, groups=1, norms=(OFF, CUM), signal="plain", pads="one", draws=1):
    return Row("glue", path, B=B, F=F, T=T, la=la, nb=nb, groups=groups, norms=norms, signal=signal, pads=pads, draws=draws)


ADAM_SIZES = (1, 255, 4095, 4096, 4097, 3 * 4096 + 5)


def _table():
    rows = []
    # Tp = T + la edges: scan segments ceil(Tp / 8) with empty trailing ones, 64-frame chunks, 32-frame tiles, Tp > 256.
    # R = 38 rows: a second, partial 32-row block of the scans
    for Tp, la in ((1, 0), (2, 0), (7, 2), (8, 0), (9, 2), (31, 0), (32, 2), (33, 0), (63, 2), (64, 0), (65, 2), (129, 0),
                   (257, 2), (300, 2)):
        rows.append(G(f"frames-Tp{Tp}-la{la}", 2, 19, Tp - la, la, 2))
    # F edges: both mirrors on one bin, partial 32-bin tiles, the f >= 256 stride, windows wider than the spectrum
    for F, nb in ((2, 0), (2, 1), (3, 2), (31, 15), (32, 15), (33, 0), (33, 1), (33, 7), (33, 15), (257, 15), (300, 15), (16, 15)):
        rows.append(G(f"bins-F{F}-nb{nb}", 2, F, 5, 2, nb))
    # band dropping: every residue of B % groups, F % groups != 0 (F = 11), B = 1, B <= groups at the C entry
    for g in (1, 2, 3):
        for B in (1, 2, 3, 4, 5, 7):
            rows.append(G(f"dropband-g{g}-B{B}", B, 11, 6, 2, 2, groups=g))
    # every padded size and leading dimension, the same bits
    rows.append(G("pads-all", 3, 21, 34, 2, 3, groups=2, pads="all"))
    # signals
    rows.append(G("zero-utterance", 2, 9, 12, 2, 2, signal="zero-utt"))
    rows.append(G("lead-zeros", 2, 9, 12, 2, 2, norms=(CUM,), signal="lead-zeros"))
    rows.append(G("scale-1e4", 2, 9, 12, 2, 2, signal="1e4"))
    rows.append(G("scale-1e-4", 2, 9, 12, 2, 2, signal="1e-4"))
    rows.append(G("den-pool", 8, 5, 4, 2, 1, norms=(OFF,), draws=32))
    # cIRM target: T around the 256-thread block, B Fs > 65535 rows
    for T in (1, 255, 256, 257):
        rows.append(Row("target", f"target-T{T}", B=3, F=5, T=T, groups=2))
    rows.append(Row("target", "target-65792-rows", B=256, F=257, T=1, groups=1))
    # rows <-> pieces
    for T, N, W, r, n in ((3, 10, 2, 4, 3), (2, 12, 16, 4, 3), (5, 7, 32, 7, 1), (4, 9, 16, 16, 1), (3, 3341, 32, 1728, 2)):
        rows.append(Row("pieces", f"pieces-T{T}-N{N}-W{W}-r{r}-n{n}", T=T, N=N, W=W, rows=r, n=n))
    rows.append(Row("pieces-refused", "pieces-refused"))
    # MSE, scale
    for n in (1, 255, 256, 4095, 4096, 4097, 3 * 4096 + 1, (1 << 20) + 3):
        rows.append(Row("mse", f"mse-n{n}", n=n, signal="plain", draws=1))
    rows.append(Row("mse", "mse-identical", n=4097, signal="identical", draws=1))
    rows.append(Row("mse", "mse-close-1e-4-at-1e3", n=4097, signal="close", draws=1))
    rows.append(Row("mse", "mse-loss-pool", n=4097, signal="plain", draws=POOL_ELEMS))
    rows.append(Row("scale", "scale-by-scalar", n=3 * 4096 + 5))
    # Adam
    mixed = tuple(ADAM_SIZES[i % 6] + (i // 6) for i in range(32))
    A = lambda path, **kw: Row("adam", path, **dict(dict(sizes=ADAM_SIZES, step=1, betas=(0.9, 0.999), clip="none", gval=1.0,
                                                         scale=None, found_inf=None, draws=1), **kw))
    rows.append(A("adam-sizes-step1", step=1))
    rows.append(A("adam-32-tensors-step2-above-clamp", sizes=mixed, step=2, clip="above"))
    rows.append(A("adam-step10-betas0-below-clamp", step=10, betas=(0.0, 0.0), clip="below"))
    rows.append(A("adam-step1000-betas.5-.9999-clip1e-3", step=1000, betas=(0.5, 0.9999), clip="strong"))
    rows.append(A("adam-step100000", step=100000))
    rows.append(A("adam-grads-1e-30", step=2, gval=1e-30))
    rows.append(A("adam-scale65536", step=3, scale=65536.0, clip="below"))
    rows.append(A("adam-scale65536-found-inf-0", step=3, scale=65536.0, found_inf=0.0, clip="below"))
    rows.append(A("adam-norm-pool", sizes=(4097,), step=2, draws=POOL_ELEMS, norm_only=True))
    for bad in ("found_inf", "inf", "nan"):
        rows.append(Row("adam-skip", f"adam-skip-{bad}", bad=bad, sizes=ADAM_SIZES, step=5, betas=(0.9, 0.999)))
    rows.append(Row("adam-refused", "adam-33-tensors-refused"))
    return rows


TABLE = _table()
GLUE_ROWS = [r for r in TABLE if r.kind == "glue"]


def glue_dims(row, norm):
    return Dims(row.B, row.F, row.T, row.la, row.nb, row.groups, norm)


def glue_draws(row, d):
    """Draws that give the smallest multi-element output (x_tm, d_fb: Tp B F; sb_in, the cumulative den: Tp R) POOL_ELEMS
    elements; at least the row's own count."""
    return max(row.draws, -(-POOL_ELEMS // min(d.Tp * d.B * d.F, d.Tp * d.R)))


def mse_draws(row):
    return max(row.draws, -(-POOL_ELEMS // row.n))


# ---- row order, sizes ---------------------------------------------------------------------------------------------------

def row_order(d, interleave=False):
    """(b, f) of every sub-band row, in drop_band's order (feature.py:309-345): group i holds samples i, i + g, ... at bins
    i, i + g, ... below F - F % g, the groups concatenated along the batch axis.  (interleave: the wrong order that sorts
    by sample - a stand-in for the CPU module.)"""
    if d.g == 1:
        return [(b, f) for b in range(d.B) for f in range(d.F)]
    order = [(b, f) for i in range(d.g) for b in range(i, d.B, d.g) for f in range(i, d.Fd, d.g)]
    return sorted(order) if interleave else order


def needed_ws_bytes(d):
    """The regions the host code carves, added up: rowsum [B F], total [B], partial [B Tp] (fp64), dmu [B rounded to 2]
    (fp32); cumulative: S / P [Tp][ru64(R)] (fp64), G [Tp][ru64(R)], cden [B Tp] (fp32).  This follows the library's own
    formula term by term, so comparing the query with it pins that formula and its 256 bytes of slack, no more; what
    guards against a kernel writing past the queried size is FSN_WS_CANARY=1, under which this module also runs."""
    n = (d.B * d.F + d.B + d.B * d.Tp) * 8 + ru(d.B, 2) * 4
    if d.norm == CUM:
        n += d.Tp * ru(d.R, 64) * 12 + d.B * d.Tp * 4
    return n


def pad_configs(d):
    out = []
    for Bp, Fp, Rp in ((d.B, d.F, d.R), (ru(d.B, 16), ru(d.F, 16), ru(d.R, 16)), (d.B + 3, d.F + 5, ru(d.R, 64))):
        for ld_fb in (d.F, d.F + 7):
            for ld_dfb in (d.F, d.F + 9):
                out.append(dict(Bp=Bp, Fp=Fp, Rp=Rp, ld_fb=ld_fb, ld_dfb=ld_dfb))
    return out


# ---- signals --------------------------------------------------------------------------------------------------------------

def make_glue_ops(row, d, draw):
    g = torch.Generator().manual_seed(7919 * draw + 31 * d.B + 17 * d.F + 13 * d.Tp + d.nb + 3 * d.g + (d.norm == CUM))
    mag = torch.randn(d.B, d.F, d.T, generator=g).abs() + 0.05
    fb = torch.relu(torch.randn(d.B, d.F, d.Tp, generator=g))  # about half exact zeros: the gate is exercised
    if row.signal == "zero-utt":
        mag[0], fb[0] = 0.0, 0.0
    elif row.signal == "lead-zeros":
        mag[0, :, :5], fb[0, :, :5] = 0.0, 0.0
    elif row.signal == "1e4":
        mag = mag * 1e4
    elif row.signal == "1e-4":
        mag = mag * 1e-4
    return dict(mag=mag, fb=fb, dx=torch.randn(d.Tp, d.R, d.C, generator=g), y=torch.randn(d.Tp, d.R, 2, generator=g),
                dmask=torch.randn(d.B, 2, d.Fs, d.T, generator=g))


# ---- the oracle: numpy fp64 forward ---------------------------------------------------------------------------------------

def oracle_forward(d, mag, fb, dtype=np.float64):
    """numpy, float64, from oracle/fullsubnet_oracle.py in the order of model.py:85-135.  mag [B][F][T], fb [B][F][Tp]
    (numpy).  Returns x_tm [Tp][B][F], mag_tm, sb_in [Tp][R][C], den ([B] or [Tp][R]).  (dtype float32: the oracle's own
    fp32 mode - statistics in fp64, cast once - which the CPU module feeds to the checkers as the stand-in to accept.)"""
    f64 = dtype
    norm = O.offline_laplace_norm if d.norm == OFF else O.cumulative_laplace_norm
    x = np.pad(mag.astype(f64)[:, None], [(0, 0), (0, 0), (0, 0), (0, d.la)])              # model.py:85  [B, 1, F, Tp]
    fb_in = norm(x, dtype=f64)[:, 0]                                                       # model.py:92-94
    unf = O.freq_unfold(x, d.nb).reshape(d.B, d.F, 2 * d.nb + 1, d.Tp)                     # model.py:101-103
    sb = np.concatenate([unf, fb.astype(f64)[:, :, None, :]], axis=2)                      # model.py:110  [B, F, C, Tp]
    sbn = norm(sb, dtype=f64)                                                              # model.py:111 (cumulative: Q4)
    if d.norm == OFF:
        den_full = sb.mean(axis=(1, 2, 3), dtype=np.float64).astype(f64) + f64(1e-5)                                    # [B]
    else:
        den_full = (np.cumsum(sb.sum(axis=2, dtype=np.float64), axis=-1)
                    / (d.C * np.arange(1, d.Tp + 1, dtype=np.float64))).astype(f64) + f64(EPS)       # [B, F, Tp]
    order = row_order(d)
    bi, fi = np.array([b for b, _ in order]), np.array([f for _, f in order])
    rows = sbn[bi, fi]                                                                     # [R, C, Tp]
    if d.g > 1 and d.B > d.groups:  # the oracle's own drop_band accepts this case: the row order is its
        dropped = O.drop_band(sbn.transpose(0, 2, 1, 3), d.groups)                          # [B, C, Fs, Tp]
        assert np.array_equal(dropped.transpose(0, 2, 1, 3).reshape(d.R, d.C, d.Tp), rows)
    den = den_full if d.norm == OFF else den_full[bi, fi].T
    return dict(x_tm=fb_in.transpose(2, 0, 1), mag_tm=x[:, 0].transpose(2, 0, 1), sb_in=rows.transpose(2, 0, 1), den=den)


# ---- the same sequence in plain torch: fp64 autograd (backward reference), fp32 (the CPU evaluation of the sharp rule) ---

def reflect_table(d, edge_repeat=False):
    j = torch.arange(d.F)[:, None] + torch.arange(2 * d.nb + 1)[None, :] - d.nb
    if edge_repeat:  # wrong: "symmetric" padding
        j = torch.where(j < 0, -j - 1, j)
        return torch.where(j >= d.F, 2 * d.F - 1 - j, j)
    j = j.abs()
    return torch.where(j >= d.F, 2 * (d.F - 1) - j, j)


def _t_offline(x, keep=None):
    """base_model.py:204-218.  keep (wrong stand-in): [B][F] mask of the elements the mean is taken over."""
    if keep is None:
        mu = x.mean(dim=tuple(range(1, x.dim())), keepdim=True)
    else:
        k = keep[:, :, None, None].to(x.dtype)
        mu = (x * k).sum(dim=(1, 2, 3), keepdim=True) / (k.sum(dim=(1, 2, 3), keepdim=True) * x.shape[2] * x.shape[3])
    den = mu + 1e-5
    return x / den, den.reshape(-1)


def _t_cumulative(x, count_shift=0, count_cap=None):
    """base_model.py:221-251: [B][C][F][T], dim 1 folded into the batch (Q4).  Returns the normed tensor and den [B C][T]."""
    B, C, F, T = x.shape
    xr = x.reshape(B * C, F, T)
    cum = torch.cumsum(xr.sum(dim=1), dim=-1)
    n = torch.arange(1, T + 1, dtype=x.dtype) + count_shift
    if count_cap is not None:
        n = torch.clamp(n, max=count_cap)
    den = cum / (n * F) + EPS
    return (xr / den[:, None, :]).reshape(B, C, F, T), den


def torch_sequence(d, mag, fb, variant=""):
    """mag [B][F][T], fb [B][F][Tp] (torch, one dtype; fb may require grad) -> the four tensors of oracle_forward.
    variant names one of the deliberately wrong versions the CPU module feeds to the checkers."""
    x = torch.nn.functional.pad(mag, (0, d.la))                                            # [B, F, Tp]
    order = row_order(d, interleave=variant == "interleave")
    bi, fi = torch.tensor([b for b, _ in order]), torch.tensor([f for _, f in order])
    unf = x[:, reflect_table(d, variant == "edge_repeat"), :]                             # [B, F, W, Tp]
    sb = torch.cat([unf, fb[:, :, None, :]], dim=2)                                        # [B, F, C, Tp]
    if d.norm == OFF:
        keep = None
        if variant == "mean_kept_rows":
            keep = torch.zeros(d.B, d.F, dtype=torch.bool)
            keep[bi, fi] = True
        fb_in = _t_offline(x[:, None])[0][:, 0]
        sbn, den = _t_offline(sb, keep)
    else:
        kw = dict(count_shift=1) if variant == "count_off_by_one" else dict(count_cap=d.T) if variant == "no_lookahead_count" else {}
        fb_in = _t_cumulative(x[:, None], **kw)[0][:, 0]
        sbn, den = _t_cumulative(sb, **kw)
        den = den.reshape(d.B, d.F, d.Tp)[bi, fi].t()
    return dict(x_tm=fb_in.permute(2, 0, 1), mag_tm=x.permute(2, 0, 1), sb_in=sbn[bi, fi].permute(2, 0, 1), den=den)


def torch_backward(d, mag, fb, dx, variant=""):
    """d loss / d fb_out for loss = sum(sb_in * dx), times fb_out > 0: [Tp][B][F]."""
    fb = fb.clone().requires_grad_(True)
    out = torch_sequence(d, mag, fb)
    grad = torch.autograd.grad((out["sb_in"] * dx).sum(), fb)[0]
    if variant in ("stop_at_frame", "no_dmu_dropped"):
        # the direct term alone: the same graph with the divisors held constant
        den = out["den"].detach()
        order = row_order(d)
        bi, fi = torch.tensor([b for b, _ in order]), torch.tensor([f for _, f in order])
        direct = torch.zeros_like(grad)
        direct[bi, fi] = (dx[:, :, -1] / (den[bi][None, :] if d.norm == OFF else den)).t()
        rest = grad - direct  # offline: dmu[b] everywhere; cumulative: G[t] = sum over t' >= t of P[t']
        if variant == "stop_at_frame":
            rest = rest - torch.cat([rest[:, :, 1:], torch.zeros_like(rest[:, :, :1])], dim=2)  # P[t] alone
        else:
            kept = torch.zeros(d.B, d.F, dtype=torch.bool)
            kept[bi, fi] = True
            rest = rest * kept[:, :, None]
        grad = direct + rest
    if variant != "no_gate":
        grad = grad * (fb.detach() > 0)
    return grad.permute(2, 0, 1)


def glue_exact(d, ops):
    """The outputs that are data movement: the padded magnitude time-major, the mask and its adjoint."""
    mag_tm = torch.nn.functional.pad(ops["mag"], (0, d.la)).permute(2, 0, 1).contiguous()
    mask = ops["y"][d.la:].reshape(d.T, d.B, d.Fs, 2).permute(1, 3, 2, 0).contiguous()    # model.py:129-135
    dy = torch.zeros(d.Tp, d.R, 2)
    dy[d.la:] = ops["dmask"].permute(3, 0, 2, 1).reshape(d.T, d.R, 2)
    return dict(mag_tm=mag_tm.numpy(), mask=mask.numpy(), dy=dy.numpy())


def glue_standin(d, ops, variant="", dtype=torch.float32):
    """What the entries return, evaluated by torch on the CPU at `dtype` and rounded to fp32 (float32: the evaluation the
    sharp rule measures against); with a variant, one of the wrong versions."""
    mag, fb, dx = (ops[k].to(dtype) for k in ("mag", "fb", "dx"))
    out = {k: v.detach().float().contiguous().numpy() for k, v in torch_sequence(d, mag, fb, variant).items()}
    out["d_fb"] = torch_backward(d, mag, fb, dx, variant).float().contiguous().numpy()
    out.update({k: v for k, v in glue_exact(d, ops).items() if k != "mag_tm"})
    return out


def glue_reference(d, ops):
    """name -> (fp64 reference, S, CPU fp32 evaluation) of every arithmetic output, and the exact outputs."""
    mag, fb, dx = ops["mag"], ops["fb"], ops["dx"]
    ref = oracle_forward(d, mag.numpy(), fb.numpy())
    cpu = glue_standin(d, ops)
    d_fb = torch_backward(d, mag.double(), fb.double(), dx.double()).numpy()
    order = row_order(d)
    bi, fi = np.array([b for b, _ in order]), np.array([f for _, f in order])
    dx64, y64, den = dx.numpy().astype(np.float64), ref["sb_in"], ref["den"]
    A = np.abs(dx64 * y64).sum(axis=2)                                                     # [Tp, R]
    S = np.zeros((d.Tp, d.B, d.F))
    if d.norm == OFF:
        per_b = np.zeros(d.B)
        np.add.at(per_b, bi, A.sum(axis=0))
        S += (per_b / den / (d.F * d.C * d.Tp))[None, :, None]
        S[:, bi, fi] += np.abs(dx64[:, :, -1]) / den[bi][None, :]
    else:
        Q = A / den / (d.C * np.arange(1, d.Tp + 1, dtype=np.float64))[:, None]
        S[:, bi, fi] = np.abs(dx64[:, :, -1]) / den + np.cumsum(Q[::-1], axis=0)[::-1]
    S *= (fb.numpy() > 0).transpose(2, 0, 1)
    arith = dict(x_tm=(ref["x_tm"], np.abs(ref["x_tm"]), cpu["x_tm"]), sb_in=(ref["sb_in"], np.abs(ref["sb_in"]), cpu["sb_in"]),
                 den=(ref["den"], np.abs(ref["den"]), cpu["den"]), d_fb=(d_fb, S, cpu["d_fb"]))
    exact = glue_exact(d, ops)
    assert np.array_equal(exact["mag_tm"], ref["mag_tm"].astype(np.float32))
    return arith, exact


# ---- cIRM target, MSE, Adam ---------------------------------------------------------------------------------------------

def make_target_ops(row, draw=0):
    g = torch.Generator().manual_seed(101 + draw + row.T + row.B)
    nr, ni, cr, ci = (torch.randn(row.B, row.F, row.T, generator=g) for _ in range(4))
    n = nr.numel()
    nr.view(-1)[0], ni.view(-1)[0] = 0.0, 0.0  # a noisy bin that is exactly 0 + 0i
    tiny = torch.arange(n) % 7 == 3              # |clean / noisy| ~ 1e3: far beyond the clamp and the saturation
    nr.view(-1)[tiny] *= 1e-3
    ni.view(-1)[tiny] *= 1e-3
    for t, v in zip((nr, ni, cr, ci), (1e-3, 0.0, -1.0, 1.0)):  # real part -893: the -100 clamp; imaginary +893: |m| > 50
        t.view(-1)[2 * row.T] = v  # (b 0, f 2, t 0): a bin every grouping keeps
    return dict(nr=nr, ni=ni, cr=cr, ci=ci)


def torch_target(nr, ni, cr, ci):
    """mask.py:7-44 in plain torch, [B][F][T][2]."""
    den = nr * nr + ni * ni + EPS
    m = torch.stack(((nr * cr + ni * ci) / den, (nr * ci - ni * cr) / den), dim=-1)
    m = -100 * (m <= -100) + m * (m > -100)
    e = torch.exp(-0.1 * m)
    return 10 * (1 - e) / (1 + e)


def target_draws(row):
    """Draws that pool POOL_ELEMS elements of the target."""
    d = Dims(row.B, row.F, row.T, 0, 0, row.groups, OFF)
    return max(1, -(-POOL_ELEMS // (d.R * 2 * d.T)))


def target_reference(row, ops):
    d = Dims(row.B, row.F, row.T, 0, 0, row.groups, OFF)
    a = {k: v.numpy().astype(np.float64) for k, v in ops.items()}
    ref = O.build_complex_ideal_ratio_mask(a["nr"], a["ni"], a["cr"], a["ci"], dtype=np.float64)        # [B, F, T, 2]
    den = a["nr"] ** 2 + a["ni"] ** 2 + EPS
    Sm = np.stack(((np.abs(a["nr"] * a["cr"]) + np.abs(a["ni"] * a["ci"])) / den,
                   (np.abs(a["nr"] * a["ci"]) + np.abs(a["ni"] * a["cr"])) / den), axis=-1)
    m = np.stack(((a["nr"] * a["cr"] + a["ni"] * a["ci"]) / den, (a["nr"] * a["ci"] - a["ni"] * a["cr"]) / den), axis=-1)
    e = np.exp(-0.1 * np.maximum(m, -100.0))
    S = 20 * e / (1 + e) ** 2 * (0.1 * Sm + 1) + np.abs(ref)
    cpu = torch_target(ops["nr"], ops["ni"], ops["cr"], ops["ci"]).numpy()
    order = row_order(d)
    bi, fi = np.array([b for b, _ in order]), np.array([f for _, f in order])
    lay = lambda t: t[bi, fi].reshape(d.B, d.Fs, d.T, 2).transpose(0, 3, 1, 2)                           # [B][2][Fs][T]
    assert float(m.min()) < -100 and float(m.max()) > 50
    return d, (lay(ref), lay(S), lay(cpu))


def pieces_reference(src, T, N, W, rows, n):
    """[T][N][W] -> [n][T][rows][W], rows beyond N zero."""
    full = np.zeros((T, n * rows, W), np.float32)
    full[:, :N] = src
    return np.ascontiguousarray(full.reshape(T, n, rows, W).transpose(1, 0, 2, 3))


def make_mse_ops(row, draw):
    g = torch.Generator().manual_seed(row.n + draw)
    x = torch.randn(row.n, generator=g)
    if row.signal == "identical":
        y = x.clone()
    elif row.signal == "close":
        x = 1e3 + torch.randn(row.n, generator=g)
        y = x + 1e-4 * torch.randn(row.n, generator=g).sign()
    else:
        y = torch.randn(row.n, generator=g)
    return x, y


def mse_reference(x, y):
    d = x.numpy().astype(np.float64) - y.numpy().astype(np.float64)
    n = d.size
    xg = x.clone().requires_grad_(True)
    loss32 = torch.nn.functional.mse_loss(xg, y)
    g32 = torch.autograd.grad(loss32, xg)[0]
    loss = np.array([(d * d).sum() / n])
    return dict(loss=(loss, loss, np.array([float(loss32.detach())])), grad=(2 * d / n, np.abs(2 * d / n), g32.numpy()))


class AdamCase:
    """Operands of one fsn_clip_adam_step call: fp32 numpy p, g, m, v per tensor; cfg values as the fp32 the C struct holds."""

    def __init__(self, sizes, step, betas, clip="none", gval=1.0, scale=None, seed=0, lr=1e-3, eps=1e-8):
        rng = np.random.default_rng(seed + 1000 * len(sizes) + step)
        s = 1.0 if scale is None else scale
        self.p = [(rng.standard_normal(n) * 0.05).astype(np.float32) for n in sizes]
        self.g = [(rng.standard_normal(n) * gval * s).astype(np.float32) for n in sizes]
        self.m = [(rng.standard_normal(n) * 0.1 * gval).astype(np.float32) for n in sizes]
        self.v = [((rng.standard_normal(n) * gval) ** 2 * 0.01).astype(np.float32) for n in sizes]
        self.step, self.scale = step, scale
        self.lr, self.b1, self.b2, self.eps = (float(np.float32(a)) for a in (lr, betas[0], betas[1], eps))
        norm = math.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in self.g)) / s
        self.max_norm = float(np.float32(dict(none=0.0, above=norm * (1 + 1e-3), below=norm * (1 - 1e-3), strong=1e-3 * norm)[clip]))


def adam_oracle(c, step=None, variant=""):
    """float64: clip_grad_norm_ (coefficient max_norm / (norm + 1e-6) clamped to 1), then torch.optim.Adam without weight
    decay: lerp, mul / addcmul, sqrt(v) / sqrt(bc2) + eps, both bias corrections from the step count.
    Returns name -> list per tensor of (ref, S); norm: one (ref, S)."""
    k = c.step if step is None else step
    s = 1.0 if c.scale is None else c.scale
    gs = [g.astype(np.float64) / s for g in c.g]
    norm = math.sqrt(sum(float((g * g).sum()) for g in gs))
    coef = 1.0
    if c.max_norm > 0:
        coef = c.max_norm / (norm + 1e-6)
        if variant != "no_clamp":
            coef = min(coef, 1.0)
    bc1, bc2 = 1 - c.b1 ** k, 1 - c.b2 ** (k - 1 if variant == "bc2_prev_step" else k)
    out = dict(norm=(np.array([norm]), np.array([norm])), g=[], m=[], v=[], p=[])
    for p, g, m, v in zip(c.p, gs, c.m, c.v):
        p, m, v = p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
        gc = g * coef
        m1 = m + (1 - c.b1) * (gc - m)                         # lerp
        v1 = v * c.b2 + (1 - c.b2) * gc * gc                   # mul, addcmul
        denom = np.sqrt(v1) / math.sqrt(bc2) + c.eps if bc2 > 0 else np.full_like(v1, np.inf)
        Sm = np.abs(m) + (1 - c.b1) * (np.abs(gc) + np.abs(m))
        out["g"].append((gc, np.abs(gc)))
        out["m"].append((m1, Sm))
        out["v"].append((v1, v1))
        out["p"].append((p - c.lr / bc1 * m1 / denom, np.abs(p) + c.lr / bc1 * Sm / denom))
    return out


def adam_torch(c, dtype, step=None):
    """clip_grad_norm_ + torch.optim.Adam themselves on the CPU at `dtype`, the moments and the step count preset."""
    k = c.step if step is None else step
    ps = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dtype)) for p in c.p]
    for p, g in zip(ps, c.g):
        p.grad = torch.from_numpy(g.copy()).to(dtype)
        if c.scale is not None:
            p.grad.mul_(1.0 / c.scale)  # GradScaler.unscale_
    opt = torch.optim.Adam(ps, lr=c.lr, betas=(c.b1, c.b2), eps=c.eps, foreach=False)
    for p, m, v in zip(ps, c.m, c.v):
        opt.state[p] = dict(step=torch.tensor(float(k - 1)), exp_avg=torch.from_numpy(m).to(dtype).clone(),
                            exp_avg_sq=torch.from_numpy(v).to(dtype).clone())
    norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in ps]))
    if c.max_norm > 0:
        norm = torch.nn.utils.clip_grad_norm_(ps, c.max_norm, foreach=False)
    opt.step()
    return dict(norm=np.array([float(norm)]), g=[p.grad.numpy() for p in ps], m=[opt.state[p]["exp_avg"].numpy() for p in ps],
                v=[opt.state[p]["exp_avg_sq"].numpy() for p in ps], p=[p.detach().numpy() for p in ps])


# ---- the checkers -----------------------------------------------------------------------------------------------------------

class Stat:
    """Error of one arithmetic output against fp64, accumulated over draws."""

    def __init__(self, name, scalar=False, k=None, no_hard=None):
        """scalar: an output of one element per call or utterance (offline den, loss, total norm), whose sharp rule is
        asserted by the *-pool rows; every other output must have pooled POOL_ELEMS elements when it is checked.
        k, no_hard: for the sweeps that share this checker and keep a k table of their own (default: this module's)."""
        self.name, self.k, self.scalar = name, K[name] if k is None else k, scalar
        self.no_hard = name in NO_HARD if no_hard is None else no_hard
        self.tiny = TINY if name in ("g", "m", "v", "p") else 0.0  # gradients of 1e-30: squares below the fp32 range
        self.n = 0
        self.hard = 0.0
        self.ss = {"hip": 0.0, "cpu": 0.0}

    def add(self, got, ref64, S, cpu, k=None):
        """k: per-element rounding counts where they differ within one output (default: the output's own)."""
        k = self.k if k is None else np.asarray(k, dtype=np.float64)
        got, ref64, S, cpu = (np.asarray(a, dtype=np.float64) for a in (got, ref64, S, cpu))
        assert got.shape == ref64.shape == S.shape == cpu.shape, f"{self.name}: shapes {got.shape} {ref64.shape} {S.shape} {cpu.shape}"
        self.n += ref64.size
        pos = S > 0
        for key, t in (("hip", got), ("cpu", cpu)):
            with np.errstate(invalid="ignore"):
                err = np.abs(t - ref64)
            err = np.where(np.isnan(err), np.inf, err)
            if key == "hip":
                bound = k * (U * S + self.tiny)
                ok = bound > 0
                self.hard = max(self.hard, float(np.where(ok, err / np.where(ok, bound, 1.0), np.where(err > 0, np.inf, 0.0)).max()))
            rel = np.where(pos, err / np.where(pos, S, 1.0), np.where(err > 0, np.inf, 0.0))
            self.ss[key] += float((rel * rel).sum())

    def rms(self, key):
        return math.sqrt(self.ss[key] / max(self.n, 1)) / U

    def report(self, row_id):
        print(f"[glue-sweep] {row_id} {self.name}: n {self.n} hard {self.hard:.4f} rms hip {self.rms('hip'):.4f} u cpu {self.rms('cpu'):.4f} u")

    def check(self):
        if not self.no_hard:
            assert self.hard <= 1.0, f"{self.name}: worst element at {self.hard:.3f} of the {self.k} 2^-24 S bound"
        if not self.scalar:
            assert self.n >= POOL_ELEMS, f"{self.name}: {self.n} elements pooled, the sharp rule needs {POOL_ELEMS}"
        if self.n >= POOL_ELEMS:
            assert self.rms("hip") <= SHARP * self.rms("cpu"), \
                f"{self.name}: rms relative error {self.rms('hip'):.4f} u against {self.rms('cpu'):.4f} u of the CPU fp32 evaluation"


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def check_exact(name, got, want):
    """Bit for bit: -0 is not +0, a NaN is compared by its payload."""
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, f"{name}: shape {got.shape}, expected {want.shape}"
    bad = got != want
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} elements differ; first at {i}: "
                             f"got {got.view(np.float32)[i]!r}, expected {want.view(np.float32)[i]!r}")


def check_glue(stats, arith, exact, outs):
    """outs: the declared regions of the entries' outputs (numpy fp32)."""
    for name in ("mag_tm", "mask", "dy"):
        if name in outs:
            check_exact(name, outs[name], exact[name])
    for name, (ref, S, cpu) in arith.items():
        if name in outs:
            stats.setdefault(name, Stat(name, scalar=name == "den" and np.ndim(ref) == 1)).add(outs[name], ref, S, cpu)


def finish(row_id, stats):
    for s in stats.values():
        s.report(row_id)
    for s in stats.values():
        s.check()


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


def _untouched(buf, lo, what):
    assert bool((buf[lo:] == SENTINEL).all()), f"{what}: written outside its declared region"


def _all_zero_bits(t, what):
    assert bool((t == 0).all()), f"{what}: not exactly +0"


def _embed(t, shape, dev):
    """t in the leading corner of a sentinel-filled tensor of `shape`: padding that must not be read."""
    out = torch.full(shape, SENTINEL, dtype=torch.int32).view(torch.float32)
    out[tuple(slice(0, s) for s in t.shape)] = t
    return out.to(dev)


def run_glue(fsn, d, ops, pad):
    """fsn_train_fb_input -> fsn_train_sb_input -> fsn_train_sb_input_backward on one workspace, as train.py does, then
    the mask entries.  Returns the declared regions as numpy."""
    lib, L, dev = fsn._lib, fsn._lib.lib(), torch.device("cuda:0")
    dims = lib.TrainDims(d.B, d.F, d.T, d.la, d.nb, d.groups, NORM_ID[d.norm])
    dp, p, st = ctypes.byref(dims), lib.dev_ptr, lib.stream_ptr(dev)
    Bp, Fp, Rp, ld_fb, ld_dfb = (pad[k] for k in ("Bp", "Fp", "Rp", "ld_fb", "ld_dfb"))
    Tp, B, F, R, C = d.Tp, d.B, d.F, d.R, d.C
    nbytes = L.fsn_train_glue_workspace_bytes(dp)
    assert needed_ws_bytes(d) <= nbytes <= needed_ws_bytes(d) + 256
    ws = lib.workspace(nbytes, dev).fill_(0xFF)
    f32 = lambda buf: buf.view(torch.float32)
    out = {}
    # full-band input
    mag = ops["mag"].to(dev).contiguous()
    xb, mb = _sentinel(Tp * Bp * Fp, dev), _sentinel(Tp * Bp * Fp, dev)
    lib.check(L.fsn_train_fb_input(dp, p(mag), p(f32(xb)), p(f32(mb)), Bp, Fp, ws.data_ptr(), ws.numel(), st))
    for name, buf in (("x_tm", xb), ("mag_tm", mb)):
        _untouched(buf, Tp * Bp * Fp, name)
        v = buf[:Tp * Bp * Fp].view(Tp, Bp, Fp)
        _all_zero_bits(v[:, B:, :], f"{name} rows >= B")
        _all_zero_bits(v[:, :, F:], f"{name} columns >= F")
        out[name] = f32(v)[:, :B, :F].cpu().numpy()
    # sub-band input
    fb_tm = _embed(ops["fb"].permute(2, 0, 1), (Tp, Bp, ld_fb), dev)
    n_den = L.fsn_train_den_elems(dp, Rp)
    assert n_den == (B if d.norm == OFF else Tp * Rp)
    sb, den = _sentinel(Tp * Rp * 32, dev), _sentinel(n_den, dev)
    mag_tm = f32(mb)[:Tp * Bp * Fp]
    lib.check(L.fsn_train_sb_input(dp, p(mag_tm), p(fb_tm), ld_fb, Bp, Fp, p(f32(sb)), Rp, p(f32(den)), ws.data_ptr(), ws.numel(), st))
    _untouched(sb, Tp * Rp * 32, "sb_in")
    _untouched(den, n_den, "den")
    v = sb[:Tp * Rp * 32].view(Tp, Rp, 32)
    _all_zero_bits(v[:, R:, :], "sb_in rows >= R")
    _all_zero_bits(v[:, :, C:], "sb_in columns >= 2 nb + 2")
    out["sb_in"] = f32(v)[:, :R, :C].cpu().numpy()
    dv = f32(den)[:n_den]
    out["den"] = (dv if d.norm == OFF else dv.view(Tp, Rp)[:, :R]).cpu().numpy()
    # its backward, on the forward's own sb_in and den
    dx = _embed(ops["dx"], (Tp, Rp, 32), dev)
    dfb = _sentinel(Tp * Bp * ld_dfb, dev)
    lib.check(L.fsn_train_sb_input_backward(dp, p(dx), p(f32(sb)[:Tp * Rp * 32]), Rp, p(dv), p(fb_tm), ld_fb, Bp, p(f32(dfb)), ld_dfb,
                                            ws.data_ptr(), ws.numel(), st))
    _untouched(dfb, Tp * Bp * ld_dfb, "d_fb")
    v = dfb[:Tp * Bp * ld_dfb].view(Tp, Bp, ld_dfb)
    _all_zero_bits(v[:, B:, :], "d_fb rows >= B")
    _all_zero_bits(v[:, :, F:], "d_fb columns >= F")
    out["d_fb"] = f32(v)[:, :B, :F].cpu().numpy()
    # the mask and its gradient
    y = _embed(ops["y"], (Tp, Rp, 2), dev)
    mk = _sentinel(B * 2 * d.Fs * d.T, dev)
    lib.check(L.fsn_train_mask_out(dp, p(y), Rp, p(f32(mk)), st))
    _untouched(mk, B * 2 * d.Fs * d.T, "mask")
    out["mask"] = f32(mk)[:B * 2 * d.Fs * d.T].view(B, 2, d.Fs, d.T).cpu().numpy()
    dmask = ops["dmask"].to(dev).contiguous()
    for ld in (2, 3, 16):
        dy = _sentinel(Tp * Rp * ld, dev)
        lib.check(L.fsn_train_mask_grad(dp, p(dmask), p(f32(dy)), Rp, ld, st))
        _untouched(dy, Tp * Rp * ld, f"dy ld {ld}")
        v = dy[:Tp * Rp * ld].view(Tp, Rp, ld)
        _all_zero_bits(v[:, R:, :], "dy rows >= R")
        _all_zero_bits(v[:, :, 2:], "dy columns >= 2")
        _all_zero_bits(v[:d.la], "dy look-ahead frames")
        got = f32(v)[:, :R, :2].cpu().numpy()
        if "dy" in out:
            check_exact(f"dy: ld {ld} against ld 2", got, out["dy"])
        out["dy"] = got
    torch.cuda.synchronize()
    return out


def _same_outs(a, b, what):
    for k in a:
        check_exact(f"{k}: {what}", a[k], b[k])


def run_glue_row(fsn, row):
    for norm in row.norms:
        d = glue_dims(row, norm)
        Fs, R = ctypes.c_int(0), ctypes.c_int(0)
        dims = fsn._lib.TrainDims(d.B, d.F, d.T, d.la, d.nb, d.groups, NORM_ID[norm])
        assert fsn._lib.lib().fsn_train_rows(ctypes.byref(dims), ctypes.byref(Fs), ctypes.byref(R)) == 0
        assert (Fs.value, R.value) == (d.Fs, len(row_order(d)))
        pads = pad_configs(d)
        stats = {}
        for draw in range(glue_draws(row, d)):
            ops = make_glue_ops(row, d, draw)
            arith, exact = glue_reference(d, ops)
            first = pads[(GLUE_ROWS.index(row) + 5 * draw) % len(pads)]
            outs = run_glue(fsn, d, ops, first)
            for v in outs.values():
                assert np.isfinite(v).all(), "a declared element was not written, or is not finite"
            if draw == 0:
                _same_outs(run_glue(fsn, d, ops, first), outs, "two calls in a row")
                for pad in (pads if row.pads == "all" else pads[-1:]):
                    _same_outs(run_glue(fsn, d, ops, pad), outs, f"padded sizes {pad}")
            if row.signal == "zero-utt":  # divisor 1e-5 resp. eps: exact zeros, no NaN
                for k, sl in (("x_tm", np.s_[:, 0]), ("d_fb", np.s_[:, 0])):
                    assert not bits(outs[k][sl]).any(), f"{k}: the all-zero utterance is not exactly +0"
                zr = [i for i, (b, _) in enumerate(row_order(d)) if b == 0]
                assert not bits(outs["sb_in"][:, zr]).any(), "sb_in: the all-zero utterance is not exactly +0"
            check_glue(stats, arith, exact, outs)
        finish(f"{row.id} {norm}", stats)


def run_glue_refusals(fsn):
    """Cumulative norm with Rp = ru64(R) + 1: refused, fsn_last_error set, nothing written."""
    lib, L, dev = fsn._lib, fsn._lib.lib(), torch.device("cuda:0")
    d = Dims(2, 9, 4, 2, 2, 1, CUM)
    dims = lib.TrainDims(d.B, d.F, d.T, d.la, d.nb, d.groups, 1)
    dp, p, st = ctypes.byref(dims), lib.dev_ptr, lib.stream_ptr(dev)
    Rp = ru(d.R, 64) + 1
    nbytes = L.fsn_train_glue_workspace_bytes(dp)
    ws = lib.workspace(nbytes, dev).fill_(0xFF)
    z = torch.zeros(d.Tp * Rp * 32, device=dev)
    sb, den, dfb = _sentinel(d.Tp * Rp * 32, dev), _sentinel(d.Tp * Rp, dev), _sentinel(d.Tp * d.B * d.F, dev)
    f32 = lambda b: b.view(torch.float32)
    rc = L.fsn_train_sb_input(dp, p(z), p(z), d.F, d.B, d.F, p(f32(sb)), Rp, p(f32(den)), ws.data_ptr(), ws.numel(), st)
    assert rc != 0 and b"64" in L.fsn_last_error()
    rc = L.fsn_train_sb_input_backward(dp, p(z), p(z), Rp, p(z), p(z), d.F, d.B, p(f32(dfb)), d.F, ws.data_ptr(), ws.numel(), st)
    assert rc != 0 and b"64" in L.fsn_last_error()
    torch.cuda.synchronize()
    for b in (sb, den, dfb):
        _untouched(b, 0, "a refused call")
    assert bool((ws == 0xFF).all()), "a refused call wrote to its workspace"


def run_target_row(fsn, row):
    lib, L, dev = fsn._lib, fsn._lib.lib(), torch.device("cuda:0")
    stats = {"target": Stat("target")}
    for draw in range(target_draws(row)):
        ops = make_target_ops(row, draw)
        d, (ref, S, cpu) = target_reference(row, ops)
        dims = lib.TrainDims(d.B, d.F, d.T, 0, 0, d.groups, 0)
        dev_ops = {k: v.to(dev).contiguous() for k, v in ops.items()}
        n = d.B * 2 * d.Fs * d.T
        got = []
        for _ in range(2):
            buf = _sentinel(n, dev)
            lib.check(L.fsn_train_cirm_target(ctypes.byref(dims), *(lib.dev_ptr(dev_ops[k]) for k in ("nr", "ni", "cr", "ci")),
                                              lib.dev_ptr(buf.view(torch.float32)), lib.stream_ptr(dev)))
            torch.cuda.synchronize()
            _untouched(buf, n, "target")
            got.append(buf.view(torch.float32)[:n].view(d.B, 2, d.Fs, d.T).cpu().numpy())
        check_exact("target: two calls in a row", got[1], got[0])
        assert np.isfinite(got[0]).all() and float(np.abs(got[0]).max()) <= 10.0
        assert not bits(got[0][0, :, 0, 0]).any(), "the 0 + 0i noisy bin does not give exactly +0"
        stats["target"].add(got[0], ref, S, cpu)
    finish(row.id, stats)


def run_pieces_row(fsn, row):
    lib, L, dev = fsn._lib, fsn._lib.lib(), torch.device("cuda:0")
    T, N, W, rows, n = row.T, row.N, row.W, row.rows, row.n
    src = torch.randn(T, N, W, generator=torch.Generator().manual_seed(N + W))
    want = pieces_reference(src.numpy(), T, N, W, rows, n)
    s_dev = src.to(dev)
    pieces = _sentinel(n * T * rows * W, dev)
    lib.check(L.fsn_train_rows_pieces(lib.dev_ptr(s_dev), lib.dev_ptr(pieces.view(torch.float32)), T, N, W, rows, n, 1, lib.stream_ptr(dev)))
    _untouched(pieces, n * T * rows * W, "pieces")
    check_exact("pieces", pieces.view(torch.float32)[:n * T * rows * W].view(n, T, rows, W).cpu().numpy(), want)
    back = _sentinel(T * N * W, dev)
    lib.check(L.fsn_train_rows_pieces(lib.dev_ptr(pieces.view(torch.float32)[:n * T * rows * W]), lib.dev_ptr(back.view(torch.float32)),
                                      T, N, W, rows, n, 0, lib.stream_ptr(dev)))
    _untouched(back, T * N * W, "rows")
    check_exact("rows -> pieces -> rows", back.view(torch.float32)[:T * N * W].view(T, N, W).cpu().numpy(), src.numpy())


def run_pieces_refused(fsn):
    lib, L, dev = fsn._lib, fsn._lib.lib(), torch.device("cuda:0")
    src, dst = torch.zeros(64, device=dev), _sentinel(64, dev)
    for T, N, W, rows, n in ((1, 4, 3, 4, 1), (1, 9, 2, 4, 2), (65536, 1, 2, 1, 1)):  # odd W, n rows < N, T = 65536
        for to_pieces in (0, 1):
            rc = L.fsn_train_rows_pieces(lib.dev_ptr(src), lib.dev_ptr(dst.view(torch.float32)), T, N, W, rows, n, to_pieces, lib.stream_ptr(dev))
            assert rc != 0 and L.fsn_last_error(), (T, N, W, rows, n)
    torch.cuda.synchronize()
    _untouched(dst, 0, "a refused call")


def run_mse_row(fsn, row):
    lib, L, dev = fsn._lib, fsn._lib.lib(), torch.device("cuda:0")
    stats = {}
    for draw in range(mse_draws(row)):
        x, y = make_mse_ops(row, draw)
        ref = mse_reference(x, y)
        xd, yd = x.to(dev), y.to(dev)
        nbytes = L.fsn_mse_loss_workspace_bytes(row.n)
        res = []
        for with_grad in (True, False, True):
            ws = lib.workspace(nbytes, dev).fill_(0xFF)
            loss, grad = _sentinel(1, dev), _sentinel(row.n, dev)
            lib.check(L.fsn_mse_loss(lib.dev_ptr(xd), lib.dev_ptr(yd), row.n, lib.dev_ptr(loss.view(torch.float32)),
                                     lib.dev_ptr(grad.view(torch.float32)) if with_grad else None, ws.data_ptr(), ws.numel(),
                                     lib.stream_ptr(dev)))
            _untouched(loss, 1, "loss")
            _untouched(grad, row.n if with_grad else 0, "grad_input")
            res.append((loss.view(torch.float32)[:1].cpu().numpy(), grad.view(torch.float32)[:row.n].cpu().numpy()))
            if draw > 0:
                break
        if draw == 0:
            check_exact("loss: without grad_input", res[1][0], res[0][0])
            check_exact("loss: two calls in a row", res[2][0], res[0][0])
            check_exact("grad: two calls in a row", res[2][1], res[0][1])
        if row.signal == "identical":
            assert not bits(res[0][0]).any() and not bits(res[0][1]).any(), "identical inputs: loss and gradient are exactly +0"
        for name, got in (("loss", res[0][0]), ("grad", res[0][1])):
            stats.setdefault(name, Stat(name, scalar=name == "loss")).add(got, *ref[name])
    finish(row.id, stats)


def run_scale_row(fsn, row):
    lib, L, dev = fsn._lib, fsn._lib.lib(), torch.device("cuda:0")
    x = torch.randn(row.n, generator=torch.Generator().manual_seed(3))
    s = torch.tensor([0.3])
    y = _sentinel(row.n, dev)
    lib.check(L.fsn_scale_by_scalar(lib.dev_ptr(x.to(dev)), lib.dev_ptr(s.to(dev)), lib.dev_ptr(y.view(torch.float32)), row.n, lib.stream_ptr(dev)))
    _untouched(y, row.n, "y")
    ref = x.numpy().astype(np.float64) * float(s)
    stats = {"scale": Stat("scale")}
    stats["scale"].add(y.view(torch.float32)[:row.n].cpu().numpy(), ref, np.abs(ref), (x * s).numpy())
    finish(row.id, stats)


class AdamDevice:
    """One set of tensors on the device, every one behind a sentinel."""

    def __init__(self, fsn, c):
        self.lib, self.L, self.dev, self.c = fsn._lib, fsn._lib.lib(), torch.device("cuda:0"), c
        self.n = len(c.p)
        self.buf = {k: [self._put(a) for a in getattr(c, k)] for k in ("p", "g", "m", "v")}
        self.numel = (ctypes.c_size_t * self.n)(*[a.size for a in c.p])
        self.skipped = torch.zeros(2, dtype=torch.int32, device=self.dev)
        self.norm = _sentinel(1, self.dev)

    def _put(self, a):
        b = _sentinel(a.size, self.dev)
        b[:a.size] = torch.from_numpy(a).view(torch.int32).to(self.dev)
        return b

    def set_grads(self, gs):
        for b, a in zip(self.buf["g"], gs):
            b[:a.size] = torch.from_numpy(a).view(torch.int32).to(self.dev)

    def step(self, step, found_inf=None, n_tensors=None):
        c, n = self.c, self.n if n_tensors is None else n_tensors
        arr = ctypes.c_void_p * n
        ptrs = [arr(*[self.buf[k][i % self.n].data_ptr() for i in range(n)]) for k in ("p", "g", "m", "v")]
        numel = (ctypes.c_size_t * n)(*[self.c.p[i % self.n].size for i in range(n)])
        cfg = self.lib.AdamCfg(c.lr, c.b1, c.b2, c.eps, c.max_norm, step)
        nbytes = self.L.fsn_clip_adam_workspace_bytes(n, numel)
        ws = self.lib.workspace(nbytes, self.dev).fill_(0xFF)
        scale = None if c.scale is None else torch.tensor([c.scale], device=self.dev)
        found = None if found_inf is None else torch.tensor([found_inf], device=self.dev)
        rc = self.L.fsn_clip_adam_step(n, *ptrs, numel, ctypes.byref(cfg), self.lib.dev_ptr(self.norm.view(torch.float32)),
                                       self.lib.dev_ptr(scale, allow_none=True), self.lib.dev_ptr(found, allow_none=True),
                                       ctypes.c_void_p(self.skipped.data_ptr()), ws.data_ptr(), ws.numel(), self.lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc

    def read(self):
        out = {}
        for k in ("p", "g", "m", "v"):
            out[k] = []
            for b, a in zip(self.buf[k], self.c.p):
                _untouched(b, a.size, k)
                out[k].append(b[:a.size].view(torch.float32).cpu().numpy())
        _untouched(self.norm, 1, "total norm")
        out["norm"] = self.norm[:1].view(torch.float32).cpu().numpy()
        return out


def check_adam(stats, ref, got, cpu, names=("norm", "g", "m", "v", "p")):
    for name in names:
        st = stats.setdefault(name, Stat(name, scalar=name == "norm"))
        if name == "norm":
            st.add(got["norm"], *ref["norm"], cpu["norm"])
        else:
            for g, (r, S), c in zip(got[name], ref[name], cpu[name]):
                st.add(g, r, S, c)


def run_adam_row(fsn, row):
    stats = {}
    norm_only = row.kw.get("norm_only", False)
    for draw in range(row.draws):
        c = AdamCase(row.sizes, row.step, row.betas, row.clip, row.gval, row.scale, seed=draw)
        ref = adam_oracle(c)
        a = AdamDevice(fsn, c)
        fsn._lib.check(a.step(row.step, row.found_inf))
        got = a.read()
        assert int(a.skipped[0]) == 0
        if norm_only:
            gs = [torch.from_numpy(g) * (1.0 / (c.scale or 1.0)) for g in c.g]
            cpu = dict(norm=np.array([float(torch.linalg.vector_norm(torch.cat(gs)))]))
            check_adam(stats, ref, got, cpu, names=("norm",))
            continue
        b = AdamDevice(fsn, c)
        fsn._lib.check(b.step(row.step, row.found_inf))
        again = b.read()
        for k in ("p", "g", "m", "v"):
            for x, y in zip(again[k], got[k]):
                check_exact(f"{k}: two calls in a row", x, y)
        for k in ("p", "g", "m", "v"):
            assert all(np.isfinite(t).all() for t in got[k]), f"{k}: not finite"
        check_adam(stats, ref, got, adam_torch(c, torch.float32))
    finish(row.id, stats)


def run_adam_skip_row(fsn, row):
    """A bad gradient (or found_inf) at call `step`: everything bit-identical, skipped[0] + 1; the next good call at
    `step + 1` uses the step count minus the skips, i.e. `step`."""
    c = AdamCase(row.sizes, row.step, row.betas, "below")
    good = [g.copy() for g in c.g]
    bad = [g.copy() for g in c.g]
    if row.bad == "inf":
        bad[3][4095] = np.inf
    elif row.bad == "nan":
        bad[5][4096 * 3 + 4] = np.nan
    a = AdamDevice(fsn, c)
    a.set_grads(bad)
    before = {k: [b.clone() for b in a.buf[k]] for k in ("p", "g", "m", "v")}
    fsn._lib.check(a.step(row.step, 1.0 if row.bad == "found_inf" else None))
    for k in before:
        for x, y in zip(a.buf[k], before[k]):
            assert torch.equal(x, y), f"{k}: a skipped update changed it"
    assert int(a.skipped[0]) == 1, "skipped[0] did not go up by one"
    a.set_grads(good)
    fsn._lib.check(a.step(row.step + 1, 0.0 if row.bad == "found_inf" else None))
    assert int(a.skipped[0]) == 1
    stats = {}
    check_adam(stats, adam_oracle(c, step=row.step), a.read(), adam_torch(c, torch.float32, step=row.step))
    finish(row.id, stats)


def run_adam_refused(fsn):
    c = AdamCase((5, 7), 1, (0.9, 0.999))
    a = AdamDevice(fsn, c)
    before = {k: [b.clone() for b in a.buf[k]] for k in ("p", "g", "m", "v")}
    assert a.step(1, n_tensors=33) != 0 and b"32" in a.L.fsn_last_error()
    for k in before:
        for x, y in zip(a.buf[k], before[k]):
            assert torch.equal(x, y), f"{k}: a refused call changed it"
    fsn._lib.check(a.step(1, n_tensors=2))


RUNNERS = {"glue": run_glue_row, "target": run_target_row, "pieces": run_pieces_row, "mse": run_mse_row, "scale": run_scale_row,
           "adam": run_adam_row, "adam-skip": run_adam_skip_row}


@pytest.mark.parametrize("row", TABLE, ids=[r.id for r in TABLE])
def test_train_glue_sweep(fsn, row):
    t0 = time.time()
    if row.kind == "pieces-refused":
        run_pieces_refused(fsn)
    elif row.kind == "adam-refused":
        run_adam_refused(fsn)
    else:
        RUNNERS[row.kind](fsn, row)
    print(f"[glue-sweep] {row.id}: {time.time() - t0:.1f} s")


def test_cumulative_padded_rows_beyond_the_workspace_are_refused(fsn):
    run_glue_refusals(fsn)
