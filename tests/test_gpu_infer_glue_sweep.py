"""The glue between the model blocks on the inference path - the seven kernels of fast_glue_kernels.hip behind their eleven
fsn_fast_* entries, the section input, front, the two transposes and the mask product of section_kernels.hip, and the three
cIRM entries of elementwise_kernels.hip - held to fp64 references over a sweep of shapes.  Needs an MI355X:
python -m pytest tests/test_gpu_infer_glue_sweep.py -m gpu -s

The whole-model tests see these kernels at F = 257 / M = 64 and at the shipped section configurations, with mask
tolerances.  TABLE below has one row per code path, named after the path it is there for: 32 x 32 and 64-frame tile edges,
ragged `frames` with rows of one frame and clamped values, a short last down-sampling block of every length, windows that
mirror at both ends, padded sizes a whole tile beyond the data, the chunked grid.y launch and R < 8 rows per workgroup of
mask_apply_kernel, the workgroup-stride loop of improved_front_kernel, the window multiplicities of fast_ds_kernel and
section_mean_kernel.  The C entries are called through fullsubnet_amd._lib directly, so that padded sizes, leading dimensions
and `frames` are the test's to choose.  The checkers (Stat, check_exact, the sentinel / guard helpers) are those of
tests/test_gpu_train_glue_sweep.py.

References (numpy, fp64, the unfolded tensors formed explicitly)
* fast glue: oracle/model_family_oracle.py (real_time_downsampling, real_time_upsampling) and oracle/fullsubnet_oracle.py
  (freq_unfold, offline_laplace_norm) in the order of fast_fullsubnet_forward: cat(unfold(mel), unfold(enc)) is down-sampled
  and then averaged as a real tensor, which makes the kernel's multiplicity-weighted sum a tested claim.  A ragged row b is
  the same sequence on a batch of one with clamp(frames[b], 1, T0) + look_ahead frames; what the kernels promise beyond that
  length is exact zero.
* section input: banded_unfold twice, concatenated, the mean over the whole section per utterance, x / (mean + eps); a unit
  shard takes the whole section's mean.
* cIRM: fp64 transcriptions of mask.py's three functions with the constants as the fp32 values the code holds.
* everything else is an index map plus at most one correctly rounded operation.

Assertions
* exact (bits): spec_rows, decoder_input, mask_out, front (mode 1: numpy's fp32 sqrt), both transposes, mask_apply (one fp32
  product), ds of a one-frame block, and every promised zero (rows >= B, columns >= F / W / 2 num_mels, spec_rows frames
  >= T_b, ds low-rate frames >= Ts_b, mask_out frames >= T_b, units rows in [B M, Np), section rows >= B (u_hi - u_lo), bins no
  mask section covers).  Outputs are allocated GUARD elements larger than declared and pre-filled with the NaN sentinel, which
  must survive outside; input padding that must not be read (enc columns >= M, o columns >= 2F / 2 center, slow between its
  strides, rows >= B, ragged frames >= T_b of mag) holds the sentinel too.  A -0.0 that meets decoder_input's relu is compared by
  value.
* hard, per element: |hip - ref64| <= k 2^-24 S, S = the sum of the absolute values of the terms, k = the fp32 roundings on the
  kernel's own longest path:
    den, sden   k = 2      (float)(fp64 sum / count) + eps                                      S = den
    norm        k = 3      den, one division                                                    S = |x / den|
    section     k = 3      the same
    ds          k = n + 1  a block of n > 1 frames: n - 1 adds, fl(1 / n), the product;            S = mean |x| of the block
                           n = 1: a copy, asserted by bits (k = 0)
    bden        k = kb + 2 kb = the utterance's worst block; the cast and + eps                 S = mean |ds| unfolded + eps
    units       k = kb + 3 one division more                                                    S = mean |x| of the block / den
  compress / decompress / build: PRINTED ONLY (k = 6 / 5 / 8 with expf / logf at 1 ULP) - the install documents no error bound
  for them; the sharp rule governs, plus the exact bits of the kernel's own saturation values (decompress at |m| >= 9.9f equals
  its value at +-9.9f; compress at m <= -100 equals its value at -100, and is exactly 10 where expf underflows) and NaN -> NaN.
* sharp: the rms of err / S is at most SHARP = 4 times that of the CPU fp32 evaluation (the oracle at np.float32; torch on the
  CPU for the cIRM algebra) against the same fp64 result, from POOL_ELEMS pooled elements on (rows repeat their draws until
  then; the three dens, one element per utterance, are held to it by the rows *-den-pool).
* every row: the workspace is exactly the queried size and pre-filled with 0xFF; two calls give the same bits; the rectangular
  entry and the _ragged entry with frames[b] = T0 everywhere give the same bits; rows with several padded sizes give the same
  bits in the valid region for all of them.

Found by writing this module: see DESIGN.md section 3 (the +-inf inputs of the cIRM entries, the workspace of
fsn_fast_norm_rows at T = 1).

With -s every row prints, per output, `hard` and the two rms figures of the sharp rule in units of 2^-24.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O
from oracle import model_family_oracle as MF

import test_gpu_train_glue_sweep as G
from test_gpu_train_glue_sweep import (GUARD, POOL_ELEMS, SENTINEL, SHARP, U, Row, Stat, bits, check_exact, finish, ru,  # noqa: F401
                                       fsn, _all_zero_bits, _sentinel, _untouched)

pytestmark = pytest.mark.gpu

SENT = np.array([SENTINEL], np.int32).view(np.float32)[0]
K = dict(den=2, norm=3, sden=2, section=3, ds=1, bden=1, units=1, compress=6, decompress=5, build=8)  # ds, bden, units: per element
NO_HARD = ("compress", "decompress", "build")
SCALAR = ("den", "sden", "bden")
C99, C01, CEPS = float(np.float32(9.9)), float(np.float32(0.1)), float(np.float32(1.1920929e-07))
F99 = np.float32(9.9)


def stat(stats, name):
    return stats.setdefault(name, Stat(name, scalar=name in SCALAR, k=K[name], no_hard=name in NO_HARD))


def embed(a, shape):
    """a in the leading corner of a sentinel-filled fp32 array of `shape`: padding that must not be read."""
    out = np.full(shape, SENT, np.float32)
    out[tuple(slice(0, s) for s in a.shape)] = a
    return out


def row_frames(frames, b, T0):
    return T0 if frames is None else min(max(int(frames[b]), 1), T0)


def ragged_frames(T0, B):
    """T0, one frame, 0 and -3 (both clamp to 1), T0 + 5 (clamps to T0), a value just past a tile edge."""
    return ([T0, 1, 0, -3, T0 + 5, min(T0, 33), max(T0 - 1, 1), min(T0, 2)] * B)[:B]


def low_rate(T, s):
    return 1 + (T - 1 + s - 1) // s


def rng_of(row, draw=0):
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(row.path)) + 7919 * draw)


# ---- the table ----------------------------------------------------------------------------------------------------------

def _table():
    rows = []
    edge = (1, 31, 32, 33)
    # spec_rows: tile edges of both axes, a tile of look-ahead frames only (la 33), a tile of zero columns only (Fp = F + 40)
    for i, (F, T0) in enumerate([(F, T0) for F in (1, 31, 32, 33, 70) for T0 in (1, 31, 32, 33, 65)]):
        rows.append(Row("spec", f"spec-F{F}-T{T0}-la{(0, 2, 33)[i % 3]}", B=6, F=F, T0=T0, la=(0, 2, 33)[i % 3]))
    # norm_rows: T C around the 256-thread pass; ragged rows of one frame and of T - la frames
    for T, C in ((1, 1), (255, 1), (4, 64), (257, 1), (769, 1), (5, 65), (3, 64)):
        rows.append(Row("norm", f"norm-T{T}-C{C}", T=T, C=C, B=3, la=0, frames=None, signal="plain"))
    for la in (0, 2):
        rows.append(Row("norm", f"norm-ragged-la{la}", T=9 + la, C=7, B=6, la=la, frames=ragged_frames(9, 6), signal="plain"))
    for sig in ("lead-zeros", "1e4", "1e-4"):
        rows.append(Row("norm", f"norm-{sig}", T=12, C=9, B=3, la=2, frames=[10, 4, 1], signal=sig))
    rows.append(Row("norm", "norm-den-pool", T=3, C=2, B=64, la=0, frames=None, signal="plain", draws=4))
    # bottleneck input: a last block of every length, shrink > T - 1
    bn = dict(B=3, M=5, nm=1, ne=0, la=0, frames=None, ld_extra=0, np_mode=0, wp_mode=0)
    BN = lambda path, **kw: Row("bneck", path, **dict(bn, **kw))
    for s in (1, 2, 3, 4, 7):
        for T in sorted({2, 3, s, s + 1, s + 2, 2 * s + 1, 2 * s + 2} - {1}):
            rows.append(BN(f"bneck-s{s}-T{T}", shrink=s, T=T, ld_extra=7 * (T % 2), np_mode=T % 3, wp_mode=(T + s) % 3))
    for M in (2, 3, 64, 65, 300):  # 300: Ts M and M (windows) cross the 256-thread stride
        rows.append(BN(f"bneck-M{M}", shrink=2, T=6, M=M, nm=min(2, M - 1), ne=1, B=2, np_mode=2, wp_mode=1))
    for nm, ne in ((0, 0), (1, 0), (5, 0), (2, 1), (0, 3)):
        rows.append(BN(f"bneck-nb{nm}-{ne}", shrink=2, T=5, M=7, nm=nm, ne=ne, ld_extra=7, np_mode=1, wp_mode=2))
    rows.append(BN("bneck-nb-M-1-both-mirrors-on-one-band", shrink=3, T=5, M=4, nm=3, ne=3, wp_mode=1))
    rows.append(BN("bneck-B1-zero-rows", shrink=2, T=5, M=3, B=1, np_mode=2))
    for s in (2, 3, 4):  # ragged: rows of one frame, every residue of (T_b + la - 1) % shrink
        rows.append(BN(f"bneck-ragged-s{s}", shrink=s, T=11, la=2, B=8, M=6, nm=2, ne=1, frames=[9, 1, 0, 14, 2, 3, 4, 5], ld_extra=7,
                       np_mode=2, wp_mode=2))
    rows.append(BN("bneck-den-pool", shrink=3, T=5, M=3, B=64, draws=4))
    rows.append(Row("bneck-refused", "bneck-refused"))
    # decoder input
    for s in (1, 2, 3, 5):
        for T in sorted({1, max(s - 1, 1), s, s + 1, 3 * s + 1}):
            rows.append(Row("dec", f"dec-s{s}-T{T}", shrink=s, T=T, B=2, Bp=2 + T % 2, M=31 + T % 3, ldr=1 + 2 * (T % 2), ldf_extra=5 * (s % 2),
                            ld_extra=3 * (T % 2)))
    rows.append(Row("dec", "dec-shrink-above-T", shrink=9, T=4, B=3, Bp=5, M=64, ldr=3, ldf_extra=2, ld_extra=1))
    rows.append(Row("dec", "dec-2MBp-below-256", shrink=2, T=3, B=1, Bp=1, M=127, ldr=1, ldf_extra=0, ld_extra=0))
    rows.append(Row("dec-refused", "dec-T65536-refused"))
    # mask out
    for i, (F, T0) in enumerate([(F, T0) for F in (1, 16, 17, 40) for T0 in (1, 31, 32, 33, 65)]):
        rows.append(Row("mask", f"mask-F{F}-T{T0}-la{(0, 2, 40)[i % 3]}", B=6, F=F, T0=T0, la=(0, 2, 40)[i % 3], ld_extra=6 * (i % 2)))
    # section input
    sec = dict(B=3, T=5, eps=1.1920929e-07, shard="whole", np_mode=0, ldo_mode=0)
    SE = lambda path, **kw: Row("section", path, **dict(sec, **kw))
    rows.append(SE("section-low-mirror", F=33, lower=0, upper=16, sc=2, sn=3, fc=2, fn=1))
    rows.append(SE("section-high-mirror", F=33, lower=17, upper=33, sc=8, sn=5, fc=8, fn=0, ldo_mode=1))
    rows.append(SE("section-middle", F=70, lower=20, upper=50, sc=1, sn=4, fc=1, fn=2, ldo_mode=2, np_mode=1))
    rows.append(SE("section-F3-one-window-mirrors-at-both-ends", F=3, lower=0, upper=2, sc=2, sn=1, fc=2, fn=1))
    rows.append(SE("section-F2", F=2, lower=0, upper=2, sc=1, sn=1, fc=1, fn=0, B=1, np_mode=2))
    rows.append(SE("section-unitsW-above-256", F=70, lower=0, upper=70, sc=1, sn=3, fc=1, fn=1, eps=1e-5))   # 70 x 10
    rows.append(SE("section-W240-ldo240", F=70, lower=0, upper=64, sc=8, sn=60, fc=8, fn=52, B=1))
    for T in (1, 63, 64, 65, 130):
        rows.append(SE(f"section-T{T}", F=33, lower=8, upper=24, sc=2, sn=2, fc=2, fn=3, T=T, B=1 + T % 2 * 2, np_mode=T % 3, ldo_mode=T % 3))
    for shard in ("first", "last", "tail"):
        rows.append(SE(f"section-shard-{shard}", F=33, lower=0, upper=20, sc=2, sn=3, fc=2, fn=1, shard=shard, np_mode=2, ldo_mode=1))
    rows.append(SE("section-den-pool", F=5, lower=1, upper=5, sc=2, sn=1, fc=2, fn=0, B=64, T=3, draws=4))
    rows.append(Row("section-refused", "section-refused"))
    # front, the transposes
    rows.append(Row("front", "front-F2", B=2, F=2, T=7))
    rows.append(Row("front", "front-special-values", B=1, F=3, T=300))
    rows.append(Row("front", "front-stride-loop", B=1, F=2, T=4096 * 256 + 5))
    for i, (F, T) in enumerate([(F, T) for F in (1, 31, 32, 33, 65) for T in (1, 31, 32, 33, 65)]):
        rows.append(Row("transpose", f"transpose-F{F}-T{T}", B=3, F=F, T=T, Np=3 + i % 3, Ip=F + (0, 5, 40)[i % 3], ld=F + 3 * (i % 2),
                        O=max(F - i % 2, 1)))
    # mask apply: rows per workgroup R = 8 .. 1, tiles that straddle Np, uncovered bins, an empty section
    for i, ld in enumerate((2, 16, 60, 61, 96, 240, 241, 480)):
        c = 1 if ld == 2 else (1, 2, 8)[i % 3]
        for T in ((1, 31, 32, 33, 70)[i % 5], (32, 33, 70, 1, 31)[i % 5]):
            rows.append(Row("apply", f"apply-ld{ld}-c{c}-T{T}", B=3, T=T, secs=[(1, 3, c, ld, i % 3), (2, 0, c, ld, 0), (1, 5, c, ld, (i + 1) % 3)]))
    rows.append(Row("apply", "apply-one-section", B=2, T=9, secs=[(0, 7, 2, 5, 1)]))
    rows.append(Row("apply", "apply-eight-sections", B=2, T=9, secs=[(i % 2, 1 + i, (1, 2, 8)[i % 3], 16 + i, i % 3) for i in range(8)]))
    rows.append(Row("apply", "apply-second-grid-y-launch", B=1, T=1, secs=[(0, 8 * 65535 + 9, 1, 2, 0)]))
    rows.append(Row("apply-refused", "apply-ld481-refused"))
    # cIRM
    for kind in ("compress", "decompress", "build"):
        for n in (1, 255, 256, 257, 2048 * 256 + 3):
            rows.append(Row(kind, f"{kind}-n{n}", n=n))
    return rows


TABLE = _table()


def pooled(row, stats, draw):
    """Draws go on until the row's own count is done and every multi-element output has pooled POOL_ELEMS elements."""
    return draw >= getattr(row, "draws", 1) and all(s.scalar or s.n >= POOL_ELEMS for s in stats.values())


# ---- fast glue: references ----------------------------------------------------------------------------------------------

def make_spec_ops(row):
    return rng_of(row).standard_normal((row.B, row.F, row.T0)).astype(np.float32)


def spec_reference(row, mag, frames, Bp, Fp):
    out = np.zeros((row.T0 + row.la, Bp, Fp), np.float32)
    for b in range(row.B):
        Tb = row_frames(frames, b, row.T0)
        out[:Tb, b, :row.F] = mag[b, :, :Tb].T
    return out


def make_norm_ops(row, draw):
    x = (np.abs(rng_of(row, draw).standard_normal((row.T, row.B, row.C))) + 0.05).astype(np.float32)
    if row.signal == "lead-zeros":
        x[:3, 0] = 0.0
    elif row.signal in ("1e4", "1e-4"):
        x *= np.float32(float(row.signal))
    return x


def norm_reference(row, x, frames, dtype=np.float64, variant=""):
    """x [T][B][C].  Returns out [T][B][C], den [B], valid [T][B] (the frames of a row's own length)."""
    T, B, C = x.shape
    out, den, valid = np.zeros((T, B, C), dtype), np.zeros(B, dtype), np.zeros((T, B), bool)
    for b in range(B):
        Tr = row_frames(frames, b, T - row.la) + (0 if variant == "no_lookahead" else row.la)
        xb = x[:Tr, b].astype(dtype)[None]
        if variant == "padded_count":
            d = dtype(xb.sum(dtype=np.float64) / (T * C)) + dtype(1e-5)
            out[:Tr, b] = (xb / d)[0]
        else:
            d = xb.mean(dtype=np.float64).astype(dtype) + dtype(1e-5)
            out[:Tr, b] = O.offline_laplace_norm(xb, dtype)[0]
        den[b], valid[:Tr, b] = d, True
    return out, den, valid


def norm_want(row, x, frames):
    ref, den, valid = norm_reference(row, x, frames)
    cpu, cden, _ = norm_reference(row, x, frames, np.float32)
    return dict(norm=(ref[valid], np.abs(ref[valid]), cpu[valid], None), den=(den, np.abs(den), cden, None)), valid


def make_bneck_ops(row, draw):
    g = rng_of(row, draw)
    mel = (np.abs(g.standard_normal((row.B, row.M, row.T))) + 0.05).astype(np.float32)
    enc = np.maximum(g.standard_normal((row.B, row.M, row.T)), 0).astype(np.float32)  # a ReLU output: about half exact zeros
    return mel, enc


def _unfold(x, n, edge_repeat=False):
    """x [1, 1, M, T] -> [1, M, 2n + 1, T]"""
    M = x.shape[2]
    if not edge_repeat:
        return O.freq_unfold(x, n).reshape(1, M, 2 * n + 1, x.shape[3])
    j = np.arange(M)[:, None] + np.arange(2 * n + 1)[None, :] - n
    j = np.where(j < 0, -j - 1, j)  # wrong: "symmetric" padding
    j = np.where(j >= M, 2 * M - 1 - j, j)
    return x[:, 0][:, j, :]


def _down(x, s, variant=""):
    if variant == "short_block_by_shrink":
        rest = x[..., 1:]
        cols = [x[..., 0:1]] + [rest[..., i:i + s].sum(axis=-1, keepdims=True) / x.dtype.type(s) for i in range(0, rest.shape[-1], s)]
        return np.concatenate(cols, axis=-1)
    if variant == "frame0_in_block":
        out = MF.real_time_downsampling(x, s)
        out[..., 1] = x[..., 0:1 + s].mean(axis=-1, dtype=x.dtype)
        return out
    return MF.real_time_downsampling(x, s)


def bneck_reference(row, mel, enc, frames, dtype=np.float64, variant=""):
    """mel, enc [B][M][T] -> units [Ts][B M][W], ds [2][Ts][B][M], den [B], with S and k of each (fp64 only) and Ts_b."""
    B, M, T, s, nm, ne = row.B, row.M, row.T, row.shrink, row.nm, row.ne
    Ts, W = low_rate(T, s), 2 * nm + 1 + 2 * ne + 1
    r = dict(units=np.zeros((Ts, B * M, W), dtype), ds=np.zeros((2, Ts, B, M), dtype), den=np.zeros(B, dtype), Tsb=[],
             S_units=np.zeros((Ts, B * M, W)), S_ds=np.zeros((2, Ts, B, M)), S_den=np.zeros(B), k_ds=np.zeros((2, Ts, B, M)),
             k_den=np.zeros(B), k_units=np.zeros((Ts, B * M, W)))
    for b in range(B):
        Tr = row_frames(frames, b, T - row.la) + row.la
        Tsb = low_rate(Tr, s)
        src = [a[b:b + 1, None, :, :Tr].astype(dtype) for a in (mel, enc)]
        er = variant == "edge_repeat"
        dsu = _down(np.concatenate([_unfold(src[0], nm, er), _unfold(src[1], ne, er)], axis=2), s, variant)   # [1, M, W, Tsb]
        if variant == "gathered_mean":
            mu = _down(np.concatenate(src, axis=2), s).mean(dtype=np.float64)
        else:
            mu = dsu.mean(dtype=np.float64)
        d = np.asarray(mu).astype(dtype) + dtype(1e-5)
        out = (dsu / d).astype(dtype) if variant else O.offline_laplace_norm(dsu, dtype)
        rs = slice(b * M, (b + 1) * M)
        r["units"][:Tsb, rs] = out[0].transpose(2, 0, 1)
        r["den"][b] = d
        r["Tsb"].append(Tsb)
        n = np.array([1] + [min(s, Tr - 1 - i * s) for i in range(Tsb - 1)])
        kb = np.where(n > 1, n + 1, 0)
        for i in range(2):
            r["ds"][i, :Tsb, b] = _down(src[i][0, 0], s, variant).T
            r["S_ds"][i, :Tsb, b] = MF.real_time_downsampling(np.abs(src[i][0, 0]).astype(np.float64), s).T
            r["k_ds"][i, :Tsb, b] = kb[:, None]
        Su = MF.real_time_downsampling(np.concatenate([_unfold(np.abs(src[0]).astype(np.float64), nm),
                                                       _unfold(np.abs(src[1]).astype(np.float64), ne)], axis=2), s)
        r["S_den"][b] = Su.mean() + 1e-5
        r["k_den"][b] = kb.max() + 2
        r["S_units"][:Tsb, rs] = (Su / float(d))[0].transpose(2, 0, 1)
        r["k_units"][:Tsb, rs] = kb.max() + 3
    return r


def bneck_want(row, mel, enc, frames):
    r, c = bneck_reference(row, mel, enc, frames), bneck_reference(row, mel, enc, frames, np.float32)
    live = np.zeros(r["units"].shape[:2], bool)
    for b, Tsb in enumerate(r["Tsb"]):
        live[:Tsb, b * row.M:(b + 1) * row.M] = True
    dl = np.broadcast_to(live.reshape(live.shape[0], row.B, row.M)[None], r["ds"].shape)
    want = dict(units=(r["units"][live], r["S_units"][live], c["units"][live], r["k_units"][live]),
                ds=(r["ds"][dl], r["S_ds"][dl], c["ds"][dl], r["k_ds"][dl]), bden=(r["den"], r["S_den"], c["den"], r["k_den"]))
    return want, live, dl, r


def bneck_sizes(row):
    W = 2 * row.nm + 1 + 2 * row.ne + 1
    N = row.B * row.M
    return W, (N, ru(N, 16), N + 37)[row.np_mode], (W, W + 3, ru(W, 16))[row.wp_mode], row.M + row.ld_extra


def judge(stats, want, outs):
    """want: name -> (ref64, S, cpu32, k or None); outs: name -> the same elements as the kernel gave them."""
    for name, (ref, S, cpu, k) in want.items():
        if name in outs:
            stat(stats, name).add(outs[name], ref, S, cpu, k=k)


# ---- decoder input, mask out ----------------------------------------------------------------------------------------------

def make_dec_ops(row):
    g = rng_of(row)
    Ts = (row.T - 1) // row.shrink + 1  # the low-rate frames the kernel reads
    enc = g.standard_normal((row.T, row.B, row.M)).astype(np.float32)
    slow = g.standard_normal((Ts, row.B * row.M)).astype(np.float32)
    slow[0, 0] = -0.0
    return enc, slow


def dec_reference(row, enc, slow, relu, variant=""):
    T, B, M, s = row.T, row.B, row.M, row.shrink
    out = np.zeros((T, row.Bp, 2 * M), np.float32)
    out[:, :B, :M] = enc
    up = slow.reshape(-1, B, M).transpose(1, 2, 0)                          # [B, M, Ts]
    if variant == "t_plus_1":
        idx = np.minimum((np.arange(T) + 1) // s, up.shape[-1] - 1)
        held = up[..., idx]
    else:
        held = MF.real_time_upsampling(up, s, T)
    held = held.transpose(2, 0, 1)
    out[:, :B, M:] = np.maximum(held, np.float32(0)) + np.float32(0) if relu else held
    return out


def make_mask_ops(row):
    return rng_of(row).standard_normal((row.T0 + row.la, row.B, 2 * row.F)).astype(np.float32)


def mask_reference(row, o, frames, variant=""):
    out = np.zeros((row.B, 2 * row.F, row.T0), np.float32)
    for b in range(row.B):
        Tb = row_frames(frames, b, row.T0)
        la = 0 if variant == "shift_wrong" else row.la
        out[b, :, :Tb] = o[la:la + Tb, b].T
    return out


# ---- section input ----------------------------------------------------------------------------------------------------------

def section_dims(row):
    units = (row.upper - row.lower) // row.sc
    W = row.sc + 2 * row.sn + row.fc + 2 * row.fn
    lo, hi = dict(whole=(0, units), first=(0, 1), last=(units - 1, units), tail=(1, units))[row.shard]
    n = row.B * (hi - lo)
    return units, W, lo, hi, (n, ru(n, 16), n + 5)[row.np_mode], (W, min(W + 1, 240), min(ru(W, 16), 240))[row.ldo_mode]


def make_section_ops(row, draw):
    g = rng_of(row, draw)
    return ((np.abs(g.standard_normal((row.B, row.F, row.T))) + 0.05).astype(np.float32),
            np.maximum(g.standard_normal((row.B, row.F, row.T)), -0.25).astype(np.float32))


def section_reference(row, noisy, fb, dtype=np.float64, variant=""):
    """-> rows [T][B (u_hi - u_lo)][W], den [B]"""
    units, W, lo, hi, _, _ = section_dims(row)
    x, y = noisy.astype(dtype)[:, None], fb.astype(dtype)[:, None]
    a = MF.banded_unfold(x, row.lower, row.upper, row.sc, row.sn)
    if variant == "fb_noisy_neighbors":  # the window starts at lower - sn instead of lower - fn
        b_ = MF.banded_unfold(y, row.lower, row.upper, row.fc, row.sn)[:, :, :, :row.fc + 2 * row.fn]
    else:
        b_ = MF.banded_unfold(y, row.lower, row.upper, row.fc, row.fn)
    sec = np.concatenate([a, b_], axis=3)[:, :, 0]                                        # [B, units, W, T]
    mu = (sec[:, lo:hi] if variant == "shard_mean" else sec).mean(axis=(1, 2, 3), dtype=np.float64)
    den = mu.astype(dtype) + dtype(np.float32(row.eps))
    out = (sec / den[:, None, None, None]).astype(dtype)[:, lo:hi]
    return out.transpose(3, 0, 1, 2).reshape(row.T, row.B * (hi - lo), W), den


def section_want(row, noisy, fb):
    ref, den = section_reference(row, noisy, fb)
    cpu, cden = section_reference(row, noisy, fb, np.float32)
    return dict(section=(ref, np.abs(ref), cpu, None), sden=(den, np.abs(den), cden, None))


# ---- front, transposes, mask apply -------------------------------------------------------------------------------------------

FRONT_SPECIALS = np.array([0.0, 1e-40, 1.4e-45, 3.4028235e38, 1.0, 4.0, 9.0, 16.0, 1.0e10, 2.0, 1.1754944e-38, 0.25], np.float32)


def make_front_ops(row):
    mag = np.abs(rng_of(row).standard_normal((row.B, row.F, row.T))).astype(np.float32)
    if row.T >= FRONT_SPECIALS.size:
        mag[0, 0, :FRONT_SPECIALS.size] = FRONT_SPECIALS
    return mag


def front_reference(mag, mode):
    x = np.ascontiguousarray(mag[:, :-1])
    return np.sqrt(x) if mode else x


def apply_layout(row):
    """secs: (gap before, units, center, ld, Np mode) -> the sections' (lower, units, center, ld, Np, R) and F."""
    out, f = [], 0
    for gap, units, c, ld, npm in row.secs:
        ld = max(ld, 2 * c)
        R = min(8, max(1, 480 // ld))
        n = row.B * units
        out.append(dict(lower=f + gap, units=units, center=c, ld=ld, Np=(n, n + 1, n + R)[npm] if units else max(n, 1), R=R))
        f += gap + units * c
    return out, f + 1  # one uncovered bin at the end


def make_apply_ops(row):
    g = rng_of(row)
    secs, F = apply_layout(row)
    real = g.standard_normal((row.B, F, row.T)).astype(np.float32)
    imag = g.standard_normal((row.B, F, row.T)).astype(np.float32)
    os_ = [g.standard_normal((row.T, row.B * s["units"], 2 * s["center"])).astype(np.float32) for s in secs]
    return secs, F, real, imag, os_


def apply_reference(row, secs, F, real, imag, os_, variant=""):
    er = np.full((row.B, F, row.T), SENT if variant == "uncovered_unwritten" else 0, np.float32)
    ei = er.copy()
    for s, o in zip(secs, os_):
        if not s["units"]:
            continue
        c, u = s["center"], s["units"]
        m = o.reshape(row.T, row.B, u, 2, c).transpose(3, 1, 2, 4, 0).reshape(2, row.B, u * c, row.T)
        if variant == "swap_planes":
            m = m[::-1]
        sl = slice(s["lower"], s["lower"] + u * c)
        er[:, sl], ei[:, sl] = m[0] * real[:, sl], m[1] * imag[:, sl]   # one fp32 product
    return er, ei


# ---- cIRM -------------------------------------------------------------------------------------------------------------------

def compress64(m):
    """mask.py:32-44 at fp64, C = float32(0.1)."""
    with np.errstate(invalid="ignore", over="ignore"):
        m = -100.0 * (m <= -100) + m * (m > -100)
        e = np.exp(-C01 * m)
        return 10.0 * (1 - e) / (1 + e)


def decompress64(m, lim=C99):
    """mask.py:47-64 at fp64, limit = float32(9.9)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        m = lim * (m >= lim) - lim * (m <= -lim) + m * (np.abs(m) < lim)
        return -10.0 * np.log((10.0 - m) / (10.0 + m))


def build64(nr, ni, cr, ci):
    """mask.py:7-29 at fp64, eps = float32(1.1920929e-07): [n] x 4 -> [n][2]."""
    den = nr * nr + ni * ni + CEPS
    return compress64(np.stack(((nr * cr + ni * ci) / den, (nr * ci - ni * cr) / den), axis=-1))


def t_compress(m):
    m = -100 * (m <= -100) + m * (m > -100)
    e = torch.exp(-0.1 * m)
    return 10 * (1 - e) / (1 + e)


def t_decompress(m, limit=9.9):
    m = limit * (m >= limit) - limit * (m <= -limit) + m * (m.abs() < limit)
    return -10 * torch.log((10 - m) / (10 + m))


def _ulp(v, up):
    return np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf), dtype=np.float32)


DECOMPRESS_SPECIALS = np.array([F99, -F99, _ulp(F99, False), _ulp(F99, True), -_ulp(F99, False), -_ulp(F99, True), 0.0, -0.0, 1e-30,
                                np.inf, -np.inf, np.nan, 10.0, -10.0, 11.0], np.float32)
COMPRESS_SPECIALS = np.array([-100.0, _ulp(-100.0, True), _ulp(-100.0, False), 0.0, -0.0, -np.inf, np.inf, np.nan, 2000.0, 1e4, -1e4,
                              3e38], np.float32)


def make_cirm_ops(row, draw):
    g, n = rng_of(row, draw), row.n
    if row.kind == "decompress":
        x = g.uniform(-12, 12, n).astype(np.float32)
        sp = DECOMPRESS_SPECIALS
    elif row.kind == "compress":
        x = (np.exp(g.uniform(np.log(1e-4), np.log(1e4), n)) * g.choice([-1.0, 1.0], n)).astype(np.float32)
        sp = COMPRESS_SPECIALS
    else:
        scale = np.array([1e-3, 1.0, 1e3])[g.integers(0, 3, (2, n))]
        nr, ni, cr, ci = (g.standard_normal(n) * scale[i // 2] for i in range(4))
        if n >= 32:
            nr[0], ni[0] = 0.0, 0.0                        # den = eps
            nr[1], ni[1] = 1e-6, -1e-6                     # |noisy|^2 far below eps
            nr[2], ni[2], cr[2], ci[2] = 1e-3, 0.0, -1.0, 1.0  # raw mask -893 + 893i: across -100
            nr[3], ni[3], cr[3], ci[3] = 0.01, 0.0, -1.0, 0.0  # raw mask about -99.9: just inside
        return tuple(a.astype(np.float32) for a in (nr, ni, cr, ci))
    if n >= 32:
        x[:sp.size] = sp
    return (x,)


def cirm_want(row, ops, variant=""):
    """-> (ref64, S, cpu32), keep (the elements the statistics cover: finite inputs)."""
    a = [o.astype(np.float64) for o in ops]
    t = [torch.from_numpy(o) for o in ops]
    with np.errstate(all="ignore"):
        if row.kind == "compress":
            ref, cpu = compress64(a[0]), t_compress(t[0]).numpy()
            e = np.exp(-C01 * np.maximum(a[0], -100.0))
            S = 20 * e / (1 + e) ** 2 * (C01 * np.abs(np.maximum(a[0], -100.0)) + 1) + np.abs(ref)
            keep = np.isfinite(a[0])
        elif row.kind == "decompress":
            ref, cpu = decompress64(a[0], 10.0 if variant == "clamp10" else C99), t_decompress(t[0]).numpy()
            S = 10.0 + np.abs(ref)
            keep = np.isfinite(a[0])
        else:
            nr, ni, cr, ci = a
            ref, cpu = build64(nr, ni, cr, ci), G.torch_target(*t).numpy()
            den = nr ** 2 + ni ** 2 + CEPS
            Sm = np.stack(((np.abs(nr * cr) + np.abs(ni * ci)) / den, (np.abs(nr * ci) + np.abs(ni * cr)) / den), axis=-1)
            m = np.stack(((nr * cr + ni * ci) / den, (nr * ci - ni * cr) / den), axis=-1)
            e = np.exp(-C01 * np.maximum(m, -100.0))
            S = 20 * e / (1 + e) ** 2 * (C01 * np.minimum(Sm, 1e30) + 1) + np.abs(ref)
            keep = np.ones(ref.shape, bool)
    return (ref, S, cpu), keep


def check_cirm_specials(kind, x, got):
    """The kernel's own saturation values, bit for bit, and NaN -> NaN."""
    nan = np.isnan(x)
    assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any(), f"{kind}: NaN in must be NaN out, and nothing else"
    if kind == "decompress":
        for sign in (1.0, -1.0):
            anchor = np.flatnonzero(x == np.float32(sign) * F99)
            sat = (x >= F99) if sign > 0 else (x <= -F99)
            if anchor.size:
                check_exact(f"decompress beyond {sign * 9.9}", got[sat], np.full(int(sat.sum()), got[anchor[0]], np.float32))
    else:
        anchor = np.flatnonzero(x == np.float32(-100.0))
        if anchor.size:
            sat = x <= -100.0
            check_exact("compress at and below -100", got[sat], np.full(int(sat.sum()), got[anchor[0]], np.float32))
        under = x >= 2000.0  # expf(-200) is below the smallest subnormal
        check_exact("compress where expf underflows", got[under], np.full(int(under.sum()), 10.0, np.float32))


# ---- the device side ----------------------------------------------------------------------------------------------------------

DEV = "cuda:0"


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _frames(fr):
    return torch.tensor(fr, dtype=torch.int32, device=DEV)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _f32(buf, n):
    return buf.view(torch.float32)[:n]


def _ws(lib, nbytes):
    return lib.workspace(nbytes, torch.device(DEV)).fill_(0xFF)


def _twice(call):
    a, b = call(), call()
    for k in a:
        check_exact(f"{k}: two calls in a row", b[k], a[k])
    return a


def run_spec_row(fsn, row):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    mag = make_spec_ops(row)
    T = row.T0 + row.la
    ragged = ragged_frames(row.T0, row.B)
    for Bp, Fp in ((row.B, row.F), (row.B + 3, row.F + 5), (row.B, row.F + 40)):
        def call(frames, full=False):
            m = mag.copy()
            if frames is not None and not full:
                for b in range(row.B):
                    m[b, :, row_frames(frames, b, row.T0):] = SENT  # never read
            md, buf = _up(m), _sentinel(T * Bp * Fp, DEV)
            if frames is None:
                lib.check(L.fsn_fast_spec_rows(lib.dev_ptr(md), row.B, row.F, row.T0, row.la, lib.dev_ptr(_f32(buf, T * Bp * Fp)), Bp, Fp, st))
            else:
                fr = _frames(frames)
                lib.check(L.fsn_fast_spec_rows_ragged(lib.dev_ptr(md), _vp(fr), row.B, row.F, row.T0, row.la,
                                                      lib.dev_ptr(_f32(buf, T * Bp * Fp)), Bp, Fp, st))
            _untouched(buf, T * Bp * Fp, "rows")
            return dict(rows=_f32(buf, T * Bp * Fp).view(T, Bp, Fp).cpu().numpy())
        plain = _twice(lambda: call(None))
        check_exact("rows", plain["rows"], spec_reference(row, mag, None, Bp, Fp))
        check_exact("rows: ragged entry, every row T0 frames", call([row.T0] * row.B, full=True)["rows"], plain["rows"])
        check_exact("rows: ragged", _twice(lambda: call(ragged))["rows"], spec_reference(row, mag, ragged, Bp, Fp))


def device_norm(fsn, row, x, frames, Bp):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    T, B, C = x.shape
    xd = _up(embed(x, (T, Bp, C)))
    nbytes = L.fsn_fast_glue_workspace_bytes(T, B, C, T) if T >= 2 else ru(4 * B, 256)  # T = 1: the size fsn_hip.h states
    assert nbytes >= ru(4 * B, 256)
    ws, buf = _ws(lib, nbytes), _sentinel(T * Bp * C, DEV)
    if frames is None:
        lib.check(L.fsn_fast_norm_rows(lib.dev_ptr(xd), T, B, Bp, C, lib.dev_ptr(_f32(buf, T * Bp * C)), ws.data_ptr(), ws.numel(), st))
    else:
        fr = _frames(frames)
        lib.check(L.fsn_fast_norm_rows_ragged(lib.dev_ptr(xd), _vp(fr), row.la, T, B, Bp, C, lib.dev_ptr(_f32(buf, T * Bp * C)),
                                              ws.data_ptr(), ws.numel(), st))
    _untouched(buf, T * Bp * C, "norm")
    v = buf[:T * Bp * C].view(T, Bp, C)
    _all_zero_bits(v[:, B:], "norm rows >= B")
    return dict(norm=v.view(torch.float32)[:, :B].cpu().numpy(), den=ws[:4 * B].view(torch.float32).cpu().numpy())


def run_norm_row(fsn, row):
    stats, draw = {}, -1
    while not pooled(row, stats, draw := draw + 1):
        x = make_norm_ops(row, draw)
        for frames in ((None,) if row.frames is None else (None, row.frames)) if row.la == 0 else (row.frames,):
            want, valid = norm_want(row, x, frames)
            got = device_norm(fsn, row, x, frames, row.B + 2)
            if draw == 0:
                again = device_norm(fsn, row, x, frames, row.B + 2)
                other = device_norm(fsn, row, x, frames, row.B)
                for k in got:
                    check_exact(f"{k}: two calls in a row", again[k], got[k])
                    check_exact(f"{k}: Bp = B", other[k], got[k])
                if frames is None:
                    same = device_norm(fsn, row, x, [row.T] * row.B, row.B + 2)
                    for k in got:
                        check_exact(f"{k}: ragged entry, every row T frames", same[k], got[k])
            assert np.isfinite(got["norm"]).all()
            judge(stats, want, dict(norm=got["norm"][valid], den=got["den"]))
    finish(row.id, stats)


def device_bneck(fsn, row, mel, enc, frames):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    B, M, T, s = row.B, row.M, row.T, row.shrink
    W, Np, Wp, ld_enc = bneck_sizes(row)
    Bp, Ts = B + 1, L.fsn_fast_low_rate_frames(T, s)
    assert Ts == low_rate(T, s)
    md = _up(embed(mel.transpose(2, 0, 1), (T, Bp, M)))
    ed = _up(embed(enc.transpose(2, 0, 1), (T, Bp, ld_enc)))
    nbytes = L.fsn_fast_glue_workspace_bytes(T, B, M, s)
    assert nbytes == ru(2 * Ts * B * M * 4, 256) + ru(B * 4, 256)
    ws, buf = _ws(lib, nbytes), _sentinel(Ts * Np * Wp, DEV)
    out = lib.dev_ptr(_f32(buf, Ts * Np * Wp))
    if frames is None:
        lib.check(L.fsn_fast_bottleneck_input(lib.dev_ptr(md), lib.dev_ptr(ed), ld_enc, T, B, Bp, M, row.nm, row.ne, s, out, Np, Wp,
                                              ws.data_ptr(), ws.numel(), st))
    else:
        fr = _frames(frames)
        lib.check(L.fsn_fast_bottleneck_input_ragged(lib.dev_ptr(md), lib.dev_ptr(ed), ld_enc, _vp(fr), row.la, T, B, Bp, M, row.nm, row.ne,
                                                     s, out, Np, Wp, ws.data_ptr(), ws.numel(), st))
    _untouched(buf, Ts * Np * Wp, "units")
    v = buf[:Ts * Np * Wp].view(Ts, Np, Wp)
    _all_zero_bits(v[:, B * M:], "units rows in [B M, Np)")
    _all_zero_bits(v[:, :, W:], "units columns >= W")
    n_ds = 2 * Ts * B * M
    return dict(units=v.view(torch.float32)[:, :B * M, :W].cpu().numpy(),
                ds=ws[:4 * n_ds].view(torch.float32).view(2, Ts, B, M).cpu().numpy(),
                bden=ws[ru(4 * n_ds, 256):ru(4 * n_ds, 256) + 4 * B].view(torch.float32).cpu().numpy())


def judge_bneck(stats, row, mel, enc, frames, got):
    want, live, dl, r = bneck_want(row, mel, enc, frames)
    assert not bits(got["ds"][~dl]).any(), "ds: low-rate frames >= Ts_b are not exactly +0"
    one = dl & (r["k_ds"] == 0)
    check_exact("ds of a one-frame block", got["ds"][one], r["ds"][one].astype(np.float32))
    assert np.isfinite(got["units"]).all()
    judge(stats, want, dict(units=got["units"][live], ds=got["ds"][dl], bden=got["bden"]))


def run_bneck_row(fsn, row):
    stats, draw = {}, -1
    while not pooled(row, stats, draw := draw + 1):
        mel, enc = make_bneck_ops(row, draw)
        if row.la == 0:
            got = device_bneck(fsn, row, mel, enc, None)
            if draw == 0:
                for what, other in (("two calls in a row", device_bneck(fsn, row, mel, enc, None)),
                                    ("ragged entry, every row T frames", device_bneck(fsn, row, mel, enc, [row.T] * row.B))):
                    for k in got:
                        check_exact(f"{k}: {what}", other[k], got[k])
            judge_bneck(stats, row, mel, enc, None, got)
        if row.frames is not None:
            got = device_bneck(fsn, row, mel, enc, row.frames)
            if draw == 0:
                again = device_bneck(fsn, row, mel, enc, row.frames)
                for k in got:
                    check_exact(f"{k}: two calls in a row (ragged)", again[k], got[k])
            judge_bneck(stats, row, mel, enc, row.frames, got)
    finish(row.id, stats)


BNECK_REFUSALS = [  # (T, M, nm, ne, Wp - W, Np - B M, workspace short by)
    (1, 4, 1, 0, 0, 0, 0), (4, 1, 0, 0, 0, 0, 0), (4, 4097, 1, 0, 0, 0, 0), (4, 4, 4, 0, 0, 0, 0), (4, 4, 0, 4, 0, 0, 0),
    (4, 4, 1, 0, -1, 0, 0), (4, 4, 1, 0, 0, -1, 0), (4, 4, 1, 0, 0, 0, 1)]


def bneck_refusal_call(L, lib_mod, ptr, ws_ptr, T, M, nm, ne, dW, dN, short, st, B=2):
    W = 2 * nm + 1 + 2 * ne + 1
    nbytes = L.fsn_fast_glue_workspace_bytes(max(T, 2), B, M, 2)
    return L.fsn_fast_bottleneck_input(ptr, ptr, M, T, B, B, M, nm, ne, 2, ptr, B * M + dN, W + dW, ws_ptr, nbytes - short, st)


def run_bneck_refused(fsn):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    buf = _sentinel(1 << 16, DEV)
    ws = _ws(lib, 1 << 18)
    for case in BNECK_REFUSALS:
        rc = bneck_refusal_call(L, lib, lib.dev_ptr(buf.view(torch.float32)), ws.data_ptr(), *case, st)
        assert rc != 0 and L.fsn_last_error(), case
    torch.cuda.synchronize()
    _untouched(buf, 0, "a refused call")
    assert bool((ws == 0xFF).all()), "a refused call wrote to its workspace"


def run_dec_row(fsn, row):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    enc, slow = make_dec_ops(row)
    T, B, Bp, M = row.T, row.B, row.Bp, row.M
    ld_enc, ldr = M + row.ld_extra, row.ldr
    ldf = B * M * ldr + row.ldf_extra
    sl = np.full((slow.shape[0], ldf), SENT, np.float32)
    sl[:, :B * M * ldr:ldr] = slow
    ed, sd = _up(embed(enc, (T, Bp, ld_enc))), _up(sl)
    for relu in (0, 1):
        def call():
            buf = _sentinel(T * Bp * 2 * M, DEV)
            lib.check(L.fsn_fast_decoder_input(lib.dev_ptr(ed), ld_enc, lib.dev_ptr(sd), ldf, ldr, relu, T, B, Bp, M, row.shrink,
                                               lib.dev_ptr(_f32(buf, T * Bp * 2 * M)), st))
            _untouched(buf, T * Bp * 2 * M, "decoder input")
            return dict(out=_f32(buf, T * Bp * 2 * M).view(T, Bp, 2 * M).cpu().numpy())
        got = _twice(call)["out"]
        check_dec(row, enc, slow, relu, got)


def check_dec(row, enc, slow, relu, got):
    want = dec_reference(row, enc, slow, relu)
    if relu:  # fmaxf(-0.0, 0) may return either zero: by value
        held = np.broadcast_to((slow == 0).reshape(-1, row.B, row.M)[np.minimum(np.arange(row.T) // row.shrink, slow.shape[0] - 1)],
                               (row.T, row.B, row.M))
        part = got[:, :row.B, row.M:]
        assert (part[held] == 0).all()
        got = got.copy()
        got[:, :row.B, row.M:][held] = 0.0
    check_exact(f"decoder input relu {relu}", got, want)


def run_dec_refused(fsn):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    buf = _sentinel(64, DEV)
    p = lib.dev_ptr(buf.view(torch.float32))
    assert L.fsn_fast_decoder_input(p, 1, p, 1, 1, 0, 65536, 1, 1, 1, 1, p, st) != 0 and L.fsn_last_error()
    torch.cuda.synchronize()
    _untouched(buf, 0, "a refused call")


def run_mask_row(fsn, row):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    o = make_mask_ops(row)
    T, B, F = row.T0 + row.la, row.B, row.F
    ld, n = 2 * F + row.ld_extra, B * 2 * F * row.T0
    ragged = ragged_frames(row.T0, B)
    for Bp in (B, B + 2):
        od = _up(embed(o, (T, Bp, ld)))

        def call(frames):
            buf = _sentinel(n, DEV)
            if frames is None:
                lib.check(L.fsn_fast_mask_out(lib.dev_ptr(od), ld, T, B, Bp, F, row.la, lib.dev_ptr(_f32(buf, n)), st))
            else:
                fr = _frames(frames)
                lib.check(L.fsn_fast_mask_out_ragged(lib.dev_ptr(od), ld, _vp(fr), T, B, Bp, F, row.la, lib.dev_ptr(_f32(buf, n)), st))
            _untouched(buf, n, "mask")
            return dict(mask=_f32(buf, n).view(B, 2 * F, row.T0).cpu().numpy())
        plain = _twice(lambda: call(None))
        check_exact("mask", plain["mask"], mask_reference(row, o, None))
        check_exact("mask: ragged entry, every row T0 frames", call([row.T0] * B)["mask"], plain["mask"])
        check_exact("mask: ragged", _twice(lambda: call(ragged))["mask"], mask_reference(row, o, ragged))


def device_section(fsn, row, noisy, fb, Np, ldo):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    units, W, lo, hi, _, _ = section_dims(row)
    B, F, T = row.B, row.F, row.T
    nbytes = L.fsn_improved_section_input_workspace_bytes(B, F)
    assert nbytes == ru((4 * B * F + B + 16) * 4, 256)
    ws, buf = _ws(lib, nbytes), _sentinel(T * Np * ldo, DEV)
    nd, fd = _up(noisy), _up(fb)
    lib.check(L.fsn_improved_section_input(lib.dev_ptr(nd), lib.dev_ptr(fd), B, F, T, row.lower, row.upper, row.sc, row.sn, row.fc, row.fn,
                                           lo, hi, row.eps, lib.dev_ptr(_f32(buf, T * Np * ldo)), Np, ldo, ws.data_ptr(), ws.numel(), st))
    _untouched(buf, T * Np * ldo, "section")
    v = buf[:T * Np * ldo].view(T, Np, ldo)
    n = B * (hi - lo)
    _all_zero_bits(v[:, n:], "section rows >= B (u_hi - u_lo)")
    _all_zero_bits(v[:, :, W:], "section columns >= W")
    return dict(section=v.view(torch.float32)[:, :n, :W].cpu().numpy(),
                sden=ws[16 * B * F:16 * B * F + 4 * B].view(torch.float32).cpu().numpy())


def run_section_row(fsn, row):
    units, W, lo, hi, Np, ldo = section_dims(row)
    n = row.B * (hi - lo)
    stats, draw = {}, -1
    while not pooled(row, stats, draw := draw + 1):
        noisy, fb = make_section_ops(row, draw)
        got = device_section(fsn, row, noisy, fb, Np, ldo)
        if draw == 0:
            for what, other in (("two calls in a row", device_section(fsn, row, noisy, fb, Np, ldo)),
                                ("Np + 5, ldo = W", device_section(fsn, row, noisy, fb, Np + 5, W)),
                                ("Np = rows, ldo rounded to 16", device_section(fsn, row, noisy, fb, n, min(ru(W, 16), 240)))):
                for k in got:
                    check_exact(f"{k}: {what}", other[k], got[k])
        assert np.isfinite(got["section"]).all()
        judge(stats, section_want(row, noisy, fb), got)
    finish(row.id, stats)


SECTION_REFUSALS = [  # (F, lower, upper, sc, sn, fc, fn, ldo, Np - rows, workspace short by)
    (70, 0, 64, 8, 60, 8, 52, 241, 0, 0), (33, 0, 16, 2, 3, 2, 1, 11, 0, 0), (33, 0, 16, 2, 3, 2, 1, 12, -1, 0), (33, 0, 16, 2, 3, 2, 1, 12, 0, 1),
    (33, 0, 15, 2, 3, 2, 1, 12, 0, 0), (4, 0, 4, 2, 3, 2, 1, 12, 0, 0)]


def section_refusal_call(L, ptr, ws_ptr, F, lower, upper, sc, sn, fc, fn, ldo, dN, short, st, B=2):
    units = max((upper - lower) // sc, 1)
    return L.fsn_improved_section_input(ptr, ptr, B, F, 3, lower, upper, sc, sn, fc, fn, 0, units, 1e-5, ptr, B * units + dN, ldo, ws_ptr,
                                        L.fsn_improved_section_input_workspace_bytes(B, F) - short, st)


def run_section_refused(fsn):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    buf, ws = _sentinel(1 << 16, DEV), _ws(lib, 1 << 16)
    for case in SECTION_REFUSALS:
        assert section_refusal_call(L, lib.dev_ptr(buf.view(torch.float32)), ws.data_ptr(), *case, st) != 0 and L.fsn_last_error(), case
    torch.cuda.synchronize()
    _untouched(buf, 0, "a refused call")
    assert bool((ws == 0xFF).all()), "a refused call wrote to its workspace"


def run_front_row(fsn, row):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    mag = make_front_ops(row)
    md, n = _up(mag), row.B * (row.F - 1) * row.T
    for mode in (0, 1):
        def call():
            buf = _sentinel(n, DEV)
            lib.check(L.fsn_improved_front(lib.dev_ptr(md), row.B, row.F, row.T, mode, lib.dev_ptr(_f32(buf, n)), st))
            _untouched(buf, n, "front")
            return dict(front=_f32(buf, n).view(row.B, row.F - 1, row.T).cpu().numpy())
        check_exact(f"front mode {mode}", _twice(call)["front"], front_reference(mag, mode))


def run_transpose_row(fsn, row):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    B, F, T, Np, Ip = row.B, row.F, row.T, row.Np, row.Ip
    x = rng_of(row).standard_normal((B, F, T)).astype(np.float32)
    xd = _up(x)

    def to_rows():
        buf = _sentinel(T * Np * Ip, DEV)
        lib.check(L.fsn_bft_to_rows(lib.dev_ptr(xd), B, F, T, lib.dev_ptr(_f32(buf, T * Np * Ip)), Np, Ip, st))
        _untouched(buf, T * Np * Ip, "rows")
        return dict(h=_f32(buf, T * Np * Ip).view(T, Np, Ip).cpu().numpy())
    want = np.zeros((T, Np, Ip), np.float32)
    want[:, :B, :F] = x.transpose(2, 0, 1)
    check_exact("bft_to_rows", _twice(to_rows)["h"], want)
    ld, Oc = row.ld, row.O
    o = embed(x.transpose(2, 0, 1), (T, Np, ld))  # columns >= F and rows >= B: never read when O <= F
    od = _up(o)

    def to_bft():
        buf = _sentinel(B * Oc * T, DEV)
        lib.check(L.fsn_rows_to_bft(lib.dev_ptr(od), T, Np, ld, B, Oc, lib.dev_ptr(_f32(buf, B * Oc * T)), st))
        _untouched(buf, B * Oc * T, "bft")
        return dict(y=_f32(buf, B * Oc * T).view(B, Oc, T).cpu().numpy())
    check_exact("rows_to_bft", _twice(to_bft)["y"], np.ascontiguousarray(x[:, :Oc]))


def run_apply_row(fsn, row):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    secs, F, real, imag, os_ = make_apply_ops(row)
    B, T = row.B, row.T
    rd, idv = _up(real), _up(imag)
    ods = [_up(embed(o, (T, s["Np"], s["ld"]))) for s, o in zip(secs, os_)]
    arr = (lib.MaskSection * len(secs))(*[lib.MaskSection(od.data_ptr(), s["Np"], s["ld"], s["lower"], s["units"], s["center"])
                                          for s, od in zip(secs, ods)])

    def call():
        er, ei = _sentinel(B * F * T, DEV), _sentinel(B * F * T, DEV)
        lib.check(L.fsn_improved_mask_apply(len(secs), ctypes.cast(arr, ctypes.c_void_p), lib.dev_ptr(rd), lib.dev_ptr(idv), B, F, T,
                                            lib.dev_ptr(_f32(er, B * F * T)), lib.dev_ptr(_f32(ei, B * F * T)), st))
        _untouched(er, B * F * T, "er")
        _untouched(ei, B * F * T, "ei")
        return dict(er=_f32(er, B * F * T).view(B, F, T).cpu().numpy(), ei=_f32(ei, B * F * T).view(B, F, T).cpu().numpy())
    got = _twice(call)
    wr, wi = apply_reference(row, secs, F, real, imag, os_)
    check_exact("er", got["er"], wr)
    check_exact("ei", got["ei"], wi)


def run_apply_refused(fsn):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    buf = _sentinel(4096, DEV)
    p = lib.dev_ptr(buf.view(torch.float32))
    arr = (lib.MaskSection * 1)(lib.MaskSection(buf.data_ptr(), 1, 481, 0, 1, 1))
    assert L.fsn_improved_mask_apply(1, ctypes.cast(arr, ctypes.c_void_p), p, p, 1, 2, 1, p, p, st) != 0 and L.fsn_last_error()
    torch.cuda.synchronize()
    _untouched(buf, 0, "a refused call")


def run_cirm_row(fsn, row):
    lib, L, st = fsn._lib, fsn._lib.lib(), fsn._lib.stream_ptr(torch.device(DEV))
    stats = {}
    n_out = row.n * (2 if row.kind == "build" else 1)
    draw = -1
    while stat(stats, row.kind).n < POOL_ELEMS:
        ops = make_cirm_ops(row, draw := draw + 1)
        dv = [_up(o) for o in ops]

        def call():
            buf = _sentinel(n_out, DEV)
            fn = getattr(L, f"fsn_{row.kind}_cirm")
            lib.check(fn(*(lib.dev_ptr(d) for d in dv), lib.dev_ptr(_f32(buf, n_out)), row.n, st))
            _untouched(buf, n_out, row.kind)
            return {row.kind: _f32(buf, n_out).cpu().numpy()}
        got = (_twice(call) if draw == 0 else call())[row.kind]
        (ref, S, cpu), keep = cirm_want(row, ops)
        if row.kind == "build":
            got = got.reshape(row.n, 2)
            assert np.isfinite(got).all() and float(np.abs(got).max()) <= 10.0
            if row.n >= 32:
                assert not bits(got[0]).any(), "the 0 + 0i noisy bin does not give exactly +0"
        else:
            check_cirm_specials(row.kind, ops[0], got)
        stat(stats, row.kind).add(got[keep], ref[keep], S[keep], cpu[keep])
    finish(row.id, stats)


RUNNERS = {"spec": run_spec_row, "norm": run_norm_row, "bneck": run_bneck_row, "dec": run_dec_row, "mask": run_mask_row,
           "section": run_section_row, "front": run_front_row, "transpose": run_transpose_row, "apply": run_apply_row,
           "compress": run_cirm_row, "decompress": run_cirm_row, "build": run_cirm_row}
REFUSALS = {"bneck-refused": run_bneck_refused, "dec-refused": run_dec_refused, "section-refused": run_section_refused,
            "apply-refused": run_apply_refused}


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """A row that leaves the device in an error state ends the module: nothing more is launched on a faulted device."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, no further rows are run: {e}", returncode=3)


@pytest.mark.parametrize("row", TABLE, ids=[r.id for r in TABLE])
def test_infer_glue_sweep(fsn, row):
    t0 = time.time()
    if row.kind in REFUSALS:
        REFUSALS[row.kind](fsn)
    else:
        RUNNERS[row.kind](fsn, row)
    torch.cuda.synchronize()
    print(f"[infer-glue-sweep] {row.id}: {time.time() - t0:.1f} s")
