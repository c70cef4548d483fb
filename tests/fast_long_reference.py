"""The reference and the checkers of tests/test_gpu_fast_long.py; importable without a device (tests/test_fast_long_cpu.py
runs all of it on the CPU).

Fast FullSubNet under the offline norm divides by two utterance means (model.py:170,187), so a recording in segments takes
three passes (include/fsn_hip.h, fsn_fast_segment_*).  Here they are as three stateful functions over the fields of the
device's state blob, built from fast_stream_reference's pieces (`_block`, `units_of`, the state of `new_state`):

  `stats`     mag [U, 1, F, k] -> mel [U, M, k]; every frame's band sum joins st["acc_mel"] (fp64), in frame order
  `encoder`   mel / den_mel through the encoder pair from the carried (h, c) -> enc [U, M, k]; the unit windows are
              down-sampled as a running block sum carried in st["stat_partial"], and every low-rate frame of row b that
              completes at a step < total[b] - the closing short block at step total[b] - 1 included - joins st["acc_unit"]
  `decoder`   the whole blocks that complete in the segment, divided by den_unit, through the bottleneck, the held output,
              the decoder pair -> crm [U, 2, F, k] (every step; step s is the mask of frame s - look_ahead)
  `run`       the three passes over a split of the steps

total[b] = T_b + look_ahead is row b's own step count; a row's mag is zero from its frame T_b on.  tests/test_fast_long_cpu.py
holds `run` in fp64 to fast_stream_reference.forward(..., "offline", np.float64) of each row alone, to 1e-12, in every
segmentation.  `WRONG` lists deliberately wrong stand-ins, each of which the checkers below must catch.

The checkers: `check_divisors` holds the two divisors to one ulp of float32(float32(mean) + 1e-5) with the mean formed in
fp64 numpy from the mel and enc planes themselves (the closing block included, through the oracle's real_time_downsampling);
`check_mask` holds a mask to the project's standing 1e-4 absolute against the fp64 reference, over each row's own frames."""
import collections

import numpy as np

import fast_stream_reference as R
from oracle import model_family_oracle as MF

M, F = R.M, R.F
EPS = 1e-5        # offline_laplace_norm's epsilon (base_model.py:204-218)
MASK_TOL = 1e-4   # the standing bound of a compressed mask against the fp64 oracle (tests/test_gpu_parity.py)
WRONG = ("closing-block-left-out", "count-of-the-longest-row", "look-ahead-not-counted", "block-sum-not-carried",
         "steps-past-the-end-counted")

Result = collections.namedtuple("Result", "crm mel enc den_mel den_unit state")


def low_frames(total, shrink):
    """real_time_downsampling's frame count of `total` frames: 1 + ceil((total - 1) / shrink)."""
    return 1 + -(-(total - 1) // shrink)


def new_state(U, cfg):
    st = R.new_state(U, cfg)
    st.update(acc_mel=np.zeros(U), acc_unit=np.zeros(U), stat_partial=np.zeros((U, M, R.unit_width(cfg)), dtype=np.float32))
    return st


def ragged_mag(totals, cfg, seed):
    """[U, 1, F, max(totals)]: row b random over its T_b = totals[b] - look_ahead frames, zero from there on."""
    mag = R.make_mag(len(totals), max(totals), seed)
    for b, n in enumerate(totals):
        mag[b, :, :, n - cfg.la:] = 0.0
    return mag


def divisors(st, total, cfg, dtype, wrong=None):
    """(den_mel, den_unit) [U] from the accumulators: float(sum / count) + 1e-5 in `dtype`."""
    tot = np.asarray(total, dtype=np.int64)
    if wrong == "count-of-the-longest-row":
        tot = np.full_like(tot, tot.max())
    if wrong == "look-ahead-not-counted":
        tot = tot - cfg.la
    ts = np.array([1 + (t - 1) // cfg.shrink if wrong == "closing-block-left-out" else low_frames(t, cfg.shrink) for t in tot])
    den_mel = (st["acc_mel"] / (M * tot.astype(np.float64))).astype(dtype) + dtype(EPS)
    den_unit = (st["acc_unit"] / (float(M * R.unit_width(cfg)) * ts)).astype(dtype) + dtype(EPS)
    return den_mel.astype(dtype), den_unit.astype(dtype)


def stats(st, mag, params, dtype):
    x = np.asarray(mag, dtype=dtype)
    fb = np.asarray(params["mel_scale.fb"], dtype=dtype)
    mel = (x.transpose(0, 1, 3, 2) @ fb).transpose(0, 1, 3, 2).astype(dtype)[:, 0]  # [U, M, k]
    for t in range(mel.shape[-1]):
        st["acc_mel"] = st["acc_mel"] + mel[..., t].sum(axis=1, dtype=np.float64)
    return mel


def encoder(st, mel, t0, total, params, cfg, dtype, act, wrong=None):
    den, _ = divisors(st, total, cfg, dtype, wrong)
    enc_in = (mel / den[:, None, None]).astype(dtype)
    e = R._block(enc_in, params, "encoder.0", 1, False, False, dtype, act, st["enc0"])
    e = R._block(e, params, "encoder.1", 1, True, True, dtype, act, st["enc1"])  # [U, M, k]
    units = R.units_of(mel[:, None], e[:, None], cfg)  # [U, M, W, k]
    s = cfg.shrink
    partial = np.asarray(st["stat_partial"], dtype=dtype)
    if wrong == "block-sum-not-carried":
        partial = np.zeros_like(partial)
    for t in range(mel.shape[-1]):
        T = t0 + t
        partial = (partial + units[..., t]).astype(dtype)  # frame order
        for b, end in enumerate(total):
            if T >= end and wrong != "steps-past-the-end-counted":
                continue
            whole = T % s == 0
            closing = not whole and T == end - 1 and wrong != "closing-block-left-out"
            if whole or closing:
                n = T % s if closing else (s if T > 0 else 1)
                v = (partial[b] / dtype(n)).astype(dtype) if n > 1 else partial[b]
                st["acc_unit"][b] += v.sum(dtype=np.float64)
        if T % s == 0:
            partial = np.zeros_like(partial)
    st["stat_partial"] = partial
    return e


def decoder(st, mel, enc, t0, total, params, cfg, dtype, act, wrong=None):
    _, den = divisors(st, total, cfg, dtype, wrong)
    U, _, k = mel.shape
    s, W = cfg.shrink, R.unit_width(cfg)
    units = R.units_of(mel[:, None], enc[:, None], cfg)
    partial, held = np.asarray(st["partial"], dtype=dtype), np.asarray(st["held"], dtype=dtype)
    low = []
    for t in range(k):
        T = t0 + t
        partial = (partial + units[..., t]).astype(dtype)
        if T % s:
            continue
        v = (partial / dtype(s)).astype(dtype) if T > 0 and s > 1 else partial
        low.append((v / den[:, None, None]).astype(dtype))
        partial = np.zeros_like(partial)
    slow = None
    if low:
        bn_in = np.stack(low, axis=-1).reshape(U * M, W, len(low))
        slow = R._block(bn_in, params, "bottleneck", cfg.bn_layers, True, True, dtype, act, st["bn"]).reshape(U, M, len(low))
    j0 = -(-t0 // s)  # the first low-rate frame that completes in this call
    gain = np.empty((U, M, k), dtype=dtype)
    for t in range(k):
        j = (t0 + t) // s - j0
        gain[..., t] = slow[..., j] if j >= 0 else held
    if low:
        held = slow[..., -1]
    d = R._block(np.concatenate([enc, gain], axis=1), params, "decoder_lstm.0", 1, False, False, dtype, act, st["dec0"])
    d = R._block(d, params, "decoder_lstm.1", 1, True, False, dtype, act, st["dec1"])
    st["partial"], st["held"] = partial, np.ascontiguousarray(held)
    return np.ascontiguousarray(d.reshape(U, 2, F, k))


def run(mag, total, params, cfg, split, dtype=np.float64, act="torch", wrong=None):
    """The three passes over the calls `split` (sum(split) = max(total) steps) on mag [U, 1, F, max(total)] -> Result: the mask
    of every step [U, 2, F, steps], the mel and enc planes [U, M, steps], the divisors, the final state."""
    assert wrong is None or wrong in WRONG
    assert sum(split) == max(total) == mag.shape[-1]
    st = new_state(mag.shape[0], cfg)
    edges = np.concatenate([[0], np.cumsum(split)])
    calls = list(zip(edges[:-1], edges[1:]))
    mel = np.concatenate([stats(st, mag[..., a:b], params, dtype) for a, b in calls], axis=-1)
    enc = np.concatenate([encoder(st, mel[..., a:b], a, total, params, cfg, dtype, act, wrong) for a, b in calls], axis=-1)
    den_mel, den_unit = divisors(st, total, cfg, dtype, wrong)
    crm = np.concatenate([decoder(st, mel[..., a:b], enc[..., a:b], a, total, params, cfg, dtype, act, wrong) for a, b in calls], axis=-1)
    return Result(crm, mel, enc, den_mel, den_unit, st)


def rows_alone(mag, total, params, cfg, dtype=np.float64):
    """fast_stream_reference.forward under the offline norm of each row alone over its own T_b frames: a list of [2, F, T_b]."""
    return [R.forward(mag[b:b + 1, :, :, :n - cfg.la], params, cfg, "offline", dtype)[0] for b, n in enumerate(total)]


# ---- the checkers -----------------------------------------------------------------------------------------------------------

def expected_divisors(mel, enc, total, cfg):
    """mel, enc [U, M, steps] (fp32 planes) -> per row (float32(float32(mean of mel) + 1e-5), the same of the down-sampled unit
    tensor), the means in fp64 numpy over the row's own total[b] steps, the closing block included."""
    out = []
    for b, n in enumerate(total):
        m, e = (np.asarray(a, dtype=np.float32)[b:b + 1, None, :, :n] for a in (mel, enc))
        low = MF.real_time_downsampling(R.units_of(m, e, cfg), cfg.shrink)  # [1, M, W, Ts_b]: fp32 block means, as formed on the device
        assert low.shape[-1] == low_frames(n, cfg.shrink)
        out.append(tuple(np.float32(np.float32(x.astype(np.float64).mean()) + np.float32(EPS)) for x in (m, low)))
    return out


def check_divisors(den_mel, den_unit, mel, enc, total, cfg, log=print):
    """Each divisor within one ulp of expected_divisors.  Returns the worst distance in ulps."""
    worst = 0.0
    for b, (want_mel, want_unit) in enumerate(expected_divisors(mel, enc, total, cfg)):
        for name, got, want in (("mel", den_mel[b], want_mel), ("unit", den_unit[b], want_unit)):
            ulps = abs(np.float64(got) - np.float64(want)) / np.float64(np.spacing(want))
            log(f"[flong] row {b} ({total[b]} steps) den_{name}: {float(got)!r} vs {float(want)!r}, {ulps:.2f} ulp")
            assert ulps <= 1.0, f"row {b} ({total[b]} steps) den_{name}: {float(got)!r}, expected {float(want)!r} ({ulps:.1f} ulp apart)"
            worst = max(worst, float(ulps))
    return worst


def check_mask(crm, want, total, cfg, log=print, what="mask"):
    """crm [U, 2, F, >= T_b]: the masks of the frames (not the steps); want: rows_alone's list.  Each row over its own frames
    within MASK_TOL of the fp64 reference, and finite.  Returns the worst error."""
    worst = 0.0
    for b, n in enumerate(total):
        g = np.asarray(crm[b][..., :n - cfg.la], dtype=np.float64)
        assert g.shape == want[b].shape, f"{what} row {b}: shape {g.shape}, expected {want[b].shape}"
        assert np.isfinite(g).all(), f"{what} row {b}: not finite"
        d = float(np.abs(g - want[b]).max())
        log(f"[flong] {what} row {b} ({n} steps): max |d cIRM| vs the fp64 reference {d:.3e}")
        assert d <= MASK_TOL, f"{what} row {b} ({n} steps): {d:.3e} from the fp64 reference, allowed {MASK_TOL:g}"
        worst = max(worst, d)
    return worst
