"""numpy reference of the dereverberation targets (fsn_rir_shorten / fsn_mix_pairs_target): the window of the reference's
audio_zen/acoustics/rvb.py:reverberation_time_shortening restated in fp64 (held to the reference's own outputs,
tests/golden/rts_windows.npz, bit for bit), the target row as tests/mix_reference.py:snr_mix's scalar chain applied to the
fp64 convolution of the clean row with the fp32 shortened taps, and the checkers of tests/test_gpu_mix_target.py - which
tests/test_mix_target_cpu.py feeds wrong stand-ins.  numpy only."""
import json
import math
import os

import numpy as np

import mix_reference as R

TAP_REL = 2.0 ** -22   # a tap of the device against the golden: one fp32 ulp of the window (an fp64 10^x that differs from
TAP_ABS = 2.0 ** -126  # numpy's in the last place can move its fp32 rounding by one) + half an ulp of the product, rounded
#                        up to 2 ulp = 2^-22 relative; the floor covers a product flushed in the denormal range


def first_argmax_abs(h):
    """np.argmax(np.abs(h)) spelled out: the FIRST index of the largest magnitude."""
    best, at = -1.0, 0
    for i, v in enumerate(np.abs(np.asarray(h, np.float64))):
        if v > best:
            best, at = float(v), i
    return at


def rts_window(h, q, after_max, mode=1):
    """(shortened h fp32, window fp32, idx) of a response: window 1 before N1 = idx + after_max; from N1 on 10^(-q (n - N1))
    in fp64 rounded to fp32 (mode 1) or 0 (mode 2); mode 0 leaves the response alone.  The product is one fp32 product."""
    h = np.asarray(h, np.float32)
    idx = first_argmax_abs(h)
    win = np.ones(len(h), np.float64)
    n1 = idx + int(after_max)
    if mode == 1:
        win[n1:] = np.power(10.0, -float(q) * np.arange(max(len(h) - n1, 0), dtype=np.float64))
    elif mode == 2:
        win[n1:] = 0.0
    else:
        assert mode == 0
    win = win.astype(np.float32)
    out = h * win
    assert out.dtype == np.float32
    return out, win, idx


def host_descriptor(original_T60, target_T60, sr, time_after_max):
    """(q, after_max) as the host forms them."""
    return 3 / (target_T60 * sr) - 3 / (original_T60 * sr), int(math.floor(time_after_max * sr))


def golden_cases(golden_dir):
    """[dict(name, h, rir, win, q, after_max, kw)]: the reference's inputs and outputs, with the descriptor of each."""
    z = np.load(os.path.join(golden_dir, "rts_windows.npz"))
    out = []
    for kw in json.loads(str(z["meta"])):
        kw = dict(kw)
        name = kw.pop("name")
        q, after_max = host_descriptor(**kw)
        out.append(dict(name=name, h=z[f"{name}_h"], rir=z[f"{name}_rir"], win=z[f"{name}_win"], q=q, after_max=after_max, kw=kw))
    return out


def check_shorten(case, out, win, idx):
    """One row of fsn_rir_shorten against the reference's output for `case`: idx exact, out and win within
    TAP_REL |ref| + TAP_ABS, zeros behind the response.  Returns the number of elements that are not bit-equal."""
    n = len(case["h"])
    want_idx = first_argmax_abs(case["h"])
    assert int(idx) == want_idx, (case["name"], int(idx), want_idx)
    out, win = np.asarray(out), np.asarray(win)
    assert out.dtype == np.float32 and win.dtype == np.float32
    assert not out[n:].any() and not win[n:].any(), (case["name"], "not zero behind the response")
    differ = 0
    for what, got, ref in (("win", win[:n], case["win"]), ("out", out[:n], case["rir"])):
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        allow = TAP_REL * np.abs(ref.astype(np.float64)) + TAP_ABS
        worst = int(np.argmax(err - allow))
        assert np.isfinite(got).all() and (err <= allow).all(), (case["name"], what, worst, float(got[worst]), float(ref[worst]))
        differ += int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    return differ


# ---- the target row ---------------------------------------------------------------------------------------------------------
def target_rows(item, clean_list, noise_list, rir_list, L, eps=R.EPS):
    """The fp64 reference of one row of fsn_mix_pairs_target and the allowance of its target:
    (noisy64, clean64, target64, allowance [L], mode).  The target is snr_mix's scalar chain - the factor s that takes the
    reverberant clean row to its `clean` output, every scalar of it formed from the REVERBERANT row - applied to
    fft_conv(clean row, fp32 shortened taps).  Allowance: what the mix sweep allows `clean` on this row (4 x the fp32
    port's own error, not below 2^-23, of the row's peak) plus the tap allowance carried through the convolution,
    TAP_REL s conv(|x|, |h_s|)[n]."""
    c, n = R.rows_of(item, clean_list, noise_list, L)
    h = R.rir_of(item, rir_list)
    noisy64, clean64, _ = R.snr_mix(c, n, item.snr, item.target_dB_FS, item.noisy_target_dB_FS, h, eps, np.float64)
    _, clean32, _ = R.snr_mix(c, n, item.snr, item.target_dB_FS, item.noisy_target_dB_FS, h, eps, np.float32)
    rel = max(4.0 * R.mix_error(clean32, clean64), R.MIX_FLOOR)
    mode = effective_mode(item)
    if mode == 0:
        return noisy64, clean64, clean64, np.zeros(L), 0
    hs, _, _ = rts_window(h, item.target_q, item.target_after_max, mode)
    rev = R.fft_conv(c, h)
    e = float(np.dot(rev, rev))
    s = float(np.dot(clean64, rev)) / e if e > 0 else 0.0  # clean64 = s rev: the chain is one factor
    assert e == 0 or np.abs(clean64 - s * rev).max() <= 1e-12 * np.abs(clean64).max()
    target64 = s * R.fft_conv(c, hs)
    allow = rel * float(np.abs(target64).max()) + TAP_REL * abs(s) * R.fft_conv(np.abs(c), np.abs(hs))
    return noisy64, clean64, target64, allow, mode


def effective_mode(item):
    """The mode pack_targets must give the row: no response, or a shortening with q <= 0, keeps the reverberant row."""
    if item.rir_index < 0 or item.target_mode == 0 or (item.target_mode == 1 and not item.target_q > 0):
        return 0
    return item.target_mode


def check_target(name, got, target64, allow):
    """A target row of the device against its reference, sample by sample (where the allowance is zero - nothing reaches
    the sample - the row must be exact); returns the worst error / allowance."""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), name
    err = np.abs(got - target64)
    worst = int(np.argmax(err - allow))
    assert (err <= allow).all(), (name, worst, float(err[worst]), float(allow[worst]))
    some = allow > 0
    return float((err[some] / allow[some]).max()) if some.any() else 0.0


# ---- the rows of the sweep (tests/test_gpu_mix_target.py) -----------------------------------------------------------------
SR = 16000
AFTER_MAX = 32  # floor(0.002 * 16000)


def sweep_items():
    """[(name, MixItem)] on mix_reference.mix_sources() at L = MIX_L: shortened and early rows on the 1-D response (800 taps,
    e-folding 120 samples: T60 = 120 ln(1000) / 16000 = 0.0518 s) and on rows of the 2-D one (300 taps, T60 = 0.0173 s),
    one on each clip branch, a dry row, a row whose q <= 0 (mode 0 on a reverberant row), digital silence, a huge q."""
    import dataclasses
    cases = {name: it for name, it, _ in R.mix_cases()}
    q1 = 3 / (0.02 * SR) - 3 / (0.0518 * SR)    # 0.0518 s -> 0.02 s
    q2 = 3 / (0.008 * SR) - 3 / (0.0173 * SR)   # 0.0173 s -> 0.008 s
    rows = [
        ("shortened_1d", "reverb_snr-5_two_segments", dict(target_mode=1, target_q=q1, target_after_max=AFTER_MAX)),
        ("early_2d", "reverb_2d_five_segments", dict(target_mode=2, target_q=0.0, target_after_max=AFTER_MAX)),
        ("dry_asks_for_shortened", "plain_snr20", dict(target_mode=1, target_q=q1, target_after_max=AFTER_MAX)),
        ("shortened_2d_clipped", "clipped_spikes_reverb", dict(target_mode=1, target_q=q2, target_after_max=AFTER_MAX)),
        ("q_not_positive", "silent_noise", dict(target_mode=1, target_q=-q1, target_after_max=AFTER_MAX)),
        ("shortened_silence", "zero_clean_reverb", dict(target_mode=1, target_q=q1, target_after_max=AFTER_MAX)),
        ("huge_q_short_clean", "short_clean_file", dict(target_mode=1, target_q=0.37, target_after_max=3)),
        ("early_clean_len_1", "clean_len_1_reverb", dict(target_mode=2, target_q=0.0, target_after_max=5)),
    ]
    return [(name, dataclasses.replace(cases[base], **kw)) for name, base, kw in rows]
