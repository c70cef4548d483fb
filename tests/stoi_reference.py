"""fp64 numpy reference of fsn_stoi / fsn_si_sdr: the short-time objective intelligibility measure of Taal,
Hendriks, Heusdens and Jensen (2011), not extended, with the constants the published method and pystoi document, and the
SI-SDR of audio_zen/metrics.py:19-31.  pystoi itself is on no machine this project has been built on: equality with
pystoi is NOT demonstrated, the kernels are held to this file.  Also here: the seeded fixture table of
tests/test_gpu_metrics.py and the quantities tests/test_metrics_cpu.py asserts on it.  numpy only (torch.fft for the fp32
variant of the spectra; scipy appears in the CPU test alone, as the resampler's cross-check)."""
import functools

import numpy as np

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
N_SEG = 30
BETA_DB = -15.0
DYN_RANGE_DB = 40.0
EPS = float(np.finfo(np.float64).eps)  # 2^-52
BANDS = ((7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
         (109, 138), (138, 174), (174, 219))
RATES = {10000: (1, 1), 16000: (5, 8), 48000: (5, 24)}
SHORT = 1e-5  # the score of a pair with fewer than N_SEG spectral frames


def third_octave_bins(fs=FS, nfft=NFFT, num_bands=15, min_freq=150.0):
    """[lo, hi) bins of the one-third-octave bands, derived the published way (nearest bin to each band edge)."""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    freq_low = min_freq * 2.0 ** ((2 * k - 1) / 6)
    freq_high = min_freq * 2.0 ** ((2 * k + 1) / 6)
    return tuple((int(np.argmin((f - lo) ** 2)), int(np.argmin((f - hi) ** 2))) for lo, hi in zip(freq_low, freq_high))


@functools.lru_cache(maxsize=None)
def resample_taps(up, down):
    """(hn, L): the 2 L + 1 taps of the resampler, normalised to unit sum."""
    P = max(up, down)
    fc = 1.0 / (2 * P)
    L = int(np.ceil(52 / (28.714 * fc / 10)))
    t = np.arange(-L, L + 1)
    h = np.kaiser(2 * L + 1, 0.1102 * (60 - 8.7)) * 2 * up * fc * np.sinc(2 * fc * t)
    return h / np.sum(h), L


def resample(x, up, down):
    """out[k] = up * sum_m hn[k down + L - m up] x[m], k < ceil(n up / down): one convolution per phase of the filter."""
    x = np.asarray(x, dtype=np.float64)
    if up == down:
        return x.copy()
    hn, L = resample_taps(up, down)
    n = len(x)
    n_out = -(-n * up // down)
    q = np.arange(n_out) * down + L
    out = np.zeros(n_out)
    for r in range(up):
        g = hn[r::up]                      # taps r, r + up, ..: tap r + i up meets x[q // up - i]
        full = np.convolve(x, g)
        sel = np.nonzero(q % up == r)[0]
        idx = q[sel] // up
        ok = idx < len(full)
        out[sel[ok]] = up * full[idx[ok]]
    return out


def window():
    return np.hanning(N_FRAME + 2)[1:-1]


def frame_energies(x):
    """E_i = 20 log10(|w x_i| + eps) of the frames starting at 0, 128, .. < len - 256 (the last full frame is not taken)."""
    w = window()
    starts = range(0, len(x) - N_FRAME, HOP)
    frames = np.array([w * x[i:i + N_FRAME] for i in starts]).reshape(-1, N_FRAME)
    return 20 * np.log10(np.sqrt(np.sum(frames * frames, axis=1)) + EPS), frames


def remove_silent_frames(x, y):
    """The frames of x within 40 dB of its loudest, and the same frames of y, overlap-added in their kept order."""
    w = window()
    energies, x_frames = frame_energies(x)
    if len(energies) == 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, dtype=bool)
    y_frames = np.array([w * y[i:i + N_FRAME] for i in range(0, len(x) - N_FRAME, HOP)])
    mask = (np.max(energies) - DYN_RANGE_DB - energies) < 0
    x_frames, y_frames = x_frames[mask], y_frames[mask]
    n_sil = (len(x_frames) - 1) * HOP + N_FRAME
    x_sil, y_sil = np.zeros(n_sil), np.zeros(n_sil)
    for i in range(len(x_frames)):
        x_sil[i * HOP:i * HOP + N_FRAME] += x_frames[i]
        y_sil[i * HOP:i * HOP + N_FRAME] += y_frames[i]
    return x_sil, y_sil, mask


def band_magnitudes(x, dtype=np.float64):
    """[15][M]: sqrt of the band sums of |rfft(w x_m, 512)|^2 over the frames starting at 0, 128, .. < len - 256."""
    w = window().astype(dtype)
    x = x.astype(dtype)
    starts = range(0, len(x) - N_FRAME, HOP)
    if len(starts) == 0:
        return np.zeros((len(BANDS), 0), dtype=dtype)
    frames = np.array([w * x[i:i + N_FRAME] for i in starts])
    if dtype == np.float32:
        import torch
        spec = torch.fft.rfft(torch.from_numpy(frames), n=NFFT).numpy()
    else:
        spec = np.fft.rfft(frames, n=NFFT)
    power = (spec.real * spec.real + spec.imag * spec.imag).astype(dtype)
    return np.array([np.sqrt(np.sum(power[:, lo:hi], axis=1)) for lo, hi in BANDS], dtype=dtype)


def segments(tob):
    """[J][15][30] from [15][M], stride 1."""
    M = tob.shape[1]
    return np.array([tob[:, m:m + N_SEG] for m in range(M - N_SEG + 1)])


def correlate(x_tob, y_tob, dtype=np.float64):
    """Step 5 of the method on the band magnitudes (M >= 30)."""
    eps = dtype(EPS)
    clip = dtype(10 ** (-BETA_DB / 20))
    xs, ys = segments(x_tob.astype(dtype)), segments(y_tob.astype(dtype))
    norm = lambda a: np.sqrt(np.sum(a * a, axis=2, keepdims=True))
    ys = ys * (norm(xs) / (norm(ys) + eps))
    yp = np.minimum(ys, xs * (1 + clip))
    yp = yp - np.mean(yp, axis=2, keepdims=True)
    xs = xs - np.mean(xs, axis=2, keepdims=True)
    yp = yp / (norm(yp) + eps)
    xs = xs / (norm(xs) + eps)
    return dtype(np.sum(yp * xs) / (xs.shape[0] * xs.shape[1]))


def stoi(x, y, sr, resampled_dtype=None, late_dtype=np.float64):
    """d of the clean signal x and the estimate y at sample rate sr.  resampled_dtype / late_dtype: what a slip to fp32
    would do - the 10 kHz signals rounded to that type / bands and correlations evaluated in it (fixture condition d)."""
    up, down = RATES[sr]
    x10, y10 = resample(x, up, down), resample(y, up, down)
    if resampled_dtype is not None:
        x10, y10 = x10.astype(resampled_dtype).astype(np.float64), y10.astype(resampled_dtype).astype(np.float64)
    x_sil, y_sil, _ = remove_silent_frames(x10, y10)
    x_tob, y_tob = band_magnitudes(x_sil, late_dtype), band_magnitudes(y_sil, late_dtype)
    if x_tob.shape[1] < N_SEG:
        return SHORT
    return float(correlate(x_tob, y_tob, late_dtype))


def spectral_frames(x, sr):
    """(M, kept frames, all frames) of a clean signal."""
    up, down = RATES[sr]
    x10 = resample(x, up, down)
    energies, _ = frame_energies(x10)
    if len(energies) == 0:
        return 0, 0, 0
    kept = int(np.sum((np.max(energies) - DYN_RANGE_DB - energies) < 0))
    return max(kept - 1, 0), kept, len(energies)


def mask_margin(x, sr):
    """min_i |max(E) - 40 - E_i| in dB: how far the nearest frame is from changing sides (fixture condition a)."""
    up, down = RATES[sr]
    energies, _ = frame_energies(resample(x, up, down))
    return float(np.min(np.abs(np.max(energies) - DYN_RANGE_DB - energies)))


def segment_conditioning(x, y, sr):
    """max over segments, bands and both signals of |segment| / |segment - mean| (fixture condition b); segments whose
    centred norm is exactly zero (an all-zero signal) are left out."""
    up, down = RATES[sr]
    x_sil, y_sil, _ = remove_silent_frames(resample(x, up, down), resample(y, up, down))
    x_tob, y_tob = band_magnitudes(x_sil), band_magnitudes(y_sil)
    if x_tob.shape[1] < N_SEG:
        return 0.0
    xs, ys = segments(x_tob), segments(y_tob)
    norm = lambda a: np.sqrt(np.sum(a * a, axis=2))
    yp = np.minimum(ys * (norm(xs) / (norm(ys) + EPS))[..., None], xs * (1 + 10 ** (-BETA_DB / 20)))
    worst = 0.0
    for s in (xs, yp):
        full, centred = norm(s), norm(s - np.mean(s, axis=2, keepdims=True))
        ok = centred > 0
        if ok.any():
            worst = max(worst, float(np.max(full[ok] / centred[ok])))
    return worst


def si_sdr(reference, estimate):
    """audio_zen/metrics.py:19-31 in fp64 on the given (fp32) samples."""
    r, e = np.asarray(reference, dtype=np.float64), np.asarray(estimate, dtype=np.float64)
    projection = (np.sum(r * e) / np.sum(r * r)) * r
    noise = e - projection
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10 * np.log10(np.sum(projection ** 2) / np.sum(noise ** 2)))


# ---- the fixture table -------------------------------------------------------------------------------------------------
def speech_like(n, sr, rng, steady=False):
    """A voiced, syllable-modulated signal: harmonics of a drifting pitch under a formant-like tilt, times a 3 - 5 Hz
    envelope that falls 50 dB and more between syllables (steady: a shallow one, so that no frame is 40 dB down)."""
    t = np.arange(n) / sr
    f0 = rng.uniform(100, 180) * (1 + 0.05 * np.sin(2 * np.pi * rng.uniform(0.5, 1.5) * t))
    phase = 2 * np.pi * np.cumsum(f0) / sr
    x = np.zeros(n)
    for h in range(1, 25):
        x += np.sin(h * phase + rng.uniform(0, 2 * np.pi)) / h ** rng.uniform(0.8, 1.4)
    rate = rng.uniform(3, 5)
    env = 0.5 * (1 + np.sin(2 * np.pi * rate * t + rng.uniform(0, 2 * np.pi)))
    env = 0.6 + 0.4 * env if steady else 10 ** ((env - 1) * 3.0)  # 0 .. -60 dB
    x = x * env + 1e-3 * rng.standard_normal(n) * (1.0 if steady else env)
    return 0.3 * x / np.max(np.abs(x))


def add_noise(x, snr_db, rng):
    noise = rng.standard_normal(len(x))
    gain = np.sqrt(np.sum(x * x) / (np.sum(noise * noise) * 10 ** (snr_db / 10)))
    return x + gain * noise


def length_for_frames(sr, want_m, rng_seed):
    """The smallest length at `sr` whose steady signal has `want_m` spectral frames with nothing removed."""
    up, down = RATES[sr]
    nf = want_m + 1
    n10 = N_FRAME + (nf - 1) * HOP + 1
    n = n10 * down // up
    while -(-n * up // down) < n10:
        n += 1
    x = speech_like(n, sr, np.random.default_rng(rng_seed), steady=True).astype(np.float32)
    m, kept, total = spectral_frames(x, sr)
    assert (m, kept) == (want_m, total), (sr, n, m, kept, total)
    return n


def _row(name, sr, n, seed, snr_db=None, steady=False, pause=False, estimate="noisy"):
    rng = np.random.default_rng(seed)
    x = speech_like(n, sr, rng, steady=steady)
    if pause:  # 120 ms at 1e-4 of the level, a third of the way in
        a = n // 3
        x[a:a + int(0.120 * sr)] *= 1e-4
    x = x.astype(np.float32)
    if estimate == "clean":
        y = x.copy()
    elif estimate == "zero":
        y = np.zeros_like(x)
    else:
        y = add_noise(x.astype(np.float64), snr_db, rng).astype(np.float32)
    return {"name": name, "sr": sr, "clean": x, "estimate": y, "exact": None}


@functools.lru_cache(maxsize=None)
def fixture_table():
    """{batch name: (sr, L_max, ragged, rows)}.  Every row: name, sr, clean, estimate (fp32), d (this file's stoi) and
    exact (the value the device must give to the bit: 1e-5 for a short row, 0 for a zero estimate; else None)."""
    batches = {}
    n30 = {sr: length_for_frames(sr, 30, 100 + sr) for sr in RATES}
    n29 = {sr: length_for_frames(sr, 29, 200 + sr) for sr in RATES}
    batches["16k"] = (16000, 32000, True, [
        _row("30 frames, 20 dB", 16000, n30[16000], 100 + 16000, snr_db=20, steady=True),
        _row("29 frames, 0 dB", 16000, n29[16000], 200 + 16000, snr_db=0, steady=True),
        _row("pause, 0 dB", 16000, 24000, 3, snr_db=0, steady=True, pause=True),
        _row("full length, 20 dB", 16000, 32000, 4, snr_db=20),
        _row("estimate == clean", 16000, 20000, 5, estimate="clean"),
        _row("zero estimate", 16000, 16000, 6, estimate="zero"),
    ])
    for tag, sr, L in (("48k", 48000, 48000), ("10k", 10000, 20000)):
        batches[tag] = (sr, L, True, [
            _row("30 frames, 20 dB", sr, n30[sr], 100 + sr, snr_db=20, steady=True),
            _row("full length, pause, 0 dB", sr, L, 7 + sr, snr_db=0, pause=True),
            _row("29 frames, 20 dB", sr, n29[sr], 200 + sr, snr_db=20, steady=True),
        ])
    batches["rect"] = (16000, 12000, False, [
        _row("rect, 20 dB", 16000, 12000, 11, snr_db=20),
        _row("rect, pause, 0 dB", 16000, 12000, 12, snr_db=0, steady=True, pause=True),
        _row("rect, steady, 0 dB", 16000, 12000, 13, snr_db=0, steady=True),
    ])
    for sr, _, _, rows in batches.values():
        for row in rows:
            row["d"] = stoi(row["clean"], row["estimate"], sr)
            if row["d"] == SHORT:
                row["exact"] = SHORT
            elif not row["estimate"].any():
                row["exact"] = 0.0
    return batches


def pad_rows(rows, L_max):
    """(clean [B][L_max], estimate [B][L_max], lengths [B]) of a batch, zero padded."""
    B = len(rows)
    clean, est = np.zeros((B, L_max), dtype=np.float32), np.zeros((B, L_max), dtype=np.float32)
    lengths = np.zeros(B, dtype=np.int32)
    for b, row in enumerate(rows):
        n = len(row["clean"])
        clean[b, :n], est[b, :n], lengths[b] = row["clean"], row["estimate"], n
    return clean, est, lengths
