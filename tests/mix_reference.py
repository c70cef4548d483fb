"""numpy reference of the on-device mixing (fsn_conv_rows / fsn_mix_pairs): the formulas of the reference's
Dataset.snr_mix (recipes/dns_interspeech_2020/dataset_train.py:137-195 with audio_zen/acoustics/feature.py:99-114) in a
chosen dtype - fp64 is the reference the kernels are held to, fp32 the yardstick whose own error sets the allowance - the
convolution as an fp64 np.fft product, the sweep tables of tests/test_gpu_mix.py, the checkers and the loaders of the
goldens.  numpy only (torch.fft for the fp32 yardstick of the convolution)."""
import numpy as np

EPS = float(np.float32(1e-6))  # the library takes eps as a float


def fft_conv(x, h, n_out=None):
    """fftconvolve(x, h)[:n_out] through an fp64 transform; taps from n_out on cannot reach those outputs."""
    x = np.asarray(x, dtype=np.float64)
    n_out = len(x) if n_out is None else n_out
    h = np.asarray(h, dtype=np.float64)[:n_out]
    n = 1
    while n < len(x) + len(h) - 1:
        n *= 2
    return np.fft.irfft(np.fft.rfft(x, n) * np.fft.rfft(h, n), n)[:n_out]


def four_step_conv(x, h, log_n=None):
    """The kernels' plan (csrc/mix_kernels.hip) index for index, in numpy: z = x + i h, N = N1 N2, column transforms by
    decimation in frequency, step twiddle, row transforms, Hermitian split and product over row pairs (k1, N1 - k1),
    inverse rows / twiddle / inverse columns by decimation in time; bit-reversed orders are never undone."""
    L = len(x)
    hl = min(len(h), L)
    need = L + hl - 1
    if log_n is None:
        log_n = 2
        while (1 << log_n) < need:
            log_n += 1
    N = 1 << log_n
    assert N >= need
    l1 = log_n // 2
    l2 = log_n - l1
    N1, N2 = 1 << l1, 1 << l2

    def brev(v, bits):
        return int(format(v, f"0{bits}b")[::-1], 2) if bits else 0

    def dif(a):  # natural in, bit-reversed out
        a = a.copy()
        M = len(a)
        h_ = M // 2
        while h_ >= 1:
            for g in range(0, M, 2 * h_):
                for p in range(h_):
                    w = np.exp(-2j * np.pi * p / (2 * h_))
                    u, v = a[g + p], a[g + p + h_]
                    a[g + p], a[g + p + h_] = u + v, (u - v) * w
            h_ //= 2
        return a

    def dit_inv(a):  # bit-reversed in, natural out, unscaled inverse
        a = a.copy()
        M = len(a)
        h_ = 1
        while h_ < M:
            for g in range(0, M, 2 * h_):
                for p in range(h_):
                    w = np.exp(2j * np.pi * p / (2 * h_))
                    u, v = a[g + p], a[g + p + h_] * w
                    a[g + p], a[g + p + h_] = u + v, u - v
            h_ *= 2
        return a

    z = np.zeros(N, np.complex128)
    z[:L] = np.asarray(x, np.float64)
    z[:hl] += 1j * np.asarray(h[:hl], np.float64)
    Z = z.reshape(N1, N2)
    for n2 in range(N2):  # conv_cols_fwd_kernel
        col = dif(Z[:, n2])
        for p in range(N1):
            Z[p, n2] = col[p] * np.exp(-2j * np.pi * (n2 * brev(p, l1)) / N)
    out = np.zeros_like(Z)
    for k1a in range(N1 // 2 + 1):  # conv_rows_kernel
        k1b = (N1 - k1a) % N1
        ks = [k1a] if k1b == k1a else [k1a, k1b]
        rows = [dif(Z[brev(k, l1)]) for k in ks]
        prod = [np.zeros(N2, np.complex128) for _ in ks]
        for r, k1 in enumerate(ks):
            for q in range(N2):
                k2 = brev(q, l2)
                k2p = (N2 - k2) % N2 if k1 == 0 else N2 - 1 - k2
                rp = 1 - r if len(ks) == 2 else r
                zk, zp = rows[r][q], rows[rp][brev(k2p, l2)]
                prod[r][q] = (zk * zk - np.conj(zp) ** 2) / (4j * N)
        for r, k1 in enumerate(ks):
            t = dit_inv(prod[r])
            out[brev(k1, l1)] = t * np.exp(2j * np.pi * (np.arange(N2) * k1) / N)
    y = np.zeros(N)
    for n2 in range(N2):  # conv_cols_inv_kernel
        y[n2::N2] = dit_inv(out[:, n2]).real
    return y[:L]


def snr_mix(clean, noise, snr, target_db, noisy_target_db, rir=None, eps=EPS, dtype=np.float64):
    """Dataset.snr_mix with the level of the mixture given instead of drawn, every array and scalar in `dtype`.
    Returns (noisy, clean, max|noisy| before the clip check)."""
    dt = np.dtype(dtype).type
    eps = dt(eps)
    clean = np.asarray(clean, dtype=np.float32)
    if rir is not None:
        clean = fft_conv(clean, np.asarray(rir, dtype=np.float32))
    clean = np.asarray(clean, dtype=dt)
    noise = np.asarray(noise, dtype=dt)

    def norm_amplitude(y):
        return y / dt(np.max(np.abs(y)) + eps)

    def tailor(y, db):
        rms = dt(np.sqrt(np.mean(y * y)))
        scalar = dt(dt(10.0) ** dt(db / 20)) / dt(rms + eps)
        return y * scalar, scalar

    clean, _ = tailor(norm_amplitude(clean), target_db)
    clean_rms = dt(np.sqrt(np.mean(clean * clean)))
    noise, _ = tailor(norm_amplitude(noise), target_db)
    noise_rms = dt(np.sqrt(np.mean(noise * noise)))
    gain = dt(dt(clean_rms / dt(dt(10.0) ** dt(snr / 20))) / dt(noise_rms + eps))
    noisy = clean + noise * gain
    noisy, scalar = tailor(noisy, noisy_target_db)
    clean = clean * scalar
    peak = dt(np.max(np.abs(noisy)))
    if peak > dt(0.999):
        d = dt(peak / dt(dt(0.99) - eps))
        noisy, clean = noisy / d, clean / d
    assert noisy.dtype == dt and clean.dtype == dt
    return noisy, clean, float(peak)


# ---- descriptors (fullsubnet_amd.mix.MixItem fields) on the host ------------------------------------------------------
def rows_of(item, clean_list, noise_list, L):
    """The clean row (crop, zero-padded) and the noise row (silence + segments) of a descriptor, fp32."""
    c = np.zeros(L, np.float32)
    c[:item.clean_len] = np.asarray(clean_list[item.clean_index], np.float32)[item.clean_start:item.clean_start + item.clean_len]
    n = np.zeros(L, np.float32)
    for k, src, dst, ln in item.segments:
        n[dst:dst + ln] = np.asarray(noise_list[k], np.float32)[src:src + ln]
    return c, n


def rir_of(item, rir_list):
    if item.rir_index < 0:
        return None
    r = np.asarray(rir_list[item.rir_index], np.float32)
    return r if r.ndim == 1 else r[item.rir_row]


def mix_item(item, clean_list, noise_list, rir_list, L, dtype=np.float64, eps=EPS):
    c, n = rows_of(item, clean_list, noise_list, L)
    return snr_mix(c, n, item.snr, item.target_dB_FS, item.noisy_target_dB_FS, rir_of(item, rir_list), eps, dtype)


def pcm(a):
    """Floats in [-1, 1) as 16-bit PCM values v / 32768 (exact in fp32): one array serves both slab formats."""
    return (np.clip(np.rint(np.asarray(a, np.float64) * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


# ---- convolution sweep ---------------------------------------------------------------------------------------------------
CONV_L = (1, 2, 511, 512, 513, 4097, 49152, 131072)


def conv_rir_lengths(L):
    """The response lengths of the sweep that mean something at L (L + min(h, L) - 1 hits 2^k at (512, 1), (513, 512),
    (4097, 4096) and 2^k + 1 at (512, 2), (513, 513), (4097, 4097))."""
    return sorted({h for h in (1, 2, 255, 512, 513, L - 1, L, L + 7, 3 * L) if h >= 1})


def conv_batches(L):
    """[(B, [h_len per row])]: B = 1, 3 and 16, response lengths mixed in a batch, 0 (a copied row) among them."""
    R = conv_rir_lengths(L)
    if L > 49152:  # the largest transform: the extremes, few rows
        return [(1, [L - 1]), (3, [3 * L, 0, 513])]
    full = R + [0]
    b16 = [full[i % len(full)] for i in range(16)]
    return [(1, [R[-1]]), (3, [R[len(R) // 2], 0, R[0]]), (16, b16)]


def conv_inputs(L, h_lens, seed):
    """x [B, L] fp32 and the responses (16-bit PCM values, decaying noise) of one batch."""
    rng = np.random.default_rng(seed)
    x = (0.1 * rng.standard_normal((len(h_lens), L))).astype(np.float32)
    hs = []
    for hl in h_lens:
        k = np.arange(hl)
        h = rng.standard_normal(hl) * np.exp(-k / max(hl / 6.0, 1.0))
        hs.append(pcm(0.9 * h / max(np.abs(h).max(), 1e-9)) if hl else np.zeros(0, np.float32))
    return x, hs


def conv_error(y, y64, x, h):
    """max |y - y64| over the peak of |h| * |x|."""
    L = len(x)
    scale = np.abs(fft_conv(np.abs(x), np.abs(h[:L]))).max() if len(h) else np.abs(x).max()
    return float(np.abs(np.asarray(y, np.float64) - y64).max() / scale)


def conv_fp32_error(x, h, y64):
    """The same figure for a CPU fp32 FFT convolution (torch.fft, fp32) of the case."""
    import torch
    L = len(x)
    hh = np.ascontiguousarray(h[:L])
    n = 1
    while n < L + len(hh) - 1:
        n *= 2
    X = torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(x)), n)
    H = torch.fft.rfft(torch.from_numpy(hh), n)
    y = torch.fft.irfft(X * H, n)[:L].numpy()
    assert y.dtype == np.float32
    return conv_error(y, y64, x, h)


CONV_FLOOR = 4.0 * 2.0 ** -24
MIX_FLOOR = 2.0 ** -23


# ---- mix sweep --------------------------------------------------------------------------------------------------------------
MIX_L = 4097  # odd, several workgroups of the gather, several strides of the level kernel


def mix_sources(seed=11):
    """Source lists of the sweep (16-bit PCM values): clean [speech-like, spiky, zeros, short], noise, rir [1-D, 2-D]."""
    rng = np.random.default_rng(seed)
    L = MIX_L
    t = np.arange(L + 900)
    speech = 0.3 * rng.standard_normal(L + 900) * (0.55 + 0.45 * np.sin(2 * np.pi * t / 1700.0))
    spiky = np.zeros(L)
    spiky[[37, 1500, 2901, L - 1]] = [0.9, -0.7, 0.8, 0.5]
    spiky += 1e-3 * rng.standard_normal(L)
    clean = [pcm(speech), pcm(spiky), np.zeros(L, np.float32), pcm(0.2 * rng.standard_normal(700))]
    noise = [pcm(0.05 * rng.standard_normal(n)) for n in (L + 300, 1200, 640, 900, 333)]
    r1 = rng.standard_normal(800) * np.exp(-np.arange(800) / 120.0)
    r2 = rng.standard_normal((3, 300)) * np.exp(-np.arange(300) / 40.0)
    rir = [pcm(0.8 * r1 / np.abs(r1).max()), pcm(0.8 * r2 / np.abs(r2).max())]
    return clean, noise, rir


def mix_cases():
    """[(name, MixItem, clipped)] - and every case is decisive on the clip branch: its fp64 max|noisy| before the check
    lies outside 0.999 (1 +- 1e-4), so that fp32 and fp64 arithmetic take the same branch."""
    from fullsubnet_amd.mix import MixItem
    L = MIX_L
    clean, noise, rir = mix_sources()
    whole = [(0, 100, 0, L)]
    two = [(1, 0, 0, 1200), (2, 10, 1200 + 700, 630)]                       # a silence between, silence to the end
    five = [(3, 5, 0, 895), (4, 0, 1000, 333), (2, 0, 1500, 640), (1, 0, 2200, 1200), (0, 7, 3500, L - 3500)]  # ends at L
    T = -25
    cases = [
        ("plain_snr20", MixItem(0, 450, L, whole, 20, -1, 0, -30, T)),
        ("reverb_snr-5_two_segments", MixItem(0, 0, L, two, -5, 0, 0, -22, T)),
        ("reverb_2d_five_segments", MixItem(0, 900, L, five, 7, 1, 2, -35, T)),
        ("clean_len_1", MixItem(3, 5, 1, whole, 20, -1, 0, -33, T)),
        ("clean_len_1_reverb", MixItem(3, 5, 1, whole, 20, 0, 0, -33, T)),
        ("clean_len_L-1", MixItem(0, 3, L - 1, two, -5, -1, 0, -25, T)),
        ("short_clean_file", MixItem(3, 0, 700, five, 20, 1, 0, -28, T)),
        ("clipped_spikes", MixItem(1, 0, L, whole, 20, -1, 0, -16, T)),
        ("clipped_spikes_reverb", MixItem(1, 0, L, two, 20, 1, 1, -16, T)),
        ("zero_clean", MixItem(2, 0, L, whole, -5, -1, 0, -25, T)),
        ("zero_clean_reverb", MixItem(2, 0, L, whole, 20, 0, 0, -25, T)),
        ("silent_noise", MixItem(0, 10, L, [], 20, 0, 0, -20, T)),
    ]
    out = []
    for name, it in cases:
        _, _, peak = mix_item(it, clean, noise, rir, L, np.float64)
        assert not (0.999 * (1 - 1e-4) <= peak <= 0.999 * (1 + 1e-4)), (name, peak)
        out.append((name, it, peak > 0.999))
    assert {c for _, _, c in out} == {True, False}
    return out


def mix_error(y, y64):
    """max |y - y64| over the row's peak (a row of zeros must be reproduced exactly: 0, or inf)."""
    d = float(np.abs(np.asarray(y, np.float64) - y64).max())
    peak = float(np.abs(y64).max())
    if peak == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / peak


# ---- goldens (tests/golden/make_golden_mix.py) -----------------------------------------------------------------------------
class HostTables:
    """What draw_item reads of a MixBank, without a device."""

    def __init__(self, clean, noise, rir):
        self.clean_len = np.asarray([len(w) for w in clean], np.int64)
        self.noise_len = np.asarray([len(w) for w in noise], np.int64)
        self.rir_rows = [1 if np.ndim(r) == 1 else int(np.shape(r)[0]) for r in rir]
        self.rir_2d = [np.ndim(r) > 1 for r in rir]


class LoggedRandom:
    """`random` / `np.random` stand-in for draw_item that keeps the log format of make_golden_mix.py's Recorder."""

    def __init__(self, py_seed, np_seed, log):
        import random
        self.py, self.np, self.log = random.Random(py_seed), np.random.RandomState(np_seed), log

    def choice(self, seq):
        r = self.py.choice(seq)
        self.log.append(["choice", len(seq), list(seq).index(r)])
        return r

    def randint(self, *a):
        r = self.np.randint(*a)
        self.log.append(["randint", [int(v) for v in a], int(r)])
        return r

    def random(self, *a):
        r = self.np.random_sample(*a)
        self.log.append(["random", float(np.ravel(r)[0])])
        return r


def golden_sources(golden_dir):
    """(clean, noise, rir lists as fp32 = v / 32768, the same lists as int16, the dataset arguments)."""
    import json
    import os
    z = np.load(os.path.join(golden_dir, "mix_sources.npz"))
    meta = json.loads(str(z["meta"]))
    pcm16 = [[z[f"{kind}_{i}"] for i in range(meta[f"n_{kind}"])] for kind in ("clean", "noise", "rir")]
    f32 = [[(w.astype(np.float32) / np.float32(32768.0)) for w in lst] for lst in pcm16]
    return f32, pcm16, meta


def golden_items(golden_dir):
    """The goldens as descriptors: [(name, MixItem, reference noisy, reference clean)], the dozen __getitem__ items replayed
    through draw_item under the recorded seeds (with the logs of both sides) and the direct snr_mix calls."""
    import json
    import os
    from fullsubnet_amd.mix import MixConfig, MixItem, draw_item
    (clean, noise, rir), _, meta = golden_sources(golden_dir)
    a = meta["args"]
    cfg = MixConfig(sr=a["sr"], sub_sample_length=a["sub_sample_length"], silence_length=a["silence_length"],
                    snr_range=tuple(a["snr_range"]), reverb_proportion=a["reverb_proportion"], target_dB_FS=a["target_dB_FS"],
                    target_dB_FS_floating_value=a["target_dB_FS_floating_value"])
    assert cfg.samples == meta["L"]
    z = np.load(os.path.join(golden_dir, "mix_items.npz"))
    ref_logs = json.loads(str(z["logs"]))
    tables = HostTables(clean, noise, rir)
    out, logs = [], []
    for i, (ps, ns) in enumerate(z["seeds"]):
        log = []
        rnd = LoggedRandom(int(ps), int(ns), log)
        out.append((f"getitem_{i}", draw_item(i, tables, cfg, rnd, rnd), z["noisy"][i], z["clean"][i]))
        logs.append((ref_logs[i], log))
    for j, d in enumerate(json.loads(str(z["direct"]))):
        it = MixItem(d["clean_index"], d["clean_start"], d["clean_len"], [(d["noise_index"], d["noise_start"], 0, meta["L"])],
                     d["snr"], d["rir_index"], d["rir_row"], d["noisy_target_dB_FS"], a["target_dB_FS"])
        out.append((f"direct_{j}{'_clipped' if d['clipped'] else ''}", it, z["direct_noisy"][j], z["direct_clean"][j]))
    return out, logs, meta["L"]


# ---- sweep runners: shared by tests/test_gpu_mix.py (asserts) and tools/bench_mix.py (records the worst ratios) ---------
def run_conv_sweep(conv_fn, L):
    """conv_fn(x [B, L] fp32, responses (list of PCM-valued fp32 arrays), fmt) -> y [B, L] from fsn_conv_rows.  Returns
    [(case, error, allowance)] per row with a response, both slab formats; asserts what is exact: the two formats give
    the same bits (the responses are 16-bit PCM values in both) and a row without a response is copied."""
    out = []
    for bi, (B, h_lens) in enumerate(conv_batches(L)):
        x, hs = conv_inputs(L, h_lens, seed=L * 31 + bi)
        y = {fmt: np.asarray(conv_fn(x, hs, fmt)) for fmt in ("f32", "i16")}
        assert y["f32"].shape == (B, L) and np.isfinite(y["f32"]).all() and np.isfinite(y["i16"]).all(), (L, B)
        assert np.array_equal(y["f32"], y["i16"]), (L, B)
        for b, h in enumerate(hs):
            if len(h) == 0:
                assert np.array_equal(y["f32"][b], x[b]), (L, B, b)
                continue
            y64 = fft_conv(x[b], h)
            allow = max(4.0 * conv_fp32_error(x[b], h, y64), CONV_FLOOR)
            out.append((f"L={L} B={B} row={b} taps={len(h)}", conv_error(y["f32"][b], y64, x[b], h), allow))
    return out


def run_mix_rows(outputs, items, clean, noise, rir, L, eps=EPS):
    """outputs: (noisy [B, L], clean [B, L]) of fsn_mix_pairs for `items`.  [(row, error, allowance)] for both outputs:
    error against the fp64 port over the row's peak, allowance 4 x the fp32 port's own error, not below 2^-23."""
    out = []
    for b, it in enumerate(items):
        n64, c64, _ = mix_item(it, clean, noise, rir, L, np.float64, eps)
        n32, c32, _ = mix_item(it, clean, noise, rir, L, np.float32, eps)
        for what, got, want, yard in (("noisy", outputs[0][b], n64, n32), ("clean", outputs[1][b], c64, c32)):
            assert np.isfinite(got).all(), (b, what)
            out.append((f"row {b} {what}", mix_error(got, want), max(4.0 * mix_error(yard, want), MIX_FLOOR)))
    return out
