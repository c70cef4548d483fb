"""The resampler of libfsn_hip (fsn_resample) in numpy fp64, index for index:

    u = sr_out / g, d = sr_in / g, P = max(u, d), H = zeros P, fc = rolloff / P
    g[t] = kaiser(2H + 1, beta)[t] fc sinc(fc t), t = -H .. H;  h = u g / sum(g)
    n_out = ceil(n u / d);  y[k] = sum_m h[k d + H - m u] x[m] over the m in [0, n) whose tap index lies in [0, 2H]

``resample`` evaluates whole rows (phase by phase, one dot product per output over exactly the terms above),
``resample_at`` chosen outputs only, ``abs_sum_at`` the sum of |h| |x| the GPU test's bound needs."""
import math

import numpy as np

DESIGNS = {"scipy": (10, 5.0, 1.0), "sharp": (32, 12.0, 0.92)}


def ratio(sr_in, sr_out):
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def out_length(n, sr_in, sr_out):
    u, d = ratio(sr_in, sr_out)
    return -(-n * u // d)


def taps(sr_in, sr_out, design="scipy"):
    """(h [2H + 1] float64, H)."""
    zeros, beta, rolloff = DESIGNS[design] if isinstance(design, str) else design
    u, d = ratio(sr_in, sr_out)
    P = max(u, d)
    H = zeros * P
    t = np.arange(-H, H + 1, dtype=np.float64)
    fc = rolloff / P
    w = np.kaiser(2 * H + 1, beta)
    g = w * fc * np.sinc(fc * t)
    return u * g / np.sum(g), H


def _terms(k, n, u, d, H):
    """(m_lo, m_hi): the inputs of output k, the m in [0, n) with 0 <= k d + H - m u <= 2H."""
    c = k * d + H
    m_lo = max(0, -(-(c - 2 * H) // u))
    m_hi = min(n - 1, c // u)
    return m_lo, m_hi


def resample_at(x, sr_in, sr_out, ks, design="scipy", h=None, absolute=False):
    """y[k] for the k in ``ks`` (float64, not rounded); ``absolute``: sum |h| |x| instead."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    u, d = ratio(sr_in, sr_out)
    if u == d == 1:
        return np.abs(x[np.asarray(ks)]) if absolute else x[np.asarray(ks)].copy()
    if h is None:
        h = taps(sr_in, sr_out, design)[0]
    H = (len(h) - 1) // 2
    if absolute:
        h, x = np.abs(h), np.abs(x)
    out = np.zeros(len(ks), dtype=np.float64)
    for i, k in enumerate(ks):
        k = int(k)
        m_lo, m_hi = _terms(k, n, u, d, H)
        if m_hi < m_lo:
            continue
        j = k * d + H - m_lo * u  # tap of m_lo; falls by u per sample
        out[i] = np.dot(h[j - (m_hi - m_lo) * u:j + 1:u][::-1], x[m_lo:m_hi + 1])
    return out


def resample(x, sr_in, sr_out, design="scipy", absolute=False):
    """The whole row: float64 [n_out], not rounded."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    u, d = ratio(sr_in, sr_out)
    if u == d == 1:
        return np.abs(x) if absolute else x.copy()
    h, H = taps(sr_in, sr_out, design)
    n_out = -(-n * u // d)
    if absolute:
        h, x = np.abs(h), np.abs(x)
    # per phase p = (k d + H) mod u: outputs k = k0, k0 + u, .. read x[q - j] against h[p + j u], q = (k d + H) / u
    J = -(-len(h) // u)
    q_max = ((n_out - 1) * d + H) // u if n_out else 0
    xp = np.concatenate([np.zeros(J - 1), x, np.zeros(max(0, q_max - n + 1))])  # zeros outside the row
    y = np.zeros(n_out, dtype=np.float64)
    for k0 in range(min(u, n_out)):
        ks = np.arange(k0, n_out, u)
        p = (k0 * d + H) % u
        hp = h[p::u]                                      # h[p + j u], j = 0 ..
        q = (ks * d + H) // u                             # newest input of every output
        idx = q[:, None] + (J - 1) - np.arange(len(hp))[None, :]   # xp index of x[q - j]
        y[ks] = np.einsum("kj,j->k", xp[idx], hp)
    return y


def bound(r, s):
    """The GPU test's bound on |y - r|: one fp32 rounding of r plus 2^-40 of sum |h| |x| (``s``)."""
    return 2.0 ** -24 * np.abs(r) + 2.0 ** -40 * s


def response_db(h, u, freqs_hz, sr_in):
    """|H(f)| / u in dB at the frequencies, the filter running at u sr_in."""
    fs = u * sr_in
    t = np.arange(len(h))
    return np.array([20 * np.log10(max(abs(np.sum(h * np.exp(-2j * np.pi * f / fs * t))) / u, 1e-300)) for f in freqs_hz])


# ---- the cases of tests/test_gpu_resample.py (tests/test_resample_cpu.py shows its bound can be met on them) ------------
# (sr_in, sr_out): the ratios 1/3, 3/1, 1/2, 2/1, 5/8, 160/441, 441/160 and 1/1
RATIOS = [(3, 1), (1, 3), (2, 1), (1, 2), (8, 5), (441, 160), (160, 441), (1, 1)]
SHARP_RATIOS = [(3, 1), (1, 3), (441, 160), (160, 441)]  # the steeper design: 44.1 kHz reads its table through the cache


def signal(n, seed):
    """Unit-variance noise, fp32."""
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def case_lengths(sr_in, sr_out, design, tile_inputs):
    """Rows shorter than the filter (1, 2, H / u rounded down and up), one less than, equal to and one more than the
    inputs one workgroup covers (``tile_inputs``, from the library's plan), and 4099."""
    u, d = ratio(sr_in, sr_out)
    H = DESIGNS[design][0] * max(u, d)
    return sorted({1, 2, max(1, H // u), -(-H // u), tile_inputs - 1, tile_inputs, tile_inputs + 1, 4099})


def cases(tile_inputs_of):
    """[(sr_in, sr_out, design, n, seed)]; ``tile_inputs_of(sr_in, sr_out, design)`` asks the library."""
    out = []
    for design, ratios in (("scipy", RATIOS), ("sharp", SHARP_RATIOS)):
        for sr_in, sr_out in ratios:
            for n in case_lengths(sr_in, sr_out, design, tile_inputs_of(sr_in, sr_out, design)):
                out.append((sr_in, sr_out, design, n, 1000 * len(out) + n))
    return out
