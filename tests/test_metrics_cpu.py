"""The metric entries without a GPU: the fp64 numpy reference the kernels are held to (tests/stoi_reference.py) against
the published constants and scipy's resampler, the host side of fsn_stoi / fsn_si_sdr (size query, refusals, header =
exports = bindings), and the conditions on the seeded fixture table that make the GPU test's bound of 5e-11 meaningful."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stoi_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fsn_stoi_workspace_bytes", "fsn_stoi", "fsn_si_sdr")
BOUND = 5e-11  # tests/test_gpu_metrics.py


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_band_table_is_the_published_third_octave_grid():
    assert R.third_octave_bins() == R.BANDS
    assert R.BANDS[0] == (7, 9) and R.BANDS[-1] == (174, 219) and len(R.BANDS) == 15
    assert all(a[1] == b[0] for a, b in zip(R.BANDS, R.BANDS[1:]))


def test_resampler_taps():
    for (up, down), n in (((5, 8), 581), ((5, 24), 1741)):
        hn, L = R.resample_taps(up, down)
        assert len(hn) == n == 2 * L + 1
        assert abs(np.sum(hn) - 1) < 1e-15 and np.array_equal(hn, hn[::-1])


@pytest.mark.parametrize("up,down,n", [(5, 8, 4001), (5, 8, 8000), (5, 24, 4801), (5, 24, 9000), (5, 8, 100), (5, 24, 7)])
def test_closed_form_resampler_against_scipy(up, down, n):
    from scipy.signal import resample_poly
    x = np.random.default_rng(n).standard_normal(n)
    hn, _ = R.resample_taps(up, down)
    got, want = R.resample(x, up, down), resample_poly(x, up, down, window=hn)
    assert len(got) == len(want) == -(-n * up // down)
    assert np.max(np.abs(got - want)) <= 1e-13


def test_identical_signals_score_one():
    for sr in R.RATES:
        x = R.speech_like(2 * sr, sr, np.random.default_rng(sr)).astype(np.float32)
        assert abs(R.stoi(x, x, sr) - 1) <= 1e-14


def test_29_frames_score_1e_5_and_30_do_not():
    for sr in R.RATES:
        n29, n30 = R.length_for_frames(sr, 29, 200 + sr), R.length_for_frames(sr, 30, 100 + sr)
        x = R.speech_like(n30, sr, np.random.default_rng(100 + sr), steady=True).astype(np.float32)
        y = R.add_noise(x.astype(np.float64), 10, np.random.default_rng(1)).astype(np.float32)
        assert R.spectral_frames(x, sr)[0] == 30
        d = R.stoi(x, y, sr)
        assert d != R.SHORT and 0.1 < d < 1
        x = R.speech_like(n29, sr, np.random.default_rng(200 + sr), steady=True).astype(np.float32)
        assert R.spectral_frames(x, sr)[0] == 29
        assert R.stoi(x, x, sr) == 1e-5


def test_all_zero_rows_score_zero():
    x = R.speech_like(16000, 16000, np.random.default_rng(2)).astype(np.float32)
    zero = np.zeros_like(x)
    assert R.stoi(x, zero, 16000) == 0.0
    assert R.stoi(zero, x, 16000) == 0.0
    assert R.stoi(zero, zero, 16000) == 0.0


def test_score_falls_with_the_noise():
    x = R.speech_like(32000, 16000, np.random.default_rng(3)).astype(np.float32)
    d = [R.stoi(x, R.add_noise(x.astype(np.float64), snr, np.random.default_rng(4)).astype(np.float32), 16000)
         for snr in (20, 5, -5)]
    assert 1 > d[0] > d[1] > d[2] > 0, d


def test_si_sdr_reference_recovers_the_mixing_ratio():
    rng = np.random.default_rng(5)
    r = rng.standard_normal(20000)
    n = rng.standard_normal(20000)
    n -= r * np.dot(r, n) / np.dot(r, r)
    for snr in (-5, 20, 60):
        e = 0.3 * r + n * np.sqrt(np.sum((0.3 * r) ** 2) / np.sum(n * n) / 10 ** (snr / 10))
        assert abs(R.si_sdr(r, e) - snr) < 1e-9


# ---- the host side of the entries ---------------------------------------------------------------------------------------
def test_header_exports_and_bindings_agree_on_the_metric_entries():
    from fullsubnet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fsn_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    assert "fsn_*" in open(os.path.join(ROOT, "fullsubnet_amd", "csrc", "fsn_exports.map")).read()
    for name in ENTRIES:
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert name in _lib.ADDED_IN_118
    assert "#define FSN_ABI_VERSION 118" in src and _lib.ABI_VERSION == 118
    import fullsubnet_amd
    assert fullsubnet_amd.metrics.stoi and fullsubnet_amd.metrics.si_sdr


def expected_workspace(B, L_max, sr):
    """The layout of csrc/fsn_api_metrics.hip: taps, the two signals at 10 kHz, energies, kept list, counts, band
    magnitudes, partial sums, each rounded up to 256 bytes."""
    up, down = R.RATES[sr]
    half = 0 if sr == 10000 else R.resample_taps(up, down)[1]
    n10 = L_max if sr == 10000 else -(-L_max * up // down)
    nf = len(range(0, n10 - 256, 128))
    m = max(nf - 1, 1)
    jb = -(-(m - 29 if m >= 30 else 1) // 256)
    parts = [8 * (2 * half + 1), 8 * B * 2 * n10, 8 * B * max(nf, 1), 4 * B * max(nf, 1), 4 * B, 8 * B * 2 * 15 * m,
             8 * B * 15 * jb]
    return sum(-(-p // 256) * 256 for p in parts)


def test_size_query_arithmetic_and_refusals_without_a_gpu():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    for B, L_max, sr in [(1, 1, 10000), (1, 257, 10000), (6, 32000, 16000), (3, 48000, 48000), (3, 20000, 10000),
                         (150, 160000, 16000), (32, 480000, 48000), (2, 6555, 16000)]:
        assert L.fsn_stoi_workspace_bytes(B, L_max, sr) == expected_workspace(B, L_max, sr), (B, L_max, sr)
    for args, word in (((1, 16000, 8000), b"sr = 8000"), ((1, 16000, 44100), b"sr = 44100"), ((0, 16000, 16000), b"B = 0"),
                       ((1, 0, 16000), b"L_max = 0")):
        assert L.fsn_stoi_workspace_bytes(*args) == 0
        assert word in L.fsn_last_error(), (args, L.fsn_last_error())
    # refused before anything is launched: no device is needed to be told so
    fake = ctypes.c_void_p(256 * 1024)
    need = L.fsn_stoi_workspace_bytes(2, 16000, 16000)
    for call, word in ((lambda: L.fsn_stoi(fake, fake, None, 2, 16000, 8000, fake, fake, need, None), b"sr = 8000"),
                       (lambda: L.fsn_stoi(fake, fake, None, 0, 16000, 16000, fake, fake, need, None), b"B = 0"),
                       (lambda: L.fsn_stoi(fake, fake, None, 2, 0, 16000, fake, fake, need, None), b"L_max = 0"),
                       (lambda: L.fsn_stoi(fake, fake, None, 2, 16000, 16000, fake, None, need, None), b"NULL workspace"),
                       (lambda: L.fsn_stoi(fake, fake, None, 2, 16000, 16000, fake, fake, need - 1, None), b"at least"),
                       (lambda: L.fsn_stoi(fake, fake, None, 2, 16000, 16000, fake, ctypes.c_void_p(256 * 1024 + 8), need,
                                           None), b"aligned"),
                       (lambda: L.fsn_stoi(None, fake, None, 2, 16000, 16000, fake, fake, need, None), b"NULL pointer"),
                       (lambda: L.fsn_si_sdr(fake, fake, None, 0, 16000, fake, None), b"B = 0"),
                       (lambda: L.fsn_si_sdr(fake, None, None, 1, 16000, fake, None), b"NULL pointer")):
        assert call() == -1  # FSN_ERR_ARG
        assert word in L.fsn_last_error(), L.fsn_last_error()
    with pytest.raises(_lib.FsnError):
        import fullsubnet_amd
        fullsubnet_amd.metrics.stoi(torch.zeros(2, 4000), torch.zeros(2, 4000))  # CPU tensors: no fallback
    with pytest.raises(_lib.FsnError):
        fullsubnet_amd.metrics.si_sdr(torch.zeros(4000), torch.zeros(4000))


# ---- the fixture table of the GPU test ------------------------------------------------------------------------------------
def all_rows():
    return [(tag, sr, row) for tag, (sr, _, _, rows) in R.fixture_table().items() for row in rows]


def test_fixture_table_has_the_cases():
    table = R.fixture_table()
    assert {tag: (sr, L, ragged, len(rows)) for tag, (sr, L, ragged, rows) in table.items()} == {
        "16k": (16000, 32000, True, 6), "48k": (48000, 48000, True, 3), "10k": (10000, 20000, True, 3),
        "rect": (16000, 12000, False, 3)}
    for tag, (sr, L, ragged, rows) in table.items():
        lengths = [len(r["clean"]) for r in rows]
        assert max(lengths) == L and (ragged or min(lengths) == L)
        frames = [R.spectral_frames(r["clean"], sr)[0] for r in rows]
        if ragged:
            assert 30 in frames and 29 in frames, (tag, frames)   # J = 1, and one frame short of it
            assert any(n == L for n in lengths)
        for r, m in zip(rows, frames):
            assert (r["exact"] == R.SHORT) == (m < 30) and (r["d"] == R.SHORT) == (m < 30)
    names = [r["name"] for r in table["16k"][3]]
    assert "estimate == clean" in names and "zero estimate" in names and any("pause" in n for n in names)
    equal = table["16k"][3][names.index("estimate == clean")]
    assert np.array_equal(equal["clean"], equal["estimate"]) and abs(equal["d"] - 1) <= 1e-14
    zero = table["16k"][3][names.index("zero estimate")]
    assert zero["d"] == 0.0 and zero["exact"] == 0.0


def test_fixture_condition_a_no_frame_near_the_40_db_decision():
    for tag, sr, row in all_rows():
        assert R.mask_margin(row["clean"], sr) >= 1e-6, (tag, row["name"])


def test_fixture_condition_b_segments_are_well_conditioned():
    for tag, sr, row in all_rows():
        assert R.segment_conditioning(row["clean"], row["estimate"], sr) <= 1e3, (tag, row["name"])


def test_fixture_condition_c_silence_removal_fires():
    counts = [R.spectral_frames(row["clean"], sr)[1:] for _, sr, row in all_rows()]
    fired = sum(kept < total for kept, total in counts)
    assert 3 * fired >= len(counts), (fired, len(counts))
    assert any(kept == total for kept, total in counts)


def test_fixture_condition_d_a_slip_to_fp32_cannot_pass():
    """Rounding the 10 kHz signals to fp32 moves d by a median of more than 4 x the bound, over the rows that have a
    resampled signal and a score that is not exact by construction (the 10 kHz rows are fp32 samples to begin with, so
    for them the rounding is the identity); evaluating the later stages in fp32 moves every scored row by more."""
    early, late = [], []
    for tag, sr, row in all_rows():
        if row["exact"] is not None or np.array_equal(row["clean"], row["estimate"]):
            continue
        late.append(abs(R.stoi(row["clean"], row["estimate"], sr, late_dtype=np.float32) - row["d"]))
        if sr != 10000:
            early.append(abs(R.stoi(row["clean"], row["estimate"], sr, resampled_dtype=np.float32) - row["d"]))
    assert len(early) >= 5 and np.median(early) > 4 * BOUND, early
    assert len(late) >= 7 and min(late) > 4 * BOUND, late
