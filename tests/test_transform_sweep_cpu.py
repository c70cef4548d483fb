"""The reference and the checkers of tests/test_gpu_transform_sweep.py, tried without a GPU.

1. The oracle's stft / istft against torch.stft / torch.istft on the CPU at every size, hop, signal length and iSTFT
   `length` of the sweep's table (tolerances of test_stft_istft_other_transform_shapes: 2e-6 / 3e-6 of the maximum), the
   lengths beyond the last frame included - where torch.istft refuses (its window envelope falls below 1e-11 at the last
   taps of n_fft >= 2048) that refusal is asserted instead, and the oracle is still held to torch on the samples before.
2. The derived iSTFT bound: the oracle at float32 stays inside it against the oracle at float64 on every row and length.
3. The checkers reject deliberately wrong stand-ins: reflect padding that repeats the edge sample, a conjugated spectrum,
   DC / Nyquist imaginary parts that are not ignored, an envelope missing one frame's term, frame B of a pair leaking into a
   ragged row's zero frames at 1e-7, one bin off by 2 ULP at frame-max scale - and accept the oracle itself."""
import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O

import test_gpu_transform_sweep as S

IDS = [r.id for r in S.TABLE]
WORST = {"complete": 0.0, "derived": 0.0}


def _torch_stft(y, N, hop):
    c = torch.stft(torch.from_numpy(y), N, hop, N, window=torch.hann_window(N), return_complex=True)
    return c.real.numpy(), c.imag.numpy()


@pytest.mark.parametrize("row", S.TABLE, ids=IDS)
def test_oracle_against_torch(row):
    N, hop = row.N, row.hop
    win = S.window_of(N)
    y = S.make_signal(row)
    omag, _, ore, oim = O.stft(y, N, hop, N, window=win)
    tre, tim = _torch_stft(y, N, hop)
    assert ore.shape == tre.shape == (row.B, N // 2 + 1, row.T)
    scale = np.abs(tre + 1j * tim).max()
    assert np.abs(ore - tre).max() <= 2e-6 * scale and np.abs(oim - tim).max() <= 2e-6 * scale
    assert np.abs(omag - np.abs(tre + 1j * tim)).max() <= 2e-6 * scale
    if not row.inverse:
        with pytest.raises(RuntimeError):
            torch.istft(torch.complex(torch.from_numpy(ore), torch.from_numpy(oim)), N, hop, N, window=torch.hann_window(N))
        return
    fr, fi = S.istft_input(ore, oim)
    c = torch.complex(torch.from_numpy(fr), torch.from_numpy(fi))
    D = hop * (row.T - 1)
    a_max = np.abs(np.fft.irfft((fr.astype(np.float64) + 1j * fi).transpose(0, 2, 1), n=N, axis=-1)).max()
    for length in S.istft_lengths(N, hop, row.T):
        got = O.istft(fr, fi, N, hop, N, length=length, window=win)
        assert got.shape == (row.B, D if length is None else length)
        wsq = (win * win).astype(np.float32)
        env, wsum = np.zeros(2 * N + D + 5, dtype=np.float32), np.zeros(2 * N + D + 5, dtype=np.float32)
        for t in range(row.T):
            env[t * hop: t * hop + N] += wsq
            wsum[t * hop: t * hop + N] += win
        end = N // 2 + (D if length is None else length)
        t_len = length
        if env[N // 2: min(end, N + D)].min() < 1e-11:  # torch.istft's own check
            with pytest.raises(RuntimeError):
                torch.istft(c, N, hop, N, window=torch.hann_window(N), length=length)
            t_len = D + N // 4  # ... still pinned up to here
        want = torch.istft(c, N, hop, N, window=torch.hann_window(N), length=t_len).numpy()
        n = min(want.shape[1], got.shape[1])
        # 3e-6 of the maximum, as test_stft_istft_other_transform_shapes has it; ATen's fp32 C2R carries that error in every
        # frame value v (|v| <= a_max), and a sample that few frames cover is sum(v w) / sum(w^2): there the same error is
        # worth 3e-6 a_max sum(w) / sum(w^2)
        with np.errstate(divide="ignore", invalid="ignore"):
            amp = np.where(env > 0, wsum / env, 0.0)[N // 2: N // 2 + n]
        tol = 3e-6 * (np.abs(want).max() + a_max * amp[None, :])
        assert (np.abs(got[:, :n] - want[:, :n]) <= tol).all(), (row.id, length)
        if length is not None and length > D + N // 2:
            assert not got[:, D + N // 2:].any(), "past the last frame the reference pads zeros"


@pytest.mark.parametrize("row", [r for r in S.TABLE if r.inverse], ids=[r.id for r in S.TABLE if r.inverse])
def test_derived_bound_holds_for_the_fp32_oracle(row):
    N, hop = row.N, row.hop
    win = S.window_of(N)
    _, _, ore, oim = O.stft(S.make_signal(row), N, hop, N, window=win)
    fr, fi = S.istft_input(ore, oim)
    for length in S.istft_lengths(N, hop, row.T):
        ref = O.istft(fr, fi, N, hop, N, length=length, window=win, dtype=np.float64)
        got = O.istft(fr, fi, N, hop, N, length=length, window=win, dtype=np.float32)
        bound, complete = S.istft_bound(fr, fi, N, hop, win, ref.shape[1], ref)
        rc, rd = S.check_istft(got, ref, bound, complete, f"{row.id} length {length}")
        WORST["complete"], WORST["derived"] = max(WORST["complete"], rc), max(WORST["derived"], rd)
    print(f"\n{row.id}: worst so far {WORST['complete']:.3f} of 2e-6 max|ref|, {WORST['derived']:.3f} of the derived bound", end="")


# ---- wrong stand-ins -----------------------------------------------------------------------------------------------------

def _standin_stft(y, N, hop, win, pad_mode="reflect", conj=False):
    yp = np.pad(y, [(0, 0), (N // 2, N // 2)], mode=pad_mode)
    T = 1 + (yp.shape[1] - N) // hop
    idx = np.arange(N)[None, :] + hop * np.arange(T)[:, None]
    frames = (yp[:, idx] * win[None, None, :]).astype(np.float32)
    spec = np.fft.rfft(frames.astype(np.float64), axis=-1).transpose(0, 2, 1)
    re, im = spec.real.astype(np.float32), spec.imag.astype(np.float32)
    if conj:
        im = -im
    return re, im, np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2).astype(np.float32)


def _standin_istft(fr, fi, N, hop, win, length, use_edge_imag=False, drop_env_term=False):
    B, F, T = fr.shape
    spec = (fr.astype(np.float64) + 1j * fi.astype(np.float64)).transpose(0, 2, 1)
    frames = np.fft.irfft(spec, n=N, axis=-1)
    if use_edge_imag:  # a C2R that folds the imaginary DC / Nyquist parts into its complex half-size transform
        n = np.arange(N)
        frames = frames + (fi[:, 0, :, None] * 0.5 / N + fi[:, -1, :, None] * 0.5 / N * (-1.0) ** n[None, None, :])
    frames = (frames.astype(np.float32) * win[None, None, :]).astype(np.float32)
    total = N + hop * (T - 1)
    y, env = np.zeros((B, total), np.float32), np.zeros(total, np.float32)
    wsq = (win * win).astype(np.float32)
    for t in range(T):
        y[:, t * hop: t * hop + N] += frames[:, t]
        if not (drop_env_term and t == T // 2):
            env[t * hop: t * hop + N] += wsq
    y = y[:, N // 2: N // 2 + length] / env[None, N // 2: N // 2 + length]
    return np.pad(y, [(0, 0), (0, length - y.shape[1])]).astype(np.float32)


CASES = [(512, 256, 3, 1000), (254, 127, 2, 700), (30, 7, 2, 100), (16, 4, 2, 40)]


@pytest.mark.parametrize("N,hop,B,L", CASES)
def test_checkers_accept_the_oracle_and_reject_wrong_standins(N, hop, B, L):
    win = S.window_of(N)
    y = O.make_noisy(B, L, seed=N)
    omag, _, ore, oim = O.stft(y, N, hop, N, window=win)
    S.check_stft(*_standin_stft(y, N, hop, win), ore, oim, omag)
    with pytest.raises(AssertionError):  # the edge sample repeated
        S.check_stft(*_standin_stft(y, N, hop, win, pad_mode="symmetric"), ore, oim, omag)
    with pytest.raises(AssertionError):
        S.check_stft(*_standin_stft(y, N, hop, win, conj=True), ore, oim, omag)
    # one bin 2 ULP (at frame-max scale) off, the frame's largest bin and its smallest alike
    fmax = np.maximum(np.abs(ore), np.abs(oim)).max(axis=1)
    for pick in (np.argmax, np.argmin):
        re = ore.copy()
        k = int(pick(np.abs(ore[0, :, 1])))
        re[0, k, 1] += 2 * np.spacing(np.float32(fmax[0, 1]))
        with pytest.raises(AssertionError):
            S.check_stft(re, oim, omag, ore, oim, omag)

    fr, fi = S.istft_input(ore, oim)
    fi = fi.copy()
    fi[:, 0, :], fi[:, -1, :] = 0.3 * np.abs(fr).max(), -0.2 * np.abs(fr).max()  # must be ignored
    T = fr.shape[-1]
    for length in (hop * (T - 1), hop * (T - 1) + N // 4, hop * (T - 1) + N // 2 + 5):
        ref = O.istft(fr, fi, N, hop, N, length=length, window=win, dtype=np.float64)
        bound, complete = S.istft_bound(fr, fi, N, hop, win, length, ref)
        S.check_istft(_standin_istft(fr, fi, N, hop, win, length), ref, bound, complete)
        with pytest.raises(AssertionError):
            S.check_istft(_standin_istft(fr, fi, N, hop, win, length, use_edge_imag=True), ref, bound, complete)
        with pytest.raises(AssertionError):
            S.check_istft(_standin_istft(fr, fi, N, hop, win, length, drop_env_term=True), ref, bound, complete)
    # a non-zero sample past the last frame
    length = hop * (T - 1) + N // 2 + 5
    ref = O.istft(fr, fi, N, hop, N, length=length, window=win, dtype=np.float64)
    bound, complete = S.istft_bound(fr, fi, N, hop, win, length, ref)
    bad = _standin_istft(fr, fi, N, hop, win, length)
    bad[0, -1] = 1e-30
    with pytest.raises(AssertionError):
        S.check_istft(bad, ref, bound, complete)


def test_zero_frames_of_a_ragged_row_must_be_exact():
    """Frame B of a pair transforms zeros beside a live frame A: what the split leaves of A (1e-7 here; the kernel's own
    residue is ~1e-16) must not be taken for zero - neither by the zero-frame check nor by the ULP check of a zero frame."""
    win = S.window_of(512)
    y = O.make_noisy(1, 512, seed=3)
    omag, _, ore, oim = O.stft(y, window=win)  # 3 frames
    pad = lambda a: np.concatenate([a, np.zeros_like(a[..., :1])], axis=-1)  # T_max = 4: frame 3 is frame B of the pair (2, 3)
    re, im, mag = pad(ore), pad(oim), pad(omag)
    S.check_zero_frames(re, im, mag, 3)
    leak = re.copy()
    leak[0, :, 3] = 1e-7 * ore[0, :, 2]
    with pytest.raises(AssertionError):
        S.check_zero_frames(leak, im, mag, 3)
    with pytest.raises(AssertionError):
        S.check_stft(leak, im, mag, re, im, mag)


def test_table_covers_what_it_is_there_for():
    """Host-side facts the row names rest on (dft_kernels.hip: dft2_factor, the LDS sizes, the 1024-workgroup grid)."""
    def factor(N):
        if N > 2048:
            return 0
        best = 0
        p = 4
        while p * p <= N:
            if N % p == 0:
                best = p
            p += 1
        return best
    for r in S.TABLE:
        assert r.N % 2 == 0 and 16 <= r.N <= 4096 and 1 <= r.hop <= r.N and r.L > r.N // 2, r.id
        assert r.inverse == (r.hop < r.N), r.id
        assert not r.inverse or r.T >= 2, r.id
        if r.N >= 2048:
            assert r.B == 1 and r.T <= 4, r.id
        if r.path.startswith("direct"):
            assert factor(r.N) == 0, r.id
        if r.path.startswith("two-level"):
            P = factor(r.N)
            assert P and f"{P}x{r.N // P}" in r.path, r.id
    by = {r.path: r for r in S.TABLE}
    g = by["two-level-4x4-grid-stride"]
    assert g.B * g.T > 1024
    assert 5 * 2048 * 8 > 64 * 1024 and 3 * 2050 * 8 < 64 * 1024 < 3 * 2732 * 8 and 3 * 2730 * 8 < 64 * 1024
    assert by["direct-2x257-two-blocks"].N // 2 + 1 > 256
    assert {r.L for r in S.TABLE if r.N == 16} >= {9, 40}  # shortest, a multiple of hop
    assert 2730 * 24 <= 64 * 1024 < 2731 * 24 and S.NORM_MAX_FRAMES * 24 == 144 * 1024  # norm_scan_kernel's LDS
