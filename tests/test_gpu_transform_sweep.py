"""fsn_stft / fsn_istft / fsn_stft_ragged / fsn_mask_istft, the streaming pool's frame transforms and fsn_norm held to fp64
over a sweep of the host-side paths.  Needs an MI355X:  python -m pytest tests/test_gpu_transform_sweep.py -m gpu -s

TABLE has one row per path the host code of dft_kernels.hip / fft_kernels.hip can take, named after it: the radix-8 pair
kernels (512 / 256), the two-level kernels (composite n_fft <= 2048: even and odd factor pairs, the grid-stride loop above
1024 frames, 2048 = the one size above 64 KB of LDS), the direct kernels (n_fft = 2 p, 2 * 3 * p and everything above 2048: a
second blockIdx.y block at 514, 64 KB of dynamic LDS crossed at 2732, 96 KB at 4096), hops that do not divide n_fft, hop 1,
n_fft - 1 and n_fft (forward only), the shortest signal the entry accepts, and every kind of iSTFT `length`.

Reference: oracle.fullsubnet_oracle.stft / istft (numpy's fp64 FFT of the fp32 windowed frame; held to torch.stft /
torch.istft at every swept shape by tests/test_transform_sweep_cpu.py).  The iSTFT reference is the oracle at
dtype=float64: nothing of it is rounded to fp32.

Bounds (the project's own or derived; the checkers below are also run on the CPU against wrong stand-ins):
  STFT re / im   <= 1 fp32 ULP of the frame's largest |re|, |im| (test_stft's criterion; an all-zero frame must be exact)
  STFT mag       <= 4 ULP of the largest magnitude (test_stft)
  iSTFT sample whose overlap is complete (every frame that covers it exists) and hop <= n_fft / 2:
                 <= 2e-6 max|ref| (test_istft)
  iSTFT sample covered by fewer frames (the first and last n_fft - hop samples, the last half frame) or hop > n_fft / 2:
                 the quotient acc / env of an fp32 sum of m <= ceil(n_fft / hop) windowed-frame values of size <= A =
                 max|windowed frame| and an fp32 sum of m squared taps.  Each term carries two roundings (irfft -> fp32,
                 x window) <= spacing(A), the m - 1 additions <= spacing(m A) / 2 each, the envelope's 2 m - 1 roundings move
                 the quotient by <= m spacing(m A) / env: together < 4 (m + 1) spacing(float32(m A)) / env_j, plus 2 ULP of
                 the quotient for the division and the final rounding.
  samples at and past n_fft / 2 + hop (T - 1): exactly zero.
Largest ratios to these bounds, oracle at float32 against the oracle at float64 over every row and length of TABLE (CPU,
tests/test_transform_sweep_cpu.py prints them): complete 0.090, derived 0.056.  On an MI355X (-s prints every row): STFT
0.03 ULP at worst (0.00 on most rows: the same fp32 value as the oracle), mag 0.00; fsn_istft complete 0.090, derived 0.056;
fsn_mask_istft (fp32 decompression and mask product included) complete 0.36, derived 0.20; the pool complete 0.27, derived
0.11.  The flat bound's scale is the default-length result of the same spectrum, so that neither a `length` of one sample nor
the last half frame's quotients by a vanishing envelope set it.
The sweep found stft_kernel / pool_analysis_kernel writing ~1e-18 instead of 0 for an all-zero frame packed beside a live one
(impulse-last rows: 8.7e27 "ULP" of a zero frame's scale before, exact zeros since).

Every output is allocated between two NaN guard bands that must survive, every call is made twice - once through the
package's function, once through the C entry into the guarded buffers - and the two must agree bit for bit.
"""
import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 1024  # NaN elements in front of and behind every output
NORM_MAX_FRAMES = 6144  # FSN_NORM_MAX_FRAMES of include/fsn_hip.h


# ---- the table --------------------------------------------------------------------------------------------------------

class Row:
    """One fsn_stft (+ fsn_istft unless inverse=False) shape.  signal: "noise" or one of SIGNALS."""

    def __init__(self, path, N, hop, B, L, inverse=True, signal="noise"):
        self.path, self.N, self.hop, self.B, self.L, self.inverse, self.signal = path, N, hop, B, L, inverse, signal

    @property
    def id(self):
        return f"{self.path}-N{self.N}-h{self.hop}-B{self.B}-L{self.L}" + ("" if self.signal == "noise" else "-" + self.signal)

    @property
    def T(self):
        return 1 + self.L // self.hop


SIGNALS = ("impulse0", "impulse-last", "constant", "alternating")


def _table():
    r = [
        Row("two-level-4x4-shortest", 16, 4, 3, 9),             # L = n_fft / 2 + 1
        Row("two-level-4x4-hop-half", 16, 8, 3, 40),            # L a multiple of hop
        Row("two-level-4x4-grid-stride", 16, 1, 2, 600),        # B T = 1202 frames > 1024 workgroups
        Row("two-level-4x4-hop-n-1", 16, 15, 3, 47),
        Row("two-level-4x4-hop-n", 16, 16, 2, 50, inverse=False),
        Row("direct-2x9", 18, 9, 3, 10),                        # shortest
        Row("direct-2x9-odd-hop", 18, 5, 2, 33),
        Row("direct-2x11", 22, 11, 3, 44),
        Row("direct-2x11-odd-hop", 22, 5, 2, 31),
        Row("direct-2x11-hop-n", 22, 22, 2, 50, inverse=False),
        Row("direct-2x127", 254, 127, 3, 508),
        Row("direct-2x127-odd-hop", 254, 63, 2, 300),
        Row("direct-2x127-hop-n-1", 254, 253, 2, 600),
        Row("direct-2x257-two-blocks", 514, 257, 2, 771),      # F = 258: blockIdx.y = 1 holds one bin
        Row("direct-2x257-two-blocks-quarter", 514, 128, 2, 258),
        Row("two-level-5x6", 30, 15, 3, 16),
        Row("two-level-5x6-odd-hop", 30, 7, 3, 50),
        Row("two-level-5x6-hop-n-1", 30, 29, 2, 100),
        Row("two-level-14x15", 210, 105, 2, 106),
        Row("two-level-14x15-quarter", 210, 52, 2, 333),
        Row("two-level-14x73", 1022, 511, 2, 1022),
        Row("two-level-14x73-quarter", 1022, 255, 1, 700),
        Row("two-level-20x20-odd-hop", 400, 160, 2, 1000),
        Row("two-level-16x32", 512, 128, 2, 1000),
        Row("radix8", 512, 256, 3, 1000),
        Row("radix8-shortest", 512, 256, 2, 257),
        Row("radix8-multiple", 512, 256, 2, 1024),
        Row("radix8-hop-n", 512, 512, 2, 1100, inverse=False),  # not the radix-8 kernels: hop != 256
        Row("two-level-32x64-lds80k", 2048, 512, 1, 1025),
        Row("two-level-32x64-lds80k-half", 2048, 1024, 1, 2048),
        Row("direct-by-size", 2050, 1025, 1, 1026),
        Row("direct-lds-64k", 2732, 683, 1, 1367),
        Row("direct-lds-64k-half", 2732, 1366, 1, 2732),
        Row("direct-lds-96k", 4096, 1024, 1, 2049),
        Row("direct-lds-96k-half", 4096, 2048, 1, 4096),
        Row("direct-lds-96k-hop-n", 4096, 4096, 1, 4100, inverse=False),
    ]
    for s in SIGNALS:
        r.append(Row("radix8", 512, 256, 2, 1000, signal=s))
        r.append(Row("direct-2x127", 254, 127, 2, 508, signal=s))
    return r


TABLE = _table()


def istft_lengths(N, hop, T):
    """`length` of fsn_istft for T frames: the default, 1, an odd value below the default, a value inside the last half
    frame, a value beyond n_fft / 2 + hop (T - 1) (the tail must be zeros)."""
    D = hop * (T - 1)
    out = [None, 1]
    odd = D - 1 if D % 2 == 0 else D - 2
    if odd > 1:
        out.append(odd)
    return out + [D + N // 4, D + N // 2 + 5]


def window_of(N):
    return torch.hann_window(N).numpy()


def make_signal(row):
    if row.signal == "noise":
        return O.make_noisy(row.B, row.L, seed=row.N + 7 * row.hop + row.L)
    y = np.zeros((row.B, row.L), dtype=np.float32)
    if row.signal == "impulse0":
        y[:, 0] = 1.0
    elif row.signal == "impulse-last":
        y[:, -1] = 1.0
    elif row.signal == "constant":
        y[:] = 0.75
    elif row.signal == "alternating":
        y[:, 0::2], y[:, 1::2] = 1.0, -1.0
    return y


def istft_input(re, im):
    """A spectrum that is no STFT of anything (so the overlap-add does not cancel errors): the oracle's, mixed."""
    return (re * np.float32(0.5)).astype(np.float32), (im * np.float32(0.5) + re * np.float32(0.25)).astype(np.float32)


# ---- the checkers (numpy only: tests/test_transform_sweep_cpu.py runs them on stand-ins) -------------------------------

def check_stft(re, im, mag, ore, oim, omag, what=""):
    """-> (worst ULP at frame-max scale, worst |d mag| in units of the 4 ULP bound)."""
    assert re.shape == ore.shape and im.shape == oim.shape and mag.shape == omag.shape, what
    assert np.isfinite(re).all() and np.isfinite(im).all() and np.isfinite(mag).all(), f"{what}: non-finite output"
    fmax = np.maximum(np.abs(ore), np.abs(oim)).max(axis=1, keepdims=True)
    ulp = np.spacing(fmax.astype(np.float32)).astype(np.float64)  # a zero frame: the smallest denormal, i.e. exact zeros
    u = max((np.abs(re.astype(np.float64) - ore) / ulp).max(), (np.abs(im.astype(np.float64) - oim) / ulp).max())
    assert u <= 1.0, f"{what}: {u:.3g} ULP at frame-max scale against the fp64 transform"
    mb = 4.0 * float(np.spacing(np.float32(np.abs(omag).max())))
    mu = float(np.abs(mag.astype(np.float64) - omag).max()) / mb
    assert mu <= 1.0, f"{what}: mag off by {mu:.3g} x (4 ULP of the largest magnitude)"
    return float(u), mu


def istft_bound(fr, fi, N, hop, win, n, ref):
    """Per-sample bound [.., n] for an iSTFT of the spectrum fr / fi [B, F, T] (see the module docstring) and the mask of
    the samples held to the flat 2e-6 bound."""
    T = fr.shape[-1]
    spec = (fr.astype(np.float64) + 1j * fi.astype(np.float64)).transpose(0, 2, 1)
    A = float(np.abs(np.fft.irfft(spec, n=N, axis=-1) * win.astype(np.float64)).max())
    m = -(-N // hop)
    total = N + hop * (T - 1)
    env = np.zeros(max(total, N // 2 + n), dtype=np.float32)
    wsq = (win * win).astype(np.float32)
    for t in range(T):
        env[t * hop: t * hop + N] += wsq
    p = np.arange(n) + N // 2
    env = env[N // 2: N // 2 + n].astype(np.float64)
    complete = (p - N + 1 > -hop) & (p // hop <= T - 1) & (2 * hop <= N)
    # the flat bound is test_istft's, of a whole signal: its scale is the default-length result of the same spectrum - also
    # where `length` keeps one sample of it, and without the last half frame, whose quotients by a vanishing envelope would
    # otherwise set the scale
    whole = O.istft(fr.astype(np.float64), fi.astype(np.float64), N, hop, N, window=win, dtype=np.float64)
    flat = 2e-6 * float(np.abs(whole).max())
    with np.errstate(divide="ignore"):
        derived = 4.0 * (m + 1) * float(np.spacing(np.float32(m * A))) / env
    derived = derived + 2.0 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    bound = np.where(complete, flat, derived)
    bound = np.where(p >= total, 0.0, bound)
    return bound, complete & (p < total)


def check_istft(y, ref, bound, complete, what=""):
    """-> (worst ratio on the flat-bound samples, worst ratio on the derived-bound samples)."""
    assert y.shape == ref.shape, f"{what}: shape {y.shape} != {ref.shape}"
    assert np.isfinite(y).all(), f"{what}: non-finite output"
    err = np.abs(y.astype(np.float64) - ref)
    zero = np.broadcast_to(bound == 0.0, err.shape)
    assert not y[zero].any(), f"{what}: samples past the last frame must be exact zeros"
    ratio = np.where(zero, 0.0, err / np.where(bound == 0.0, 1.0, bound))
    c = np.broadcast_to(complete, err.shape)
    rc = float(ratio[c].max()) if c.any() else 0.0
    rd = float(ratio[~c].max()) if (~c).any() else 0.0
    assert rc <= 1.0, f"{what}: {rc:.3g} x the 2e-6 max|ref| bound"
    assert rd <= 1.0, f"{what}: {rd:.3g} x the derived bound of a partly covered sample"
    return rc, rd


def masked_spectrum64(crm, re, im):
    """inferencer.py:137-140 in fp64: crm [B, 2, F, T] compressed, re / im fp32 -> the enhanced spectrum (fp64)."""
    dm = O.decompress_cIRM(np.asarray(crm, np.float64).transpose(0, 2, 3, 1), dtype=np.float64)
    r, i = re.astype(np.float64), im.astype(np.float64)
    return dm[..., 0] * r - dm[..., 1] * i, dm[..., 1] * r + dm[..., 0] * i


def check_zero_frames(re, im, mag, T_b, what=""):
    """Frames t >= T_b of a ragged row must be exactly zero."""
    for a in (re, im, mag):
        assert not a[..., T_b:].any(), f"{what}: frames past the row's own {T_b} are not exact zeros"


# ---- calling the library ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    return fullsubnet_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """A float32 device tensor of `shape` between two bands of GUARD NaNs (the payload starts as NaN too)."""

    def __init__(self, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)

    def numpy(self, what=""):
        assert bool(torch.isnan(self.buf[:GUARD]).all()), f"{what}: wrote in front of the output"
        assert bool(torch.isnan(self.buf[GUARD + self.n:]).all()), f"{what}: wrote behind the output"
        return self.t.cpu().numpy()


def _nan_workspace(lib, nbytes):
    ws = lib.workspace(nbytes, torch.device("cuda"))
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    return ws


def _win(N):
    from fullsubnet_amd.acoustics import feature
    return feature.hann_window(N, torch.device("cuda", torch.cuda.current_device()))


def stft_twice(fsn, y, N, hop, what):
    """fsn.stft and the C entry into guarded buffers: (re, im, mag) as numpy, equal bit for bit."""
    lib = fsn._lib
    yd = dev(y)
    mag, _, re, im = fsn.stft(yd, N, hop, N, return_phase=False)
    B, L = y.shape
    g = [Guarded((B, N // 2 + 1, 1 + L // hop)) for _ in range(3)]
    lib.check(lib.lib().fsn_stft(lib.dev_ptr(yd), B, L, N, hop, N, lib.dev_ptr(_win(N)), lib.dev_ptr(g[0].t), lib.dev_ptr(g[1].t),
                                 lib.dev_ptr(g[2].t), lib.stream_ptr(yd.device)))
    out = [a.numpy(what) for a in g]
    for a, b in zip(out, (re, im, mag)):
        assert a.shape == tuple(b.shape) and a.tobytes() == b.cpu().numpy().tobytes(), f"{what}: two calls differ"
    return out


def istft_twice(fsn, fr, fi, N, hop, length, what):
    lib = fsn._lib
    rd, idv = dev(fr), dev(fi)
    y1 = fsn.istft((rd, idv), N, hop, N, length=length, input_type="real_imag")
    B, F, T = fr.shape
    n = hop * (T - 1) if length is None else length
    g = Guarded((B, n))
    ws = _nan_workspace(lib, lib.lib().fsn_istft_workspace_bytes(B, T, N))
    lib.check(lib.lib().fsn_istft(lib.dev_ptr(rd), lib.dev_ptr(idv), B, T, N, hop, N, lib.dev_ptr(_win(N)), n, lib.dev_ptr(g.t),
                                  ws.data_ptr(), ws.numel(), lib.stream_ptr(rd.device)))
    y2 = g.numpy(what)
    assert y2.shape == tuple(y1.shape) and y2.tobytes() == y1.cpu().numpy().tobytes(), f"{what}: two calls differ"
    return y2


# ---- fsn_stft / fsn_istft ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", TABLE, ids=[r.id for r in TABLE])
def test_stft_istft_row(fsn, row):
    N, hop = row.N, row.hop
    win = window_of(N)
    y = make_signal(row)
    omag, _, ore, oim = O.stft(y, N, hop, N, window=win)
    assert ore.shape == (row.B, N // 2 + 1, row.T)
    re, im, mag = stft_twice(fsn, y, N, hop, row.id)
    u, mu = check_stft(re, im, mag, ore, oim, omag, row.id)
    print(f"\n{row.id}: stft {u:.2f} ULP at frame max, mag {mu:.2f} of 4 ULP", end="")
    if not row.inverse:
        with pytest.raises(RuntimeError):  # hop == n_fft: the window envelope reaches zero, as torch.istft says
            fsn.istft((dev(ore), dev(oim)), N, hop, N, input_type="real_imag")
        return
    fr, fi = istft_input(ore, oim)
    worst = [0.0, 0.0]
    for length in istft_lengths(N, hop, row.T):
        what = f"{row.id} length {length}"
        ref = O.istft(fr, fi, N, hop, N, length=length, window=win, dtype=np.float64)
        got = istft_twice(fsn, fr, fi, N, hop, length, what)
        bound, complete = istft_bound(fr, fi, N, hop, win, ref.shape[1], ref)
        rc, rd = check_istft(got, ref, bound, complete, what)
        worst = [max(worst[0], rc), max(worst[1], rd)]
    print(f"; istft {worst[0]:.3f} of 2e-6 max|ref|, {worst[1]:.3f} of the derived bound", end="")


@pytest.mark.parametrize("N,hop", [(512, 256), (254, 127)])
def test_istft_ignores_imaginary_dc_and_nyquist(fsn, N, hop):
    win = window_of(N)
    y = O.make_noisy(2, 5 * hop + 3, seed=N)
    _, _, ore, oim = O.stft(y, N, hop, N, window=win)
    fr, fi = istft_input(ore, oim)
    clean = istft_twice(fsn, fr, fi, N, hop, None, "clean")
    fi2 = fi.copy()
    fi2[:, 0, :] = 3.0 + np.arange(fi.shape[-1], dtype=np.float32)
    fi2[:, -1, :] = -2.5
    got = istft_twice(fsn, fr, fi2, N, hop, None, "imaginary DC / Nyquist")
    assert got.tobytes() == clean.tobytes()
    ref = O.istft(fr, fi2, N, hop, N, window=win, dtype=np.float64)
    bound, complete = istft_bound(fr, fi, N, hop, win, ref.shape[1], ref)
    check_istft(got, ref, bound, complete, "imaginary DC / Nyquist")


# ---- ragged rows on the radix-8 kernels ------------------------------------------------------------------------------------

RAGGED = [257, 511, 512, 513, 1024, 1300]  # frames 2, 2, 3, 3, 5, 6 (odd next to even; frame B dead beside a live frame A)


def _ragged_case():
    L_max = max(RAGGED)
    y = O.make_noisy(len(RAGGED), L_max, seed=77)
    for b, Lb in enumerate(RAGGED):
        y[b, Lb:] = np.nan  # never read
    return y, L_max, 1 + L_max // 256


def test_stft_ragged_rows(fsn):
    lib = fsn._lib
    win = window_of(512)
    y, L_max, T = _ragged_case()
    B = len(RAGGED)
    yd, ld = dev(y), torch.tensor(RAGGED, dtype=torch.int32, device="cuda")
    from fullsubnet_amd.acoustics import feature
    mag, re, im = feature.stft_ragged(yd, ld, 512, 256, 512)
    g = [Guarded((B, 257, T)) for _ in range(3)]
    lib.check(lib.lib().fsn_stft_ragged(lib.dev_ptr(yd), ld.data_ptr(), B, L_max, 512, 256, 512, lib.dev_ptr(_win(512)),
                                        lib.dev_ptr(g[0].t), lib.dev_ptr(g[1].t), lib.dev_ptr(g[2].t), lib.stream_ptr(yd.device)))
    out = [a.numpy("stft_ragged") for a in g]
    for a, b in zip(out, (re, im, mag)):
        assert a.tobytes() == b.cpu().numpy().tobytes(), "two calls differ"
    for b, Lb in enumerate(RAGGED):
        Tb = 1 + Lb // 256
        omag, _, ore, oim = O.stft(y[b:b + 1, :Lb], window=win)
        r, i, m = (a[b:b + 1] for a in out)
        u, mu = check_stft(r[..., :Tb], i[..., :Tb], m[..., :Tb], ore, oim, omag, f"row {b} (L {Lb})")
        check_zero_frames(r, i, m, Tb, f"row {b} (L {Lb})")
        print(f"\nragged stft row {b} L {Lb}: {u:.2f} ULP, mag {mu:.2f} of 4 ULP", end="")


def _mask(shape, seed):
    """A compressed cIRM: mostly inside (-9.9, 9.9), some values on and beyond the limit."""
    rng = np.random.default_rng(seed)
    m = (rng.standard_normal(shape) * 4.0).astype(np.float32)
    m.flat[:: 97] = 9.9
    m.flat[5:: 89] = -12.0
    return m


@pytest.mark.parametrize("ragged", [False, True], ids=["rectangular", "lengths"])
def test_mask_istft_rows(fsn, ragged):
    from fullsubnet_amd.acoustics import feature
    lib = fsn._lib
    win = window_of(512)
    if ragged:
        y, L_max, T = _ragged_case()
        lens = RAGGED
    else:
        L_max, lens = 1000, [1000, 1000, 1000]
        y, T = O.make_noisy(3, L_max, seed=78), 1 + L_max // 256
    B = len(lens)
    re, im = np.zeros((B, 257, T), np.float32), np.zeros((B, 257, T), np.float32)
    crm = _mask((B, 2, 257, T), 5)
    for b, Lb in enumerate(lens):
        Tb = 1 + Lb // 256
        _, _, re[b:b + 1, :, :Tb], im[b:b + 1, :, :Tb] = O.stft(y[b:b + 1, :Lb], window=win)
        crm[b, :, :, Tb:] = np.nan  # the mask of frames a row does not have is never read
    ld = torch.tensor(lens, dtype=torch.int32, device="cuda") if ragged else None
    lengths_out = [L_max] if ragged else [L_max, 1, 801, 256 * (T - 1) + 300]
    for length in lengths_out:
        cd, rd, idv = dev(crm), dev(re), dev(im)
        y1 = feature.mask_istft(cd, rd, idv, 512, 256, 512, length, lengths=ld)
        g = Guarded((B, length))
        ws = _nan_workspace(lib, lib.lib().fsn_mask_istft_workspace_bytes(B, T, 512))
        lib.check(lib.lib().fsn_mask_istft(lib.dev_ptr(cd), lib.dev_ptr(rd), lib.dev_ptr(idv), None if ld is None else ld.data_ptr(),
                                           B, 257, T, 512, 256, 512, lib.dev_ptr(_win(512)), length, lib.dev_ptr(g.t), ws.data_ptr(),
                                           ws.numel(), lib.stream_ptr(cd.device)))
        got = g.numpy("mask_istft")
        assert got.tobytes() == y1.cpu().numpy().tobytes(), "two calls differ"
        for b, Lb in enumerate(lens):
            Tb = 1 + Lb // 256
            n = Lb if ragged else length
            er, ei = masked_spectrum64(crm[b:b + 1, :, :, :Tb], re[b:b + 1, :, :Tb], im[b:b + 1, :, :Tb])
            ref = O.istft(er, ei, length=n, window=win, dtype=np.float64)
            bound, complete = istft_bound(er, ei, 512, 256, win, n, ref)
            rc, rd_ = check_istft(got[b:b + 1, :n], ref, bound, complete, f"row {b} (L {Lb}) length {length}")
            assert not got[b, n:].any(), f"row {b}: samples past its own length are not exact zeros"
            print(f"\nmask_istft {'lengths' if ragged else 'rect'} row {b} length {length}: {rc:.3f} of 2e-6 max|ref|, "
                  f"{rd_:.3f} of the derived bound", end="")


# ---- the streaming pool's frame transforms ----------------------------------------------------------------------------------

POOL_KW = dict(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15,
               fb_output_activate_function="ReLU", sb_output_activate_function=False, fb_model_hidden_size=512,
               sb_model_hidden_size=384, weight_init=False, norm_type="cumulative_laplace_norm", num_groups_in_drop_band=1)
POOL_T = 5  # frames 0 .. 4 of every session


def _pool_run(fsn, pool, slots, utts, crms, tails):
    """Every session frame by frame as StreamPool does: analysis of frame t, then synthesis of output frame t - 2 (k = 1;
    negative: the look-ahead columns), the last frame with k = 3 and tail_samples.  -> mags [n, F, T], outs: list of [n, 512]
    per tick and the final [n, 1024]."""
    lib = fsn._lib
    n = len(slots)
    args = pool._state_args()
    sd = torch.tensor(slots, dtype=torch.int32, device="cuda")
    mags, outs = [], []
    for t in range(POOL_T):
        hops = np.stack([np.pad(u, (0, 256), mode="reflect")[256 * t: 256 * (t + 1)] if t == POOL_T - 1 else u[256 * t: 256 * (t + 1)]
                         for u in utts]).astype(np.float32)
        prime = dev(np.stack([u[1:257] for u in utts])) if t == 0 else None
        fno = torch.full((n,), t, dtype=torch.int32, device="cuda")
        g = Guarded((n, 257))
        lib.check(lib.lib().fsn_stream_pool_analysis(*args, sd.data_ptr(), n, lib.dev_ptr(dev(hops)), lib.dev_ptr(prime, "prime", allow_none=True),
                                                     fno.data_ptr(), 512, 256, lib.dev_ptr(_win(512)), lib.dev_ptr(g.t),
                                                     lib.stream_ptr(sd.device)))
        mags.append(g.numpy(f"pool analysis frame {t}"))
        last = t == POOL_T - 1
        k = 3 if last else 1
        m0 = t - 2
        cols = [min(max(m0 + j, 0), POOL_T - 1) for j in range(k)]  # columns of frames < 0 are never read: any mask will do
        crm = np.ascontiguousarray(np.stack([c[:, :, cols] for c in crms]))
        first = torch.full((n,), m0, dtype=torch.int32, device="cuda")
        tl = torch.tensor(tails if last else [-1] * n, dtype=torch.int32, device="cuda")
        go = Guarded((n, (k + 1) * 256))
        ws = _nan_workspace(lib, n * k * 512 * 4)
        lib.check(lib.lib().fsn_stream_pool_synthesis(*args, sd.data_ptr(), n, lib.dev_ptr(dev(crm)), k, first.data_ptr(), tl.data_ptr(),
                                                      512, 256, lib.dev_ptr(_win(512)), lib.dev_ptr(go.t), ws.data_ptr(), ws.numel(),
                                                      lib.stream_ptr(sd.device)))
        outs.append(go.numpy(f"pool synthesis frame {t}"))
    return np.stack(mags, axis=-1), outs


@pytest.mark.parametrize("slots,tails", [([2, 0, 3], [0, 1, 255]), ([2, 9, 0], [-1, 5, 256])],
                         ids=["odd-count", "partner-outside-the-pool"])
def test_stream_pool_transforms(fsn, slots, tails):
    """fsn_stream_pool_analysis / _synthesis hop by hop against the oracle's STFT and masked iSTFT of the whole utterance:
    n = 3 (the last wave has no partner), frame 0 from `prime`, k = 1 and 3, negative first_frame, every kind of
    tail_samples; a slot id outside the pool yields zero rows and touches no record."""
    win = window_of(512)
    capacity = 4
    model = fsn.Model(**POOL_KW).cuda().eval()
    pool = fsn.StreamPool(model, capacity=capacity)
    n = len(slots)
    utts = [O.make_noisy(1, 256 * (POOL_T - 1) + 100 + 17 * i, seed=90 + i)[0] for i in range(n)]
    crms = [_mask((2, 257, POOL_T), 20 + i) for i in range(n)]
    live = [0 <= s < capacity for s in slots]
    idle = [s for s in range(capacity) if s not in slots]
    sb = pool.slot_bytes
    runs = []
    for _ in range(2):
        pool.state.fill_(0xFF)  # every record NaN: the idle ones must stay so, the listed ones are reset
        pool.reset_slots([s for s in slots if 0 <= s < capacity])
        runs.append(_pool_run(fsn, pool, slots, utts, crms, tails))
        for s in idle:
            assert bool((pool.state[s * sb:(s + 1) * sb] == 0xFF).all()), f"record of idle slot {s} was written"
    (mags, outs), (mags2, outs2) = runs
    assert mags.tobytes() == mags2.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(outs, outs2)), "two runs differ"
    for i in range(n):
        if not live[i]:
            assert not mags[i].any() and not any(o[i].any() for o in outs), "a skipped row must be zeros"
            continue
        u = utts[i][None]
        omag, _, ore, oim = O.stft(u, window=win)
        assert omag.shape[-1] == POOL_T
        mb = 4.0 * float(np.spacing(np.float32(omag.max())))
        mu = float(np.abs(mags[i].astype(np.float64) - omag[0]).max()) / mb
        assert mu <= 1.0, f"session {i}: mag off by {mu:.3g} x (4 ULP of the largest magnitude)"
        er, ei = masked_spectrum64(crms[i][None], ore, oim)
        n_out = 256 * (POOL_T - 1) + max(tails[i], 0)
        ref = O.istft(er, ei, length=n_out, window=win, dtype=np.float64)
        # ticks 0 .. 3 emit output frames -2 .. 1 (frames <= 0 emit zeros), the last call frames 2, 3, 4 and the tail
        for t in range(POOL_T - 1):
            assert not outs[t][i, 256:].any(), "tail column of a tick without tail_samples"
            if t - 2 < 1:
                assert not outs[t][i].any(), f"session {i}: output frame {t - 2} emits nothing"
        got = np.concatenate([outs[3][i, :256], outs[4][i, :768], outs[4][i, 768:768 + max(tails[i], 0)]])[None]
        assert not outs[4][i, 768 + max(tails[i], 0):].any(), "past tail_samples"
        bound, complete = istft_bound(er, ei, 512, 256, win, n_out, ref)
        rc, rd = check_istft(got, ref, bound, complete, f"session {i} tail {tails[i]}")
        print(f"\npool session {i} (slot {slots[i]}, tail {tails[i]}): mag {mu:.2f} of 4 ULP, out {rc:.3f} of 2e-6 max|ref|, "
              f"{rd:.3f} of the derived bound", end="")


# ---- fsn_norm ----------------------------------------------------------------------------------------------------------------

NORM_NAMES = ["offline_laplace_norm", "cumulative_laplace_norm", "offline_gaussian_norm", "cumulative_layer_norm",
              "forgetting_norm"]
NORM_SHAPES = [(65537, 1, 1, 2),   # offline norms: one statistic row per sample, past grid.y's 65535
               (1, 65537, 1, 2),   # cumulative norms: dim 1 is folded into the batch
               (1, 1, 3, 2730), (1, 1, 3, 2731), (1, 1, 3, 2732),  # 24 bytes of scan LDS per frame: 64 KB lies between 2730 and 2731
               (1, 2, 2, NORM_MAX_FRAMES),
               (1, 1, 31, 5), (1, 1, 32, 5), (1, 1, 33, 5), (1, 3, 700, 3)]  # parts = 1, 2, many with a ragged last part


@pytest.mark.parametrize("shape", NORM_SHAPES, ids=["x".join(map(str, s)) for s in NORM_SHAPES])
@pytest.mark.parametrize("name", NORM_NAMES)
def test_norm_rows(fsn, name, shape):
    """test_feature_norms_on_the_hip_kernels' yardstick at the shapes that reach fsn_norm's other host paths."""
    from fullsubnet_amd.base_model import BaseModel
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.rand(shape, generator=g) * 3.0 + 0.01
    if name in ("offline_gaussian_norm", "cumulative_layer_norm"):
        x = x - 1.2
    fn = getattr(BaseModel, name)
    want = fn(x.double()).float()
    algebra32 = fn(x.clone())
    xd = x.cuda()
    got = fn(xd)
    assert got.is_cuda and got.shape == x.shape and bool(torch.isfinite(got).all())
    assert torch.equal(got, fn(xd)), "two calls differ"
    scale = want.abs().max().item()
    err = (got.cpu() - want).abs().max().item() / scale
    ref_err = (algebra32 - want).abs().max().item() / scale
    print(f"\n{name} {shape}: HIP vs fp64 algebra {err:.2e} (the reference's fp32 algebra: {ref_err:.2e})", end="")
    assert err <= max(3 * ref_err, 2e-6)


@pytest.mark.parametrize("name", NORM_NAMES)
def test_norm_refuses_more_frames_than_fit(fsn, name):
    """fsn_norm keeps a row's per-frame statistics in LDS: T = FSN_NORM_MAX_FRAMES + 1 is an error, not a wrong result."""
    lib = fsn._lib
    B, C, F, T = 1, 1, 2, NORM_MAX_FRAMES + 1
    x = torch.rand((B, C, F, T), device="cuda") + 0.1
    g = Guarded((B, C, F, T))
    nt = lib.ALL_NORM_TYPES[name]
    ws = _nan_workspace(lib, max(int(lib.lib().fsn_norm_workspace_bytes(nt, B, C, F, T)), 256))
    with pytest.raises(lib.FsnError):
        lib.check(lib.lib().fsn_norm(lib.dev_ptr(x), lib.dev_ptr(g.t), nt, B, C, F, T, 192, 0.0, ws.data_ptr(), ws.numel(),
                                     lib.stream_ptr(x.device)))
    torch.cuda.synchronize()
    assert np.isnan(g.numpy("refused norm")).all(), "a refused call wrote its output"
