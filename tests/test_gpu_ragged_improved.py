"""Improved FullSubNet ragged batches: utterances of different lengths in ONE call (``improved_fullsubnet.Model.forward(y,
lengths=...)``; libfsn_hip's ``fsn_stft_ragged_generic``, ``fsn_istft_ragged``, ``fsn_improved_front_norm_ragged`` and
``fsn_improved_section_input_ragged``).  Row b must be what that utterance alone gives - its own reflection in the STFT, its
own offline norms, its own iSTFT length - and zero past its end; the input past a row's end is NaN throughout and must
never be read.  Every test prints the distances it measures before it asserts (run with -s).
Needs a real MI355X:  python -m pytest tests -m gpu"""
import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O
from oracle import model_family_oracle as MF

pytestmark = pytest.mark.gpu

CONFIGS = {"16k": MF.IMPROVED_16K, "48k": MF.IMPROVED_48K, "769": MF.IMPROVED_48K_769}
# frames 3, 3, 40, 40, 64, 64, 65, 94: the shortest legal row, equal frame counts from different lengths, both sides of the
# gather kernel's 64-frame tile
MIXED_16K = [257, 300, 5000, 5100, 8064, 8191, 8192, 12000]
ORACLE_TOL = 1e-4  # of max |reference row|: the bound tests/test_gpu_family.py holds this model to


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()  # raises if libfsn_hip.so is missing: no fallback
    return fullsubnet_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_models = {}


def build(name, seed=5):
    """Seeded weights through the reference's state_dict names (tests/test_gpu_family.py)."""
    from fullsubnet_amd.improved_fullsubnet import Model
    if (name, seed) not in _models:
        cfg = CONFIGS[name]
        params = MF.make_improved_params(cfg, seed=seed)
        m = Model(**cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        _models[(name, seed)] = (m.cuda().eval(), params)
    return _models[(name, seed)]


def ragged_noisy(lengths, seed):
    """O.make_noisy rows, NaN past each row's end: whatever reads the padding shows in the result."""
    noisy = O.make_noisy(len(lengths), max(lengths), seed=seed)
    for b, n in enumerate(lengths):
        noisy[b, n:] = np.nan
    return noisy


def oracle_row(params, cfg, row):
    """model_family_oracle.improved_fullsubnet_forward on one utterance alone: [n]."""
    return MF.improved_fullsubnet_forward(row[None], params, cfg, window=torch.hann_window(cfg["n_fft"]).numpy())[0, 0]


def check_rows(m, noisy, lengths, got, rows, refs=None):
    """Rows of a ragged call against a single-utterance call of each (and the oracle's rows ``refs[b]`` where given):
    -> (worst share vs the oracle, worst share vs the single-utterance calls); zeros past every end, no NaN."""
    assert got.shape == (len(lengths), 1, noisy.shape[1]) and not torch.isnan(got).any()
    worst_o = worst_s = 0.0
    for b, n in enumerate(lengths):
        assert not got[b, :, n:].any(), (b, n, "not zero past the end")
    for b in rows:
        n = lengths[b]
        with torch.no_grad():
            solo = m(dev(noisy[b:b + 1, :n]))[0, 0]
        scale = float(solo.abs().max())
        if refs is not None and b in refs:
            scale = float(np.abs(refs[b]).max())
            d = float(np.abs(got[b, 0, :n].cpu().numpy() - refs[b]).max()) / scale
            print(f"row {b} (n {n}): {d:.3e} of max|ref| vs the oracle")
            worst_o = max(worst_o, d)
            assert d <= ORACLE_TOL, (b, n, "vs the oracle", d)
        d = float((got[b, 0, :n] - solo).abs().max()) / scale
        print(f"row {b} (n {n}): {d:.3e} of max|ref| vs the single-utterance call")
        worst_s = max(worst_s, d)
        assert d <= 2 * ORACLE_TOL, (b, n, "vs the single-utterance call", d)
    return worst_o, worst_s


# ---- 1. the transforms alone ----------------------------------------------------------------------------------------
# 94 = 2 x 47: no split into two factors above 3, so the plain direct-DFT kernels; the three others take the two-level form
TRANSFORMS = [(512, 128), (960, 480), (1536, 768), (94, 47)]


def transform_lengths(N, hop):
    """The shortest legal row, a whole number of hops and one sample less, an odd length, the longest."""
    return [N // 2 + 1, 3 * hop, 4 * hop - 1, 5 * hop + 7, 9 * hop + 3]


@pytest.mark.parametrize("N,hop", TRANSFORMS)
def test_stft_ragged_rows_are_the_rows_alone(fsn, N, hop):
    from fullsubnet_amd.acoustics.feature import stft, stft_ragged
    lengths = transform_lengths(N, hop)
    y = dev(ragged_noisy(lengths, seed=N))
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    mag, re, im = stft_ragged(y, lens, N, hop, N)
    T = 1 + max(lengths) // hop
    assert mag.shape == re.shape == im.shape == (len(lengths), N // 2 + 1, T)
    for b, n in enumerate(lengths):
        t = 1 + n // hop
        m1, _, r1, i1 = stft(y[b:b + 1, :n].contiguous(), N, hop, N, return_phase=False)
        for got, want, what in ((re, r1, "real"), (im, i1, "imag"), (mag, m1, "mag")):
            assert torch.equal(got[b, :, :t], want[0]), (b, n, what)  # the same kernel arithmetic: the same bits
            assert not got[b, :, t:].any(), (b, n, what, "frames past the end are not exact zeros")
    # equal lengths: the bits of fsn_stft
    full = dev(O.make_noisy(3, max(lengths), seed=N + 1))
    eq = stft_ragged(full, torch.full((3,), max(lengths), dtype=torch.int32, device="cuda"), N, hop, N)
    m0, _, r0, i0 = stft(full, N, hop, N, return_phase=False)
    assert torch.equal(eq[0], m0) and torch.equal(eq[1], r0) and torch.equal(eq[2], i0)


def test_stft_ragged_generic_at_512_256_holds_the_radix8_bound(fsn):
    """The generic entry at 512 / 256 (the radix-8 kernels' lengths path): each row within 1 ULP at frame-max scale of the
    fp64 transform of the fp32 windowed frame, its magnitude within 4 ULP of the largest - the bound of
    tests/test_gpu_transform_sweep.py - and the same bits as fsn_stft_ragged."""
    from fullsubnet_amd.acoustics.feature import hann_window, stft_ragged
    lib = fsn._lib
    lengths = [257, 511, 512, 513, 1024, 1300]
    noisy = ragged_noisy(lengths, seed=77)
    y, lens = dev(noisy), torch.tensor(lengths, dtype=torch.int32, device="cuda")
    B, L_max, T = len(lengths), max(lengths), 1 + max(lengths) // 256
    out = [torch.full((B, 257, T), float("nan"), device="cuda") for _ in range(3)]
    lib.check(lib.lib().fsn_stft_ragged_generic(lib.dev_ptr(y), lens.data_ptr(), B, L_max, 512, 256, 512,
                                                lib.dev_ptr(hann_window(512, y.device)), lib.dev_ptr(out[0]), lib.dev_ptr(out[1]),
                                                lib.dev_ptr(out[2]), lib.stream_ptr(y.device)))
    mag0, re0, im0 = stft_ragged(y, lens, 512, 256, 512)
    assert torch.equal(out[0], re0) and torch.equal(out[1], im0) and torch.equal(out[2], mag0)
    re, im, mag = (a.cpu().numpy() for a in out)
    win = torch.hann_window(512).numpy()
    for b, n in enumerate(lengths):
        t = 1 + n // 256
        omag, _, ore, oim = O.stft(noisy[b:b + 1, :n], window=win)
        fmax = np.maximum(np.abs(ore), np.abs(oim)).max(axis=1, keepdims=True)
        ulp = np.spacing(fmax.astype(np.float32)).astype(np.float64)
        u = max((np.abs(re[b:b + 1, :, :t].astype(np.float64) - ore) / ulp).max(),
                (np.abs(im[b:b + 1, :, :t].astype(np.float64) - oim) / ulp).max())
        mu = float(np.abs(mag[b:b + 1, :, :t].astype(np.float64) - omag).max()) / (4.0 * float(np.spacing(np.float32(omag.max()))))
        assert u <= 1.0 and mu <= 1.0, (b, n, u, mu)
        assert not re[b, :, t:].any() and not im[b, :, t:].any() and not mag[b, :, t:].any(), (b, n)


@pytest.mark.parametrize("N,hop", TRANSFORMS)
def test_istft_ragged_rows_are_the_rows_alone(fsn, N, hop):
    from fullsubnet_amd.acoustics.feature import istft, istft_ragged, stft_ragged
    lengths = transform_lengths(N, hop)
    y = dev(ragged_noisy(lengths, seed=N + 2))
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    _, re, im = stft_ragged(y, lens, N, hop, N)
    # a spectrum that is no STFT of anything (the overlap-add does not cancel errors), NaN past each row's own frames
    fr, fi = re * 0.5, im * 0.5 + re * 0.25
    for b, n in enumerate(lengths):
        fr[b, :, 1 + n // hop:] = float("nan")
        fi[b, :, 1 + n // hop:] = float("nan")
    got = istft_ragged((fr, fi), lens, N, hop, N, max(lengths))
    assert got.shape == (len(lengths), max(lengths)) and not torch.isnan(got).any()
    for b, n in enumerate(lengths):
        t = 1 + n // hop
        want = istft((fr[b:b + 1, :, :t].contiguous(), fi[b:b + 1, :, :t].contiguous()), N, hop, N, length=n,
                     input_type="real_imag")
        assert torch.equal(got[b, :n], want[0]), (b, n)
        assert not got[b, n:].any(), (b, n, "samples past the end are not exact zeros")
        assert float(want.abs().max()) > 0
    # equal lengths: the bits of fsn_istft
    L = max(lengths)
    full = dev(O.make_noisy(3, L, seed=N + 3))
    same = torch.full((3,), L, dtype=torch.int32, device="cuda")
    _, r0, i0 = stft_ragged(full, same, N, hop, N)
    r0, i0 = r0 * 0.5, i0 * 0.5 + r0 * 0.25
    assert torch.equal(istft_ragged((r0, i0), same, N, hop, N, L), istft((r0, i0), N, hop, N, length=L, input_type="real_imag"))


# ---- 2. mixed lengths: every row equals its utterance alone ---------------------------------------------------------------
def test_mixed_lengths_at_16k_match_the_oracle_and_single_utterance_calls(fsn):
    m, params = build("16k")
    noisy = ragged_noisy(MIXED_16K, seed=8)
    assert [1 + n // 128 for n in MIXED_16K] == [3, 3, 40, 40, 64, 64, 65, 94]
    y = dev(noisy)
    with torch.no_grad():
        assert m._ragged_on_kernels(y, None)
        got = m(y, lengths=MIXED_16K)
        again = m(y.unsqueeze(1), lengths=torch.tensor(MIXED_16K))
    assert torch.equal(got, again)
    refs = {b: oracle_row(params, CONFIGS["16k"], noisy[b, :n]) for b, n in enumerate(MIXED_16K)}
    worst = check_rows(m, noisy, MIXED_16K, got, range(len(MIXED_16K)), refs)
    print(f"16 kHz mixed lengths: worst {worst[0]:.3e} vs the oracle, {worst[1]:.3e} vs single-utterance calls")


def test_mixed_lengths_at_48k_on_the_one_launch_plan(fsn):
    from fullsubnet_amd.sequence_model import multi_plan
    m, params = build("48k")
    cfg = CONFIGS["48k"]
    rng = np.random.default_rng(48)
    lengths = [int(v) for v in rng.integers(481, 9601, size=32)]
    lengths[3], lengths[17], lengths[30] = 481, 9600, 960  # two frames, the longest, a whole number of hops
    assert min(lengths) == 481 and max(lengths) == 9600
    sb = m.sb_model
    widths = [(sc + 2 * sn) + (fc + 2 * fn) for sc, sn, fc, fn in
              zip(sb.sb_num_center_freqs, sb.sb_num_neighbor_freqs, sb.fb_num_center_freqs, sb.fb_num_neighbor_freqs)]
    T = 1 + 9600 // cfg["hop_length"]
    assert multi_plan(list(sb.sb_models), [(32 * n, w, T) for n, w in zip(sb.num_units(480), widths)]), \
        "this shape is meant to take the one-launch plan of the band sections"
    assert m._persistent_chunk(32, T) is None
    noisy = ragged_noisy(lengths, seed=9)
    with torch.no_grad():
        got = m(dev(noisy), lengths=lengths)
    pick = [3, 17, 30, 0, 31, int(np.argsort(lengths)[16])]
    refs = {b: oracle_row(params, cfg, noisy[b, :lengths[b]]) for b in pick}
    worst = check_rows(m, noisy, lengths, got, range(32), refs)
    print(f"48 kHz mixed lengths: worst {worst[0]:.3e} vs the oracle (six rows), {worst[1]:.3e} vs single-utterance calls")


def test_a_batch_beyond_one_persistent_launch_slices_lengths_with_the_rows(fsn):
    """The batch of tests/test_gpu_family.py's chunk test (40 utterances at 48 kHz, 31 frames): forward runs it as chunks of
    ``_persistent_chunk`` rows and every row reads its own length - bit for bit the ragged call on its chunk alone."""
    m, _ = build("48k", seed=2)
    B, L = 40, 14400
    T = 1 + L // CONFIGS["48k"]["hop_length"]
    c = m._persistent_chunk(B, T)
    assert c is not None and B > c, c
    rng = np.random.default_rng(40)
    lengths = [int(v) for v in rng.integers(481, L + 1, size=B)]
    lengths[c - 1], lengths[c], lengths[0] = 500, L, L  # a short row before the boundary, the longest right after it
    noisy = ragged_noisy(lengths, seed=77)
    y = dev(noisy)
    with torch.no_grad():
        whole = m(y, lengths=lengths)
        assert whole.shape == (B, 1, L) and not torch.isnan(whole).any()
        for i in range(0, B, c):
            part = m(y[i:i + c], lengths=lengths[i:i + c])
            assert torch.equal(whole[i:i + c], part), i
    for b, n in enumerate(lengths):
        assert not whole[b, :, n:].any() and float(whole[b, :, :n].abs().max()) > 0, b


# ---- 3. equal lengths: bit-identical to the call without them -----------------------------------------------------------
@pytest.mark.parametrize("name,B,L", [("16k", 3, 5000), ("48k", 3, 9600), ("769", 3, 15000), ("48k", 32, 9600)])
def test_equal_lengths_are_bit_identical(fsn, name, B, L):
    m, _ = build(name)
    y = dev(O.make_noisy(B, L, seed=B + L))
    with torch.no_grad():
        assert m._ragged_on_kernels(y, None)
        want = m(y)
        for lengths in ([L] * B, torch.full((B,), L, dtype=torch.int64)):
            assert torch.equal(m(y, lengths=lengths), want)
    assert want.shape == (B, 1, L) and float(want.abs().max()) > 0


# ---- 4. configurations without a single-call form run row by row --------------------------------------------------------
def _row_by_row(m, noisy, lengths):
    y = dev(noisy)
    with torch.no_grad():
        assert not m._ragged_on_kernels(y, None)
        got = m(y, lengths=lengths)
        assert got.shape == (len(lengths), 1, noisy.shape[1]) and not torch.isnan(got).any()
        for b, n in enumerate(lengths):
            solo = m(dev(noisy[b:b + 1, :n]))
            assert torch.equal(got[b:b + 1, :, :n], solo), (b, n)
            assert not got[b, :, n:].any() and float(solo.abs().max()) > 0, (b, n)


def test_tensor_algebra_glue_runs_row_by_row(fsn):
    m, _ = build("16k")
    lengths = [300, 5000, 3111]
    m.glue_kernels = False
    try:
        _row_by_row(m, ragged_noisy(lengths, seed=12), lengths)
    finally:
        m.glue_kernels = True


def test_gru_model_runs_row_by_row(fsn):
    from fullsubnet_amd.improved_fullsubnet import Model
    torch.manual_seed(4)
    m = Model(**dict(CONFIGS["16k"], sequence_model="GRU")).cuda().eval()
    lengths = [300, 5000, 3111]
    _row_by_row(m, ragged_noisy(lengths, seed=13), lengths)
