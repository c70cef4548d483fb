"""Fast FullSubNet ragged batches: utterances of different lengths in ONE call (``fast_fullsubnet.Model.forward(mix_mag,
frames=...)``, ``Model.enhance(noisy, lengths=...)``; libfsn_hip's *_ragged glue entries, ``fsn_stft_ragged`` and
``fsn_mask_istft``).  Row b must be what that utterance alone gives - its own look-ahead frames, its own offline norms,
its own last down-sampling block, its own iSTFT - and zero past its end.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import ast
import os

import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O
from oracle import model_family_oracle as MF

pytestmark = pytest.mark.gpu

FAST_KW = dict(look_ahead=2, shrink_size=2, sequence_model="LSTM", num_mels=64, encoder_input_size=257,
               bottleneck_hidden_size=384, bottleneck_num_layers=2, noisy_input_num_neighbors=5,
               encoder_output_num_neighbors=0, norm_type="offline_laplace_norm", weight_init=False)
# the shortest legal length (two frames), the same frame count from several lengths (4096, 4097, 4351: 17 frames), both
# parities of T_b + look_ahead - 1 (17 -> 18, 18 -> 19: a short and a whole last down-sampling block) and 3 s
MIXED = [257, 300, 4096, 4097, 4351, 4352, 5003, 48000]
CRM_TOL, ENH_TOL = 1e-4, 2e-3  # the bounds of tests/test_gpu_ragged.py


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()  # raises if libfsn_hip.so is missing: no fallback
    return fullsubnet_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def frames(n):
    return 1 + n // 256


def golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return z, ast.literal_eval(str(z["meta"]))


_models = {}


def build_fast(seed_w=3, gain=2.0, fb=None):
    """Seeded weights through the reference's state_dict names (tests/test_gpu_family.py); ``fb``: the golden files'
    filterbank, else the model's own."""
    from fullsubnet_amd.fast_fullsubnet import Model
    key = (seed_w, gain, fb is None)
    if key not in _models:
        params = MF.make_fast_params(seed=seed_w, gain=gain)
        m = Model(**FAST_KW)
        sd = {k: torch.from_numpy(v) for k, v in params.items()}
        sd["mel_scale.fb"] = torch.from_numpy(fb) if fb is not None else m.mel_scale.fb.clone()
        m.load_state_dict(sd, strict=True)
        params["mel_scale.fb"] = sd["mel_scale.fb"].numpy()
        _models[key] = (m.cuda().eval(), params)
    return _models[key]


def ragged_noisy(lengths, seed):
    noisy = O.make_noisy(len(lengths), max(lengths), seed=seed)
    for b, n in enumerate(lengths):
        noisy[b, n:] = 0.0
    return noisy


def oracle_crm(params, row):
    """model_family_oracle.fast_fullsubnet_forward on fullsubnet_oracle.stft of one utterance alone: [2, F, T_b]."""
    mag = O.stft(row[None], window=torch.hann_window(512).numpy())[0]
    return MF.fast_fullsubnet_forward(mag[:, None], params)[0]


def check_vs_solo(model, noisy, lengths, enh, crm, rows):
    """Rows of a ragged enhance against a single-utterance enhance of each: mask and waveform bounds, zeros past the end."""
    for b in rows:
        n, t = lengths[b], frames(lengths[b])
        assert not enh[b, n:].any() and not crm[b, :, :, t:].any(), b
        solo_e, solo_c = model.enhance(dev(noisy[b:b + 1, :n]), return_crm=True)
        solo_e, solo_c = solo_e[0].cpu().numpy(), solo_c[0].cpu().numpy()
        dc = float(np.abs(crm[b, :, :, :t] - solo_c).max())
        de = float(np.abs(enh[b, :n] - solo_e).max()) / max(float(np.abs(solo_e).max()), 1e-6)
        assert dc <= CRM_TOL and de <= ENH_TOL, (b, n, "vs single-utterance enhance", dc, de)


# ---- 1. reference-held: golden rows of 32 and 33 frames in one NaN-padded batch -----------------------
def test_forward_with_frames_holds_the_reference_rows(fsn, golden_dir):
    """The rows of fast_b3_odd (32 frames: T + look_ahead - 1 = 33, a short last down-sampling block) and fast_b2_even (33
    frames: a whole last block) in one [5, 1, 257, 33] batch, NaN past each row's end.  The two files hold different
    weights, so the batch runs once under each file's weights and each row is held to its own file's reference mask."""
    odd, m_odd = golden(golden_dir, "fast_b3_odd")
    even, m_even = golden(golden_dir, "fast_b2_even")
    mag = np.full((5, 1, 257, 33), np.nan, dtype=np.float32)
    mag[:3, 0, :, :32] = odd["mag"]
    mag[3:, 0, :, :] = even["mag"]
    lens = [32, 32, 32, 33, 33]
    for z, meta, rows in ((odd, m_odd, range(3)), (even, m_even, range(3, 5))):
        model, _ = build_fast(meta["seed_w"], meta["gain"], fb=z["fb"])
        with torch.no_grad():
            crm = model(dev(mag), frames=lens).cpu().numpy()
        assert crm.shape == (5, 2, 257, 33) and not np.isnan(crm).any()
        for b, r in zip(rows, range(len(rows))):
            d = float(np.abs(crm[b, :, :, :lens[b]] - z["crm"][r]).max())
            assert d <= CRM_TOL, (b, d)
        for b, t in enumerate(lens):
            assert np.all(crm[b, :, :, t:] == 0), b


# ---- 2. equal lengths: bit-identical to the call without them --------------------------------------
@pytest.mark.parametrize("B", [3, 64, 128, 256])
def test_equal_frames_and_lengths_are_bit_identical(fsn, B):
    """B = 3: per-step bottleneck launches; 64 / 128: the persistent kernels; 256: their fused output layer."""
    model, _ = build_fast()
    L = 8000
    noisy = dev(O.make_noisy(B, L, seed=B))
    mag = fsn.stft(noisy, 512, 256, 512)[0].unsqueeze(1)
    with torch.no_grad():
        crm = model(mag)
        for fr in ([frames(L)] * B, torch.full((B,), frames(L), dtype=torch.int64)):
            assert torch.equal(model(mag, frames=fr), crm)
    enh, crm_e = model.enhance(noisy, return_crm=True)
    assert torch.equal(crm_e, crm)
    enh_r, crm_r = model.enhance(noisy, lengths=[L] * B, return_crm=True)
    assert torch.equal(enh_r, enh) and torch.equal(crm_r, crm)


# ---- 3. mixed lengths: every row equals its utterance alone -----------------------------------------
def test_mixed_lengths_match_the_oracle_and_single_utterance_calls(fsn):
    model, params = build_fast()
    noisy = ragged_noisy(MIXED, seed=8)
    enh, crm = model.enhance(dev(noisy), lengths=MIXED, return_crm=True)
    B, L = noisy.shape
    assert enh.shape == (B, L) and crm.shape == (B, 2, 257, frames(L))
    enh, crm = enh.cpu().numpy(), crm.cpu().numpy()
    for b, n in enumerate(MIXED):
        d = float(np.abs(crm[b, :, :, :frames(n)] - oracle_crm(params, noisy[b, :n])).max())
        assert d <= CRM_TOL, (b, n, "vs oracle", d)
    check_vs_solo(model, noisy, MIXED, enh, crm, range(B))


# ---- 4. many rows, and a batch that forward runs in chunks ----------------------------------------
def _many(B, seed):
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in rng.integers(32000, 64001, size=B)]
    return lengths, ragged_noisy(lengths, seed=100 + seed)


@pytest.mark.parametrize("B", [64, 128, 256])
def test_many_rows_match_the_oracle(fsn, B):
    model, params = build_fast()
    lengths, noisy = _many(B, B)
    enh, crm = model.enhance(dev(noisy), lengths=lengths, return_crm=True)
    enh, crm = enh.cpu().numpy(), crm.cpu().numpy()
    pick = sorted({0, B - 1, int(np.argmin(lengths)), int(np.argmax(lengths))})
    for b in pick:
        n = lengths[b]
        d = float(np.abs(crm[b, :, :, :frames(n)] - oracle_crm(params, noisy[b, :n])).max())
        assert d <= CRM_TOL, (B, b, n, d)
    check_vs_solo(model, noisy, lengths, enh, crm, pick)


def test_chunked_batch_slices_frames_with_the_rows(fsn):
    """A batch of 1.5 x the chunk ``forward`` computes from the device runs as two forwards; rows on both sides of the
    chunk boundary read their own frames."""
    model, params = build_fast()
    chunk = torch.cuda.get_device_properties(0).multi_processor_count * 4 * 16 // model.num_mels
    B = chunk + chunk // 2
    lengths, noisy = _many(B, 7)
    lengths[chunk - 1], lengths[chunk] = 32003, 64000  # a short row before the boundary, the longest right after it
    noisy = ragged_noisy(lengths, seed=107)
    enh, crm = model.enhance(dev(noisy), lengths=lengths, return_crm=True)
    enh, crm = enh.cpu().numpy(), crm.cpu().numpy()
    for b in (0, chunk - 1, chunk, B - 1):
        n = lengths[b]
        d = float(np.abs(crm[b, :, :, :frames(n)] - oracle_crm(params, noisy[b, :n])).max())
        assert d <= CRM_TOL, (B, b, n, d)
        assert not crm[b, :, :, frames(n):].any() and not enh[b, n:].any()


# ---- 5. negative control: zero-padding without lengths is NOT the same -------------------------------
def test_zero_padding_without_lengths_exceeds_the_bounds(fsn):
    model, params = build_fast()
    noisy = ragged_noisy(MIXED, seed=8)
    enh, crm = model.enhance(dev(noisy), return_crm=True)
    enh, crm = enh.cpu().numpy(), crm.cpu().numpy()
    for b, n in enumerate(MIXED):
        if n == max(MIXED):
            continue
        solo_e = model.enhance(dev(noisy[b:b + 1, :n]))[0].cpu().numpy()
        dc = float(np.abs(crm[b, :, :, :frames(n)] - oracle_crm(params, noisy[b, :n])).max())
        de = float(np.abs(enh[b, :n] - solo_e).max()) / max(float(np.abs(solo_e).max()), 1e-6)
        assert dc > CRM_TOL or de > ENH_TOL, (b, n, dc, de)


# ---- 6. padding is ignored; two calls agree --------------------------------------------------------
def test_input_past_the_end_is_ignored_and_calls_repeat(fsn):
    model, _ = build_fast()
    noisy = ragged_noisy(MIXED, seed=4)
    enh, crm = model.enhance(dev(noisy), lengths=MIXED, return_crm=True)
    enh2, crm2 = model.enhance(dev(noisy), lengths=MIXED, return_crm=True)
    assert torch.equal(enh, enh2) and torch.equal(crm, crm2)
    junk = noisy.copy()
    rng = np.random.default_rng(0)
    for b, n in enumerate(MIXED):
        junk[b, n:] = rng.standard_normal(junk.shape[1] - n).astype(np.float32) * 1e3
    enh_j, crm_j = model.enhance(dev(junk), lengths=MIXED, return_crm=True)
    assert torch.equal(enh_j, enh) and torch.equal(crm_j, crm)


# ---- 7. bad input raises before anything is launched -----------------------------------------------
def test_bad_lengths_and_frames_raise_before_any_launch(fsn, monkeypatch):
    from fullsubnet_amd import _lib
    model, _ = build_fast()
    noisy = dev(ragged_noisy([3000, 2000], seed=6))
    mag = dev(np.ones((2, 1, 257, 12), dtype=np.float32))
    calls = []

    def no_library():
        calls.append(1)
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "lib", no_library)
    for bad in ([3000], [3000, 2000, 1000], [3000, 256], [3000, 0], [3001, 2000], [3000, 2000.5],
                torch.tensor([3000.0, 2000.0]), torch.tensor([[3000, 2000]]), [True, 2000], "ab"):
        with pytest.raises(ValueError):
            model.enhance(noisy, lengths=bad)
    with torch.no_grad():
        for bad in ([12], [12, 12, 12], [12, 13], [12, 0], [12, -1], [12, 5.0], torch.tensor([12.0, 5.0]), [False, 5]):
            with pytest.raises(ValueError):
                model(mag, frames=bad)
    assert not calls


# ---- 8. the back half alone ------------------------------------------------------------------------
def _aten_back_half(fsn, crm, re, im, length):
    from fullsubnet_amd.acoustics.mask import decompress_cIRM
    m = decompress_cIRM(crm.permute(0, 2, 3, 1))
    return fsn.istft((m[..., 0] * re - m[..., 1] * im, m[..., 1] * re + m[..., 0] * im), 512, 256, 512, length=length,
                     input_type="real_imag")


def test_mask_istft_matches_the_aten_sequence(fsn):
    from fullsubnet_amd.acoustics.feature import mask_istft, stft_ragged
    model, _ = build_fast()
    # rectangular batch
    L = 9000
    noisy = dev(O.make_noisy(3, L, seed=21))
    mag, _, re, im = fsn.stft(noisy, 512, 256, 512)
    with torch.no_grad():
        crm = model(mag.unsqueeze(1))
    got = mask_istft(crm, re, im, 512, 256, 512, L)
    want = _aten_back_half(fsn, crm, re, im, L)
    peak = float(want.abs().max())
    d = float((got - want).abs().max())
    print(f"fsn_mask_istft vs ATen, rectangular: max|d| = {d:.3e} (peak {peak:.3f})")
    assert d <= 1e-6 * peak
    # ragged batch, row by row
    lengths = [4097, 300, 9000]
    x = ragged_noisy(lengths, seed=22)
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    mag, re, im = stft_ragged(dev(x), lens, 512, 256, 512)
    with torch.no_grad():
        crm = model(mag.unsqueeze(1), frames=[frames(n) for n in lengths])
    got = mask_istft(crm, re, im, 512, 256, 512, max(lengths), lengths=lens)
    for b, n in enumerate(lengths):
        t = frames(n)
        m1, _, r1, i1 = fsn.stft(dev(x[b:b + 1, :n]), 512, 256, 512)
        assert torch.equal(mag[b, :, :t], m1[0]) and not mag[b, :, t:].any()
        want = _aten_back_half(fsn, crm[b:b + 1, :, :, :t].contiguous(), r1, i1, n)[0]
        d = float((got[b, :n] - want).abs().max())
        assert d <= 1e-6 * float(want.abs().max()), (b, n, d)
        assert not got[b, n:].any()


# ---- 9. the batched Inferencer loop on the Fast recipe ---------------------------------------------
def test_batched_inferencer_on_the_fast_model(fsn, tmp_path):
    from scipy.io import wavfile
    model, _ = build_fast()
    lengths = [16000, 9000, 23000, 4097, 300, 12345]
    noisy = ragged_noisy(lengths, seed=9)
    loader = [(torch.from_numpy(noisy[i:i + 1, :n].copy()), [f"utt{i}"]) for i, n in enumerate(lengths)]
    acoustics = dict(n_fft=512, hop_length=256, win_length=512, sr=16000)
    one = fsn.Inferencer(dict(inferencer=dict(type="full_band_crm_mask", args={}), acoustics=acoustics), model=model,
                         dataloader=loader, output_dir=str(tmp_path / "one"))
    one()
    calls = []

    def counted(*a, **k):
        calls.append(k.get("lengths"))
        return type(model).enhance(model, *a, **k)

    model.enhance = counted
    try:
        four = fsn.Inferencer(dict(inferencer=dict(type="full_band_crm_mask", args={}, batch_size=4), acoustics=acoustics),
                              model=model, dataloader=loader, output_dir=str(tmp_path / "four"))
        four()
    finally:
        del model.enhance
    assert [len(c) for c in calls] == [4, 2]  # two ragged calls: a full group and the last, partial one
    amp = np.iinfo(np.int16).max
    for i, n in enumerate(lengths):
        _, a = wavfile.read(str(one.enhanced_dir / f"utt{i}.wav"))
        _, b = wavfile.read(str(four.enhanced_dir / f"utt{i}.wav"))
        assert a.shape == b.shape == (n,) and b.dtype == np.int16
        assert np.abs(a.astype(np.int32) - b.astype(np.int32)).max() <= 1 + int(2 * 2e-3 * 0.8 * amp)
        _, na = wavfile.read(str(one.noisy_dir / f"utt{i}.wav"))
        _, nb = wavfile.read(str(four.noisy_dir / f"utt{i}.wav"))
        assert np.array_equal(na, nb) and nb.shape == (n,)
