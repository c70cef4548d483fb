"""Ragged batches: utterances of different lengths enhanced in ONE call (``Model.enhance(noisy, lengths=...)``, libfsn_hip
``fsn_enhance_ragged``).  Row b of the result must be what enhancing ``noisy[b, :lengths[b]]`` alone gives - the STFT
reflecting at the row's own end, the offline norm's means over the row's own frames, the iSTFT over its own frames - and
zero past the row's end.  Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O

pytestmark = pytest.mark.gpu

MODEL_KW = dict(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15,
                fb_output_activate_function="ReLU", sb_output_activate_function=False, fb_model_hidden_size=512,
                sb_model_hidden_size=384, weight_init=False)
NORMS = ["offline_laplace_norm", "cumulative_laplace_norm"]
# the shortest legal length (two frames, all reflect padding), hop multiples and their neighbours, two lengths with the
# same frame count (4100 and 4351: 17 frames) and a 3 s utterance
MIXED = [257, 300, 4096, 4097, 5003, 4100, 4351, 48000]
CRM_TOL, ENH_TOL = 1e-4, 2e-3  # the north-star bounds of tests/test_gpu_parity.py


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


def build_model(fsn, norm_type, seed_w=5):
    """As tests/test_gpu_parity.py:build_model (seeded weights through the reference's state_dict names)."""
    key = (norm_type, seed_w)
    if key not in _models:
        params = O.make_params(seed=seed_w, gain=2.0, mask_gain=24.0)
        m = fsn.Model(norm_type=norm_type, num_groups_in_drop_band=1, **MODEL_KW)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
        _models[key] = (m.cuda().eval(), params)
    return _models[key]


def ragged_noisy(lengths, seed):
    """[B, max(lengths)] with row b's utterance in its first lengths[b] samples, zeros behind it."""
    noisy = O.make_noisy(len(lengths), max(lengths), seed=seed)
    for b, n in enumerate(lengths):
        noisy[b, n:] = 0.0
    return noisy


def frames(n):
    return 1 + n // 256


_oracle = {}


def oracle_row(params, norm, noisy_row, key):
    if key not in _oracle:
        ref, inter = O.full_band_crm_mask(noisy_row[None], params, window=torch.hann_window(512).numpy(),
                                          return_intermediates=True, norm_type=norm)
        _oracle[key] = (ref[0], inter["crm"][0])
    return _oracle[key]


def row_errors(enh, crm, ref_enh, ref_crm, n):
    """(max |d crm| over the row's frames, max |d enhanced| / peak over its samples)."""
    t = frames(n)
    peak = max(float(np.abs(ref_enh).max()), 1e-6)
    return float(np.abs(crm[:, :, :t] - ref_crm).max()), float(np.abs(enh[:n] - ref_enh).max()) / peak


def check_ragged_batch(model, params, norm, noisy, lengths, oracle, tag):
    enh, crm = model.enhance(dev(noisy), lengths=lengths, return_crm=True)
    B, L = noisy.shape
    assert enh.shape == (B, L) and crm.shape == (B, 2, 257, frames(L))
    enh, crm = enh.cpu().numpy(), crm.cpu().numpy()
    for b, n in enumerate(lengths):
        t = frames(n)
        assert np.all(enh[b, n:] == 0), (b, n)
        assert np.all(crm[b, :, :, t:] == 0), (b, n)
        solo_e, solo_c = model.enhance(dev(noisy[b:b + 1, :n]), return_crm=True)
        dc, de = row_errors(enh[b], crm[b], solo_e[0].cpu().numpy(), solo_c[0].cpu().numpy(), n)
        assert dc <= CRM_TOL and de <= ENH_TOL, (tag, b, n, "vs single-utterance enhance", dc, de)
        if oracle:
            ref_e, ref_c = oracle_row(params, norm, noisy[b, :n], (norm, tag, b, n))
            dc, de = row_errors(enh[b], crm[b], ref_e, ref_c, n)
            assert dc <= CRM_TOL and de <= ENH_TOL, (tag, b, n, "vs oracle", dc, de)


# ---- 1. equal lengths: bit-identical to the rectangular call ---------------------------------------
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("B,L", [(3, 3000), (8, 5003), (64, 16000)])
def test_equal_lengths_are_bit_identical(fsn, norm, B, L):
    model, _ = build_model(fsn, norm)
    noisy = dev(O.make_noisy(B, L, seed=B))
    enh, crm = model.enhance(noisy, return_crm=True)
    for lengths in ([L] * B, torch.full((B,), L, dtype=torch.int64)):
        enh_r, crm_r = model.enhance(noisy, lengths=lengths, return_crm=True)
        assert torch.equal(enh_r, enh) and torch.equal(crm_r, crm)


# ---- 2. every row equals its utterance enhanced alone ----------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("lengths", [[257, 4097, 4351, 48000], [300, 5003, 4100], [4096, 257], MIXED],
                         ids=["B4", "B3", "B2", "B8-group"])
def test_rows_match_their_utterance_alone_vs_oracle(fsn, norm, lengths):
    """Few-row plans (B <= 5: the wavefront of per-step launches) and the group-kernel plan (B = 8), against the CPU
    oracle on each utterance alone and against the library's own single-utterance call."""
    model, params = build_model(fsn, norm)
    noisy = ragged_noisy(lengths, seed=len(lengths))
    check_ragged_batch(model, params, norm, noisy, lengths, oracle=True, tag=f"B{len(lengths)}")


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("B", [24, 64])
def test_rows_match_their_utterance_alone_on_the_persistent_pair(fsn, norm, B):
    """1 - 4 s utterances on the persistent recurrent kernels (24: 16 + 8 core calls, 64: one round), against the
    library's single-utterance calls."""
    model, params = build_model(fsn, norm)
    rng = np.random.default_rng(B)
    lengths = [int(v) for v in rng.integers(16000, 64001, size=B)]
    lengths[1] = 64000
    noisy = ragged_noisy(lengths, seed=100 + B)
    check_ragged_batch(model, params, norm, noisy, lengths, oracle=False, tag=f"B{B}")


def test_rows_match_when_the_batch_runs_as_several_core_calls(fsn):
    """A batch that the library splits into two or more calls of the model core (fsn_debug_core_chunks): each chunk
    reads its own rows' lengths."""
    from fullsubnet_amd import _lib
    model, params = build_model(fsn, "offline_laplace_norm")
    sizes = (ctypes.c_int * 80)()
    B = next((b for b in (10, 24, 40, 96) if _lib.lib().fsn_debug_core_chunks(ctypes.byref(model._cfg), b, sizes, 80) >= 2),
             None)
    assert B is not None, "no batch size runs as several core calls on this device"
    rng = np.random.default_rng(7)
    lengths = [int(v) for v in rng.integers(257, 12001, size=B)]
    lengths[-1] = 12000  # a short row at the end of the last chunk, the longest in it
    lengths[0] = 300
    noisy = ragged_noisy(lengths, seed=77)
    check_ragged_batch(model, params, "offline_laplace_norm", noisy, lengths, oracle=False, tag=f"chunks{B}")


# ---- 3. negative control: zero-padding without lengths is NOT the same -------------------------------
@pytest.mark.parametrize("norm", NORMS)
def test_zero_padding_without_lengths_exceeds_the_bounds(fsn, norm):
    """The rectangular call on the zero-padded batch reflects at the padded end, averages the offline norm over frames
    the utterance does not have and divides the tail by an envelope with a frame too many: every short row falls
    outside the bounds test 2 holds the ragged call to."""
    model, params = build_model(fsn, norm)
    noisy = ragged_noisy(MIXED, seed=len(MIXED))
    enh, crm = model.enhance(dev(noisy), return_crm=True)
    enh, crm = enh.cpu().numpy(), crm.cpu().numpy()
    for b, n in enumerate(MIXED):
        if n == max(MIXED):
            continue
        ref_e, ref_c = oracle_row(params, norm, noisy[b, :n], (norm, "B8", b, n))
        dc, de = row_errors(enh[b], crm[b], ref_e, ref_c, n)
        assert dc > CRM_TOL or de > ENH_TOL, (b, n, dc, de)


# ---- 4. input past a row's end is never read -------------------------------------------------------
@pytest.mark.parametrize("norm", NORMS)
def test_input_past_the_end_is_ignored(fsn, norm):
    model, _ = build_model(fsn, norm)
    noisy = ragged_noisy(MIXED, seed=4)
    enh, crm = model.enhance(dev(noisy), lengths=MIXED, return_crm=True)
    junk = noisy.copy()
    rng = np.random.default_rng(0)
    for b, n in enumerate(MIXED):
        junk[b, n:] = rng.standard_normal(junk.shape[1] - n).astype(np.float32) * 1e3
    enh_j, crm_j = model.enhance(dev(junk), lengths=MIXED, return_crm=True)
    assert torch.equal(enh_j, enh) and torch.equal(crm_j, crm)


# ---- 5. determinism, validation, composed configurations -------------------------------------------
def test_two_calls_are_bit_identical(fsn):
    model, _ = build_model(fsn, "offline_laplace_norm")
    noisy = dev(ragged_noisy(MIXED, seed=5))
    a = model.enhance(noisy, lengths=MIXED, return_crm=True)
    b = model.enhance(noisy, lengths=MIXED, return_crm=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_bad_lengths_raise_before_any_launch(fsn, monkeypatch):
    from fullsubnet_amd import _lib
    model, _ = build_model(fsn, "offline_laplace_norm")
    noisy = dev(ragged_noisy([3000, 2000], seed=6))

    def no_library():
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "lib", no_library)
    for bad in ([3000], [3000, 2000, 1000], [3000, 256], [3000, 0], [3001, 2000], [3000, 2000.5], [3000.0, 2000],
                torch.tensor([3000.0, 2000.0]), torch.tensor([[3000, 2000]]), [True, 2000], "ab"):
        with pytest.raises(ValueError):
            model.enhance(noisy, lengths=bad)


def test_composed_configuration_equals_its_single_utterance_calls(fsn):
    torch.manual_seed(0)
    m = fsn.Model(num_freqs=257, look_ahead=2, sequence_model="GRU", fb_num_neighbors=0, sb_num_neighbors=15,
                  fb_output_activate_function="ReLU", sb_output_activate_function=False, fb_model_hidden_size=512,
                  sb_model_hidden_size=384, norm_type="offline_laplace_norm", num_groups_in_drop_band=1,
                  weight_init=True).cuda().eval()
    assert not m._fused
    lengths = [4097, 257, 9000]
    noisy = dev(ragged_noisy(lengths, seed=8))
    enh, crm = m.enhance(noisy, lengths=lengths, return_crm=True)
    assert crm.shape == (3, 2, 257, frames(9000))
    for b, n in enumerate(lengths):
        solo_e, solo_c = m.enhance(noisy[b:b + 1, :n], return_crm=True)
        assert torch.equal(enh[b, :n], solo_e[0]) and torch.equal(crm[b, :, :, :frames(n)], solo_c[0])
        assert not enh[b, n:].any() and not crm[b, :, :, frames(n):].any()


# ---- 6. the batched Inferencer loop ----------------------------------------------------------------
def test_batched_inferencer_call_writes_the_files_of_the_one_item_loop(fsn, tmp_path):
    from scipy.io import wavfile
    model, _ = build_model(fsn, "offline_laplace_norm")
    lengths = [16000, 9000, 23000, 4097, 300, 12345]
    noisy = ragged_noisy(lengths, seed=9)
    loader = [(torch.from_numpy(noisy[i:i + 1, :n].copy()), [f"utt{i}"]) for i, n in enumerate(lengths)]
    acoustics = dict(n_fft=512, hop_length=256, win_length=512, sr=16000)
    one = fsn.Inferencer(dict(inferencer=dict(type="full_band_crm_mask", args={}), acoustics=acoustics), model=model,
                         dataloader=loader, output_dir=str(tmp_path / "one"))
    one()
    calls = []
    orig = model.enhance

    def counted(*a, **k):
        calls.append(k.get("lengths"))
        return orig(*a, **k)

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


def test_enhance_utterances_pads_calls_once_and_trims(fsn):
    model, _ = build_model(fsn, "cumulative_laplace_norm")
    lengths = [5003, 257, 30000]
    noisy = ragged_noisy(lengths, seed=10)
    inf = fsn.Inferencer(dict(inferencer=dict(type="full_band_crm_mask", args={}),
                              acoustics=dict(n_fft=512, hop_length=256, win_length=512, sr=16000)), model=model)
    outs = inf.enhance_utterances([torch.from_numpy(noisy[b, :n].copy()) for b, n in enumerate(lengths)])
    batch = inf.enhance_batch(dev(noisy), lengths=lengths)
    assert [o.shape[0] for o in outs] == lengths
    for b, n in enumerate(lengths):
        assert torch.equal(outs[b], batch[b, :n])
