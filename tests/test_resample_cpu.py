"""The resampler without a GPU: the fp64 numpy reference the kernels are held to (tests/resample_reference.py) against
scipy.signal.resample_poly and firwin, the two designs' frequency responses, the host side of the fsn_resample entries
(length and size queries, refusals, header = exports = bindings), the Inferencer's keys and its length bookkeeping, and
the condition that makes the GPU test's bound meaningful: the fp32 rounding of the reference meets it on every case."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fsn_resample_out_length", "fsn_resample_workspace_bytes", "fsn_resample_taps", "fsn_resample",
           "fsn_debug_resample_plan")
# (sr_in, sr_out): ten ratios from 1/6 to 441/160; nine lengths from 1 to 4099
TABLE_RATIOS = [(6, 1), (3, 1), (2, 1), (8, 5), (441, 160), (3, 2), (2, 3), (1, 2), (1, 3), (160, 441)]
TABLE_LENGTHS = [1, 2, 3, 10, 63, 100, 1000, 4096, 4099]


# ---- the reference ------------------------------------------------------------------------------------------------------
def test_reference_against_scipy_resample_poly():
    signal = pytest.importorskip("scipy.signal")
    worst = 0.0
    for sr_in, sr_out in TABLE_RATIOS:
        u, d = R.ratio(sr_in, sr_out)
        for n in TABLE_LENGTHS:
            x = np.random.default_rng(n + 7 * u + d).standard_normal(n)
            got, want = R.resample(x, sr_in, sr_out), signal.resample_poly(x, u, d)
            assert len(got) == len(want) == R.out_length(n, sr_in, sr_out) == -(-n * u // d), (u, d, n)
            worst = max(worst, float(np.max(np.abs(got - want))))
    print(f"worst |reference - resample_poly| = {worst:.2e}")
    assert worst <= 1e-12


def test_reference_taps_against_firwin():
    signal = pytest.importorskip("scipy.signal")
    for sr_in, sr_out in TABLE_RATIOS:
        u, d = R.ratio(sr_in, sr_out)
        h, H = R.taps(sr_in, sr_out)
        assert H == 10 * max(u, d) and len(h) == 2 * H + 1
        want = signal.firwin(2 * H + 1, 1.0 / max(u, d), window=("kaiser", 5.0))
        assert np.max(np.abs(h / u - want)) <= 1e-15, (u, d)


def test_chosen_positions_equal_the_whole_row():
    for sr_in, sr_out, design in ((3, 1, "scipy"), (1, 3, "sharp"), (441, 160, "scipy"), (160, 441, "sharp"), (1, 1, "scipy")):
        for n in (1, 2, 50, 1000):
            x = R.signal(n, n)
            whole = R.resample(x, sr_in, sr_out, design)
            ks = np.arange(len(whole))
            assert np.max(np.abs(R.resample_at(x, sr_in, sr_out, ks, design) - whole)) <= 1e-14
            s = R.resample(x, sr_in, sr_out, design, absolute=True)
            assert np.max(np.abs(R.resample_at(x, sr_in, sr_out, ks, design, absolute=True) - s)) <= 1e-14
            assert np.all(np.abs(whole) <= s * (1 + 1e-12) + 1e-300)


def test_the_two_designs_at_48_to_16_khz():
    u, d = R.ratio(48000, 16000)
    h, H = R.taps(48000, 16000, "scipy")
    assert len(h) == 61
    at = R.response_db(h, u, [7000.0, 8000.0], 48000)
    past = R.response_db(h, u, np.arange(9000.0, 24001.0, 50.0), 48000)
    print(f"scipy: {at[0]:.2f} dB at 7 kHz, {at[1]:.2f} dB at 8 kHz, at most {past.max():.1f} dB past 9 kHz")
    assert abs(at[1] + 6.0) <= 0.1
    h, H = R.taps(48000, 16000, "sharp")
    assert len(h) == 193
    at = R.response_db(h, u, [7000.0, 8000.0], 48000)
    past = R.response_db(h, u, np.arange(9000.0, 24001.0, 50.0), 48000)
    print(f"sharp: {at[0]:.2f} dB at 7 kHz, {at[1]:.2f} dB at 8 kHz, at most {past.max():.1f} dB past 9 kHz")
    assert at[0] >= -1.0 and past.max() <= -100.0


# ---- the host side of the entries ---------------------------------------------------------------------------------------
def test_header_exports_and_bindings_agree_on_the_resample_entries():
    from fullsubnet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fsn_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert name in _lib.ADDED_IN_118
    assert "#define FSN_ABI_VERSION 118" in src and _lib.ABI_VERSION == 118
    import fullsubnet_amd
    assert fullsubnet_amd.resample.resample and fullsubnet_amd.resample.out_length
    assert fullsubnet_amd.resample.DESIGNS == R.DESIGNS


def test_out_length_is_ceil_without_a_gpu():
    from fullsubnet_amd import _lib, resample
    L = _lib.lib()
    for sr_in, sr_out in TABLE_RATIOS + [(44100, 16000), (16000, 48000), (48000, 48000)]:
        u, d = R.ratio(sr_in, sr_out)
        for n in TABLE_LENGTHS + [0, 2 ** 31 - 1]:
            want = -(-n * u // d)
            assert L.fsn_resample_out_length(n, sr_in, sr_out) == want == resample.out_length(n, sr_in, sr_out), (sr_in, sr_out, n)
    assert L.fsn_resample_out_length(2 ** 31 - 1, 16000, 44100) == -(-(2 ** 31 - 1) * 441 // 160)
    for args in ((10, 0, 16000), (10, 16000, -1), (-1, 16000, 16000)):
        assert L.fsn_resample_out_length(*args) == -1
        assert b"fsn_resample_out_length" in L.fsn_last_error()


def test_size_query_plan_and_refusals_without_a_gpu():
    from fullsubnet_amd import _lib, resample
    L = _lib.lib()
    sizes = [L.fsn_resample_workspace_bytes(48000, 16000, z, 5.0, 1.0) for z in (1, 10, 32, 100)]
    assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3], sizes
    small, large = (L.fsn_resample_workspace_bytes(44100, 16000, *R.DESIGNS[k]) for k in ("scipy", "sharp"))
    assert small >= 2 * 8 * 8821 and large >= 2 * 8 * 28225 and large > 3 * small
    # the 44.1 kHz ratios: 8 821 taps sit in LDS, the 28 225 of "sharp" do not fit
    p = resample.plan(44100, 16000)
    assert (p["up"], p["down"], p["half"], p["taps"], p["taps_in_lds"]) == (160, 441, 4410, 8821, 1)
    assert p["taps_per_phase"] == -(-8821 // 160) and p["tile_outputs"] % 160 == 0
    assert p["tile_inputs"] == p["tile_outputs"] * 441 // 160
    assert p["stretch"] >= (p["tile_outputs"] - 1) * 441 // 160 + p["taps_per_phase"]
    q = resample.plan(44100, 16000, "sharp")
    assert (q["taps"], q["taps_in_lds"]) == (28225, 0)
    assert resample.plan(16000, 44100)["taps_in_lds"] == 1 and resample.plan(16000, 44100, "sharp")["taps_in_lds"] == 0
    for design in R.DESIGNS:
        for sr_in, sr_out in R.RATIOS + [(48000, 16000), (16000, 48000), (8000, 16000), (44100, 48000), (96000, 8000)]:
            p = resample.plan(sr_in, sr_out, design)
            assert 8 * p["row_stride"] * p["up"] * p["taps_in_lds"] + 4 * p["stretch"] <= 160 * 1024
            assert p["stretch"] <= 24576 and p["tile_outputs"] % (8 * p["up"]) == 0

    def size(*a):
        return L.fsn_resample_workspace_bytes(*a)

    for args, word in (((0, 16000, 10, 5.0, 1.0), b"rates must be positive"), ((16000, -5, 10, 5.0, 1.0), b"rates must be positive"),
                       ((48000, 16000, 0, 5.0, 1.0), b"zeros = 0"), ((48000, 16000, 10, -0.5, 1.0), b"beta = -0.5"),
                       ((48000, 16000, 10, 300.0, 1.0), b"beta = 300"), ((48000, 16000, 10, float("inf"), 1.0), b"beta = inf"),
                       ((48000, 16000, 10, 5.0, 0.0), b"rolloff = 0"), ((48000, 16000, 10, 5.0, 1.5), b"rolloff = 1.5"),
                       ((48000, 16000, 10, 5.0, float("nan")), b"rolloff"),
                       ((44101, 16000, 10, 5.0, 1.0), b"at most 4096"), ((4096, 1, 40, 5.0, 1.0), b"at most 262145"),
                       ((4000, 1, 10, 5.0, 1.0), b"stages at most 24576")):
        assert size(*args) == 0, args
        assert word in L.fsn_last_error(), (args, L.fsn_last_error())
    # refused before anything is launched: no device is needed to be told so
    fake = ctypes.c_void_p(256 * 1024)
    other = ctypes.c_void_p(512 * 1024)
    need = size(48000, 16000, 10, 5.0, 1.0)

    def call(x=fake, B=2, L_max=4800, sr_in=48000, sr_out=16000, zeros=10, beta=5.0, rolloff=1.0, y=other, L_out=1600, ws=fake,
             nbytes=need):
        return L.fsn_resample(x, None, B, L_max, sr_in, sr_out, zeros, beta, rolloff, y, L_out, None, ws, nbytes, None)

    for kwargs, word in ((dict(sr_in=0), b"rates must be positive"), (dict(zeros=0), b"zeros = 0"), (dict(beta=-1.0), b"beta = -1"),
                         (dict(rolloff=2.0), b"rolloff = 2"), (dict(sr_in=44101), b"at most 4096"),
                         (dict(L_out=1599), b"L_out_max = 1599"), (dict(B=0), b"B = 0"), (dict(L_max=0), b"L_max = 0"),
                         (dict(x=None), b"NULL pointer"), (dict(y=fake), b"alias"), (dict(ws=None), b"NULL workspace"),
                         (dict(ws=ctypes.c_void_p(256 * 1024 + 8)), b"aligned"), (dict(nbytes=need - 1), b"at least")):
        assert call(**kwargs) == -1, kwargs  # FSN_ERR_ARG
        assert word in L.fsn_last_error(), (kwargs, L.fsn_last_error())
    assert L.fsn_resample_taps(48000, 16000, 10, 5.0, 1.0, fake, 60, None) == -1 and b"61" in L.fsn_last_error()
    assert L.fsn_resample_taps(48000, 16000, 10, 5.0, 1.0, None, 61, None) == -1
    with pytest.raises(_lib.FsnError):
        resample.resample(torch.zeros(2, 4000), 48000, 16000)  # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        resample.design_parameters("soxr")


# ---- the GPU test's cases ------------------------------------------------------------------------------------------------
def test_fp32_rounding_of_the_reference_meets_the_gpu_bound_on_its_cases():
    from fullsubnet_amd import resample
    cases = R.cases(lambda a, b, design: resample.plan(a, b, design)["tile_inputs"])
    assert len(cases) >= 70
    worst = 0.0
    for sr_in, sr_out, design, n, seed in cases:
        x = R.signal(n, seed)
        r = R.resample(x, sr_in, sr_out, design)
        s = R.resample(x, sr_in, sr_out, design, absolute=True)
        err = np.abs(r.astype(np.float32).astype(np.float64) - r)
        assert np.all(err <= R.bound(r, s)), (sr_in, sr_out, design, n)
        nz = np.abs(r) > 1e-30
        worst = max(worst, float(np.max(err[nz] / (2.0 ** -24 * np.abs(r[nz])))) if nz.any() else 0.0)
    print(f"fp32 rounding of the reference: at most {worst:.3f} x 2^-24 |r|")
    assert worst <= 1.0
    # a fp32 accumulation would not: the second term is 2^-40, a fp32 sum of 60 terms errs by about 2^-24 of sum |h| |x|
    assert 2.0 ** -40 < 1e-5 * 2.0 ** -24 * 60


# ---- the Inferencer --------------------------------------------------------------------------------------------------------
def test_inferencer_keys():
    from fullsubnet_amd import Inferencer
    assert Inferencer.resample_keys({}) == (None, "model", "scipy")
    assert Inferencer.resample_keys({"input_sr": 48000, "output_sr": "input", "resample_design": "sharp"}) == (48000, "input", "sharp")
    assert Inferencer.resample_keys({"input_sr": 44100, "output_sr": 22050}) == (44100, 22050, "scipy")
    for bad in ({"input_sr": 0}, {"input_sr": "48000"}, {"input_sr": 48000.0}, {"input_sr": True}, {"output_sr": "same"},
                {"output_sr": -1}, {"output_sr": 16000.5}, {"resample_design": "soxr"}, {"resample_design": 3}):
        with pytest.raises(ValueError, match=r"\[inferencer\]"):
            Inferencer.resample_keys(bad)


def host_inferencer(tmp_path=None, loader=None, **keys):
    """An Inferencer without a device: the model is a stand-in that halves its input."""
    from fullsubnet_amd import Inferencer
    inf = Inferencer.__new__(Inferencer)
    inf.device = torch.device("cpu")
    inf.sr, inf.n_fft, inf.hop_length, inf.win_length = 16000, 512, 256, 512
    inf.inference_config = dict(type="full_band_crm_mask", args={}, **keys)
    inf.segment_frames = None
    inf.fused_call = True
    inf.model = None
    inf.input_sr, inf.output_sr, inf.resample_design = Inferencer.resample_keys(inf.inference_config)
    inf.dataloader = loader
    inf.seen = []

    def model_rate(utterances):
        inf.seen.append([int(u.shape[0]) for u in utterances])
        return [0.5 * u for u in utterances]

    inf._enhance_model_rate = model_rate
    inf.full_band_crm_mask = lambda noisy, args=None: (0.5 * noisy).squeeze(0).numpy()
    if tmp_path is not None:
        inf.enhanced_dir, inf.noisy_dir = tmp_path / "enhanced", tmp_path / "noisy"
        inf.enhanced_dir.mkdir(parents=True)
        inf.noisy_dir.mkdir(parents=True)
    return inf


def reference_resample(y, sr_in, sr_out, lengths=None, design="scipy"):
    """fullsubnet_amd.resample.resample on the host, by the reference."""
    B, L = y.shape
    lengths = [L] * B if lengths is None else list(lengths)
    out = np.zeros((B, R.out_length(L, sr_in, sr_out)), dtype=np.float32)
    for b, n in enumerate(lengths):
        r = R.resample(y[b, :n].numpy(), sr_in, sr_out, design)
        out[b, :len(r)] = r.astype(np.float32)
    return torch.from_numpy(out), torch.tensor([R.out_length(n, sr_in, sr_out) for n in lengths], dtype=torch.int32)


def test_inferencer_round_trip_length_bookkeeping(monkeypatch):
    import fullsubnet_amd
    monkeypatch.setattr(fullsubnet_amd.resample, "resample", reference_resample)
    lengths = [1, 63, 1000, 4099, 9600]
    for sr in (48000, 44100, 8000, 22050):
        utts = [torch.from_numpy(R.signal(n, n + sr)) for n in lengths]
        inf = host_inferencer()
        model = [R.out_length(n, sr, 16000) for n in lengths]
        back = inf.enhance_utterances(utts, sr=sr, output_sr="input", design="sharp")
        assert inf.seen == [model] and [int(o.shape[0]) for o in back] == lengths
        at_model = inf.enhance_utterances(utts, sr=sr)
        assert [int(o.shape[0]) for o in at_model] == model
        other = inf.enhance_utterances(utts, sr=sr, output_sr=24000)
        assert [int(o.shape[0]) for o in other] == [R.out_length(n, sr, 24000) for n in lengths]
        # the values: the stand-in halves, so the round trip is the two filters applied to half the input
        for u, o, n in zip(utts, back, lengths):
            down = R.resample(u.numpy(), sr, 16000, "sharp").astype(np.float32)
            up = R.resample(0.5 * down, 16000, sr, "sharp").astype(np.float32)
            assert np.array_equal(o.numpy(), up[:n])
    # utterances at the model's rate that are to come back at another: resampled once, behind the model
    inf = host_inferencer()
    out = inf.enhance_utterances([torch.from_numpy(R.signal(1000, 3))], output_sr=48000)
    assert inf.seen == [[1000]] and out[0].shape[0] == 3000


class Poison:
    def __getattr__(self, name):
        raise AssertionError(f"the existing path touched fullsubnet_amd.resample.{name}")


def test_existing_call_writes_the_same_files_with_and_without_the_module(tmp_path, monkeypatch):
    from scipy.io import wavfile
    import fullsubnet_amd
    lengths = [4097, 300, 12345]
    loader = [(torch.from_numpy(R.signal(n, n))[None], [f"utt{i}"]) for i, n in enumerate(lengths)]
    with_module = host_inferencer(tmp_path / "with", loader)
    with_module()
    monkeypatch.setattr(fullsubnet_amd, "resample", Poison())
    monkeypatch.setitem(sys.modules, "fullsubnet_amd.resample", Poison())
    without = host_inferencer(tmp_path / "without", loader)
    without()
    monkeypatch.undo()
    for i, n in enumerate(lengths):
        for a, b in ((with_module.enhanced_dir, without.enhanced_dir), (with_module.noisy_dir, without.noisy_dir)):
            assert (a / f"utt{i}.wav").read_bytes() == (b / f"utt{i}.wav").read_bytes()
        rate, data = wavfile.read(str(without.enhanced_dir / f"utt{i}.wav"))
        assert rate == 16000 and data.shape == (n,) and data.dtype == np.int16


def test_call_with_the_keys_resamples_and_stamps_the_rates(tmp_path, monkeypatch):
    from scipy.io import wavfile
    import fullsubnet_amd
    monkeypatch.setattr(fullsubnet_amd.resample, "resample", reference_resample)
    lengths = [4800, 1000, 9601]
    loader = [(torch.from_numpy(R.signal(n, n))[None], [f"utt{i}"]) for i, n in enumerate(lengths)]
    for keys, rate, want in ((dict(input_sr=48000, output_sr="input", batch_size=2), 48000, lengths),
                             (dict(input_sr=48000), 16000, [R.out_length(n, 48000, 16000) for n in lengths]),
                             (dict(input_sr=48000, output_sr=8000, resample_design="sharp"), 8000,
                              [R.out_length(n, 48000, 8000) for n in lengths])):
        inf = host_inferencer(tmp_path / f"{rate}", loader, **keys)
        inf()
        assert [len(g) for g in inf.seen] == ([2, 1] if keys.get("batch_size") == 2 else [1, 1, 1])
        for i, n in enumerate(lengths):
            got_rate, data = wavfile.read(str(inf.enhanced_dir / f"utt{i}.wav"))
            assert got_rate == rate and data.shape == (want[i],) and data.dtype == np.int16
            noisy_rate, noisy = wavfile.read(str(inf.noisy_dir / f"utt{i}.wav"))
            assert noisy_rate == 48000 and noisy.shape == (n,)
