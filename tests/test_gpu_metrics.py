"""fsn_stoi / fsn_si_sdr on the device, held to the fp64 numpy reference (tests/stoi_reference.py) on its seeded fixture
table.  Needs an MI355X:  python -m pytest tests -m gpu

STOI: |d_device - d_reference| <= 5e-11 per row.  d is a mean of correlation coefficients of 30-term fp64 sums; with no
frame within 1e-6 dB of the 40 dB decision and |segment| / |segment - mean| <= 1e3 (tests/test_metrics_cpu.py asserts
both on the table) the fp64 error is about 30 x 2^-53 x 1e3 = 3e-12 at worst, while a slip to fp32 anywhere moves d by
2e-10 and more.  Rows that are exact by construction (fewer than 30 frames: 1e-5, a zero estimate: 0) must agree to the
bit, estimate == clean must be within 1e-12 of 1.
SI-SDR: 1e-8 dB against the fp64 formula on the fp32 samples, for -5 .. 60 dB: sequential fp64 sums of up to 48 000
terms give about 1e-11 relative, the conditioning of the residual at 60 dB adds 1e3; a fp32 evaluation misses by 1e-5.
Workspaces and outputs are NaN before every call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stoi_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

STOI_BOUND = 5e-11
SDR_BOUND_DB = 1e-8
GUARD = 4096  # bytes of 0xA5 on either side of a guarded buffer


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    return fullsubnet_amd


def guarded(nbytes):
    """(whole buffer, the nbytes in the middle): guard pattern around a payload of NaN words."""
    pad = -(-nbytes // 256) * 256
    buf = torch.full((GUARD + pad + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + nbytes] = 0xFF
    return buf, buf[GUARD:GUARD + nbytes]


def guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[GUARD + nbytes:] == 0xA5).all())


def device_batch(clean, est, lengths, poison):
    """The padded rows on the device; poison: everything past a row's length is NaN."""
    clean, est = clean.copy(), est.copy()
    if poison:
        assert lengths is not None
        for b, n in enumerate(lengths):
            clean[b, n:] = np.nan
            est[b, n:] = np.nan
    d_len = torch.from_numpy(np.asarray(lengths, dtype=np.int32)).cuda() if lengths is not None else None
    return torch.from_numpy(clean).cuda(), torch.from_numpy(est).cuda(), d_len


def run_stoi(clean, est, lengths, sr, poison=False):
    """fsn_stoi through the C ABI into a guarded NaN output with a guarded NaN workspace; returns d [B] (numpy)."""
    from fullsubnet_amd import _lib
    lib = _lib.lib()
    B, L = clean.shape
    d_clean, d_est, d_len = device_batch(clean, est, lengths, poison)
    nbytes = lib.fsn_stoi_workspace_bytes(B, L, sr)
    assert nbytes > 0
    ws_buf, ws = guarded(nbytes)
    out_buf, out = guarded(8 * B)
    _lib.check(lib.fsn_stoi(d_clean.data_ptr(), d_est.data_ptr(), d_len.data_ptr() if d_len is not None else None, B, L, sr,
                            out.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(ws_buf, nbytes) and guards_intact(out_buf, 8 * B), "a write outside the workspace or the output"
    return out.view(torch.float64).cpu().numpy()


def run_si_sdr(ref, est, lengths, poison=False):
    from fullsubnet_amd import _lib
    lib = _lib.lib()
    B, L = ref.shape
    d_ref, d_est, d_len = device_batch(ref, est, lengths, poison)
    out_buf, out = guarded(8 * B)
    _lib.check(lib.fsn_si_sdr(d_ref.data_ptr(), d_est.data_ptr(), d_len.data_ptr() if d_len is not None else None, B, L,
                              out.data_ptr(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(out_buf, 8 * B)
    return out.view(torch.float64).cpu().numpy()


def batch_of(tag):
    sr, L, ragged, rows = R.fixture_table()[tag]
    clean, est, lengths = R.pad_rows(rows, L)
    return sr, L, rows, clean, est, (lengths if ragged else None)


@pytest.mark.parametrize("tag", ["16k", "48k", "10k", "rect"])
def test_stoi_against_the_fp64_reference(fsn, tag):
    """One call per fixture batch (ragged at 16 / 48 / 10 kHz, rectangular with lengths = NULL): J = 1, one frame short
    of it, a 120 ms pause 80 dB down, a full-length row, estimate == clean, a zero estimate, noise at 20 and 0 dB."""
    sr, L, rows, clean, est, lengths = batch_of(tag)
    d = run_stoi(clean, est, lengths, sr)
    worst = 0.0
    for b, row in enumerate(rows):
        err = abs(d[b] - row["d"])
        print(f"{tag} row {b} ({row['name']}): device {d[b]!r} reference {row['d']!r} difference {err:.3e}")
        if row["exact"] is None:
            worst = max(worst, err)
    print(f"{tag}: worst difference {worst:.3e} of {STOI_BOUND:.0e}")
    for b, row in enumerate(rows):
        if row["exact"] is not None:
            assert d[b] == row["exact"], (tag, row["name"], d[b])
        elif np.array_equal(row["clean"], row["estimate"]):
            assert abs(d[b] - 1) <= 1e-12, (tag, row["name"], d[b])
        assert abs(d[b] - row["d"]) <= STOI_BOUND, (tag, row["name"], d[b], row["d"])


def test_stoi_of_an_all_zero_clean_row_is_zero(fsn):
    sr, L, rows, clean, est, lengths = batch_of("16k")
    d = run_stoi(np.zeros_like(clean), clean, lengths, sr)
    for b, row in enumerate(rows):
        assert d[b] == (R.SHORT if row["exact"] == R.SHORT else 0.0), (row["name"], d[b])


def sdr_batch():
    """The 16 kHz rows' clean signals with white noise at -5 .. 60 dB."""
    sr, L, rows, clean, _, lengths = batch_of("16k")
    snrs = (-5, 10, 25, 40, 50, 60)
    est = np.zeros_like(clean)
    for b, (row, snr) in enumerate(zip(rows, snrs)):
        n = len(row["clean"])
        est[b, :n] = R.add_noise(row["clean"].astype(np.float64), snr, np.random.default_rng(900 + b)).astype(np.float32)
    want = np.array([R.si_sdr(clean[b, :n], est[b, :n]) for b, n in enumerate(lengths)])
    return clean, est, lengths, want, snrs


def test_si_sdr_against_the_fp64_formula(fsn):
    clean, est, lengths, want, snrs = sdr_batch()
    assert all(abs(w - s) < 0.5 for w, s in zip(want, snrs)), want  # the rows span -5 .. 60 dB
    got = run_si_sdr(clean, est, lengths)
    for b in range(len(want)):
        print(f"row {b}: device {got[b]!r} reference {want[b]!r} difference {abs(got[b] - want[b]):.3e} dB")
    print(f"worst difference {np.max(np.abs(got - want)):.3e} dB of {SDR_BOUND_DB:.0e}")
    assert np.all(np.abs(got - want) <= SDR_BOUND_DB), (got, want)
    rect = run_si_sdr(clean[:, :6000].copy(), est[:, :6000].copy(), None)  # lengths = NULL
    want_rect = np.array([R.si_sdr(clean[b, :6000], est[b, :6000]) for b in range(len(want))])
    assert np.all(np.abs(rect - want_rect) <= SDR_BOUND_DB), (rect, want_rect)


@pytest.mark.parametrize("tag", ["16k", "48k"])
def test_a_row_alone_has_the_bits_it_has_in_the_batch(fsn, tag):
    sr, L, rows, clean, est, lengths = batch_of(tag)
    d = run_stoi(clean, est, lengths, sr)
    s = run_si_sdr(clean, est, lengths)
    for b, n in enumerate(lengths):
        n = int(n)
        one_c, one_e = clean[b:b + 1, :n].copy(), est[b:b + 1, :n].copy()
        alone = run_stoi(one_c, one_e, np.array([n], dtype=np.int32), sr)
        assert alone[0].tobytes() == d[b].tobytes(), (tag, rows[b]["name"], alone[0], d[b])
        alone = run_si_sdr(one_c, one_e, np.array([n], dtype=np.int32))
        assert alone[0].tobytes() == s[b].tobytes(), (tag, rows[b]["name"], alone[0], s[b])


@pytest.mark.parametrize("tag", ["16k", "48k", "10k"])
def test_nothing_past_a_rows_length_is_read(fsn, tag):
    """NaN behind every row's last sample: the same bits (the guards around workspace and output are checked in every
    run of this file)."""
    sr, L, rows, clean, est, lengths = batch_of(tag)
    assert np.array_equal(run_stoi(clean, est, lengths, sr, poison=True), run_stoi(clean, est, lengths, sr))
    a, b = run_si_sdr(clean, est, lengths, poison=True), run_si_sdr(clean, est, lengths)
    assert a.tobytes() == b.tobytes()  # the zero-estimate row is NaN in both


def test_stoi_is_capturable_in_a_hip_graph(fsn):
    """One call captured on a single stream and replayed three times into a NaN output and a NaN workspace: every replay
    has the eager call's bits."""
    from fullsubnet_amd import _lib
    lib = _lib.lib()
    sr, L, rows, clean, est, lengths = batch_of("16k")
    eager = run_stoi(clean, est, lengths, sr)
    B = len(rows)
    d_clean, d_est, d_len = device_batch(clean, est, lengths, False)
    nbytes = lib.fsn_stoi_workspace_bytes(B, L, sr)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")

    def call():
        _lib.check(lib.fsn_stoi(d_clean.data_ptr(), d_est.data_ptr(), d_len.data_ptr(), B, L, sr, out.data_ptr(),
                                ws.data_ptr(), nbytes, _lib.stream_ptr()))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for _ in range(3):
        out.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == eager.tobytes()


def test_refusals_on_the_device(fsn):
    from fullsubnet_amd import _lib
    lib = _lib.lib()
    x = torch.zeros(2, 8000, device="cuda")
    out = torch.full((2,), 7.0, dtype=torch.float64, device="cuda")
    nbytes = lib.fsn_stoi_workspace_bytes(2, 8000, 16000)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    for args, word in (((2, 8000, 8000, out.data_ptr(), ws.data_ptr(), nbytes), b"sr = 8000"),
                       ((2, 8000, 16000, out.data_ptr(), ws.data_ptr(), nbytes - 256), b"at least"),
                       ((0, 8000, 16000, out.data_ptr(), ws.data_ptr(), nbytes), b"B = 0")):
        assert lib.fsn_stoi(x.data_ptr(), x.data_ptr(), None, *args, _lib.stream_ptr()) == -1
        assert word in lib.fsn_last_error(), lib.fsn_last_error()
    torch.cuda.synchronize()
    assert out.tolist() == [7.0, 7.0]  # nothing was launched
    with pytest.raises(_lib.FsnError, match="sample rates"):
        fsn.metrics.stoi(x, x, sr=8000)


def test_python_entries(fsn):
    """metrics.stoi / metrics.si_sdr: 2-D with a list or a tensor of lengths, 1-D, on the wrapper's own workspace."""
    sr, L, rows, clean, est, lengths = batch_of("16k")
    want = run_stoi(clean, est, lengths, sr)
    want_sdr = run_si_sdr(clean, est, lengths)
    c, e = torch.from_numpy(clean).cuda(), torch.from_numpy(est).cuda()
    for form in (lengths.tolist(), torch.from_numpy(lengths), torch.from_numpy(lengths).cuda()):
        d = fsn.metrics.stoi(c, e, sr, form)
        assert d.dtype == torch.float64 and d.is_cuda and d.cpu().numpy().tobytes() == want.tobytes()
        assert fsn.metrics.si_sdr(c, e, form).cpu().numpy().tobytes() == want_sdr.tobytes()
    n = int(lengths[3])
    one = fsn.metrics.stoi(c[3, :n], e[3, :n], sr)
    assert one.shape == (1,) and one.cpu().numpy()[0].tobytes() == want[3].tobytes()
    with pytest.raises(ValueError):
        fsn.metrics.stoi(c, e, sr, [L + 1] * len(rows))


class TinyMask(torch.nn.Module):
    """A stand-in model: a fixed, input-dependent compressed mask [B, 2, F, T]."""

    def __init__(self):
        super().__init__()
        self.gain = torch.nn.Parameter(torch.tensor(0.8))

    def forward(self, mag):
        real = self.gain * torch.ones_like(mag) + 0.1 * torch.tanh(mag)
        return torch.cat([real, 0.05 * torch.sin(mag)], dim=1)


def test_trainer_scores_validation_on_the_device(fsn):
    from fullsubnet_amd.trainer import Trainer
    sr = 16000
    valid = []
    for i, kind in enumerate(("With_reverb", "No_reverb", "With_reverb", "No_reverb")):
        rng = np.random.default_rng(40 + i)
        clean = R.speech_like(sr, sr, rng).astype(np.float32)
        noisy = R.add_noise(clean.astype(np.float64), 5, rng).astype(np.float32)
        valid.append((torch.from_numpy(noisy)[None], torch.from_numpy(clean)[None], [f"u{i}"], [kind]))

    def new(device_metrics):
        validation = {"validation_interval": 1, "save_max_metric_score": True}
        if device_metrics:
            validation["device_metrics"] = True
        cfg = {"meta": {"use_amp": False}, "acoustics": {"n_fft": 512, "hop_length": 256, "win_length": 512, "sr": sr},
               "trainer": {"train": {"epochs": 1}, "validation": validation, "visualization": {}}}
        model = TinyMask()
        loss = lambda target, pred: torch.mean((target - pred) ** 2)
        return Trainer(None, 0, cfg, False, False, model, loss, None, [], valid)

    t = new(True)
    t.model.eval()
    score = t._validation_epoch(1)
    assert t.validation_score_kind in ("STOI (device)", "(STOI (device) + WB_PESQ) / 2")
    lists = t.last_validation
    assert [len(lists[k]["enhanced"]) for k in ("With_reverb", "No_reverb")] == [2, 2]
    items = lists["With_reverb"]
    assert all(x.is_cuda for x in items["enhanced"])
    d = torch.cat([fsn.metrics.stoi(c, e, sr) for c, e in zip(items["clean"], items["enhanced"])])
    if t.validation_score_kind == "STOI (device)":
        assert score == float(d.mean())
    assert 0 < float(d.mean()) < 1
    per_kind = t.history["Metrics"][1]
    for kind in ("With_reverb", "No_reverb"):
        for metric in ("STOI", "SI_SDR"):
            assert set(per_kind[kind][metric]) == {"Noisy", "Enhanced"}
            assert all(np.isfinite(v) for v in per_kind[kind][metric].values())
    assert per_kind["With_reverb"]["STOI"]["Enhanced"] == float(d.mean())
    # rows against the reference: the enhanced signals the trainer scored
    for c, e, got in zip(items["clean"], items["enhanced"], d.tolist()):
        assert abs(got - R.stoi(c.cpu().numpy(), e.cpu().numpy(), sr)) <= STOI_BOUND

    # without the key: the host path, exactly as before
    from fullsubnet_amd.trainer import si_sdr
    t0 = new(False)
    t0.model.eval()
    score0 = t0._validation_epoch(1)
    assert "Metrics" not in t0.history
    if "STOI" not in t0.metrics or "WB_PESQ" not in t0.metrics:
        assert t0.validation_score_kind == "SI_SDR"
        host = t0.last_validation["With_reverb"]
        assert all(isinstance(x, np.ndarray) for x in host["enhanced"])
        assert score0 == float(np.mean([si_sdr(c, e) for c, e in zip(host["clean"], host["enhanced"])]))
        assert abs(score0 - per_kind["With_reverb"]["SI_SDR"]["Enhanced"]) <= 1e-4  # fp32 numpy sums on the host side
