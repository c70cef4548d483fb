"""fsn_resample / fsn_resample_taps on the device, held to the fp64 numpy reference (tests/resample_reference.py).
Needs an MI355X:  python -m pytest tests -m gpu

The bound is derived, not measured.  The device sums in fp64 and rounds once, so with r the reference's fp64 output
    |y - r| <= 2^-24 |r| + 2^-40 sum_m |h| |x|
at EVERY output sample: the first term is the one fp32 rounding, the second covers a fp64 sum in another order and taps
formed on the device (both about 2^-48 of that sum); a fp32 accumulation anywhere exceeds it by five decades
(tests/test_resample_cpu.py shows that the fp32 rounding of the reference itself meets it on these cases).  Taps: 2^-44 of
max |h| per tap.  Impulses, a row alone against the same row in a batch, and a graph replay against the eager call are
compared bit for bit.  Workspaces and outputs are NaN before every call and guarded on both sides."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

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


def run(x, lengths, sr_in, sr_out, design="scipy", poison=False, extra_out=0):
    """fsn_resample through the C ABI into a guarded NaN output with a guarded NaN workspace and guarded out_lengths.
    x [B, L] fp32 numpy; returns (y [B, L_out] numpy, out_lengths numpy)."""
    from fullsubnet_amd import _lib
    lib = _lib.lib()
    zeros, beta, rolloff = R.DESIGNS[design]
    B, L = x.shape
    x = x.copy()
    if poison:
        for b, n in enumerate(lengths):
            x[b, n:] = np.nan
    d_x = torch.from_numpy(x).cuda()
    d_len = torch.from_numpy(np.asarray(lengths, dtype=np.int32)).cuda() if lengths is not None else None
    L_out = R.out_length(L, sr_in, sr_out) + extra_out
    nbytes = lib.fsn_resample_workspace_bytes(sr_in, sr_out, zeros, beta, rolloff)
    assert nbytes > 0
    ws_buf, ws = guarded(nbytes)
    out_buf, out = guarded(4 * B * L_out)
    len_buf, out_len = guarded(4 * B)
    _lib.check(lib.fsn_resample(d_x.data_ptr(), d_len.data_ptr() if d_len is not None else None, B, L, sr_in, sr_out, zeros, beta,
                                rolloff, out.data_ptr(), L_out, out_len.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(ws_buf, nbytes) and guards_intact(out_buf, 4 * B * L_out) and guards_intact(len_buf, 4 * B), \
        "a write outside the workspace or an output"
    return out.view(torch.float32).view(B, L_out).cpu().numpy(), out_len.view(torch.int32).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- taps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", ["scipy", "sharp"])
@pytest.mark.parametrize("rates", [(16000, 48000), (48000, 16000), (44100, 16000), (16000, 44100)])
def test_taps_against_the_reference(fsn, rates, design):
    from fullsubnet_amd import _lib
    lib = _lib.lib()
    want, H = R.taps(*rates, design)
    n = 2 * H + 1
    buf, h = guarded(8 * n)
    _lib.check(lib.fsn_resample_taps(*rates, *R.DESIGNS[design], h.data_ptr(), n, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert guards_intact(buf, 8 * n)
    got = h.view(torch.float64).cpu().numpy()
    err = float(np.max(np.abs(got - want)))
    limit = 2.0 ** -44 * float(np.max(np.abs(want)))
    print(f"{rates} {design}: {n} taps, worst |h - reference| = {err:.3e} = {err / limit:.4f} of the bound")
    assert err <= limit
    assert bits(fsn.resample.taps(*rates, design).cpu().numpy()) == bits(got)


# ---- alignment ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("design", ["scipy", "sharp"])
@pytest.mark.parametrize("rates", [(3, 1), (1, 3), (8, 5), (441, 160), (160, 441)])
def test_impulses_reproduce_the_columns_of_h(fsn, rates, design):
    """A single 1.0 at m: y[k] = fp32(h[k d + H - m u]) exactly, 0 where the tap does not exist."""
    u, d = R.ratio(*rates)
    h = fsn.resample.taps(*rates, design).cpu().numpy()  # the device's own taps: this is the alignment test
    H = (len(h) - 1) // 2
    n = 3001
    positions = [0, n - 1, 1234]
    x = np.zeros((len(positions), n), dtype=np.float32)
    for b, m in enumerate(positions):
        x[b, m] = 1.0
    y, out_len = run(x, None, *rates, design)
    n_out = R.out_length(n, *rates)
    assert out_len.tolist() == [n_out] * len(positions)
    k = np.arange(n_out)
    for b, m in enumerate(positions):
        j = k * d + H - m * u
        want = np.where((j >= 0) & (j <= 2 * H), h[np.clip(j, 0, 2 * H)], 0.0).astype(np.float32)
        want = want + np.float32(0.0)  # a tap that is -0.0 (sinpi of an integer) sums to +0.0: the sum starts from +0.0
        assert np.count_nonzero(want) >= 1
        assert bits(y[b, :n_out]) == bits(want), (rates, design, m, int(np.argmax(y[b, :n_out] != want)))


# ---- the ratio / length sweep --------------------------------------------------------------------------------------------------
_worst = {}


def sweep_cases(fsn):
    return R.cases(lambda a, b, design: fsn.resample.plan(a, b, design)["tile_inputs"])


@pytest.mark.parametrize("design,rates", [("scipy", r) for r in R.RATIOS] + [("sharp", r) for r in R.SHARP_RATIOS])
def test_every_output_sample_within_the_derived_bound(fsn, design, rates):
    """Rows of 1, 2, H / u (down, up), the inputs of one workgroup - 1, + 0, + 1 (from the launcher's plan) and 4099 samples."""
    todo = [c for c in sweep_cases(fsn) if (c[0], c[1]) == rates and c[2] == design]
    tile_inputs = fsn.resample.plan(*rates, design)["tile_inputs"]
    assert {tile_inputs - 1, tile_inputs, tile_inputs + 1, 1, 2, 4099} <= {c[3] for c in todo}
    worst = 0.0
    for sr_in, sr_out, _, n, seed in todo:
        x = R.signal(n, seed)
        y, out_len = run(x[None], None, sr_in, sr_out, design)
        r = R.resample(x, sr_in, sr_out, design)
        assert y.shape == (1, len(r)) and out_len.tolist() == [len(r)]
        limit = R.bound(r, R.resample(x, sr_in, sr_out, design, absolute=True))
        err = np.abs(y[0].astype(np.float64) - r)
        frac = float(np.max(err / limit))
        print(f"{sr_in} -> {sr_out} {design} n = {n}: {len(r)} outputs, worst |y - r| = {frac:.4f} of the bound")
        worst = max(worst, frac)
        assert np.all(err <= limit), (sr_in, sr_out, design, n, int(np.argmax(err / limit)))
        if sr_in == sr_out:
            assert bits(y[0]) == bits(x)  # 1 / 1: the row, bit for bit
    _worst[(design, rates)] = worst
    print(f"{rates} {design}: worst over the lengths {worst:.4f} of the bound")


# ---- a ragged batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rates,design", [((48000, 16000), "scipy"), ((16000, 48000), "scipy"), ((44100, 16000), "scipy"),
                                          ((44100, 16000), "sharp"), ((16000, 44100), "sharp"), ((16000, 16000), "scipy")])
def test_ragged_batch_rows_have_the_bits_they_have_alone(fsn, rates, design):
    L_max = 30000  # two tiles and more at every ratio
    lengths = [1, 63, 1000, 4099, L_max]
    x = np.stack([np.concatenate([R.signal(n, 50 + n), np.zeros(L_max - n, dtype=np.float32)]) for n in lengths])
    extra = 37  # L_out_max beyond the longest row's n_out: zeros there too
    y, out_len = run(x, lengths, *rates, design, poison=True, extra_out=extra)
    want_len = [R.out_length(n, *rates) for n in lengths]
    assert out_len.tolist() == want_len
    assert not np.isnan(y).any()
    for b, n in enumerate(lengths):
        alone, alone_len = run(x[b:b + 1, :n].copy(), None, *rates, design)
        assert alone_len.tolist() == [want_len[b]]
        assert bits(y[b, :want_len[b]]) == bits(alone[0]), (rates, design, n)
        assert bits(y[b, want_len[b]:]) == bits(np.zeros(y.shape[1] - want_len[b], dtype=np.float32)), (rates, design, n)
    r = R.resample(x[3, :4099], *rates, design)
    assert np.all(np.abs(y[3, :len(r)] - r) <= R.bound(r, R.resample(x[3, :4099], *rates, design, absolute=True)))
    # a row of zeros: exact zeros, sign included
    x[2, :] = 0.0
    y, _ = run(x, lengths, *rates, design, poison=True)
    assert bits(y[2]) == bits(np.zeros(y.shape[1], dtype=np.float32))
    # lengths beyond the row and below zero are clamped on the device
    y2, len2 = run(x, [-5, 63, 1000, 4099, L_max + 100], *rates, design)
    assert len2.tolist() == [0] + want_len[1:] and not y2[0].any() and bits(y2[4]) == bits(y[4])


# ---- 64-bit indexing -------------------------------------------------------------------------------------------------------------
def test_one_long_row_where_k_times_down_passes_2_31(fsn):
    """13.5 M samples at 44100 -> 16000: k d reaches 2.16e9.  Checked at the last 2 000 outputs, 2 000 seeded positions and
    the 64 outputs on either side of k d = 2^31."""
    sr_in, sr_out, n = 44100, 16000, 13_500_000
    u, d = R.ratio(sr_in, sr_out)
    x = R.signal(n, 77)
    dx = torch.from_numpy(x).cuda()
    y, out_len = fsn.resample.resample(dx, sr_in, sr_out)
    n_out = R.out_length(n, sr_in, sr_out)
    assert y.shape == (n_out,) and out_len.tolist() == [n_out]
    y = y.cpu().numpy()
    edge = 2 ** 31 // d  # the last k with k d < 2^31
    assert (n_out - 1) * d > 2 ** 31 and 64 < edge < n_out - 2064
    ks = np.unique(np.concatenate([np.arange(n_out - 2000, n_out), np.arange(edge - 63, edge + 65),
                                   np.random.default_rng(5).integers(0, n_out, 2000)]))
    assert (ks * d < 2 ** 31).sum() > 500 and (ks * d >= 2 ** 31).sum() > 2000
    h = R.taps(sr_in, sr_out)[0]
    r = R.resample_at(x, sr_in, sr_out, ks, h=h)
    limit = R.bound(r, R.resample_at(x, sr_in, sr_out, ks, h=h, absolute=True))
    err = np.abs(y[ks].astype(np.float64) - r)
    print(f"{n} samples, {len(ks)} positions: worst |y - r| = {float(np.max(err / limit)):.4f} of the bound")
    assert np.all(err <= limit), int(ks[np.argmax(err / limit)])
    assert np.isfinite(y).all() and 0.2 < float(np.std(y[::97])) < 1.0  # no stretch left unwritten or zero


# ---- capture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rates,design", [((48000, 16000), "scipy"), ((44100, 16000), "sharp")])
def test_the_call_is_capturable_in_a_hip_graph(fsn, rates, design):
    """One call captured on a single stream and replayed three times into a NaN output and a NaN workspace: every replay
    has the eager call's bits (the call has no flags to clear and copies nothing from the host)."""
    from fullsubnet_amd import _lib
    lib = _lib.lib()
    zeros, beta, rolloff = R.DESIGNS[design]
    L_max = 6000
    lengths = [6000, 1, 2500]
    x = np.stack([R.signal(L_max, 300 + b) for b in range(3)])
    eager, eager_len = run(x, lengths, *rates, design)
    B, L_out = eager.shape
    d_x = torch.from_numpy(x).cuda()
    d_len = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    nbytes = lib.fsn_resample_workspace_bytes(*rates, zeros, beta, rolloff)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full((B, L_out), float("nan"), dtype=torch.float32, device="cuda")
    out_len = torch.full((B,), -1, dtype=torch.int32, device="cuda")

    def call():
        _lib.check(lib.fsn_resample(d_x.data_ptr(), d_len.data_ptr(), B, L_max, *rates, zeros, beta, rolloff, out.data_ptr(), L_out,
                                    out_len.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()))

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
        out_len.fill_(-1)
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        assert bits(out.cpu().numpy()) == bits(eager) and out_len.tolist() == eager_len.tolist()


# ---- the Python entry and the refusals ------------------------------------------------------------------------------------------
def test_python_entry_and_refusals_on_the_device(fsn):
    from fullsubnet_amd import _lib
    lib = _lib.lib()
    lengths = [4099, 63, 2000]
    x = np.stack([R.signal(4099, 400 + b) for b in range(3)])
    want, want_len = run(x, lengths, 48000, 16000)
    dx = torch.from_numpy(x).cuda()
    for form in (lengths, torch.tensor(lengths), torch.tensor(lengths, device="cuda")):
        y, n = fsn.resample.resample(dx, 48000, 16000, lengths=form)
        assert y.is_cuda and y.dtype == torch.float32 and n.dtype == torch.int32 and n.is_cuda
        assert bits(y.cpu().numpy()) == bits(want) and n.tolist() == want_len.tolist()
    one, n1 = fsn.resample.resample(dx[1, :63], 48000, 16000)
    assert one.shape == (21,) and n1.tolist() == [21] and bits(one.cpu().numpy()) == bits(want[1, :21])
    with pytest.raises(ValueError):
        fsn.resample.resample(dx, 48000, 16000, lengths=[5000, 1, 1])
    with pytest.raises(_lib.FsnError, match="at most 4096"):
        fsn.resample.resample(dx, 44101, 16000)
    out = torch.full((3, 1367), 7.0, device="cuda")
    nbytes = lib.fsn_resample_workspace_bytes(48000, 16000, 10, 5.0, 1.0)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    for args, word in (((48000, 16000, 10, 5.0, 1.0, out.data_ptr(), 1366, None, ws.data_ptr(), nbytes), b"L_out_max = 1366"),
                       ((48000, 16000, 10, 5.0, 1.0, out.data_ptr(), 1367, None, ws.data_ptr(), nbytes - 256), b"at least"),
                       ((48000, 16000, 10, 5.0, 1.5, out.data_ptr(), 1367, None, ws.data_ptr(), nbytes), b"rolloff")):
        assert lib.fsn_resample(dx.data_ptr(), None, 3, 4099, *args, _lib.stream_ptr()) == -1
        assert word in lib.fsn_last_error(), lib.fsn_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_inferencer_enhances_48_khz_utterances_and_returns_them_at_48_khz(fsn):
    from oracle import fullsubnet_oracle as O
    params = O.make_params(seed=5, gain=2.0, mask_gain=24.0)
    model = fsn.Model(norm_type="offline_laplace_norm", num_groups_in_drop_band=1, num_freqs=257, look_ahead=2,
                      sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15, fb_output_activate_function="ReLU",
                      sb_output_activate_function=False, fb_model_hidden_size=512, sb_model_hidden_size=384, weight_init=False)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    inf = fsn.Inferencer(dict(inferencer=dict(type="full_band_crm_mask", args={}),
                              acoustics=dict(n_fft=512, hop_length=256, win_length=512, sr=16000)), model=model.cuda().eval())
    lengths = [14401, 9000, 30000]  # 0.3, 0.19 and 0.63 s at 48 kHz
    utts = [torch.from_numpy(0.1 * R.signal(n, 600 + n)).cuda() for n in lengths]
    got = inf.enhance_utterances(utts, sr=48000, output_sr="input")
    assert [int(o.shape[0]) for o in got] == lengths
    # by hand: resample -> the existing call -> resample, trim
    noisy, _ = fsn.ragged.pad_utterances(utts)
    down, down_len = fsn.resample.resample(noisy, 48000, 16000, lengths=lengths)
    model_len = [R.out_length(n, 48000, 16000) for n in lengths]
    assert down_len.tolist() == model_len
    enhanced = inf.enhance_utterances([down[b, :n] for b, n in enumerate(model_len)])
    rows, _ = fsn.ragged.pad_utterances(enhanced)
    up, up_len = fsn.resample.resample(rows, 16000, 48000, lengths=model_len)
    assert all(a >= n for a, n in zip(up_len.tolist(), lengths))
    for b, n in enumerate(lengths):
        assert torch.equal(got[b], up[b, :n]), b
        assert torch.isfinite(got[b]).all() and float(got[b].abs().max()) > 0
    # at the model's rate the result is today's call
    plain = inf.enhance_utterances([u[:9000] for u in utts])
    same = inf.enhance_utterances([u[:9000] for u in utts], sr=16000, output_sr="model")
    assert all(torch.equal(a, b) for a, b in zip(plain, same))
    at_model = inf.enhance_utterances(utts, sr=48000)
    assert all(torch.equal(a, b) for a, b in zip(at_model, enhanced))
