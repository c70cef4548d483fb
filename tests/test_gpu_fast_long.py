"""Fast FullSubNet recordings of any length: ``fast_fullsubnet.Model.enhance_long`` (segments with carried state; three
passes over them for the offline norm, libfsn_hip fsn_fast_segment_*) == the one-call path == the fp64 reference, on
recordings short enough to compare.  Needs a real MI355X:  python -m pytest tests -m gpu

The bounds are the project's standing ones: mask <= 1e-4 absolute against the fp64 reference (tests/test_gpu_parity.py),
waveform <= 2e-3 x peak against the one-call result (tests/test_gpu_long.py), <= 2e-5 x peak against StreamingEnhancer under
the causal norm (tests/test_gpu_streaming.py).  Two segmentations of one recording give the same mask bit for bit: every sum's
order depends on the frames alone.  Crossing 65 535 frames is left to tools/bench_long_fast.py (too long for a test)."""
import ctypes

import numpy as np
import pytest
import torch

import fast_long_reference as LR
import fast_stream_reference as R
from oracle import fullsubnet_oracle as O
from oracle import model_family_oracle as MF
from test_gpu_family import FAST_KW

pytestmark = pytest.mark.gpu

L_SHORT, L_WHOLE = 9637, 9800  # 38 frames -> 40 steps, the closing block short; 39 frames -> 41 steps, the closing block whole
SECOND = dict(shrink_size=3, look_ahead=1, noisy_input_num_neighbors=2, encoder_output_num_neighbors=1, bottleneck_hidden_size=128,
              bottleneck_num_layers=1)
ACOUSTICS = dict(n_fft=512, hop_length=256, win_length=512, sr=16000)
SEGMENTATIONS = (1, 7, 16, 19, 64)  # 19: two whole segments and a remainder of the look-ahead's size; 64: one segment


def cfg_of(kw):
    return R.Cfg(shrink=kw["shrink_size"], la=kw["look_ahead"], n_mel=kw["noisy_input_num_neighbors"],
                 n_enc=kw["encoder_output_num_neighbors"], bn_hidden=kw["bottleneck_hidden_size"], bn_layers=kw["bottleneck_num_layers"])


def build(kw, seed=3):
    """Seeded weights through the reference's state_dict names; the filterbank is the model's own.  -> (model, params, Cfg)."""
    from fullsubnet_amd.fast_fullsubnet import Model
    cfg = cfg_of(kw)
    params = MF.make_fast_params(seed=seed, bottleneck_hidden=cfg.bn_hidden, bottleneck_layers=cfg.bn_layers, nn_noisy=cfg.n_mel,
                                 nn_enc=cfg.n_enc)
    m = Model(**kw)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    sd["mel_scale.fb"] = m.mel_scale.fb.clone()
    m.load_state_dict(sd, strict=True)
    params["mel_scale.fb"] = sd["mel_scale.fb"].numpy()
    return m.cuda().eval(), params, cfg


def peak(x):
    return float(x.abs().max()) if isinstance(x, torch.Tensor) else float(np.abs(x).max())


def frames(n):
    return 1 + n // 256


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    return fullsubnet_amd


@pytest.fixture(scope="module")
def shipped(fsn):
    return build(FAST_KW)


def recording(fsn, model, params, cfg, samples, seed):
    """B = 2: the recording on the device, the one-call result, and the fp64 reference of each row alone on the device's own
    magnitude - computed once per module, never written to."""
    xd = torch.from_numpy(O.make_noisy(2, samples, seed=seed)).cuda()
    one, one_crm = model.enhance(xd, return_crm=True)
    mag = fsn.stft(xd, 512, 256, 512)[0].cpu().numpy()[:, None]
    want = [R.forward(mag[b:b + 1], params, cfg, "offline", np.float64)[0] for b in range(2)]
    return xd, one, one_crm, want


def hold(cfg, xd, one, one_crm, want, got, crm, what):
    T = frames(xd.shape[1])
    assert got.shape == xd.shape and crm.shape == one_crm.shape and got.is_cuda
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(crm).all())  # poisoned buffers: all that was read was written
    d_mask = LR.check_mask(crm.cpu().numpy(), want, [T + cfg.la] * 2, cfg, what=what)
    d_one = peak(got - one) / peak(one)
    print(f"{what}: max |d cIRM| vs the fp64 reference {d_mask:.2e} (one call: "
          f"{max(float(np.abs(one_crm[b].cpu().numpy() - want[b]).max()) for b in range(2)):.2e}), waveform vs one call {d_one:.2e} x peak")
    assert d_one <= 2e-3


# ---- 1. basic recordings -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def basic(fsn, shipped):
    model, params, cfg = shipped
    out = {}
    for samples in (L_SHORT, L_WHOLE):
        rec = recording(fsn, model, params, cfg, samples, seed=17)
        runs = {k: model.enhance_long(rec[0], segment_frames=k, return_crm=True, poison=True) for k in SEGMENTATIONS}
        out[samples] = (rec, runs)
    return out


@pytest.mark.parametrize("samples", [L_SHORT, L_WHOLE])
@pytest.mark.parametrize("k", SEGMENTATIONS)
def test_enhance_long_equals_one_call_and_reference(shipped, basic, samples, k):
    rec, runs = basic[samples]
    hold(shipped[2], *rec, *runs[k], what=f"{samples} samples, segment_frames {k}")


@pytest.mark.parametrize("samples", [L_SHORT, L_WHOLE])
def test_two_segmentations_give_the_same_bits(basic, samples):
    _, runs = basic[samples]
    assert torch.equal(runs[7][1], runs[16][1])


# ---- 2. the second configuration -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("samples", [L_SHORT, L_WHOLE])  # 39 steps: (39 - 1) % 3 = 2, a short closing block; 40 steps: a whole one
def test_second_configuration(fsn, samples):
    model, params, cfg = build(dict(FAST_KW, **SECOND), seed=5)
    rec = recording(fsn, model, params, cfg, samples, seed=19)
    got = model.enhance_long(rec[0], segment_frames=5, return_crm=True, poison=True)
    hold(cfg, *rec, *got, what=f"shrink 3, look-ahead 1, {samples} samples, segment_frames 5")


# ---- 3. a ragged batch ---------------------------------------------------------------------------------------------------------
def test_ragged_batch(shipped):
    model, _, _ = shipped
    lengths = [9800, 8637, 300, 1100]  # T_b + la = 41, 36, 4, 7: the closing block whole, short, short, whole
    assert [(frames(n) + 2 - 1) % 2 for n in lengths] == [0, 1, 1, 0]
    noisy = O.make_noisy(4, lengths[0], seed=23)
    for b, n in enumerate(lengths):
        noisy[b, n:] = 1e3  # never read
    xd = torch.from_numpy(noisy).cuda()
    want, want_crm = model.enhance(xd, lengths=lengths, return_crm=True)
    # 12: row 1's 36 steps end exactly on a segment edge, rows 2 and 3 inside the first segment, row 0's 41 inside the last
    got, crm = model.enhance_long(xd, lengths=lengths, segment_frames=12, return_crm=True, poison=True, slab_frames=16)
    for b, n in enumerate(lengths):
        d = peak(got[b, :n] - want[b, :n]) / peak(want[b, :n])
        print(f"row {b} ({n} samples): {d:.2e} x peak, mask {peak(crm[b] - want_crm[b]):.2e}")
        assert d <= 2e-3
        assert bool((got[b, n:] == 0).all()) and bool((crm[b, :, :, frames(n):] == 0).all())
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(crm).all())


# ---- 4. the divisors and the state, through the entries ------------------------------------------------------------------------
def run_entries(fsn, model, mag, total, segments):
    """The three passes over `segments` on mag [B, F, steps] -> (state blob, den_mel, den_unit, mel, enc [steps, Bp, 64], crm)."""
    lib, L = fsn._lib, fsn._lib.lib()
    B, F, steps = mag.shape
    c = model.stream_cfg()
    cfg, st = ctypes.byref(c), lib.stream_ptr(mag.device)
    state = torch.zeros(L.fsn_fast_segment_state_bytes(cfg, B), dtype=torch.uint8, device="cuda")
    sargs = (state.data_ptr(), state.numel())
    packed = model.stream_packed_weights(norm=lib.NORM_TYPES["cumulative_laplace_norm"]).data_ptr()
    Bp = (B + 15) // 16 * 16
    mel, enc = (torch.full((steps, Bp, 64), float("nan"), device="cuda") for _ in range(2))
    crm = torch.empty(B, 2, F, steps, device="cuda")
    tot = torch.tensor(total, dtype=torch.int32, device="cuda")
    ws = lambda k: lib.workspace(L.fsn_fast_segment_workspace_bytes(cfg, B, k), mag.device)  # noqa: E731
    for s0, k in segments:
        w = ws(k)
        lib.check(L.fsn_fast_segment_stats(cfg, packed, *sargs, lib.dev_ptr(mag[:, :, s0:s0 + k].contiguous()), B, k,
                                           lib.dev_ptr(mel[s0:s0 + k]), w.data_ptr(), w.numel(), st))
    for s0, k in segments:
        w = ws(k)
        lib.check(L.fsn_fast_segment_encoder(cfg, packed, *sargs, s0, tot.data_ptr(), lib.dev_ptr(mel[s0:s0 + k]), B, k,
                                             lib.dev_ptr(enc[s0:s0 + k]), w.data_ptr(), w.numel(), st))
    den_mel, den_unit = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    lib.check(L.fsn_fast_segment_divisors(cfg, *sargs, tot.data_ptr(), B, lib.dev_ptr(den_mel), lib.dev_ptr(den_unit), st))
    for s0, k in segments:
        w, y = ws(k), torch.empty(B, 2, F, k, device="cuda")
        lib.check(L.fsn_fast_segment_decoder(cfg, packed, *sargs, s0, tot.data_ptr(), lib.dev_ptr(mel[s0:s0 + k]),
                                             lib.dev_ptr(enc[s0:s0 + k]), B, k, lib.dev_ptr(y), w.data_ptr(), w.numel(), st))
        crm[..., s0:s0 + k] = y
    return state, den_mel, den_unit, mel, enc, crm


def test_divisors_are_fp64_sums_and_the_state_does_not_depend_on_the_segments(fsn, shipped):
    model, _, cfg = shipped
    lengths = [L_SHORT, 8000]  # 40 steps (a short closing block) and 34 (a short one too, inside the last segment)
    noisy = O.make_noisy(2, L_SHORT, seed=29)
    noisy[1, lengths[1]:] = 0.0
    xd = torch.from_numpy(noisy).cuda()
    from fullsubnet_amd.acoustics.feature import stft_ragged
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    mag = torch.cat([stft_ragged(xd, lens, 512, 256, 512)[0], xd.new_zeros(2, 257, 2)], dim=-1)  # [B, F, 40]
    total = [frames(n) + 2 for n in lengths]
    state, den_mel, den_unit, mel, enc, crm = run_entries(fsn, model, mag, total, [(0, 1), (1, 30), (31, 9)])
    assert bool((mel[:, 2:] == 0).all())  # the padding rows of the mel plane
    planes = [p[:, :2].permute(1, 2, 0).cpu().numpy() for p in (mel, enc)]  # [B, 64, steps]
    LR.check_divisors(den_mel.cpu().numpy(), den_unit.cpu().numpy(), *planes, total, cfg)
    # one segment: the same divisors, planes, masks and state, bit for bit
    again = run_entries(fsn, model, mag, total, [(0, 40)])
    for name, a, b in zip(("state", "den_mel", "den_unit", "mel", "enc", "crm"), (state, den_mel, den_unit, mel[:, :2], enc[:, :2], crm),
                          (again[0], again[1], again[2], again[3][:, :2], again[4][:, :2], again[5])):
        assert torch.equal(a, b), name


# ---- 5. the causal norm through the same driver --------------------------------------------------------------------------------
def test_cumulative_norm_model_equals_streaming(fsn):
    from fullsubnet_amd.streaming import StreamingEnhancer
    model, _, _ = build(dict(FAST_KW, norm_type="cumulative_laplace_norm"))
    xd = torch.from_numpy(O.make_noisy(2, 6000, seed=5)).cuda()
    enh = StreamingEnhancer(model, batch_size=2)
    want = torch.cat([enh.process(xd[:, :2500]), enh.process(xd[:, 2500:]), enh.flush()], dim=1)
    got = model.enhance_long(xd, segment_frames=7, poison=True)
    d = peak(got - want) / peak(want)
    print(f"cumulative norm, segments of 7 vs StreamingEnhancer: {d:.2e} x peak")
    assert got.shape == want.shape and d <= 2e-5


# ---- 6. refusals, a host input, the workspace limit, the Inferencer --------------------------------------------------------------
def test_refusals(fsn, shipped, basic):
    model, _, _ = shipped
    xd = basic[L_SHORT][0][0]
    from fullsubnet_amd.fast_fullsubnet import Model
    for kw, text in ((dict(sequence_model="GRU"), "LSTM"), (dict(bottleneck_hidden_size=200), "bottleneck"),
                     (dict(norm_type="offline_gaussian_norm"), "norm")):
        with pytest.raises(fsn._lib.FsnError, match=text) as e:
            Model(**dict(FAST_KW, **kw)).cuda().eval().enhance_long(xd, segment_frames=16)
        assert "Model.enhance" in str(e.value)
    with pytest.raises(fsn._lib.FsnError, match="n_fft 512") as e:
        model.enhance_long(xd, segment_frames=16, n_fft=320, hop_length=160)
    assert "Model.enhance" in str(e.value)
    with pytest.raises(fsn._lib.FsnError, match="ROCm device") as e:
        Model(**FAST_KW).eval().enhance_long(xd.cpu(), segment_frames=16)
    assert "Model.enhance" in str(e.value)
    with pytest.raises(fsn._lib.FsnError, match="segment_frames"):
        model.enhance_long(xd, segment_frames=4097)
    with pytest.raises(ValueError):
        model.enhance_long(xd, lengths=[L_SHORT, 100], segment_frames=16)


def test_host_input_and_workspace_limit(fsn, shipped, basic):
    """noisy may live on the host; segment_frames=None takes the largest segment under the workspace limit."""
    model, _, _ = shipped
    from fullsubnet_amd.fast_long_form import FastLongPlan
    (xd, _, _, _), runs = basic[L_SHORT]
    limit = 16 << 20
    k = FastLongPlan(model.stream_cfg(), 2, 2, L_SHORT, workspace_limit=limit).segment_frames
    assert 1 < k < 40
    got = model.enhance_long(xd.cpu(), workspace_limit=limit, slab_frames=5)  # several transform slabs too
    assert got.is_cuda and peak(got - runs[7][0]) <= 2e-5 * peak(got)


def test_inferencer_routes_long_items_by_an_explicit_key(fsn, shipped, basic):
    model, _, _ = shipped
    (xd, one, _, _), _ = basic[L_SHORT]
    calls = []

    def counted(*a, **k):
        calls.append(k)
        return type(model).enhance_long(model, *a, **k)

    model.enhance_long = counted
    try:
        seg = fsn.Inferencer(dict(inferencer=dict(type="full_band_crm_mask", args={}, segment_frames=16), acoustics=ACOUSTICS),
                             model=model)
        got = seg.full_band_crm_mask(xd[:1])
        assert len(calls) == 1 and calls[0]["segment_frames"] == 16
        want = one[0].cpu().numpy()
        assert got.shape == (L_SHORT,) and np.abs(got - want).max() <= 2e-3 * np.abs(want).max()
        # an item of no more than segment_frames frames does not take the segment path
        seg.full_band_crm_mask(xd[:1, :3000])
        assert len(calls) == 1
    finally:
        del model.enhance_long
