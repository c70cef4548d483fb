"""Recordings of any length: ``Model.enhance_long`` (segments with carried LSTM state, three passes for the offline norm)
== the one-call path == the oracle, on recordings short enough to compare.  Needs a real MI355X:  python -m pytest tests -m gpu

The bounds are the project's standing ones: mask <= 1e-4 absolute against the fp64 oracle (test_gpu_parity.py), waveform
<= 2e-3 x peak against the one-call result and the oracle, <= 2e-5 x peak between two segmentations of one recording
(test_gpu_streaming.py).  The segment path runs other recurrent kernels than the one call, so no bit-equality is asked."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import fullsubnet_oracle as O

pytestmark = pytest.mark.gpu

MODEL_KW = dict(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15,
                fb_output_activate_function="ReLU", sb_output_activate_function=False, fb_model_hidden_size=512,
                sb_model_hidden_size=384, weight_init=False)
L_BASIC = 9637  # T = 38 frames, 40 model steps
ACOUSTICS = dict(n_fft=512, hop_length=256, win_length=512, sr=16000)


def build(fsn, params, norm_type):
    m = fsn.Model(norm_type=norm_type, num_groups_in_drop_band=1, **MODEL_KW)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def setup():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd as fsn
    fsn._lib.lib()
    params = O.make_params(seed=0, gain=2.0, mask_gain=24.0)
    return fsn, build(fsn, params, "offline_laplace_norm"), params


@pytest.fixture(scope="module")
def basic(setup):
    """B = 2, T = 38: the recording, the one-call result and the oracle's - computed once, never written to."""
    fsn, model, params = setup
    noisy = O.make_noisy(2, L_BASIC, seed=17)
    xd = torch.from_numpy(noisy).cuda()
    one, one_crm = model.enhance(xd, return_crm=True)
    want = O.full_band_crm_mask(noisy, params, window=torch.hann_window(512).numpy())
    mag = fsn.stft(xd, 512, 256, 512)[0].cpu().numpy()
    crm64 = np.concatenate([O.fullsubnet_forward(mag[b:b + 1, None], params, dtype=np.float64) for b in range(2)])
    return xd, one, one_crm, want, crm64


def peak(x):
    return float(x.abs().max()) if isinstance(x, torch.Tensor) else float(np.abs(x).max())


# ---- 1. basic -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def by_segmentation(setup, basic):
    """enhance_long of the basic recording at every segmentation of the test, NaN poison on, each run once."""
    _, model, _ = setup
    return {k: model.enhance_long(basic[0], segment_frames=k, return_crm=True, poison=True) for k in (1, 7, 16, 19, 64)}


@pytest.mark.parametrize("k", [1, 7, 16, 19, 64])  # 19: the last segment is only the look-ahead zeros; 64: one segment
def test_enhance_long_equals_one_call_and_oracle(basic, by_segmentation, k):
    xd, one, one_crm, want, crm64 = basic
    got, crm = by_segmentation[k]
    assert got.shape == xd.shape and crm.shape == one_crm.shape and got.is_cuda
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(crm).all())  # poisoned buffers: all read was written
    d_mask = float(np.abs(crm.cpu().numpy().astype(np.float64) - crm64).max())
    d_one, d_want = peak(got - one) / peak(one), peak(got.cpu().numpy() - want) / peak(want)
    print(f"segment_frames {k}: max |d cIRM| vs the fp64 oracle {d_mask:.2e} (one call: "
          f"{float(np.abs(one_crm.cpu().numpy() - crm64).max()):.2e}), waveform vs one call {d_one:.2e}, vs the oracle {d_want:.2e}")
    assert d_mask <= 1e-4
    assert d_one <= 2e-3 and d_want <= 2e-3


def test_two_segmentations_agree(by_segmentation):
    a, b = by_segmentation[7][0], by_segmentation[16][0]
    d = peak(a - b) / peak(a)
    print(f"segment_frames 7 vs 16: {d:.2e} x peak")
    assert d <= 2e-5


def test_host_input_and_workspace_limit(setup, basic, by_segmentation):
    """noisy may live on the host; segment_frames=None takes the largest segment under the workspace limit."""
    fsn, model, _ = setup
    from fullsubnet_amd.long_form import LongPlan
    limit = 64 << 20
    k = LongPlan(model._cfg, 2, L_BASIC, workspace_limit=limit).segment_frames
    assert 1 < k < 40
    got = model.enhance_long(basic[0].cpu(), workspace_limit=limit, slab_frames=5)  # several transform slabs too
    assert got.is_cuda and peak(got - by_segmentation[7][0]) <= 2e-5 * peak(got)


# ---- 2. ragged ------------------------------------------------------------------------------------------------------
def test_ragged_batch(setup):
    _, model, _ = setup
    lengths = [9637, 8637, 300]  # T_b + la = 40, 36, 4
    noisy = O.make_noisy(3, lengths[0], seed=23)
    for b, n in enumerate(lengths):
        noisy[b, n:] = 1e3  # never read
    xd = torch.from_numpy(noisy).cuda()
    want, want_crm = model.enhance(xd, lengths=lengths, return_crm=True)
    # 12: row 1's 36 steps end exactly on a segment edge, row 2's 4 inside the first segment, row 0's 40 inside the last
    got, crm = model.enhance_long(xd, lengths=lengths, segment_frames=12, return_crm=True, poison=True, slab_frames=16)
    for b, n in enumerate(lengths):
        d = peak(got[b, :n] - want[b, :n]) / peak(want[b, :n])
        print(f"row {b} ({n} samples): {d:.2e} x peak, mask {peak(crm[b] - want_crm[b]):.2e}")
        assert d <= 2e-3
        assert bool((got[b, n:] == 0).all()) and bool((crm[b, :, :, 1 + n // 256:] == 0).all())
    assert bool(torch.isfinite(got).all())


# ---- 3. the divisors, through the entries ---------------------------------------------------------------------------------
def test_divisors_are_fp64_sums(setup):
    fsn, model, _ = setup
    lib, L = fsn._lib, fsn._lib.lib()
    lengths = [L_BASIC, 8000]  # T = 38 and 32: row 1's 34 steps end inside the last segment
    noisy = O.make_noisy(2, L_BASIC, seed=29)
    noisy[1, lengths[1]:] = 0.0
    xd = torch.from_numpy(noisy).cuda()
    from fullsubnet_amd.acoustics.feature import stft_ragged
    lens = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    mag = torch.cat([stft_ragged(xd, lens, 512, 256, 512)[0], xd.new_zeros(2, 257, 2)], dim=-1)  # [B, F, 40]
    total = torch.tensor([1 + n // 256 + 2 for n in lengths], dtype=torch.int32, device="cuda")
    cfg, st = ctypes.byref(model._cfg), lib.stream_ptr(xd.device)
    state = torch.zeros(L.fsn_fullsubnet_segment_state_bytes(cfg, 2), dtype=torch.uint8, device="cuda")
    sargs = (state.data_ptr(), state.numel())
    segments, fb = [(0, 1), (1, 30), (31, 9)], torch.empty(2, 257, 40, device="cuda")
    for s0, k in segments:
        lib.check(L.fsn_fullsubnet_segment_stats(cfg, *sargs, lib.dev_ptr(mag[:, :, s0:s0 + k].contiguous()), 2, k, st))
    for s0, k in segments:
        ws = lib.workspace(L.fsn_fullsubnet_segment_workspace_bytes(cfg, 2, k), xd.device)
        y = torch.empty(2, 257, k, device="cuda")
        lib.check(L.fsn_fullsubnet_segment_fullband(cfg, model.packed_weights().data_ptr(), *sargs, s0, total.data_ptr(),
                                                    lib.dev_ptr(mag[:, :, s0:s0 + k].contiguous()), 2, k, lib.dev_ptr(y),
                                                    ws.data_ptr(), ws.numel(), st))
        fb[:, :, s0:s0 + k] = y
    den_fb, den_sb = torch.empty(2, device="cuda"), torch.empty(2, device="cuda")
    lib.check(L.fsn_fullsubnet_segment_divisors(cfg, *sargs, total.data_ptr(), 2, lib.dev_ptr(den_fb), lib.dev_ptr(den_sb), st))
    m64, fb64 = mag.cpu().numpy().astype(np.float64), fb.cpu().numpy().astype(np.float64)
    for b, n in enumerate(total.tolist()):
        x = m64[b:b + 1, None, :, :n]
        sb = np.concatenate([O.freq_unfold(x, 15).reshape(1, 257, 31, n), fb64[b:b + 1, :, None, :n]], axis=2)
        for name, got, mean in (("full-band", den_fb[b].item(), x.mean()), ("sub-band", den_sb[b].item(), sb.mean())):
            want = np.float32(np.float32(mean) + np.float32(1e-5))  # base_model.py:204-218 on the exact mean
            print(f"row {b} {name}: {got!r} vs {float(want)!r}, {abs(got - float(want)) / float(np.spacing(want)):.2f} ulp")
            assert abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(want)), (b, name)


# ---- 4. the causal norm through the same driver ----------------------------------------------------------------------------
def test_cumulative_norm_model_equals_streaming(setup):
    fsn, _, params = setup
    from fullsubnet_amd.streaming import StreamingEnhancer
    model = build(fsn, params, "cumulative_laplace_norm")
    xd = torch.from_numpy(O.make_noisy(2, 6000, seed=5)).cuda()
    enh = StreamingEnhancer(model, batch_size=2)
    want = torch.cat([enh.process(xd[:, :2500]), enh.process(xd[:, 2500:]), enh.flush()], dim=1)
    got = model.enhance_long(xd, segment_frames=7, poison=True)
    d = peak(got - want) / peak(want)
    print(f"cumulative norm, segments of 7 vs StreamingEnhancer: {d:.2e} x peak")
    assert got.shape == want.shape and d <= 2e-5


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(setup, basic):
    fsn, model, _ = setup
    composed = fsn.Model(norm_type="offline_laplace_norm", num_groups_in_drop_band=1,
                         **dict(MODEL_KW, sb_model_hidden_size=256)).cuda().eval()
    assert not composed._fused
    with pytest.raises(fsn._lib.FsnError, match="fused"):
        composed.enhance_long(basic[0], segment_frames=16)
    with pytest.raises(fsn._lib.FsnError, match="n_fft 512"):
        model.enhance_long(basic[0], segment_frames=16, n_fft=320, hop_length=160)
    with pytest.raises(fsn._lib.FsnError, match="segment_frames"):
        model.enhance_long(basic[0], segment_frames=4097)
    # Model.enhance is untouched, its refusal beyond 100 000 frames included (the query fails before anything is launched)
    with pytest.raises(fsn._lib.FsnError, match="frames"):
        model.enhance(torch.zeros(1, 100001 * 256, device="cuda"))


# ---- 6. Inferencer ----------------------------------------------------------------------------------------------------------
def test_inferencer_routes_long_items_by_an_explicit_key(setup, basic):
    fsn, model, _ = setup
    xd, _, _, want, _ = basic
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
        assert got.shape == (L_BASIC,) and np.abs(got - want[0]).max() <= 2e-3 * np.abs(want[0]).max()
        # an item of no more than segment_frames frames, and every item without the key: today's array
        short = seg.full_band_crm_mask(xd[:1, :3000])
        plain = fsn.Inferencer(dict(inferencer=dict(type="full_band_crm_mask", args={}), acoustics=ACOUSTICS), model=model)
        assert len(calls) == 1
        assert np.array_equal(short, model.enhance(xd[:1, :3000])[0].cpu().numpy())
        assert np.array_equal(plain.full_band_crm_mask(xd[:1]), model.enhance(xd[:1])[0].cpu().numpy())
        assert len(calls) == 1
    finally:
        del model.enhance_long
    with pytest.raises(ValueError):
        fsn.Inferencer(dict(inferencer=dict(type="full_band_crm_mask", args={}, segment_frames=5000), acoustics=ACOUSTICS),
                       model=model)
