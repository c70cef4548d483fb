"""Fast FullSubNet recordings of any length without a device: the three-pass reference of tests/fast_long_reference.py
against the whole-sequence model, its checkers against deliberately wrong stand-ins, the host book-keeping of
``fast_fullsubnet.Model.enhance_long`` (fullsubnet_amd.fast_long_form.FastLongPlan) and the size queries and refusals of
the segment entries (fsn_fast_segment_*)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import fast_long_reference as LR
import fast_stream_reference as R
from fullsubnet_amd import _lib
from fullsubnet_amd.fast_long_form import HOP, N_FFT, FastLongPlan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["fsn_fast_segment_state_bytes", "fsn_fast_segment_workspace_bytes", "fsn_fast_segment_stats", "fsn_fast_segment_encoder",
           "fsn_fast_segment_decoder", "fsn_fast_segment_divisors", "fsn_debug_fast_segment_state_layout"]
SMALL = dict(n_mel=2, n_enc=1, bn_hidden=128, bn_layers=1)
# (shrink, look_ahead) -> the rows' step counts: (total - 1) % shrink zero and every non-zero remainder
CASES = {(2, 2): (R.Cfg(), (21, 18, 4)), (3, 1): (R.Cfg(shrink=3, la=1, **SMALL), (22, 18, 20, 3))}
MINUTE = 60 * 16000


def fast_cfg(norm=0, **kw):
    f = dict(F=257, num_mels=64, shrink=2, mel_neighbors=5, enc_neighbors=0, bn_hidden=384, bn_layers=2, norm=norm)
    f.update(kw)
    return _lib.FastCfg(**f)


def splits(steps):
    out = {}
    for k in (1, 7, 16, steps):
        out[k] = tuple(min(k, steps - s) for s in range(0, steps, k))
    return out


@functools.lru_cache(maxsize=None)
def case(key):
    """The rows of a case, the fp64 masks of each row alone, and the weights - computed once, never written to."""
    cfg, totals = CASES[key]
    params = R.make_params(cfg)
    mag = LR.ragged_mag(totals, cfg, seed=100 * key[0] + key[1])
    return cfg, totals, params, mag, LR.rows_alone(mag, totals, params, cfg)


# ---- 1. the three passes are the whole-sequence model ----------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(CASES))
@pytest.mark.parametrize("k", [1, 7, 16, None])
def test_three_passes_equal_each_row_alone(key, k):
    cfg, totals, params, mag, alone = case(key)
    steps = max(totals)
    got = LR.run(mag, totals, params, cfg, splits(steps)[k or steps])
    for b, n in enumerate(totals):
        d = float(np.abs(got.crm[b][..., cfg.la:n] - alone[b]).max())
        print(f"shrink {cfg.shrink} la {cfg.la}, segments of {k}: row {b} ({n} steps, (total - 1) % shrink = {(n - 1) % cfg.shrink}): {d:.2e}")
        assert d <= 1e-12
    # the divisors are the one-call model's own: the utterance means of the mel spectrum and of the down-sampled units
    for b, (want_mel, want_unit) in enumerate(LR.expected_divisors(got.mel, got.enc, totals, cfg)):
        assert abs(got.den_mel[b] - want_mel) <= 2 * np.spacing(want_mel) and abs(got.den_unit[b] - want_unit) <= 2 * np.spacing(want_unit)


def test_two_segmentations_carry_the_same_sums():
    """The accumulators and the open block's sum do not depend on where the segments end (to the rounding of the BLAS
    products, whose order follows a call's row count; bit-equality is the device's property, tests/test_gpu_fast_long.py)."""
    cfg, totals, params, mag, _ = case((3, 1))
    a, b = (LR.run(mag, totals, params, cfg, splits(max(totals))[k]) for k in (7, 16))
    for name in ("acc_mel", "acc_unit", "stat_partial", "partial", "held"):
        assert np.allclose(a.state[name], b.state[name], rtol=1e-12, atol=1e-12), name
    assert np.allclose(a.den_mel, b.den_mel, rtol=1e-12) and np.allclose(a.den_unit, b.den_unit, rtol=1e-12)


# ---- 2. the checkers catch wrong stand-ins ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fp32_run(key, wrong):
    cfg, totals, params, mag, _ = case(key)
    return LR.run(mag, totals, params, cfg, (1, 9, 7, max(totals) - 17), dtype=np.float32, wrong=wrong)


@pytest.mark.parametrize("key", sorted(CASES))
def test_the_checkers_pass_the_fp32_run(key):
    cfg, totals, _, _, alone = case(key)
    got = fp32_run(key, None)
    assert LR.check_divisors(got.den_mel, got.den_unit, got.mel, got.enc, totals, cfg) <= 1.0
    LR.check_mask(got.crm[..., cfg.la:], alone, totals, cfg)


@pytest.mark.parametrize("key", sorted(CASES))
@pytest.mark.parametrize("wrong", LR.WRONG)
def test_the_checkers_catch(key, wrong):
    cfg, totals, _, _, _ = case(key)
    got = fp32_run(key, wrong)
    with pytest.raises(AssertionError, match="den_"):
        LR.check_divisors(got.den_mel, got.den_unit, got.mel, got.enc, totals, cfg, log=lambda s: None)


def test_low_rate_frame_count_and_the_unused_closing_frame():
    """1 + ceil((T - 1) / shrink) low-rate frames; the last one is unused by up-sampling exactly when (T - 1) % shrink != 0."""
    from oracle import model_family_oracle as MF
    for shrink in (2, 3):
        for T in range(2, 42):
            x = np.arange(T, dtype=np.float64)[None, None, None, :]
            low = MF.real_time_downsampling(x, shrink)
            assert low.shape[-1] == LR.low_frames(T, shrink)
            tagged = np.arange(low.shape[-1], dtype=np.float64)[None, None, None, :]
            used = set(MF.real_time_upsampling(tagged, shrink, T).ravel().astype(int))
            assert ((low.shape[-1] - 1) not in used) == ((T - 1) % shrink != 0), (shrink, T)


# ---- 3. the plan -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minutes", [2, 10, 60])
@pytest.mark.parametrize("k", [1, 19, 256, 4096, None])
def test_every_step_falls_in_exactly_one_segment(minutes, k):
    samples = minutes * MINUTE
    T = 1 + samples // HOP
    if k == 1:
        k = 3  # a segment per step is the same arithmetic, 225 003 tuples of it
    plan = FastLongPlan(fast_cfg(), 2, 1, samples, segment_frames=k)
    assert plan.frames == T and plan.steps == T + 2 and plan.offline
    pos = 0
    for s0, n in plan.segments:
        assert s0 == pos and 1 <= n <= 4096
        pos += n
    assert pos == T + 2
    if k is None:
        L = _lib.lib()
        kk = plan.segment_frames
        assert L.fsn_fast_segment_workspace_bytes(ctypes.byref(fast_cfg()), 1, kk) <= 4 << 30
        assert kk == min(4096, T + 2) or L.fsn_fast_segment_workspace_bytes(ctypes.byref(fast_cfg()), 1, kk + 1) > 4 << 30


def test_plan_edge_cases():
    samples = 37 * HOP + 165  # T = 38
    assert FastLongPlan(fast_cfg(), 2, 2, samples, segment_frames=19).segments == [(0, 19), (19, 19), (38, 2)]
    assert FastLongPlan(fast_cfg(), 1, 2, samples, segment_frames=16).segments == [(0, 16), (16, 16), (32, 7)]  # look_ahead 1: 39 steps
    for k in (40, 64, 4096):
        assert FastLongPlan(fast_cfg(), 2, 2, samples, segment_frames=k).segments == [(0, 40)]
    for bad in (0, -1, 4097):
        with pytest.raises(_lib.FsnError):
            FastLongPlan(fast_cfg(), 2, 2, samples, segment_frames=bad)
    with pytest.raises(_lib.FsnError):
        FastLongPlan(fast_cfg(), 2, 1, N_FFT // 2)
    ks = [FastLongPlan(fast_cfg(), 2, 1, 60 * MINUTE, workspace_limit=lim).segment_frames for lim in (16 << 20, 256 << 20, 4 << 30)]
    assert 1 < ks[0] < ks[1] < ks[2] <= 4096
    with pytest.raises(_lib.FsnError):
        FastLongPlan(fast_cfg(), 2, 1, 60 * MINUTE, workspace_limit=1 << 16)
    # the transform slabs tile the recording
    plan = FastLongPlan(fast_cfg(), 2, 1, 10 * MINUTE, segment_frames=64, slab_frames=5000)
    frame, sample = 0, 0
    for t0, t1, (a, b), (o0, o1) in plan.slabs:
        assert t0 == frame and o0 == sample and t1 > t0 and o1 > o0 and b - a > N_FFT // 2
        frame, sample = t1, o1
    assert frame == plan.frames and sample == 10 * MINUTE


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k", [256, 1024])
def test_ten_and_sixty_minutes_differ_only_in_the_linear_entries(B, k):
    a, b = (FastLongPlan(fast_cfg(), 2, B, m * MINUTE, segment_frames=k) for m in (10, 60))
    assert b.frames > 65535  # more frames than the one call takes: the plan exists all the same
    assert b.total_bytes == sum(b.bytes.values())
    extra, Bp = b.frames - a.frames, (B + 15) // 16 * 16
    for name in a.bytes:
        if name not in FastLongPlan.LINEAR:
            assert a.bytes[name] == b.bytes[name], name
    per_step = {"mag": 4 * 257 * B, "spec_re": 4 * 257 * B, "spec_im": 4 * 257 * B, "mask": 8 * 257 * B, "mel": 4 * 64 * Bp, "enc": 4 * 64 * Bp}
    for name, n in per_step.items():
        assert b.bytes[name] - a.bytes[name] == n * extra, name
    assert b.bytes["enhanced"] == 4 * B * 60 * MINUTE
    L = _lib.lib()
    assert a.bytes["state"] == L.fsn_fast_segment_state_bytes(ctypes.byref(fast_cfg()), B)
    assert a.bytes["workspace"] == L.fsn_fast_segment_workspace_bytes(ctypes.byref(fast_cfg()), B, k)
    # nothing of hidden-state width grows: one decoder hidden sequence of the hour alone would be 512 floats per step and padded row
    assert b.total_bytes - b.bytes["workspace"] - b.bytes["state"] < 4 * 512 * Bp * b.steps * 8


def test_a_cumulative_norm_plan_is_one_pass_of_the_stream_entry():
    L = _lib.lib()
    c = fast_cfg(norm=1)
    plan = FastLongPlan(c, 2, 1, 10 * MINUTE, segment_frames=256)
    assert not plan.offline and plan.bytes["mel"] == plan.bytes["enc"] == 0
    assert plan.bytes["state"] == L.fsn_fast_stream_state_bytes(ctypes.byref(c), 1)
    assert plan.bytes["workspace"] == L.fsn_fast_stream_workspace_bytes(ctypes.byref(c), 1, 256)


# ---- 4. the entries without a device ---------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported_and_the_abi_revision_stands():
    src = open(os.path.join(ROOT, "include", "fsn_hip.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in _lib.ADDED_IN_118 and hasattr(L, name), name
        decl = re.search(r"\b(?:int|size_t) " + name + r"\(([^;()]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "#define FSN_ABI_VERSION 118" in src and _lib.ABI_VERSION == 118 and L.fsn_version() == 118
    assert "fast_segment_kernels.hip" in __import__("fullsubnet_amd.build", fromlist=["SOURCES"]).SOURCES


def test_size_queries_and_the_state_layout():
    L = _lib.lib()
    c = fast_cfg()
    state = lambda B: L.fsn_fast_segment_state_bytes(ctypes.byref(c), B)  # noqa: E731
    ws = lambda B, k: L.fsn_fast_segment_workspace_bytes(ctypes.byref(c), B, k)  # noqa: E731
    stream = fast_cfg(norm=1)
    for B in (1, 3, 17):
        lay, base = _lib.fast_segment_state_layout(c, B), _lib.fast_stream_state_layout(stream, B)
        # it begins with fsn_fast_stream_step's layout ...
        for name in _lib.FAST_STREAM_STATE_LAYOUT[:16]:
            assert lay[name] == base[name], name
        assert (lay["rows"], lay["bn_rows"], lay["enc1_hidden"], lay["unit_width"]) == ((B + 15) // 16 * 16, B * 64, 320, 12)
        # ... then the two fp64 accumulators [B], then the statistic's own block sum [B][64][W]
        assert lay["stream_end"] <= lay["acc_mel"] and lay["acc_mel"] + 8 * B <= lay["acc_unit"]
        assert lay["acc_unit"] + 8 * B <= lay["stat_partial"] and lay["stat_partial"] + 4 * B * 64 * 12 <= lay["bytes"] == state(B)
        assert lay["stat_partial"] != lay["partial"]
        assert all(lay[n] % 256 == 0 for n in ("acc_mel", "acc_unit", "stat_partial"))
        assert state(B) <= L.fsn_fast_stream_state_bytes(ctypes.byref(stream), B) + 16 * B + 4 * B * 64 * 12 + 4 * 256
    assert all(ws(1, k1) > ws(1, k0) > 0 for k0, k1 in ((1, 2), (2, 64), (64, 4096)))
    assert ws(2, 16) > ws(1, 16) and ws(17, 16) > ws(16, 16)  # the bottleneck's B x 64 rows; the pairs' rows padded to 16
    assert ws(1, 64) >= 64 * 16 * 4 * 512 * 4  # the widest input projection of the segment alone
    # one size serves all passes: it is the stream step's, whose buffers every pass uses a subset of
    assert ws(3, 64) == L.fsn_fast_stream_workspace_bytes(ctypes.byref(stream), 3, 64)


def test_refusals_without_a_device():
    L = _lib.lib()
    c = fast_cfg()
    ref = ctypes.byref(c)
    for bad in ((0, 1), (-3, 1), (4097, 1), (1, 0), (1, -1), (1, 4097)):
        assert L.fsn_fast_segment_workspace_bytes(ref, *bad) == 0
        assert "out of range" in L.fsn_last_error().decode()
    for B in (0, 4097):
        assert L.fsn_fast_segment_state_bytes(ref, B) == 0 and "out of range" in L.fsn_last_error().decode()
    assert L.fsn_fast_segment_state_bytes(None, 1) == 0 and "NULL" in L.fsn_last_error().decode()
    # any norm but the offline one; the causal norm is pointed to the stream entry
    for norm in (1, 2, -1):
        assert L.fsn_fast_segment_state_bytes(ctypes.byref(fast_cfg(norm=norm)), 1) == 0
        assert "fsn_fast_stream_step" in L.fsn_last_error().decode()
    # what fsn_fast_stream_step refuses of a configuration
    for kw, text in ((dict(shrink=0), "shrink"), (dict(F=161), "257"), (dict(num_mels=80), "64"), (dict(mel_neighbors=8), "neighbours"),
                     (dict(bn_hidden=200), "bottleneck"), (dict(bn_layers=3), "bottleneck")):
        assert L.fsn_fast_segment_workspace_bytes(ctypes.byref(fast_cfg(**kw)), 1, 1) == 0
        assert text in L.fsn_last_error().decode(), kw
    # the entries themselves: arguments are checked before anything is launched (no device is touched here)
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    args = dict(mag=p, B=1, k=4)
    rc = L.fsn_fast_segment_stats(ref, p, p, 64, args["mag"], 1, 4, p, p, 64, None)
    assert rc == -2 and "too small" in L.fsn_last_error().decode()  # FSN_ERR_WORKSPACE
    rc = L.fsn_fast_segment_encoder(ref, p, p, 64, 0, p, p, 1, 4, p, p, 64, None)
    assert rc == -2 and "too small" in L.fsn_last_error().decode()
    rc = L.fsn_fast_segment_decoder(ref, p, p, 64, 0, p, p, p, 1, 4, p, p, 64, None)
    assert rc == -2 and "too small" in L.fsn_last_error().decode()
    rc = L.fsn_fast_segment_divisors(ref, p, 64, p, 1, p, p, None)
    assert rc == -2 and "too small" in L.fsn_last_error().decode()
    rc = L.fsn_fast_segment_decoder(ctypes.byref(fast_cfg(norm=1)), p, p, 64, 0, p, p, p, 1, 4, p, p, 64, None)
    assert rc == -1 and "fsn_fast_stream_step" in L.fsn_last_error().decode()  # FSN_ERR_ARG
    rc = L.fsn_fast_segment_encoder(ref, p, p, 64, 0, p, p, 1, 4097, p, p, 64, None)
    assert rc == -1 and "out of range" in L.fsn_last_error().decode()
    assert _lib.fast_segment_state_layout  # (the layout hook refuses the same way)
    with pytest.raises(_lib.FsnError):
        _lib.fast_segment_state_layout(fast_cfg(norm=1), 1)


def test_enhance_long_refuses_on_the_host_and_names_enhance():
    import torch

    from fullsubnet_amd.fast_fullsubnet import Model
    kw = dict(look_ahead=2, shrink_size=2, sequence_model="LSTM", num_mels=64, encoder_input_size=257, bottleneck_hidden_size=384,
              bottleneck_num_layers=2, noisy_input_num_neighbors=5, encoder_output_num_neighbors=0, norm_type="offline_laplace_norm",
              weight_init=False)
    x = torch.zeros(1, 4000)
    for bad, text in ((dict(sequence_model="GRU"), "LSTM"), (dict(bottleneck_hidden_size=200), "bottleneck"),
                      (dict(norm_type="offline_gaussian_norm"), "norm"), ({}, "ROCm device")):
        with pytest.raises(_lib.FsnError, match=text) as e:
            Model(**dict(kw, **bad)).eval().enhance_long(x, segment_frames=16)
        assert "Model.enhance" in str(e.value)
    with pytest.raises(_lib.FsnError, match="n_fft 512") as e:
        Model(**kw).eval().enhance_long(x, segment_frames=16, n_fft=320, hop_length=160)
    assert "Model.enhance" in str(e.value)


def test_the_driver_shares_the_slab_helpers():
    import inspect

    from fullsubnet_amd import fast_long_form, long_form, slabs
    assert fast_long_form.run_segments is long_form.run_segments  # the one driver, which calls the slab helpers of slabs.py
    assert long_form.analysis_slab is slabs.analysis_slab and long_form.synthesis_slab is slabs.synthesis_slab
    src = inspect.getsource(fast_long_form)
    assert "istft(" not in src and " stft(" not in src  # the transforms themselves are called in slabs.py only
