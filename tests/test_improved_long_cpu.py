"""Improved FullSubNet on recordings of any length, without a device: the three-pass reference of
tests/improved_long_reference.py is held to the whole-sequence model in every segmentation, ``ImprovedLongPlan`` to what it
promises, the checkers catch deliberately wrong passes, the host side refuses what ``enhance_long`` does not take, and the C
entries agree with the header and the bindings and check their arguments before anything is launched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import improved_long_reference as LR
import improved_stream_reference as R
from oracle import model_family_oracle as MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fsn_improved_segment_stats", "fsn_improved_segment_fullband", "fsn_improved_segment_sections",
           "fsn_improved_segment_divisors")
SEGMENTATIONS = (1, 7, 16, 19, 64)
SECOND = 48000  # samples at 48 kHz


def quiet(*a, **k):
    pass


def split_of(T, k):
    return tuple(min(k, T - s) for s in range(0, T, k))


def model_of(cfg, **kw):
    from fullsubnet_amd.improved_fullsubnet import Model
    return Model(**R.as_dict(cfg), **kw)


# ---- 1. the reference ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("norm", ["offline", "cumulative"])
@pytest.mark.parametrize("cfg,total", [(R.SMALL, (39, 40)), (R.SMALL, (39, 21, 2)), (R.OTHER_NEIGHBOURS, (39,)), (R.TWO_SECTIONS, (39,))],
                         ids=["small-39-40", "small-ragged", "other-neighbours", "two-sections"])
def test_three_passes_are_the_whole_sequence_model_of_each_row(cfg, total, norm):
    """`run` in fp64 = improved_stream_reference.forward(norm, "offline") of each row alone over its own frames, to 1e-12, in
    every segmentation; what lies past a row's end (random here) does not enter."""
    params = R.make_params(cfg)
    mag = LR.ragged_mag(total, cfg, seed=5)
    want = LR.rows_alone(mag, total, params, cfg, norm)
    for k in SEGMENTATIONS:
        r = LR.run(mag, total, params, cfg, split_of(max(total), k), norm)
        assert r.state["steps"] == max(total)
        for b, n in enumerate(total):
            d = np.abs(r.mask[b][..., :n] - want[b]).max()
            assert d <= 1e-12 * np.abs(want[b]).max(), (norm, k, b, d)
            assert not r.mask[b][:, -1].any()


def test_sums_and_divisors_of_the_reference_are_the_means_of_the_planes():
    """fb_sum / sb_sum are the plain sums over each row's own frames, and the divisors float(mean) + eps."""
    cfg, total = R.SMALL, (39, 21, 2)
    params = R.make_params(cfg)
    mag = LR.ragged_mag(total, cfg, seed=9)
    r = LR.run(mag, total, params, cfg, split_of(39, 7))
    for b, n in enumerate(total):
        comp = R.compress(mag[b:b + 1, :, :n], cfg, np.float64)
        assert abs(r.state["fb_sum"][b] - comp.sum()) <= 1e-12 * comp.sum()
        assert abs(r.den_fb[b] - (comp.mean() + np.finfo(np.float32).eps)) <= 1e-12
        fb = r.fb[b:b + 1, :, :n]
        for i, (lower, upper) in enumerate(R.bands(cfg)):
            s = np.concatenate([MF.banded_unfold(comp[:, None], lower, upper, cfg.centers[i], cfg.sb_n[i]),
                                MF.banded_unfold(fb[:, None], lower, upper, cfg.centers[i], cfg.fb_n[i])], axis=-2)
            assert abs(r.state["sb_sum"][i, b] - s.sum()) <= 1e-12 * abs(s.sum())
            assert abs(r.den_sb[i, b] - (s.mean() + np.finfo(np.float32).eps)) <= 1e-12


# ---- 2. the checkers ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ragged():
    return LR.reference_of("ragged", R.SMALL, (39, 40, 21))


def test_checkers_pass_the_other_fp32_run(ragged):
    case, ref = ragged
    LR.check_mask(case, ref, ref.mask["t32"][0], log=quiet)
    LR.check_state(case, ref, ref.state["t32"], log=quiet)
    r = ref.result["t32"]
    LR.check_divisors(r.den_fb, r.den_sb, r.state, case.total, case.cfg, log=quiet)


def test_checkers_ignore_what_lies_past_a_rows_end_but_not_what_lies_inside(ragged):
    case, ref = ragged
    mask = ref.mask["t32"][0].copy()
    mask[2, :, :-1, 21:] = 1e3
    LR.check_mask(case, ref, mask, log=quiet)
    mask[2, 0, 3, 20] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        LR.check_mask(case, ref, mask, log=quiet)


# what each wrong pass shows in first: the state array (or sum) that leaves the rule
CAUGHT = {"section-sum-restarts-per-segment": "sb0_h0", "divisor-over-the-longest-row": "fb_h0",
          "section-sum-over-noisy-windows-only": "sb0_h0", "frames-past-the-end-counted": "fb_h0",
          "fullband-state-reset-per-segment": "fb_h0", "mirror-off-by-one-at-the-top": "sb2_h0"}


@pytest.mark.parametrize("wrong", LR.WRONG)
def test_checkers_catch_a_wrong_pass(ragged, wrong):
    """Each stand-in is the fp32 yardstick run in segments of 16 with one thing wrong: the mask checker, the state checker and
    (where the mistake is in a sum or a count) the sum / divisor checkers reject it."""
    case, ref = ragged
    r = LR.run(ref.mag, case.total, ref.params, case.cfg, split_of(case.T, 16), "offline", np.float32, "cell", wrong=wrong)
    with pytest.raises(AssertionError, match="mask call 0"):
        LR.check_mask(case, ref, r.mask, log=quiet)
    with pytest.raises(AssertionError, match="state " + CAUGHT[wrong]):
        LR.check_state(case, ref, r.state, log=quiet)
    if wrong in ("section-sum-restarts-per-segment", "section-sum-over-noisy-windows-only", "frames-past-the-end-counted"):
        with pytest.raises(AssertionError, match="_sum"):
            LR.check_sums(case, ref, r.state, log=quiet)
    if wrong == "divisor-over-the-longest-row":
        with pytest.raises(AssertionError, match="den_"):
            LR.check_divisors(r.den_fb, r.den_sb, r.state, case.total, case.cfg, log=quiet)


def test_every_stand_in_the_issue_lists_is_there():
    assert set(CAUGHT) == set(LR.WRONG) and len(LR.WRONG) == 6


def test_sum_checker_counts_every_rows_own_terms(ragged):
    """A short row's sums are held by its own T_b terms: an fp32 ulp and a half per term is beyond what fp32 roots in an fp64
    sum can be off by, on the 21-frame row as on the 40-frame one."""
    case, ref = ragged
    for b in range(case.B):
        st = R.copy_state(ref.state["c32"])
        st["fb_sum"][b] *= 1.0 + 3.0 * 2.0 ** -24
        with pytest.raises(AssertionError, match="fb_sum: row"):
            LR.check_sums(case, ref, st, log=quiet)
    st = R.copy_state(ref.state["c32"])
    st["sb_sum"][1, 2] *= 1.0 + 1e-4
    with pytest.raises(AssertionError, match="sb_sum"):
        LR.check_sums(case, ref, st, log=quiet)
    with pytest.raises(AssertionError, match="sb_sum"):
        LR.check_state(case, ref, st, log=quiet)


def test_divisor_checker_holds_one_ulp(ragged):
    case, ref = ragged
    r = ref.result["c32"]
    den = r.den_sb.copy()
    den[1, 2] = np.nextafter(np.nextafter(den[1, 2], np.float32(np.inf)), np.float32(np.inf))
    with pytest.raises(AssertionError, match="den_sb"):
        LR.check_divisors(r.den_fb, den, r.state, case.total, case.cfg, log=quiet)


# ---- 3. the plan ----------------------------------------------------------------------------------------------------------------

def k48_cfg():
    return model_of(R.K48).stream_cfg()


def plan_of(num_samples, batch=1, passes="offline", **kw):
    from fullsubnet_amd.improved_long_form import ImprovedLongPlan
    return ImprovedLongPlan(k48_cfg(), 960, passes, batch, num_samples, **kw)


@pytest.mark.parametrize("samples,k", [(19200, 16), (60 * SECOND + 7, 256), (600 * SECOND, 4096), (481, 4096)])
def test_segments_cover_every_frame_once_and_slabs_tile_the_samples(samples, k):
    plan = plan_of(samples, segment_frames=k, slab_frames=1000)
    assert plan.frames == 1 + samples // 480
    frame = 0
    for s0, n in plan.segments:
        assert s0 == frame and 1 <= n <= min(k, 4096)
        frame += n
    assert frame == plan.frames
    frame, sample = 0, 0
    for t0, t1, (a, b), (o0, o1) in plan.slabs:
        assert t0 == frame and o0 == sample and t1 > t0 and o1 > o0 and b - a > 480 and t1 - t0 <= 1000
        frame, sample = t1, o1
    assert frame == plan.frames and sample == samples


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("passes", ["offline", "cumulative/offline", "cumulative"])
def test_ten_and_sixty_minutes_differ_only_in_the_linear_entries(B, passes):
    from fullsubnet_amd import _lib
    from fullsubnet_amd.improved_long_form import ImprovedLongPlan
    a, b = (plan_of(m * 60 * SECOND, B, passes, segment_frames=256) for m in (10, 60))
    assert b.frames == 360001 and b.total_bytes == sum(b.bytes.values())
    assert ImprovedLongPlan.LINEAR == ("mag", "spec_re", "spec_im", "mask", "fb_out", "enhanced")
    extra = b.frames - a.frames
    for name in a.bytes:
        if name not in ImprovedLongPlan.LINEAR:
            assert a.bytes[name] == b.bytes[name], name
    per_frame = {"mag": 4 * 481 * B, "spec_re": 4 * 481 * B, "spec_im": 4 * 481 * B, "mask": 8 * 481 * B,
                 "fb_out": 0 if passes == "cumulative" else 4 * 480 * B}  # unpadded in B
    for name, n in per_frame.items():
        assert b.bytes[name] - a.bytes[name] == n * extra, name
    assert (b.bytes["fb_out"] == 0) == (passes == "cumulative")
    assert b.bytes["enhanced"] == 4 * B * 3600 * SECOND
    L, c = _lib.lib(), k48_cfg()
    assert a.bytes["state"] == L.fsn_improved_stream_state_bytes(ctypes.byref(c), B)
    assert a.bytes["workspace"] == L.fsn_improved_stream_workspace_bytes(ctypes.byref(c), B, 256)
    # nothing of hidden-state width grows: ONE section's gate plane of the hour would be 4 x 384 floats per frame and row
    assert b.total_bytes - b.bytes["workspace"] - b.bytes["state"] < 4 * 4 * 384 * 16 * b.frames


def test_bisection_takes_the_largest_segment_under_the_limit():
    from fullsubnet_amd import _lib
    L, c = _lib.lib(), k48_cfg()
    query = lambda k: L.fsn_improved_stream_workspace_bytes(ctypes.byref(c), 1, k)  # noqa: E731
    limit = 256 << 20
    plan = plan_of(600 * SECOND, workspace_limit=limit)
    k = plan.segment_frames
    assert 1 < k < 4096 and query(k) <= limit < query(k + 1) and plan.bytes["workspace"] == query(k)
    assert plan_of(600 * SECOND, workspace_limit=64 << 30).segment_frames == 4096
    assert plan_of(19200, workspace_limit=64 << 30).segment_frames == 41  # never more than the recording has
    with pytest.raises(_lib.FsnError, match="limit"):
        plan_of(600 * SECOND, workspace_limit=1 << 10)
    for bad in (0, 4097):
        with pytest.raises(_lib.FsnError, match="segment_frames"):
            plan_of(600 * SECOND, segment_frames=bad)
    with pytest.raises(_lib.FsnError, match="samples"):
        plan_of(480)
    with pytest.raises(_lib.FsnError, match="passes"):
        plan_of(19200, passes="gaussian")


# ---- 4. the host-side refusals --------------------------------------------------------------------------------------------------

def test_enhance_long_refuses_on_the_host_and_names_the_model_call():
    from fullsubnet_amd import _lib
    from fullsubnet_amd.improved_fullsubnet import Model
    x = torch.zeros(1, 4000)
    causal = "cumulative_laplace_norm"
    for model, text in ((model_of(R.SMALL, sequence_model="GRU"), "LSTM"),
                        (Model(**MF.IMPROVED_16K), "hop = n_fft / 2"),                                  # 512 / 128
                        (Model(**dict(R.as_dict(R.SMALL), win_length=32)), "win_length"),
                        (model_of(R.SMALL, sb_norm_type=causal), "norm_type / sb_norm_type"),            # offline / cumulative
                        (model_of(R.SMALL, norm_type="offline_gaussian_norm"), "offline_gaussian_norm"),
                        (model_of(R.SMALL, sb_output_activate_function="Tanh"), "activations"),          # the C query's text
                        (model_of(R.SMALL), "ROCm device")):
        with pytest.raises(_lib.FsnError, match=text) as e:
            model.eval().enhance_long(x, segment_frames=16)
        assert "model(y)" in str(e.value), text
    with pytest.raises(_lib.FsnError, match="n_fft 64 / hop 32") as e:
        model_of(R.SMALL).eval().enhance_long(x, segment_frames=16, n_fft=512, hop_length=256)
    assert "model(y)" in str(e.value)
    # the model's own transform, named: not refused for that (the host model is)
    with pytest.raises(_lib.FsnError, match="ROCm device"):
        model_of(R.SMALL).eval().enhance_long(x, segment_frames=16, n_fft=64, hop_length=32)


def test_norms_decide_the_passes():
    from fullsubnet_amd.improved_long_form import refuse
    causal = "cumulative_laplace_norm"
    assert refuse(model_of(R.SMALL))[1] == "offline"
    assert refuse(model_of(R.SMALL, sb_norm_type="offline_laplace_norm"))[1] == "offline"
    assert refuse(model_of(R.SMALL, norm_type=causal))[1] == "cumulative/offline"
    assert refuse(model_of(R.SMALL, norm_type=causal, sb_norm_type=causal))[1] == "cumulative"
    cfg, _ = refuse(model_of(R.K48))
    assert bytes(cfg) == bytes(k48_cfg())


def test_the_driver_shares_the_slab_helpers():
    import inspect

    from fullsubnet_amd import improved_long_form, long_form, slabs
    assert improved_long_form.run_segments is long_form.run_segments  # the one driver, which calls the slab helpers of slabs.py
    assert long_form.analysis_slab is slabs.analysis_slab and long_form.synthesis_slab is slabs.synthesis_slab
    src = inspect.getsource(improved_long_form)
    assert "istft(" not in src and " stft(" not in src  # the transforms themselves are called in slabs.py only


# ---- 5. the entries without a device --------------------------------------------------------------------------------------------

def test_entries_are_declared_bound_and_exported_and_the_abi_revision_stands():
    from fullsubnet_amd import _lib
    src = open(os.path.join(ROOT, "include", "fsn_hip.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in _lib.ADDED_IN_118 and hasattr(L, name), name
        decl = re.search(r"\bint " + name + r"\(([^;()]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "#define FSN_ABI_VERSION 118" in src and _lib.ABI_VERSION == 118 and L.fsn_version() == 118
    sources = __import__("fullsubnet_amd.build", fromlist=["SOURCES"]).SOURCES
    assert "improved_segment_kernels.hip" in sources and "fsn_api_improved_segment.hip" in sources


def test_entries_check_their_arguments_before_anything_is_launched():
    """No device is touched here: the pointers are never read."""
    from fullsubnet_amd import _lib
    L = _lib.lib()
    c = model_of(R.SMALL).stream_cfg()
    ref = ctypes.byref(c)
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    big = 1 << 30
    err = lambda: L.fsn_last_error().decode()  # noqa: E731
    # short state / workspace: FSN_ERR_WORKSPACE
    assert L.fsn_improved_segment_stats(ref, p, 64, 0, p, p, 1, 4, None) == -2 and "too small" in err()
    assert L.fsn_improved_segment_fullband(ref, p, p, 64, 0, 0, p, p, 1, 4, p, p, big, None) == -2 and "too small" in err()
    assert L.fsn_improved_segment_fullband(ref, p, p, big, 0, 0, p, p, 1, 4, p, p, 64, None) == -2 and "too small" in err()
    assert L.fsn_improved_segment_sections(ref, p, p, 64, 0, p, p, p, 1, 4, p, p, big, None) == -2 and "too small" in err()
    assert L.fsn_improved_segment_sections(ref, p, p, big, 0, p, p, p, 1, 4, p, p, 64, None) == -2 and "too small" in err()
    assert L.fsn_improved_segment_divisors(ref, p, 64, p, 1, p, p, None) == -2 and "too small" in err()
    # fb_norm outside {0, 1}, B / k out of range, a negative frame count, NULL pointers: FSN_ERR_ARG
    for fb_norm in (2, -1):
        assert L.fsn_improved_segment_fullband(ref, p, p, big, fb_norm, 0, p, p, 1, 4, p, p, big, None) == -1 and "fb_norm" in err()
    assert L.fsn_improved_segment_stats(ref, p, big, 0, p, p, 1, 4097, None) == -1 and "out of range" in err()
    assert L.fsn_improved_segment_sections(ref, p, p, big, 0, p, p, p, 0, 4, p, p, big, None) == -1 and "out of range" in err()
    assert L.fsn_improved_segment_stats(ref, p, big, -1, p, p, 1, 4, None) == -1 and "frames_done" in err()
    assert L.fsn_improved_segment_stats(ref, p, big, 0, None, p, 1, 4, None) == -1 and "NULL" in err()
    assert L.fsn_improved_segment_fullband(ref, p, p, big, 0, 0, p, p, 1, 4, None, p, big, None) == -1 and "NULL" in err()
    assert L.fsn_improved_segment_divisors(ref, p, big, p, 1, None, p, None) == -1 and "NULL" in err()
    # what fsn_improved_stream_step refuses of a configuration
    gru = model_of(R.SMALL, sequence_model="GRU").stream_cfg()
    assert L.fsn_improved_segment_stats(ctypes.byref(gru), p, big, 0, p, p, 1, 4, None) == -1 and "LSTM" in err()
    assert L.fsn_improved_segment_divisors(ctypes.byref(gru), p, big, p, 1, p, p, None) == -1 and "LSTM" in err()
