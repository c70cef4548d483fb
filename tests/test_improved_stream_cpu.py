"""Improved FullSubNet as a stream, without a device: the reference of tests/test_gpu_improved_stream.py is held to the oracle,
the model's ``sb_norm_type`` to that reference, the checkers catch deliberately wrong steps, and the C entries answer their
size queries, refuse what the step does not take and agree with the header and the bindings."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import improved_stream_reference as R
from oracle import fullsubnet_oracle as O
from oracle import model_family_oracle as MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fsn_improved_stream_packed_bytes", "fsn_improved_stream_pack", "fsn_improved_stream_state_bytes",
           "fsn_improved_stream_workspace_bytes", "fsn_improved_stream_step", "fsn_debug_improved_stream_state_layout",
           "fsn_debug_improved_stream_form")
REDUCED = [R.SMALL, R.SMALL_FDRC1, R.OTHER_NEIGHBOURS, R.TWO_SECTIONS]
SPLITS = sorted({row.split for row in R.TABLE if row.cfg in REDUCED})


def quiet(*a, **k):
    pass


def model_of(cfg, **kw):
    from fullsubnet_amd.improved_fullsubnet import Model
    return Model(**R.as_dict(cfg), **kw)


def torch_params(cfg):
    return {k: torch.from_numpy(v) for k, v in R.make_params(cfg).items()}


# ---- the reference ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [R.SMALL, R.OTHER_NEIGHBOURS, R.TWO_SECTIONS], ids=str)
def test_whole_sequence_model_under_the_offline_norms_is_the_oracle(cfg):
    """(i) under the reference's norms, between the oracle's own transforms = model_family_oracle.improved_fullsubnet_forward
    (held to the reference's goldens), exactly."""
    d = R.as_dict(cfg)
    params = R.make_params(cfg)
    y = O.make_noisy(2, 9 * d["hop_length"] + 5, seed=5)
    window = O.hann_window(d["n_fft"])
    want = MF.improved_fullsubnet_forward(y, params, d, window)
    mag, _, re, im = O.stft(y, d["n_fft"], d["hop_length"], d["win_length"], window=window)
    crm = R.forward(mag, params, cfg, "offline", "offline")
    got = O.istft((crm[:, 0] * re).astype(np.float32), (crm[:, 1] * im).astype(np.float32), d["n_fft"], d["hop_length"],
                  d["win_length"], length=y.shape[-1], window=window)[:, None, :]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("cfg", REDUCED, ids=str)
def test_chunked_step_is_the_whole_sequence_model_under_the_cumulative_norms(cfg):
    """(ii) in every chunking of the table = (i) under the cumulative norms to 1e-12 (fp64)."""
    params = R.make_params(cfg)
    for split in SPLITS:
        T = sum(split)
        mag = R.make_mag(2, cfg.F, T, seed=T)
        want = R.forward(mag, params, cfg, "cumulative", "cumulative", np.float64)
        calls, st = R.run_chunked(mag, params, cfg, split, np.float64, "torch")
        got = np.concatenate(calls, axis=-1)
        assert st["steps"] == T
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (cfg, split, np.abs(got - want).max())


def test_section_norm_is_one_mean_per_section_over_the_frames_so_far():
    """The causal counterpart of the offline statistic: frame t of the section input is divided by the mean of all units and
    window columns of frames 0 .. t; at the last frame that is the offline norm's divisor."""
    rng = np.random.default_rng(0)
    s = (np.abs(rng.standard_normal((2, 5, 1, 7, 9))) + 0.1)
    got = R.section_cumulative(s, np.float64)
    for t in range(9):
        mean = s[..., :t + 1].mean(axis=(1, 2, 3, 4))
        assert np.allclose(got[..., t], s[..., t] / (mean[:, None, None, None] + O.EPSILON), rtol=1e-13)
    assert np.allclose(got[..., -1], MF._norm_eps32(s, np.float64)[..., -1], rtol=1e-13)


# ---- the model's sb_norm_type -------------------------------------------------------------------------------------------------

def test_default_sb_norm_type_keeps_the_reference_behaviour():
    """sb_norm_type = None: the sections take the offline norm whatever norm_type says, the state dict's keys are what they
    were, and a state dict loads under either key."""
    for norm_type in ("offline_laplace_norm", "cumulative_laplace_norm"):
        m = model_of(R.SMALL, norm_type=norm_type)
        assert m.sb_norm_type is None and m.norm_type == norm_type and m.sb_model.norm_type == "offline_laplace_norm"
        assert m.sb_model.norm == m.offline_laplace_norm
    m = model_of(R.SMALL)
    assert m.num_freqs == 33 and m.look_ahead == 0
    saved = torch_params(R.SMALL)  # the reference's names: what a state dict saved before holds
    assert set(m.state_dict()) == set(saved)
    m.load_state_dict(saved, strict=True)
    causal = model_of(R.SMALL, norm_type="cumulative_laplace_norm", sb_norm_type="cumulative_laplace_norm")
    causal.load_state_dict(m.state_dict(), strict=True)
    with pytest.raises(NotImplementedError, match="sb_norm_type"):
        model_of(R.SMALL, sb_norm_type="forgetting_norm")


def test_default_sections_are_the_offline_norm_on_the_cpu_path():
    """With sb_norm_type = None the tensor-algebra section input is exactly today's: the offline norm of the unfolded
    windows, and the same whether the key is left out or named."""
    torch.manual_seed(0)
    x, fb = torch.rand(2, 1, 32, 6) + 0.1, torch.rand(2, 1, 32, 6)
    a, b = model_of(R.SMALL).sb_model, model_of(R.SMALL, sb_norm_type="offline_laplace_norm").sb_model
    for i, (lower, upper) in enumerate(R.bands(R.SMALL)):
        unf = torch.cat([a._freq_unfold(x, lower, upper, R.SMALL.centers[i], 3), a._freq_unfold(fb, lower, upper, R.SMALL.centers[i], 3)], dim=-2)
        want = unf / (unf.mean(dim=(1, 2, 3, 4), keepdim=True) + np.finfo(np.float32).eps)
        assert torch.equal(a._section_input(x, fb, i), want) and torch.equal(b._section_input(x, fb, i), want)


@pytest.mark.parametrize("cfg", [R.SMALL, R.OTHER_NEIGHBOURS], ids=str)
def test_cumulative_section_input_is_the_reference_module(cfg):
    """sb_norm_type = "cumulative_laplace_norm" on the tensor-algebra path: every section's input is what the whole-sequence
    reference feeds its block (fp32 against fp64), frame by frame, and `_section_prepared` stays out of it."""
    rng = np.random.default_rng(1)
    x = (np.abs(rng.standard_normal((2, 1, 32, 7))) + 0.05).astype(np.float32)
    fb = rng.standard_normal((2, 1, 32, 7)).astype(np.float32) + 2.0
    sb = model_of(cfg, norm_type="cumulative_laplace_norm", sb_norm_type="cumulative_laplace_norm").sb_model
    assert sb.norm_type == "cumulative_laplace_norm"
    assert sb._section_prepared(torch.from_numpy(x), torch.from_numpy(fb), 0) is None
    for i, (lower, upper) in enumerate(R.bands(cfg)):
        unf = np.concatenate([MF.banded_unfold(x.astype(np.float64), lower, upper, cfg.centers[i], cfg.sb_n[i]),
                              MF.banded_unfold(fb.astype(np.float64), lower, upper, cfg.centers[i], cfg.fb_n[i])], axis=-2)
        want = R.section_cumulative(unf, np.float64)
        with torch.no_grad():
            got = sb._section_input(torch.from_numpy(x), torch.from_numpy(fb), i).numpy()
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 8 * 2.0 ** -24 * np.abs(want).max()  # a division, an fp32 mean of a few hundred terms
        part = sb._section_input(torch.from_numpy(x), torch.from_numpy(fb), i, units=(1, 3)).numpy()
        assert np.array_equal(part, got[:, 1:3])  # a unit range: the statistic is still the whole section's


# ---- the checkers -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    row = next(r for r in R.TABLE if r.why == "mixed")
    return row, R.reference_of(row)


def test_checkers_pass_the_other_fp32_run(mixed):
    row, ref = mixed
    R.check_calls(row, ref, ref.mask["t32"], log=quiet)
    R.check_state(row, ref, ref.state["t32"], log=quiet)


# what each wrong step shows in first: the call whose masks leave the rule, the state array (or sum) that does.  The
# mistakes of R.MASK_ONLY are in the mask's assembly alone: the state is the yardstick's own, bit for bit
CAUGHT = {"section-sum-not-carried": ("mask call 1 ", "state sb0_h0 "), "count-of-the-wrong-section": ("mask call 0 ", "state sb0_h0 "),
          "reflection-off-by-one-at-the-top": ("mask call 0 ", "state sb2_h0 "), "last-bin-not-zero": ("the last bin", None),
          "unit-major-concat": ("mask call 0 ", None), "fullband-sum-not-carried": ("mask call 1 ", "state fb_h0 "),
          "count-from-the-call": ("mask call 1 ", "state fb_h0 ")}


@pytest.mark.parametrize("wrong", R.WRONG)
def test_checkers_catch_a_wrong_step(mixed, wrong):
    """Each stand-in is the fp32 yardstick run with one thing wrong.  The mask checker catches each of them at the first call
    the mistake reaches, and the state checker each one that touches what is carried."""
    row, ref = mixed
    calls, st = R.run_chunked(ref.mag, ref.params, row.cfg, row.split, np.float32, "cell", ref.state0, wrong=wrong)
    in_calls, in_state = CAUGHT[wrong]
    with pytest.raises(AssertionError, match=in_calls):
        R.check_calls(row, ref, calls, log=quiet)
    if wrong in R.MASK_ONLY:
        assert in_state is None
        for (name, a), (_, b) in zip(R.state_arrays(st).items(), R.state_arrays(ref.state["c32"]).items()):
            assert np.array_equal(a, b), name
    else:
        with pytest.raises(AssertionError, match=in_state):
            R.check_state(row, ref, st, log=quiet)


def test_at_least_five_stand_ins_are_caught_by_both_checkers():
    assert len([w for w in R.WRONG if w not in R.MASK_ONLY]) >= 5 and set(CAUGHT) == set(R.WRONG)


def test_checkers_catch_a_wrong_step_count_and_fp32_sums(mixed):
    row, ref = mixed
    st = R.copy_state(ref.state["c32"])
    st["steps"] += 1
    with pytest.raises(AssertionError, match="steps"):
        R.check_state(row, ref, st, log=quiet)
    st = R.copy_state(ref.state["c32"])
    st["fb_sum"] = st["fb_sum"] * (1.0 + 2e-6)  # beyond what fp32 terms in an fp64 sum can be off by
    with pytest.raises(AssertionError, match="fb_sum"):
        R.check_sums(row, ref, st, log=quiet)
    st = R.copy_state(ref.state["c32"])
    st["sb_sum"] = st["sb_sum"] * (1.0 + 1e-4)
    with pytest.raises(AssertionError, match="sb_sum"):
        R.check_sums(row, ref, st, log=quiet)


def test_table_covers_what_the_issue_lists():
    rows = R.TABLE
    reduced = [r for r in rows if r.cfg.F == 33]
    assert {r.B for r in reduced} >= {1, 3, 17}
    assert {k for r in reduced for k in r.split} >= {1, 2, 7} and ONES_ROW in {r.split for r in reduced} and (3, 4) in {r.split for r in reduced}
    assert {r.cfg.fdrc for r in reduced} == {0.5, 1.0} and {r.cfg.fb_hidden for r in reduced} == {64, 128}
    assert any(r.cfg.sb_n != r.cfg.fb_n for r in reduced) and any(len(r.cfg.centers) == 2 for r in reduced)
    assert any(r.resumed == R.LONG for r in rows)
    k48 = next(r for r in rows if r.cfg.F == 481)
    assert k48.B == 2 and k48.T == 6 and R.num_units(k48.cfg) == [20, 25, 6, 4] and (k48.cfg.fb_hidden, k48.cfg.sb_hidden) == (512, 384)
    k16 = next(r for r in rows if r.cfg.F == 257)
    assert k16.B == 1 and R.num_units(k16.cfg) == [20, 15, 22]
    # B x units crosses a 16-row tile inside a section (24 rows) and the sections' ends fall between tile edges
    assert any(r.B * n % 16 for r in reduced for n in R.num_units(r.cfg)) and any(r.B * R.num_units(r.cfg)[0] > 16 for r in reduced)
    assert len({r.id for r in rows}) == len(rows)


ONES_ROW = (1,) * 7


# ---- the C entries ------------------------------------------------------------------------------------------------------------

def c_cfg(cfg=R.SMALL, sec=None, **kw):
    from fullsubnet_amd import _lib
    f = dict(F=cfg.F, fdrc=cfg.fdrc, num_sections=len(cfg.centers), fb_hidden=cfg.fb_hidden, sb_hidden=cfg.sb_hidden, cell=0,
             fb_activation=0, sb_activation=0)
    f.update(kw)
    c = _lib.ImprovedCfg(**f)
    for i, ((lower, upper), ce, sn, fn) in enumerate(zip(R.bands(cfg), cfg.centers, cfg.sb_n, cfg.fb_n)):
        c.sec[i] = _lib.ImprovedSection(lower, upper, ce, sn, ce, fn)
    for i, fields in (sec or {}).items():
        for name, v in fields.items():
            setattr(c.sec[i], name, v)
    return c


def test_model_hands_the_entry_its_configuration():
    m = model_of(R.K48, norm_type="cumulative_laplace_norm", sb_norm_type="cumulative_laplace_norm")
    c, want = m.stream_cfg(), c_cfg(R.K48)
    assert bytes(c) == bytes(want)
    assert [(q.lower, q.upper, q.sb_center) for q in list(c.sec)[:4]] == [(0, 20, 1), (20, 120, 4), (120, 240, 20), (240, 480, 60)]
    assert model_of(R.SMALL, sequence_model="GRU").stream_cfg().cell == 1
    assert model_of(R.SMALL, sb_output_activate_function="ReLU").stream_cfg().sb_activation == 1
    assert model_of(R.SMALL, fb_output_activate_function="Tanh").stream_cfg().fb_activation == -1


def test_size_queries_answer_without_a_device():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    for cfg in REDUCED + [R.K48, R.K16]:
        c = ctypes.byref(c_cfg(cfg))
        assert L.fsn_improved_stream_packed_bytes(c) > 0, L.fsn_last_error()
        s1, s3 = L.fsn_improved_stream_state_bytes(c, 1), L.fsn_improved_stream_state_bytes(c, 17)
        assert 0 < s1 < s3
        w1, w8 = L.fsn_improved_stream_workspace_bytes(c, 1, 1), L.fsn_improved_stream_workspace_bytes(c, 1, 8)
        assert 0 < w1 < w8
    big = ctypes.byref(c_cfg(R.K48))
    assert L.fsn_improved_stream_state_bytes(big, 4096) > 0 and L.fsn_improved_stream_workspace_bytes(big, 1, 4096) > 0


@pytest.mark.parametrize("kw,text", [
    (dict(cell=1), b"LSTM"), (dict(fdrc=0.3), b"fdrc"), (dict(fdrc=2.0), b"fdrc"), (dict(num_sections=1), b"sections"),
    (dict(num_sections=9), b"sections"), (dict(fb_hidden=100), b"hidden"), (dict(sb_hidden=0), b"hidden"),
    (dict(fb_activation=2), b"activations"), (dict(sb_activation=-1), b"activations"), (dict(F=2), b"F"),
    (dict(sec={0: dict(sb_neighbors=60, fb_neighbors=60)}, F=481), b"beyond 240"),           # 1 + 120 + 1 + 120 = 242 columns
    (dict(sec={1: dict(fb_center=4)}), b"unit counts"),                                 # 8 bins by 2 and by 4
    (dict(sec={1: dict(sb_center=3, fb_center=3)}), b"unit counts"),                    # 8 bins by 3
    (dict(sec={1: dict(lower=9)}), b"tile"), (dict(sec={2: dict(upper=28)}), b"tile"), (dict(sec={0: dict(sb_neighbors=-1)}), b"neighbours")])
def test_refusals_answer_without_a_device(kw, text):
    from fullsubnet_amd import _lib
    L = _lib.lib()
    cfg = R.SMALL
    if kw.get("F") == 481:  # the wide window needs the bins to mirror in
        cfg, kw = R.K48, {k: v for k, v in kw.items() if k != "F"}
    c = ctypes.byref(c_cfg(cfg, **kw))
    assert L.fsn_improved_stream_state_bytes(c, 1) == 0 and text in L.fsn_last_error(), L.fsn_last_error()
    assert L.fsn_improved_stream_workspace_bytes(c, 1, 1) == 0 and text in L.fsn_last_error()
    assert L.fsn_improved_stream_packed_bytes(c) == 0 and text in L.fsn_last_error()
    assert L.fsn_debug_improved_stream_state_layout(c, 1, (ctypes.c_long * 50)(), 50) == -1
    # the step itself: FSN_ERR_ARG before anything is launched (the pointers are never read)
    assert L.fsn_improved_stream_step(c, 1, 1, 1 << 30, 0, 1, 1, 1, 1, 1, 1 << 30, None) == -1 and text in L.fsn_last_error()


def test_batch_frame_and_buffer_ranges_are_refused():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    c = ctypes.byref(c_cfg())
    for B in (0, -1, 4097):
        assert L.fsn_improved_stream_state_bytes(c, B) == 0 and b"out of range" in L.fsn_last_error()
        assert L.fsn_improved_stream_workspace_bytes(c, B, 1) == 0
    for k in (0, -3, 4097):
        assert L.fsn_improved_stream_workspace_bytes(c, 1, k) == 0 and b"out of range" in L.fsn_last_error()
        assert L.fsn_improved_stream_step(c, 1, 1, 1 << 30, 0, 1, 1, k, 1, 1, 1 << 30, None) == -1
    # a state or workspace buffer that is too small, a negative step count: before anything is launched
    need = L.fsn_improved_stream_state_bytes(c, 1)
    assert L.fsn_improved_stream_step(c, 1, 1, need - 1, 0, 1, 1, 1, 1, 1, 1 << 30, None) == -2 and b"too small" in L.fsn_last_error()
    assert L.fsn_improved_stream_step(c, 1, 1, need, 0, 1, 1, 1, 1, 1, 16, None) == -2
    assert L.fsn_improved_stream_step(c, 1, 1, need, -1, 1, 1, 1, 1, 1, 1 << 30, None) == -1
    with pytest.raises(_lib.FsnError):
        _lib.improved_stream_state_layout(c_cfg(), 0)


@pytest.mark.parametrize("cfg", REDUCED + [R.K48], ids=str)
@pytest.mark.parametrize("B", [1, 3, 17])
def test_layout_covers_the_state_without_overlap(cfg, B):
    from fullsubnet_amd import _lib
    lay = _lib.improved_stream_state_layout(c_cfg(cfg), B)
    S = len(cfg.centers)
    assert lay["sections"] == S and lay["rows"] == -(-B // 16) * 16
    assert lay["sb_rows"] == [-(-B * n // 16) * 16 for n in R.num_units(cfg)]
    size = {("fb", a): lay["rows"] * cfg.fb_hidden * 4 for a in range(4)}
    size.update({(i, a): lay["sb_rows"][i] * cfg.sb_hidden * 4 for i in range(S) for a in range(4)})
    at = {("fb", a): lay["fb"][a] for a in range(4)}
    at.update({(i, a): lay["sb"][i][a] for i in range(S) for a in range(4)})
    at.update(fb_sum=lay["fb_sum"], sb_sum=lay["sb_sum"], steps=lay["steps"])
    size.update(fb_sum=B * 8, sb_sum=S * B * 8, steps=B * 8)
    spans = sorted((at[name], at[name] + n) for name, n in size.items())
    assert spans[0][0] == 0
    for (_, end), (start, _) in zip(spans[:-1], spans[1:]):
        assert end <= start < end + 256  # no overlap; a gap is alignment only
    assert all(v % 8 == 0 for v in at.values())
    assert spans[-1][1] <= lay["bytes"] < spans[-1][1] + 256
    assert lay["bytes"] == _lib.lib().fsn_improved_stream_state_bytes(ctypes.byref(c_cfg(cfg)), B)


def test_header_and_bindings_agree():
    from fullsubnet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fsn_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert decl, f"{name} is not declared in include/fsn_hip.h"
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert name in _lib.ADDED_IN_118
    fields = re.search(r"typedef struct fsn_improved_section \{(.*?)\} fsn_improved_section;", src, flags=re.S).group(1)
    assert re.findall(r"int (\w+);", fields) == [n for n, _ in _lib.ImprovedSection._fields_]
    fields = re.search(r"typedef struct fsn_improved_cfg \{(.*?)\} fsn_improved_cfg;", src, flags=re.S).group(1)
    assert re.findall(r"(?:int|float|fsn_improved_section) (\w+)[;\[]", fields) == [n for n, _ in _lib.ImprovedCfg._fields_]
    assert "#define FSN_IMPROVED_MAX_SECTIONS %d" % _lib.IMPROVED_MAX_SECTIONS in src
    assert ctypes.sizeof(_lib.ImprovedParams) == 8 * 10 * (1 + _lib.IMPROVED_MAX_SECTIONS) and len(_lib.IMPROVED_BLOCK_FIELDS) == 10


def test_form_switch_takes_zero_and_one_only():
    """fsn_debug_improved_stream_form: 0 / 1 select a form, anything else only reads it; the default is the per-section chains
    (the faster form as measured, profiles/improved_stream.md)."""
    from fullsubnet_amd import _lib
    L = _lib.lib()
    default = L.fsn_debug_improved_stream_form(-1)
    assert default == 0
    try:
        assert L.fsn_debug_improved_stream_form(1) == 1 and L.fsn_debug_improved_stream_form(7) == 1
        assert L.fsn_debug_improved_stream_form(0) == 0 and L.fsn_debug_improved_stream_form(-1) == 0
    finally:
        L.fsn_debug_improved_stream_form(default)


def test_abi_revision_is_still_118():
    from fullsubnet_amd import _lib
    assert _lib.ABI_VERSION == 118 and _lib.lib().fsn_version() == 118
    assert "#define FSN_ABI_VERSION 118" in open(os.path.join(ROOT, "include", "fsn_hip.h")).read()


def test_streaming_enhancer_refuses_what_the_step_does_not_take():
    """A norm that is not causal: a ValueError that names the key to set, before anything touches a device; the 16 kHz default
    of 512 / 128: NotImplementedError."""
    from fullsubnet_amd.improved_fullsubnet import Model
    from fullsubnet_amd.streaming import StreamingEnhancer
    causal = dict(norm_type="cumulative_laplace_norm", sb_norm_type="cumulative_laplace_norm")
    with pytest.raises(ValueError, match="norm_type = 'cumulative_laplace_norm'"):
        StreamingEnhancer(model_of(R.K48))
    with pytest.raises(ValueError, match="sb_norm_type = 'cumulative_laplace_norm'"):
        StreamingEnhancer(model_of(R.K48, norm_type="cumulative_laplace_norm"))
    with pytest.raises(NotImplementedError, match="512 / 128"):
        StreamingEnhancer(Model(**dict(MF.IMPROVED_16K, **causal)))
    with pytest.raises(NotImplementedError, match="hop = n_fft / 2"):
        StreamingEnhancer(model_of(R.K48, **causal), n_fft=960, hop_length=240)
    with pytest.raises(ValueError, match="481"):
        StreamingEnhancer(model_of(R.K48, **causal), n_fft=512, hop_length=256)
