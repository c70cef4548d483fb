"""Fast FullSubNet as a stream, without a device: the reference of tests/test_gpu_fast_stream.py is held to the oracle, its
checkers catch deliberately wrong steps, and the C entries answer their size queries, refuse what the step does not take and
agree with the header, the exports and the bindings."""
import ctypes
import os
import re

import numpy as np
import pytest

import fast_stream_reference as R
from oracle import model_family_oracle as MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("fsn_fast_stream_packed_bytes", "fsn_fast_stream_pack", "fsn_fast_stream_state_bytes", "fsn_fast_stream_workspace_bytes",
           "fsn_fast_stream_step", "fsn_debug_fast_stream_state_layout")
CONFIGS = sorted({row.cfg for row in R.TABLE})
SPLITS = sorted({row.split for row in R.TABLE})


def quiet(*a, **k):
    pass


# ---- the reference ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [R.SHIPPED, R.Cfg(shrink=3, la=1, n_mel=2, n_enc=1, bn_hidden=128, bn_layers=1)], ids=str)
def test_whole_sequence_model_under_the_offline_norm_is_the_oracle(cfg):
    """(i) under the offline norm = model_family_oracle.fast_fullsubnet_forward (held to the reference's goldens), exactly."""
    params = R.make_params(cfg)
    mag = R.make_mag(2, 11, seed=5)
    want = MF.fast_fullsubnet_forward(mag, params, look_ahead=cfg.la, shrink_size=cfg.shrink, noisy_input_num_neighbors=cfg.n_mel,
                                      encoder_output_num_neighbors=cfg.n_enc, bottleneck_num_layers=cfg.bn_layers)
    assert np.array_equal(R.forward(mag, params, cfg, "offline"), want)


@pytest.mark.parametrize("cfg", CONFIGS, ids=str)
def test_chunked_step_is_the_whole_sequence_model_under_the_cumulative_norm(cfg):
    """(ii) in every chunking of the table = (i) under the cumulative norm to 1e-12 (fp64): step t is frame t - look_ahead, the
    caller appends the look_ahead zero frames."""
    params = R.make_params(cfg)
    for split in SPLITS:
        T = sum(split)
        mag = R.make_mag(2, T - cfg.la, seed=T)
        want = R.forward(mag, params, cfg, "cumulative", np.float64)
        fed = np.pad(mag, [(0, 0), (0, 0), (0, 0), (0, cfg.la)])
        calls, st = R.run_chunked(fed, params, cfg, split, np.float64, "torch")
        got = np.concatenate(calls, axis=-1)[..., cfg.la:]
        assert st["steps"] == T
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (cfg, split, np.abs(got - want).max())


def test_open_frames_follow_the_block_phase():
    # low-rate frame j >= 1 is the mean over steps (j - 1) s + 1 .. j s: after `steps` steps the open block holds (steps - 1) % s
    assert [R.open_frames(n, 2) for n in range(6)] == [0, 0, 1, 0, 1, 0]
    assert [R.open_frames(n, 3) for n in range(8)] == [0, 0, 1, 2, 0, 1, 2, 0]
    assert [R.open_frames(n, 1) for n in range(4)] == [0, 0, 0, 0]
    assert R.open_frames(R.LONG, 2) == 1 and R.open_frames(R.LONG + 1, 2) == 0


# ---- the checkers -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    row = next(r for r in R.TABLE if r.why == "mixed")
    return row, R.reference_of(row)


def test_checkers_pass_the_other_fp32_run(mixed):
    row, ref = mixed
    R.check_calls(row, ref, ref.crm["t32"], log=quiet)
    R.check_state(row, ref, ref.state["t32"], log=quiet)


# what each wrong step shows in first: the call whose masks leave the rule, the state array that does
CAUGHT = {"short-block-in-sum": ("crm call 3", "state bn_h0"), "upsampling-off-by-one": ("crm call 1", "state dec0_h0"),
          "count-W-j": ("crm call 1", "state bn_h0"), "block-mean-of-the-call": ("crm call 3", "state bn_h0"),
          "held-not-carried": ("crm call 1", "state dec0_h0")}


@pytest.mark.parametrize("wrong", R.WRONG)
def test_checkers_catch_a_wrong_step(mixed, wrong):
    """Each stand-in is the fp32 yardstick run with one thing wrong.  Both checkers catch each of them, on their own: the masks
    leave the rule at the first call the mistake reaches (call 1 begins inside a block; call 3 is the first to end inside one),
    and the final state does."""
    row, ref = mixed
    calls, st = R.run_chunked(ref.mag, ref.params, row.cfg, row.split, np.float32, "cell", ref.state0, wrong=wrong)
    in_calls, in_state = CAUGHT[wrong]
    with pytest.raises(AssertionError, match=in_calls + " "):
        R.check_calls(row, ref, calls, log=quiet)
    with pytest.raises(AssertionError, match=in_state + " "):
        R.check_state(row, ref, st, log=quiet)


def test_sum_checker_catches_the_short_block_in_the_sum(mixed):
    row, ref = mixed
    _, st = R.run_chunked(ref.mag, ref.params, row.cfg, row.split, np.float32, "cell", ref.state0, wrong="short-block-in-sum")
    with pytest.raises(AssertionError, match="unit_sum"):
        R.check_sums(row, ref, st, log=quiet)


def test_checkers_catch_a_wrong_step_count_and_an_fp32_sum(mixed):
    row, ref = mixed
    st = R.copy_state(ref.state["c32"])
    st["steps"] += 1
    with pytest.raises(AssertionError, match="steps"):
        R.check_state(row, ref, st, log=quiet)
    st = R.copy_state(ref.state["c32"])
    st["mel_sum"] = st["mel_sum"] * (1.0 + 2e-4)  # far beyond what fp32 terms in an fp64 sum can be off by
    with pytest.raises(AssertionError, match="mel_sum"):
        R.check_sums(row, ref, st, log=quiet)


def test_table_covers_what_the_issue_lists():
    rows = R.TABLE
    assert {r.B for r in rows} >= {1, 3, 16, 17}
    assert {(r.cfg.shrink, r.cfg.la) for r in rows} >= {(2, 2), (1, 0), (3, 1), (4, 2)}
    assert {(r.cfg.n_mel, r.cfg.n_enc) for r in rows} >= {(5, 0), (2, 1)}
    assert {(r.cfg.bn_hidden, r.cfg.bn_layers) for r in rows} >= {(384, 2), (128, 1)}
    assert {r.cfg.bn_hidden for r in rows} == {128, 256, 384, 512}  # every width the entry takes
    assert any(set(r.split) == {1} and r.cfg.shrink >= 2 for r in rows) and any(len(r.split) == 1 for r in rows)
    assert {r.resumed for r in rows} >= {R.LONG, R.LONG + 1}
    for s in (2, 3, 4):  # the mixed chunking begins a call at every phase of a block
        starts = np.concatenate([[0], np.cumsum(R.MIXED)])[:-1]
        assert {int(t) % s for t in starts if t > 0} == set(range(s))
    assert len({r.id for r in rows}) == len(rows)


# ---- the C entries ------------------------------------------------------------------------------------------------------------

def c_cfg(cfg=R.SHIPPED, **kw):
    from fullsubnet_amd import _lib
    f = dict(F=257, num_mels=64, shrink=cfg.shrink, mel_neighbors=cfg.n_mel, enc_neighbors=cfg.n_enc, bn_hidden=cfg.bn_hidden,
             bn_layers=cfg.bn_layers, norm=_lib.NORM_TYPES["cumulative_laplace_norm"])
    f.update(kw)
    return _lib.FastCfg(**f)


def test_size_queries_answer_without_a_device():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    for cfg in CONFIGS:
        c = ctypes.byref(c_cfg(cfg))
        assert L.fsn_fast_stream_packed_bytes(c) > 0
        s1, s3 = L.fsn_fast_stream_state_bytes(c, 1), L.fsn_fast_stream_state_bytes(c, 17)
        assert 0 < s1 < s3
        w1, w8 = L.fsn_fast_stream_workspace_bytes(c, 1, 1), L.fsn_fast_stream_workspace_bytes(c, 1, 8)
        assert 0 < w1 < w8
    big = ctypes.byref(c_cfg())
    assert L.fsn_fast_stream_state_bytes(big, 4096) > 0 and L.fsn_fast_stream_workspace_bytes(big, 1, 4096) > 0


@pytest.mark.parametrize("kw,text", [
    (dict(norm=0), b"causal norm"), (dict(norm=2), b"causal norm"), (dict(shrink=0), b"shrink"), (dict(F=161), b"257"),
    (dict(num_mels=80), b"64"), (dict(mel_neighbors=8), b"neighbours"), (dict(enc_neighbors=-1), b"neighbours"),
    (dict(bn_hidden=100), b"bottleneck"), (dict(bn_hidden=192), b"bottleneck"), (dict(bn_hidden=448), b"bottleneck"), (dict(bn_hidden=64), b"bottleneck"), (dict(bn_hidden=576), b"bottleneck"),
    (dict(bn_layers=3), b"bottleneck"), (dict(bn_layers=0), b"bottleneck")])
def test_refusals_answer_without_a_device(kw, text):
    from fullsubnet_amd import _lib
    L = _lib.lib()
    c = ctypes.byref(c_cfg(**kw))
    assert L.fsn_fast_stream_state_bytes(c, 1) == 0 and text in L.fsn_last_error()
    assert L.fsn_fast_stream_workspace_bytes(c, 1, 1) == 0 and text in L.fsn_last_error()
    assert L.fsn_fast_stream_packed_bytes(c) == 0 and text in L.fsn_last_error()
    assert L.fsn_debug_fast_stream_state_layout(c, 1, (ctypes.c_long * 21)(), 21) == -1
    # the step itself: FSN_ERR_ARG before anything is launched (the pointers are never read)
    assert L.fsn_fast_stream_step(c, 1, 1, 1 << 30, 0, 1, 1, 1, 1, 1, 1 << 30, None) == -1 and text in L.fsn_last_error()


def test_batch_and_frame_ranges_are_refused():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    c = ctypes.byref(c_cfg())
    for B in (0, -1, 4097):
        assert L.fsn_fast_stream_state_bytes(c, B) == 0 and b"out of range" in L.fsn_last_error()
        assert L.fsn_fast_stream_workspace_bytes(c, B, 1) == 0
    for k in (0, -3, 4097):
        assert L.fsn_fast_stream_workspace_bytes(c, 1, k) == 0 and b"out of range" in L.fsn_last_error()
    with pytest.raises(_lib.FsnError):
        _lib.fast_stream_state_layout(c_cfg(), 0)


@pytest.mark.parametrize("cfg", CONFIGS, ids=str)
@pytest.mark.parametrize("B", [1, 3, 17])
def test_layout_covers_the_state_without_overlap(cfg, B):
    from fullsubnet_amd import _lib
    lay = _lib.fast_stream_state_layout(c_cfg(cfg), B)
    rows, bn_rows, W, H = lay["rows"], lay["bn_rows"], lay["unit_width"], cfg.bn_hidden
    assert rows == -(-B // 16) * 16 and bn_rows == B * 64 and W == R.unit_width(cfg) and lay["enc1_hidden"] == 320
    size = {"enc0_h": rows * 384 * 4, "enc0_c": rows * 384 * 4, "enc1_h": rows * 320 * 4, "enc1_c": rows * 320 * 4,
            "dec0_h": rows * 512 * 4, "dec0_c": rows * 512 * 4, "dec1_h": rows * 512 * 4, "dec1_c": rows * 512 * 4,
            "bn_h0": bn_rows * H * 4, "bn_c0": bn_rows * H * 4, "mel_sum": B * 8, "unit_sum": bn_rows * 8, "partial": bn_rows * W * 4,
            "held": bn_rows * 4}
    if cfg.bn_layers == 2:
        size.update(bn_h1=bn_rows * H * 4, bn_c1=bn_rows * H * 4)
    else:
        assert lay["bn_h1"] == lay["bn_c1"] == -1
    spans = sorted((lay[name], lay[name] + n) for name, n in size.items())
    assert spans[0][0] == 0
    for (_, end), (start, _) in zip(spans[:-1], spans[1:]):
        assert end <= start < end + 256  # no overlap; a gap is alignment only
    assert all(lay[name] % 8 == 0 for name in size)
    assert spans[-1][1] <= lay["bytes"] < spans[-1][1] + 256
    assert lay["bytes"] == _lib.lib().fsn_fast_stream_state_bytes(ctypes.byref(c_cfg(cfg)), B)


def test_header_exports_and_bindings_agree():
    from fullsubnet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fsn_hip.h")).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        assert decl, f"{name} is not declared in include/fsn_hip.h"
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert name in _lib.ADDED_IN_118
    fields = re.search(r"typedef struct fsn_fast_cfg \{(.*?)\} fsn_fast_cfg;", src, flags=re.S).group(1)
    assert re.findall(r"int (\w+);", fields) == [n for n, _ in _lib.FastCfg._fields_]
    fields = re.search(r"typedef struct fsn_fast_params \{(.*?)\} fsn_fast_params;", src, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)", fields) == list(_lib.FAST_PARAM_FIELDS)
    assert _lib.SIGNATURES["fsn_fast_stream_step"][1][4:] == _lib.SIGNATURES["fsn_fullsubnet_stream_step"][1][4:]  # the same contract


def test_abi_revision_is_still_118():
    from fullsubnet_amd import _lib
    assert _lib.ABI_VERSION == 118 and _lib.lib().fsn_version() == 118
    assert "#define FSN_ABI_VERSION 118" in open(os.path.join(ROOT, "include", "fsn_hip.h")).read()


def test_streaming_enhancer_refuses_what_the_step_does_not_take():
    """The offline norm: FullSubNet's message, before anything touches a device.  GRU cells: NotImplementedError."""
    from fullsubnet_amd.fast_fullsubnet import Model
    from fullsubnet_amd.streaming import StreamingEnhancer
    kw = dict(look_ahead=2, shrink_size=2, sequence_model="LSTM", num_mels=64, encoder_input_size=257, bottleneck_hidden_size=384,
              bottleneck_num_layers=2, noisy_input_num_neighbors=5, encoder_output_num_neighbors=0)
    with pytest.raises(ValueError, match="streaming needs a causal norm"):
        StreamingEnhancer(Model(**kw))
    with pytest.raises(NotImplementedError, match="LSTM"):
        StreamingEnhancer(Model(**dict(kw, sequence_model="GRU", norm_type="cumulative_laplace_norm")))
    m = Model(**dict(kw, norm_type="cumulative_laplace_norm"))
    cfg = m.stream_cfg()
    assert [getattr(cfg, n) for n, _ in cfg._fields_] == [257, 64, 2, 5, 0, 384, 2, 1]
