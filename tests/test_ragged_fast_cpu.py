"""Fast FullSubNet ragged batches without a device: ``frames`` validation (fullsubnet_amd/ragged.py), the row-by-row
form of ``forward(mix_mag, frames=...)`` on CPU tensors, and the new C entries' size queries / argument checks
(include/fsn_hip.h, the ctypes table)."""
import os
import re

import numpy as np
import pytest
import torch

from fullsubnet_amd import ragged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST_KW = dict(look_ahead=2, shrink_size=2, sequence_model="LSTM", num_mels=64, encoder_input_size=257,
               bottleneck_hidden_size=384, bottleneck_num_layers=2, noisy_input_num_neighbors=5,
               encoder_output_num_neighbors=0, norm_type="offline_laplace_norm", weight_init=False)
NEW_ENTRIES = ["fsn_fast_spec_rows_ragged", "fsn_fast_norm_rows_ragged", "fsn_fast_bottleneck_input_ragged",
               "fsn_fast_mask_out_ragged", "fsn_stft_ragged", "fsn_mask_istft_workspace_bytes", "fsn_mask_istft"]


# ---- frames validation ------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", [[33, 32, 1], (33, 33, 33), np.array([1, 2, 33]), torch.tensor([33, 5, 1], dtype=torch.int32),
                                    [np.int64(3), np.int32(33), 1]])
def test_valid_frames_become_python_ints(frames):
    got = ragged.check_frames(frames, 3, 33, look_ahead=2)
    assert got == [int(v) for v in list(frames)] and all(type(v) is int for v in got)


@pytest.mark.parametrize("frames,what", [
    ([3, 4], "2 frames"),
    ([3, 4, 5, 6], "4 frames"),
    ([3, 0, 5], "outside"),
    ([3, -1, 5], "outside"),
    ([3, 34, 5], "outside"),                          # > T0
    ([3, 4.0, 5], "integers"),
    ([3, True, 5], "integers"),
    (["3", 4, 5], "integers"),
    (torch.tensor([3.0, 4.0, 5.0]), "integers"),
    (np.array([3.0, 4.0, 5.0]), "integers"),
    (torch.tensor([[3, 4, 5]]), "1-D"),
    (3, "sequence"),
])
def test_bad_frames_are_rejected(frames, what):
    with pytest.raises(ValueError, match=what):
        ragged.check_frames(frames, 3, 33, look_ahead=2)


def test_the_lower_bound_follows_the_look_ahead():
    """The down-sampling needs two frames with the look-ahead: one frame is legal only with look_ahead >= 1."""
    assert ragged.check_frames([1], 1, 10, look_ahead=1) == [1]
    assert ragged.check_frames([2], 1, 10, look_ahead=0) == [2]
    with pytest.raises(ValueError, match=r"\[2, 10\]"):
        ragged.check_frames([1], 1, 10, look_ahead=0)


def test_lengths_messages_are_unchanged_by_the_shared_parser():
    with pytest.raises(ValueError, match="lengths must hold integers"):
        ragged.check_lengths([300, 1.5], 2, 4096)


# ---- the row-by-row form on CPU tensors -------------------------------------------------------------
def _cpu_sequence_forward(self, x):
    """SequenceModel.forward as the reference's tensor algebra (the package's own blocks have no CPU implementation)."""
    o, _ = self.sequence_model(x.transpose(1, 2))
    if self.output_size:
        o = self.fc_output_layer(o)
    if self.output_activate_function:
        o = self.activate_function(o)
    return o.transpose(1, 2)


@pytest.fixture
def cpu_fast_model(monkeypatch):
    from fsn_synthetic import make_fast_params
    from fullsubnet_amd.fast_fullsubnet import Model
    from fullsubnet_amd.sequence_model import SequenceModel
    monkeypatch.setattr(SequenceModel, "forward", _cpu_sequence_forward)
    m = Model(**FAST_KW)
    sd = {k: torch.from_numpy(v) for k, v in make_fast_params(seed=3).items()}
    sd["mel_scale.fb"] = m.mel_scale.fb.clone()
    m.load_state_dict(sd, strict=True)
    return m.eval()


@pytest.mark.parametrize("frames", [[12, 5, 8], [12, 12, 12], [1, 12, 2]])
def test_cpu_forward_with_frames_equals_each_row_alone(cpu_fast_model, frames):
    m = cpu_fast_model
    torch.manual_seed(0)
    x = torch.rand(3, 1, 257, 12)
    for b, t in enumerate(frames):
        x[b, :, :, t:] = float("nan")  # never read
    with torch.no_grad():
        y = m(x, frames=frames)
        assert y.shape == (3, 2, 257, 12)
        for b, t in enumerate(frames):
            assert torch.equal(y[b:b + 1, :, :, :t], m(x[b:b + 1, :, :, :t])), b
            assert not y[b, :, :, t:].any(), b


def test_cpu_forward_with_bad_frames_raises(cpu_fast_model):
    with pytest.raises(ValueError):
        cpu_fast_model(torch.rand(2, 1, 257, 12), frames=[12, 13])
    with pytest.raises(ValueError):
        cpu_fast_model(torch.rand(2, 1, 257, 12), frames=[12])


def test_ragged_enhance_ok_on_both_model_classes():
    import fullsubnet_amd
    from fullsubnet_amd.fast_fullsubnet import Model
    fast = Model(**FAST_KW)
    assert fast.ragged_enhance_ok(512, 256)
    assert not fast.ragged_enhance_ok(512, 128) and not fast.ragged_enhance_ok(960, 480)
    assert not Model(**dict(FAST_KW, norm_type="cumulative_laplace_norm")).ragged_enhance_ok(512, 256)
    assert not Model(**dict(FAST_KW, sequence_model="GRU")).ragged_enhance_ok(512, 256)
    fsn = fullsubnet_amd.Model(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15,
                               fb_output_activate_function="ReLU", sb_output_activate_function=False,
                               fb_model_hidden_size=512, sb_model_hidden_size=384, norm_type="offline_laplace_norm",
                               num_groups_in_drop_band=1, weight_init=False)
    assert fsn.ragged_enhance_ok(512, 256) == fsn._fused and not fsn.ragged_enhance_ok(512, 128)


# ---- the C entries ----------------------------------------------------------------------------------
def test_header_declares_the_new_entries_and_the_table_matches():
    from fullsubnet_amd import _lib
    src = open(os.path.join(ROOT, "include", "fsn_hip.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\b" + name + r"\(", src), name
        assert name in _lib.SIGNATURES, name
    # each ragged glue entry is the plain one plus the frames pointer (and the look-ahead where the plain one lacks it)
    for name, extra in (("fsn_fast_spec_rows", 1), ("fsn_fast_norm_rows", 2), ("fsn_fast_bottleneck_input", 2),
                        ("fsn_fast_mask_out", 1)):
        assert len(_lib.SIGNATURES[name + "_ragged"][1]) == len(_lib.SIGNATURES[name][1]) + extra
    assert len(_lib.SIGNATURES["fsn_stft_ragged"][1]) == len(_lib.SIGNATURES["fsn_stft"][1]) + 1
    assert len(_lib.SIGNATURES["fsn_mask_istft"][1]) == 16
    L = _lib.lib()
    assert all(hasattr(L, n) for n in NEW_ENTRIES)


def test_new_entries_check_their_arguments_without_a_gpu():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    # the back half's workspace: the iSTFT's frame buffer, 512 / 256 only
    assert L.fsn_mask_istft_workspace_bytes(4, 100, 512) == L.fsn_istft_workspace_bytes(4, 100, 512) > 0
    assert L.fsn_mask_istft_workspace_bytes(4, 100, 960) == 0
    assert L.fsn_mask_istft_workspace_bytes(0, 100, 512) == 0
    # the glue's workspace query is shared with the plain entries
    assert L.fsn_fast_glue_workspace_bytes(35, 5, 64, 2) > 0
    one = 1 << 12  # a non-NULL host address: every check below fails before anything could be enqueued
    assert L.fsn_stft_ragged(one, one, 2, 4000, 512, 128, 512, one, one, one, one, None) == -1
    assert b"512" in L.fsn_last_error()
    assert L.fsn_stft_ragged(one, None, 2, 4000, 512, 256, 512, one, one, one, one, None) == -1
    assert b"NULL" in L.fsn_last_error()
    assert L.fsn_mask_istft(one, one, one, None, 2, 481, 100, 960, 480, 960, one, 48000, one, one, 1 << 30, None) == -1
    assert b"512" in L.fsn_last_error()
    assert L.fsn_mask_istft(one, one, one, None, 2, 200, 16, 512, 256, 512, one, 4000, one, one, 1 << 30, None) == -1
    assert b"F = 200" in L.fsn_last_error()
    assert L.fsn_mask_istft(one, one, one, one, 2, 257, 10, 512, 256, 512, one, 4000, one, one, 1 << 30, None) == -1
    assert b"T = 1 + length" in L.fsn_last_error()
    assert L.fsn_mask_istft(one, one, one, None, 2, 257, 16, 512, 256, 512, one, 4000, one, one, 16, None) == -2
    for call in (lambda: L.fsn_fast_spec_rows_ragged(one, None, 2, 257, 33, 2, one, 16, 272, None),
                 lambda: L.fsn_fast_norm_rows_ragged(one, None, 2, 35, 2, 16, 64, one, one, 1 << 20, None),
                 lambda: L.fsn_fast_bottleneck_input_ragged(one, one, 64, None, 2, 35, 2, 16, 64, 5, 0, 2, one, 128, 16, one,
                                                            1 << 20, None),
                 lambda: L.fsn_fast_mask_out_ragged(one, 514, None, 35, 2, 16, 257, 2, one, None)):
        assert call() == -1 and b"NULL" in L.fsn_last_error()
    assert L.fsn_fast_norm_rows_ragged(one, one, 35, 35, 2, 16, 64, one, one, 1 << 20, None) == -1
    assert b"look_ahead" in L.fsn_last_error()
    assert L.fsn_fast_bottleneck_input_ragged(one, one, 64, one, 2, 35, 2, 16, 64, 5, 0, 2, one, 128, 16, one, 16, None) == -2
