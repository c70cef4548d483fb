"""Ragged batches without a device: the host-side length validation and padding helpers (fullsubnet_amd/ragged.py) and
the C entry fsn_enhance_ragged in include/fsn_hip.h / the ctypes table."""
import os
import re

import numpy as np
import pytest
import torch

from fullsubnet_amd import ragged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("lengths", [[300, 4096, 257], (4096, 4096, 4096), np.array([257, 300, 4096]),
                                     torch.tensor([257, 300, 4096], dtype=torch.int32), torch.tensor([4096, 1000, 999]),
                                     [np.int64(300), np.int32(4096), 257]])
def test_valid_lengths_become_python_ints(lengths):
    got = ragged.check_lengths(lengths, 3, 4096)
    assert got == [int(v) for v in list(lengths)] and all(type(v) is int for v in got)


@pytest.mark.parametrize("lengths,what", [
    ([300, 400], "2 lengths"),                       # wrong count
    ([300, 400, 500, 600], "4 lengths"),
    ([300, 256, 500], "outside"),                    # <= n_fft // 2: the STFT's reflect padding needs more
    ([300, 0, 500], "outside"),
    ([300, -5, 500], "outside"),
    ([300, 4097, 500], "outside"),                   # > L_max
    ([300, 400.0, 500], "integers"),                 # non-integer values
    ([300, 400.5, 500], "integers"),
    ([300, True, 500], "integers"),
    (["300", 400, 500], "integers"),
    (torch.tensor([300.0, 400.0, 500.0]), "integers"),
    (np.array([300.0, 400.0, 500.0]), "integers"),
    (torch.tensor([[300, 400, 500]]), "1-D"),
    (300, "sequence"),
])
def test_bad_lengths_are_rejected(lengths, what):
    with pytest.raises(ValueError, match=what):
        ragged.check_lengths(lengths, 3, 4096)


def test_the_bound_follows_n_fft():
    assert ragged.check_lengths([129], 1, 4096, n_fft=256) == [129]
    with pytest.raises(ValueError):
        ragged.check_lengths([128], 1, 4096, n_fft=256)


def test_frames_of_an_utterance():
    assert [ragged.frames(n) for n in (257, 511, 512, 4096, 4100, 4351, 48000)] == [2, 2, 3, 17, 17, 17, 188]


def test_pad_and_trim_round_trip():
    rng = np.random.default_rng(0)
    utts = [torch.from_numpy(rng.standard_normal(n).astype(np.float32)) for n in (300, 5003, 257)]
    utts.append(rng.standard_normal(1000))  # arrays (any float dtype) are accepted too
    noisy, lengths = ragged.pad_utterances(utts)
    assert lengths == [300, 5003, 257, 1000]
    assert noisy.shape == (4, 5003) and noisy.dtype == torch.float32 and noisy.device.type == "cpu"
    for b, n in enumerate(lengths):
        assert torch.equal(noisy[b, :n], torch.as_tensor(utts[b]).float())
        assert not noisy[b, n:].any()
    back = ragged.trim_rows(noisy, lengths)
    assert [r.shape[0] for r in back] == lengths
    assert all(torch.equal(r, noisy[b, :lengths[b]]) for b, r in enumerate(back))
    with pytest.raises(ValueError):
        ragged.pad_utterances([])
    with pytest.raises(ValueError):
        ragged.pad_utterances([torch.zeros(2, 300)])


def test_header_declares_the_ragged_entry_and_the_abi_revision():
    from fullsubnet_amd import _lib
    src = open(os.path.join(ROOT, "include", "fsn_hip.h")).read()
    assert re.search(r"int fsn_enhance_ragged\(const fsn_fullsubnet_cfg\* cfg, const void\* packed, const float\* window,"
                     r"\s+const float\* noisy, const int\* lengths, int B, int L_max, int n_fft, int hop,", src)
    assert "#define FSN_ABI_VERSION 118" in src and _lib.ABI_VERSION == 118
    restype, argtypes = _lib.SIGNATURES["fsn_enhance_ragged"]
    assert len(argtypes) == 14 and argtypes[:4] == _lib.SIGNATURES["fsn_enhance"][1][:4]
    L = _lib.lib()
    assert L.fsn_version() == 118 and hasattr(L, "fsn_enhance_ragged")

