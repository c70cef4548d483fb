"""Improved FullSubNet ragged batches without a device: the new C entries are declared in include/fsn_hip.h, exported and
bound with matching argument counts; each refuses bad arguments with its error code before any device call; and
``improved_fullsubnet.Model.forward(y, lengths=...)`` validates ``lengths`` before anything is launched."""
import fnmatch
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["fsn_stft_ragged_generic", "fsn_istft_ragged_workspace_bytes", "fsn_istft_ragged",
               "fsn_improved_front_norm_ragged_workspace_bytes", "fsn_improved_front_norm_ragged",
               "fsn_improved_section_input_ragged"]
ONE = 1 << 12  # a non-NULL host address: every refusal below comes before anything could be enqueued


def _header():
    return open(os.path.join(ROOT, "include", "fsn_hip.h")).read()


def _declared_args(src, name):
    """Argument count of ``name`` as include/fsn_hip.h declares it."""
    m = re.search(r"^(?:int|size_t) " + name + r"\(([^;{]*)\);", src, re.M)
    assert m, f"{name} is not declared in include/fsn_hip.h"
    args = m.group(1).strip()
    return 0 if args in ("", "void") else args.count(",") + 1


def test_new_entries_are_declared_exported_and_bound():
    from fullsubnet_amd import _lib
    src = _header()
    text = open(os.path.join(ROOT, "fullsubnet_amd", "csrc", "fsn_exports.map")).read()
    exported = re.search(r"global:\s*([^;]+);", text).group(1).split()
    L = _lib.lib()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES, name
        assert _declared_args(src, name) == len(_lib.SIGNATURES[name][1]), name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), f"{name} is not in the export map"
        assert hasattr(L, name), name
    # each ragged entry is the rectangular one plus the lengths / frames pointer
    for ragged, plain in (("fsn_stft_ragged_generic", "fsn_stft"), ("fsn_istft_ragged", "fsn_istft"),
                          ("fsn_improved_section_input_ragged", "fsn_improved_section_input")):
        assert len(_lib.SIGNATURES[ragged][1]) == len(_lib.SIGNATURES[plain][1]) + 1
        assert _declared_args(src, ragged) == _declared_args(src, plain) + 1
    assert len(_lib.SIGNATURES["fsn_stft_ragged_generic"][1]) == len(_lib.SIGNATURES["fsn_stft_ragged"][1])
    # the reference lines each new entry restates
    for name in ("fsn_stft_ragged_generic", "fsn_istft_ragged", "fsn_improved_front_norm_ragged",
                 "fsn_improved_section_input_ragged"):
        comment = src[:re.search(r"^int " + name + r"\(", src, re.M).start()].rsplit("/*", 1)[1]
        assert re.search(r"(model|feature)\.py:\d+", comment), f"{name}: no reference lines in its comment"


def test_the_abi_revision_is_unchanged():
    from fullsubnet_amd import _lib
    assert re.search(r"#define FSN_ABI_VERSION 118\b", _header())
    assert _lib.ABI_VERSION == 118 and _lib.lib().fsn_version() == 118


def test_stft_ragged_generic_refuses_bad_arguments():
    from fullsubnet_amd import _lib
    L = _lib.lib()

    def call(lengths=ONE, B=2, L_max=4000, n_fft=960, hop=480, win=None, y=ONE, window=ONE):
        return L.fsn_stft_ragged_generic(y, lengths, B, L_max, n_fft, hop, n_fft if win is None else win, window, ONE, ONE, ONE,
                                         None)

    assert call(lengths=None) == -1 and b"NULL" in L.fsn_last_error()
    assert call(y=None) == -1 and call(window=None) == -1
    for n_fft in (961, 14, 4098, 0):
        assert call(n_fft=n_fft, hop=4) == -1 and b"n_fft" in L.fsn_last_error(), n_fft
    for hop in (0, -1, 961):
        assert call(hop=hop) == -1 and b"hop" in L.fsn_last_error(), hop
    assert call(win=512) == -1 and b"win_length" in L.fsn_last_error()
    assert call(L_max=480) == -1 and call(B=0) == -1
    for n_fft, hop in ((512, 256), (512, 128), (94, 47), (1536, 768)):  # every shape fsn_stft takes, 512 / 256 included
        assert call(lengths=None, n_fft=n_fft, hop=hop) == -1 and b"NULL" in L.fsn_last_error()


def test_istft_ragged_refuses_bad_arguments():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.fsn_istft_ragged_workspace_bytes(4, 100, 960) == L.fsn_istft_workspace_bytes(4, 100, 960) > 0
    assert L.fsn_istft_ragged_workspace_bytes(4, 100, 961) == 0 and L.fsn_istft_ragged_workspace_bytes(0, 100, 960) == 0
    assert L.fsn_istft_ragged_workspace_bytes(4, 100, 8192) == 0

    def call(lengths=ONE, B=2, T=21, n_fft=960, hop=480, length=9600, ws=ONE, ws_bytes=1 << 30, real=ONE):
        return L.fsn_istft_ragged(real, ONE, lengths, B, T, n_fft, hop, n_fft, ONE, length, ONE, ws, ws_bytes, None)

    assert call(lengths=None) == -1 and b"NULL" in L.fsn_last_error()
    assert call(real=None) == -1 and call(ws=None) == -1
    for n_fft in (961, 14, 4098):
        assert call(n_fft=n_fft, hop=4) == -1 and b"n_fft" in L.fsn_last_error(), n_fft
    for hop in (0, 961):
        assert call(hop=hop) == -1 and b"hop" in L.fsn_last_error(), hop
    assert call(T=20) == -1 and b"T = 1 + length" in L.fsn_last_error()
    assert call(length=480, T=2) == -1
    assert call(B=0) == -1
    assert call(ws_bytes=L.fsn_istft_ragged_workspace_bytes(2, 21, 960) - 1) == -2


def test_front_norm_ragged_refuses_bad_arguments():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    need = L.fsn_improved_front_norm_ragged_workspace_bytes(2, 481, 21)
    assert need == L.fsn_norm_workspace_bytes(0, 2, 1, 480, 21) > 0
    assert L.fsn_improved_front_norm_ragged_workspace_bytes(2, 1, 21) == 0
    assert L.fsn_improved_front_norm_ragged_workspace_bytes(0, 481, 21) == 0

    def call(frames=ONE, B=2, F=481, T=21, mode=1, eps=1e-7, ws_bytes=1 << 30, mag=ONE, normed=ONE):
        return L.fsn_improved_front_norm_ragged(mag, frames, B, F, T, mode, eps, ONE, normed, ONE, ws_bytes, None)

    assert call(frames=None) == -1 and b"NULL" in L.fsn_last_error()
    assert call(mag=None) == -1 and call(normed=None) == -1
    assert call(F=1) == -1 and call(B=0) == -1 and call(T=0) == -1 and call(mode=2) == -1 and call(eps=0.0) == -1
    assert call(ws_bytes=need - 1) == -2


def test_section_input_ragged_refuses_bad_arguments():
    from fullsubnet_amd import _lib
    L = _lib.lib()

    def call(frames=ONE, Np=48, ldo=64, ws_bytes=1 << 30, hi=20, upper=20):
        # section 0 of the 48 kHz configuration: band [0, 20), windows 1 + 2 x 15 twice = 62 columns, 2 x 20 rows
        return L.fsn_improved_section_input_ragged(ONE, ONE, frames, 2, 480, 21, 0, upper, 1, 15, 1, 15, 0, hi, 1e-7, ONE, Np, ldo,
                                                   ONE, ws_bytes, None)

    assert call(frames=None) == -1 and b"NULL" in L.fsn_last_error()
    assert call(ldo=256) == -1 and b"240" in L.fsn_last_error()  # beyond the 64-frame tile in LDS
    assert call(ldo=48) == -1                                     # narrower than the window
    assert call(Np=65536) == -1 and b"65535" in L.fsn_last_error()
    assert call(Np=32) == -1                                      # fewer rows than B x units
    assert call(hi=21) == -1 and call(upper=481) == -1
    assert call(ws_bytes=L.fsn_improved_section_input_workspace_bytes(2, 480) - 1) == -2
    # the rectangular entry refuses the same way: one body
    assert L.fsn_improved_section_input(ONE, ONE, 2, 480, 21, 0, 20, 1, 15, 1, 15, 0, 20, 1e-7, ONE, 48, 256, ONE, 1 << 30,
                                        None) == -1


def test_existing_refusals_are_unchanged():
    """fsn_stft_ragged and fsn_mask_istft stay 512 / 256 only (tests/test_ragged_fast_cpu.py)."""
    from fullsubnet_amd import _lib
    L = _lib.lib()
    assert L.fsn_stft_ragged(ONE, ONE, 2, 4000, 512, 128, 512, ONE, ONE, ONE, ONE, None) == -1
    assert b"512" in L.fsn_last_error()
    assert L.fsn_stft_ragged(ONE, ONE, 2, 9600, 960, 480, 960, ONE, ONE, ONE, ONE, None) == -1
    assert L.fsn_mask_istft_workspace_bytes(4, 100, 960) == 0
    assert L.fsn_mask_istft(ONE, ONE, ONE, None, 2, 481, 100, 960, 480, 960, ONE, 48000, ONE, ONE, 1 << 30, None) == -1
    assert b"512" in L.fsn_last_error()


@pytest.mark.parametrize("cfg_name", ["IMPROVED_16K", "IMPROVED_48K"])
def test_forward_validates_lengths_before_any_launch(monkeypatch, cfg_name):
    import fsn_synthetic
    from fullsubnet_amd import _lib
    from fullsubnet_amd.improved_fullsubnet import Model
    cfg = getattr(fsn_synthetic, cfg_name)
    m = Model(**cfg).eval()
    half, L = cfg["n_fft"] // 2, 12000
    y = torch.zeros(2, L)
    calls = []

    def no_library():
        calls.append(1)
        raise AssertionError("the library was called")

    monkeypatch.setattr(_lib, "lib", no_library)
    bad = ([L], [L, L, L], [L, half], [L, 0], [L, -5], [L + 1, L], [L, 6000.0], torch.tensor([float(L), 6000.0]),
           torch.tensor([[L, 6000]]), [True, L], "ab", 7)
    with torch.no_grad():
        for lengths in bad:
            with pytest.raises(ValueError):
                m(y, lengths=lengths)
            with pytest.raises(ValueError):
                m(y.unsqueeze(1), lengths=lengths)
    assert not calls
