"""Validation metrics on the device (libfsn_hip ``fsn_stoi`` / ``fsn_si_sdr``): the scores of audio_zen/metrics.py that
select checkpoints, for whole ragged batches of clean / estimate pairs that are already on the device.

``stoi`` is the short-time objective intelligibility measure of Taal, Hendriks, Heusdens and Jensen (2011), what the
reference calls as ``pystoi.stoi(ref, est, sr, extended=False)``, evaluated in fp64.  It is built from the published
method and held to the fp64 numpy reference in tests/stoi_reference.py; equality with the pystoi package itself has
not been demonstrated.  There is no host fallback: a CPU tensor raises."""
import ctypes

import torch

from . import _lib
from .ragged import _integers

SAMPLE_RATES = (10000, 16000, 48000)


def _rows(a, b, names, lengths):
    """The two signals as contiguous fp32 [B, L_max] device tensors, the lengths as a device int32 tensor or None."""
    for t, name in zip((a, b), names):
        if not isinstance(t, torch.Tensor):
            raise _lib.FsnError(f"{name} must be a tensor on a ROCm device, got {type(t).__name__}")
        if not t.is_cuda:
            raise _lib.FsnError(f"{name} must live on a ROCm device (got {t.device}); this path has no CPU implementation")
    if a.dim() == 1 and b.dim() == 1:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"{names[0]} {tuple(a.shape)} and {names[1]} {tuple(b.shape)} must be two equal 1-D or 2-D shapes")
    if b.device != a.device:
        raise ValueError(f"{names[0]} is on {a.device}, {names[1]} on {b.device}")
    B, L = a.shape
    if B < 1 or L < 1:
        raise ValueError(f"an empty batch: shape {tuple(a.shape)}")
    a = a.to(torch.float32).contiguous()
    b = b.to(torch.float32).contiguous()
    d_len = None
    if lengths is not None:
        if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            if lengths.dim() != 1 or lengths.shape[0] != B or lengths.dtype.is_floating_point:
                raise ValueError(f"lengths must be {B} integers, got {tuple(lengths.shape)} {lengths.dtype}")
            d_len = lengths.to(device=a.device, dtype=torch.int32).contiguous()  # clamped into [0, L] on the device
        else:
            values = _integers(lengths, "lengths")
            if len(values) != B:
                raise ValueError(f"{len(values)} lengths for a batch of {B} rows")
            for i, v in enumerate(values):
                if not 0 <= v <= L:
                    raise ValueError(f"lengths[{i}] = {v} is outside [0, {L}]")
            d_len = torch.tensor(values, dtype=torch.int32, device=a.device)
    return a, b, d_len, B, L


def stoi(clean, estimate, sr=16000, lengths=None):
    """STOI of every row: ``clean`` / ``estimate`` [B, L_max] (or 1-D) device tensors, ``lengths`` the rows' sample counts
    (list, array or tensor; None: all L_max).  Returns a float64 tensor [B].  A row left with fewer than 30 spectral
    frames scores 1e-5, an all-zero clean or estimate row 0."""
    clean, estimate, d_len, B, L = _rows(clean, estimate, ("clean", "estimate"), lengths)
    sr = int(sr)
    if sr not in SAMPLE_RATES:
        raise _lib.FsnError(f"stoi: sr = {sr}: the sample rates are {SAMPLE_RATES}")
    lib = _lib.lib()
    with torch.cuda.device(clean.device):
        nbytes = lib.fsn_stoi_workspace_bytes(B, L, sr)
        ws = _lib.workspace(nbytes, clean.device)
        d = torch.empty(B, dtype=torch.float64, device=clean.device)
        _lib.check(lib.fsn_stoi(_lib.dev_ptr(clean, "clean"), _lib.dev_ptr(estimate, "estimate"),
                                ctypes.c_void_p(d_len.data_ptr()) if d_len is not None else None, B, L, sr,
                                ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                _lib.stream_ptr(clean.device)))
    return d


def si_sdr(reference, estimate, lengths=None):
    """SI-SDR in dB of every row (audio_zen/metrics.py:6-31, fp64 sums): float64 tensor [B]."""
    reference, estimate, d_len, B, L = _rows(reference, estimate, ("reference", "estimate"), lengths)
    lib = _lib.lib()
    with torch.cuda.device(reference.device):
        out = torch.empty(B, dtype=torch.float64, device=reference.device)
        _lib.check(lib.fsn_si_sdr(_lib.dev_ptr(reference, "reference"), _lib.dev_ptr(estimate, "estimate"),
                                  ctypes.c_void_p(d_len.data_ptr()) if d_len is not None else None, B, L,
                                  ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr(reference.device)))
    return out
