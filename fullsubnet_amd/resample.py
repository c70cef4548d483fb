"""Sample-rate conversion on the device (libfsn_hip ``fsn_resample``): what the reference gets from
``librosa.load(path, sr=sr)``, for whole ragged batches that are already on the device.

The method is ``scipy.signal.resample_poly``'s - a Kaiser-windowed sinc applied as a polyphase filter, nothing read
outside the row - with three design parameters; fp64 sums, one rounding to fp32.  It is held to the fp64 numpy reference
in tests/resample_reference.py; equality with librosa's or soxr's resamplers is not claimed.  There is no
host fallback: a CPU tensor raises."""
import ctypes
import math

import torch

from . import _lib
from .ragged import _integers

# name -> (zeros, beta, rolloff): zero crossings of the sinc on either side per unit of max(up, down), the Kaiser
# window's beta, the cutoff as a fraction of the lower Nyquist rate
DESIGNS = {"scipy": (10, 5.0, 1.0),    # resample_poly(x, up, down) with its default window
           "sharp": (32, 12.0, 0.92)}  # -43 dB at the new Nyquist rate, below -120 dB past 9 / 8 of it (3 : 1)


def design_parameters(design):
    """(zeros, beta, rolloff) of a named design, or of a 3-tuple passed through."""
    if isinstance(design, str):
        if design not in DESIGNS:
            raise ValueError(f"resample design {design!r}: one of {sorted(DESIGNS)}")
        return DESIGNS[design]
    zeros, beta, rolloff = design
    return int(zeros), float(beta), float(rolloff)


def ratio(sr_in, sr_out):
    """(up, down) of sr_in -> sr_out in lowest terms."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in < 1 or sr_out < 1:
        raise ValueError(f"sample rates must be positive, got {sr_in} -> {sr_out}")
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def out_length(n, sr_in, sr_out):
    """Samples of an ``n``-sample signal after sr_in -> sr_out: ceil(n up / down).  Host arithmetic."""
    up, down = ratio(sr_in, sr_out)
    n = int(n)
    if n < 0:
        raise ValueError(f"n = {n}")
    return -(-n * up // down)


def resample(y, sr_in, sr_out, lengths=None, design="scipy"):
    """``y`` [B, L_max] (or 1-D) fp32 on the device at ``sr_in`` -> ``(out, out_lengths)`` at ``sr_out``: ``out``
    [B, out_length(L_max)] (1-D for a 1-D input), row b holding ``out_lengths[b] = out_length(lengths[b])`` samples and
    zeros behind them; ``out_lengths`` an int32 device tensor [B].  ``lengths``: the rows' sample counts (list, array or
    tensor; None: all L_max); nothing behind a row's length is read.  One library call, no copy, no synchronisation."""
    if not isinstance(y, torch.Tensor):
        raise _lib.FsnError(f"y must be a tensor on a ROCm device, got {type(y).__name__}")
    if not y.is_cuda:
        raise _lib.FsnError(f"y must live on a ROCm device (got {y.device}); this path has no CPU implementation")
    one_d = y.dim() == 1
    if one_d:
        y = y.unsqueeze(0)
    if y.dim() != 2 or y.shape[0] < 1 or y.shape[1] < 1:
        raise ValueError(f"y must be a non-empty 1-D or 2-D signal batch, got shape {tuple(y.shape)}")
    zeros, beta, rolloff = design_parameters(design)
    B, L = y.shape
    L_out = out_length(L, sr_in, sr_out)
    if L_out > 2 ** 31 - 1:
        raise ValueError(f"{L} samples at {sr_in} -> {sr_out} Hz are {L_out}: more than a row holds")
    y = y.to(torch.float32).contiguous()
    d_len = None
    if lengths is not None:
        if isinstance(lengths, torch.Tensor) and lengths.is_cuda:
            if lengths.dim() != 1 or lengths.shape[0] != B or lengths.dtype.is_floating_point:
                raise ValueError(f"lengths must be {B} integers, got {tuple(lengths.shape)} {lengths.dtype}")
            d_len = lengths.to(device=y.device, dtype=torch.int32).contiguous()  # clamped into [0, L] on the device
        else:
            values = _integers(lengths, "lengths")
            if len(values) != B:
                raise ValueError(f"{len(values)} lengths for a batch of {B} rows")
            for i, v in enumerate(values):
                if not 0 <= v <= L:
                    raise ValueError(f"lengths[{i}] = {v} is outside [0, {L}]")
            d_len = torch.tensor(values, dtype=torch.int32, device=y.device)
    lib = _lib.lib()
    with torch.cuda.device(y.device):
        nbytes = lib.fsn_resample_workspace_bytes(int(sr_in), int(sr_out), zeros, beta, rolloff)
        ws = _lib.workspace(nbytes, y.device)
        out = torch.empty((B, L_out), dtype=torch.float32, device=y.device)
        out_lengths = torch.empty(B, dtype=torch.int32, device=y.device)
        _lib.check(lib.fsn_resample(_lib.dev_ptr(y, "y"), ctypes.c_void_p(d_len.data_ptr()) if d_len is not None else None,
                                    B, L, int(sr_in), int(sr_out), zeros, beta, rolloff, _lib.dev_ptr(out, "out"), L_out,
                                    ctypes.c_void_p(out_lengths.data_ptr()), ctypes.c_void_p(ws.data_ptr()), nbytes,
                                    _lib.stream_ptr(y.device)))
    return (out[0] if one_d else out), out_lengths


def taps(sr_in, sr_out, design="scipy", device="cuda"):
    """The filter ``h`` [2H + 1] of sr_in -> sr_out as the library forms it (float64, on the device)."""
    zeros, beta, rolloff = design_parameters(design)
    up, down = ratio(sr_in, sr_out)
    n = 2 * zeros * max(up, down) + 1
    device = torch.device(device)
    h = torch.empty(n, dtype=torch.float64, device=device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().fsn_resample_taps(int(sr_in), int(sr_out), zeros, beta, rolloff, ctypes.c_void_p(h.data_ptr()), n,
                                                _lib.stream_ptr(device)))
    return h


def plan(sr_in, sr_out, design="scipy"):
    """How the library spreads sr_in -> sr_out over workgroups (fsn_debug_resample_plan; a test hook)."""
    zeros = design_parameters(design)[0]
    buf = (ctypes.c_int * 10)()
    _lib.check(_lib.lib().fsn_debug_resample_plan(int(sr_in), int(sr_out), zeros, buf, 10))
    keys = ("up", "down", "half", "taps", "taps_per_phase", "row_stride", "tile_outputs", "tile_inputs", "stretch", "taps_in_lds")
    return dict(zip(keys, list(buf)))
