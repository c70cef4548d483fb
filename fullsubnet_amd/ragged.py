"""Host-side helpers of ragged batches: utterances of different lengths enhanced in one call
(``Model.enhance(noisy, lengths=...)``, libfsn_hip ``fsn_enhance_ragged``).

A ragged batch is ``noisy [B, L_max]`` plus ``lengths[b]`` in ``(n_fft // 2, L_max]``: row ``b`` holds one utterance
in its first ``lengths[b]`` samples, the rest of the row is padding that is never read.  Nothing here touches a device."""
import numbers

import numpy as np
import torch


def _integers(values, what):
    """A sequence of integers or a 1-D integer tensor / array -> a list of Python ints; ValueError naming ``what``."""
    if isinstance(values, (torch.Tensor, np.ndarray)):
        if values.ndim != 1:
            raise ValueError(f"{what} must be 1-D, got shape {tuple(values.shape)}")
        is_int = (not values.dtype.is_floating_point and not values.dtype.is_complex and values.dtype != torch.bool
                  if isinstance(values, torch.Tensor) else np.issubdtype(values.dtype, np.integer))
        if not is_int:
            raise ValueError(f"{what} must hold integers, got dtype {values.dtype}")
        return [int(v) for v in values.tolist()]
    try:
        out = list(values)
    except TypeError:
        raise ValueError(f"{what} must be a sequence of integers, got {type(values).__name__}") from None
    for v in out:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral):
            raise ValueError(f"{what} must hold integers, got {v!r}")
    return [int(v) for v in out]


def check_lengths(lengths, batch, max_length, n_fft=512):
    """Validated per-row sample counts as a list of Python ints.  ``lengths`` is a sequence of integers or a 1-D integer
    tensor / array with one entry per row; every value must lie in ``(n_fft // 2, max_length]`` (the STFT reflects up
    to ``n_fft // 2`` samples at both ends of an utterance).  Raises ``ValueError`` otherwise."""
    values = _integers(lengths, "lengths")
    if len(values) != batch:
        raise ValueError(f"{len(values)} lengths for a batch of {batch} rows")
    lo = n_fft // 2
    for b, v in enumerate(values):
        if not lo < v <= max_length:
            raise ValueError(f"lengths[{b}] = {v} is outside ({lo}, {max_length}]")
    return values


def check_frames(frames, batch, max_frames, look_ahead=0):
    """Validated per-row STFT frame counts of a ragged magnitude batch ``[B, 1, F, T0]`` (Fast FullSubNet's
    ``forward(mix_mag, frames=...)``), as a list of Python ints.  Same forms as ``check_lengths``; every value must lie
    in ``[max(1, 2 - look_ahead), max_frames]`` (the model's down-sampling needs two frames with the look-ahead).
    Raises ``ValueError`` otherwise."""
    values = _integers(frames, "frames")
    if len(values) != batch:
        raise ValueError(f"{len(values)} frames for a batch of {batch} rows")
    lo = max(1, 2 - look_ahead)
    for b, v in enumerate(values):
        if not lo <= v <= max_frames:
            raise ValueError(f"frames[{b}] = {v} is outside [{lo}, {max_frames}]")
    return values


def frames(length, hop=256):
    """Frames of the centred STFT of an utterance of ``length`` samples (torch.stft, center=True)."""
    return 1 + length // hop


def pad_utterances(utterances, device=None):
    """1-D utterances (tensors or arrays) -> ``(noisy [B, L_max] fp32, lengths)``: every row zero-padded to the longest.
    ``device``: where the padded batch is built (default: the first tensor's device, else the CPU)."""
    utterances = [u if isinstance(u, torch.Tensor) else torch.from_numpy(np.asarray(u)) for u in utterances]
    if not utterances:
        raise ValueError("no utterances")
    for i, u in enumerate(utterances):
        if u.dim() != 1:
            raise ValueError(f"utterance {i} is not 1-D (shape {tuple(u.shape)})")
    if device is None:
        device = utterances[0].device
    lengths = [int(u.shape[0]) for u in utterances]
    noisy = torch.zeros((len(utterances), max(lengths)), dtype=torch.float32, device=device)
    for i, u in enumerate(utterances):
        noisy[i, :lengths[i]] = u.to(device=device, dtype=torch.float32)
    return noisy, lengths


def trim_rows(batch, lengths):
    """Rows of ``batch [B, L_max]`` cut back to their lengths: a list of B 1-D views."""
    return [batch[i, :n] for i, n in enumerate(lengths)]
