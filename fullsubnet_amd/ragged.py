"""Host-side helpers of ragged batches: utterances of different lengths enhanced in one call
(``Model.enhance(noisy, lengths=...)``, libfsn_hip ``fsn_enhance_ragged``).

A ragged batch is ``noisy [B, L_max]`` plus ``lengths[b]`` in ``(n_fft // 2, L_max]``: row ``b`` holds one utterance
in its first ``lengths[b]`` samples, the rest of the row is padding that is never read.  Nothing here touches a device."""
import numbers

import numpy as np
import torch


def check_lengths(lengths, batch, max_length, n_fft=512):
    """Validated per-row sample counts as a list of Python ints.  ``lengths`` is a sequence of integers or a 1-D integer
    tensor / array with one entry per row; every value must lie in ``(n_fft // 2, max_length]`` (the STFT reflects up
    to ``n_fft // 2`` samples at both ends of an utterance).  Raises ``ValueError`` otherwise."""
    if isinstance(lengths, (torch.Tensor, np.ndarray)):
        if lengths.ndim != 1:
            raise ValueError(f"lengths must be 1-D, got shape {tuple(lengths.shape)}")
        is_int = (not lengths.dtype.is_floating_point and not lengths.dtype.is_complex and lengths.dtype != torch.bool
                  if isinstance(lengths, torch.Tensor) else np.issubdtype(lengths.dtype, np.integer))
        if not is_int:
            raise ValueError(f"lengths must hold integers, got dtype {lengths.dtype}")
        values = [int(v) for v in lengths.tolist()]
    else:
        try:
            values = list(lengths)
        except TypeError:
            raise ValueError(f"lengths must be a sequence of integers, got {type(lengths).__name__}") from None
        for v in values:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral):
                raise ValueError(f"lengths must hold integers, got {v!r}")
        values = [int(v) for v in values]
    if len(values) != batch:
        raise ValueError(f"{len(values)} lengths for a batch of {batch} rows")
    lo = n_fft // 2
    for b, v in enumerate(values):
        if not lo < v <= max_length:
            raise ValueError(f"lengths[{b}] = {v} is outside ({lo}, {max_length}]")
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
