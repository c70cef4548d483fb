"""audio_zen/acoustics/rvb.py on the device: the reverberation-time-shortening target of Zhou, Zhu and Li (2022),
"Speech Dereverberation With a Reverberation Time Shortening Target" (fsn_rir_shorten, include/fsn_hip.h)."""
import math

import numpy as np
import torch

from .. import _lib
from ..mix import TARGET_DTYPE, shortening_q


def reverberation_time_shortening(rir, original_T60, target_T60, sr=16000, time_after_max=0.002):
    """(shortened rir, window), both fp32 device tensors of rir's shape: the window is 1 up to `time_after_max` behind the
    FIRST maximum of |rir| and 10^(-q n) from there on, q = 3 / (target_T60 sr) - 3 / (original_T60 sr), formed in fp64 and
    rounded to fp32; the result is rir * window in fp32 - the reference's arithmetic on a float32 response.

    rir: a 1-D fp32 device tensor, as the reference takes it, or - an extension - a 2-D batch [B, n] of responses, for
    which original_T60 and target_T60 may be sequences with a value per row.  One launch, enqueued on the current stream
    (the small descriptor table goes up from pinned memory without a synchronisation)."""
    if rir.dim() not in (1, 2):
        raise _lib.FsnError("rir must be a 1-D response or a 2-D batch of responses")
    rows = rir.reshape(1, -1) if rir.dim() == 1 else rir
    _lib.dev_ptr(rows, "rir")
    B, n = rows.shape
    if B < 1 or n < 1:
        raise _lib.FsnError("rir is empty")
    orig = np.broadcast_to(np.asarray(original_T60, dtype=np.float64).reshape(-1), (B,))
    tgt = np.broadcast_to(np.asarray(target_T60, dtype=np.float64).reshape(-1), (B,))
    if rir.dim() == 1 and (np.ndim(original_T60) or np.ndim(target_T60)):
        raise _lib.FsnError("a 1-D response takes one original_T60 and one target_T60")
    tab = np.zeros(B, TARGET_DTYPE)
    for b in range(B):
        tab[b] = (shortening_q(float(orig[b]), float(tgt[b]), sr), int(math.floor(time_after_max * sr)), 1)
    # one pinned block: offsets (long), lengths (int), descriptors - each part 16-byte aligned
    off_at, len_at = 0, (8 * B + 15) // 16 * 16
    tab_at = (len_at + 4 * B + 15) // 16 * 16
    host = torch.empty(tab_at + tab.nbytes, dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    hv[off_at:off_at + 8 * B] = (np.arange(B, dtype=np.int64) * n).view(np.uint8)
    hv[len_at:len_at + 4 * B] = np.full(B, n, np.int32).view(np.uint8)
    hv[tab_at:] = tab.view(np.uint8)
    dev = rows.device
    with torch.cuda.device(dev):
        desc = host.to(dev, non_blocking=True)
        out, win = torch.empty_like(rows), torch.empty_like(rows)
        p = desc.data_ptr()
        _lib.check(_lib.lib().fsn_rir_shorten(rows.data_ptr(), 0, p + off_at, p + len_at, B, n, p + tab_at,
                                              _lib.dev_ptr(out, "out"), n, _lib.dev_ptr(win, "win"), None,
                                              _lib.stream_ptr(dev)))
    return out.reshape(rir.shape), win.reshape(rir.shape)
