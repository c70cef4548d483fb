"""The centred STFT and its inverse in slabs of frames: what ``StreamingEnhancer`` (frames as their samples arrive) and
``enhance_long`` (a recording too long for one transform call) share.  hop = n_fft / 2 throughout, like every FullSubNet
TOML.

Analysis: frame t >= 1 covers the samples ``t hop - half .. t hop + half - 1``; frame 0 mirrors sample ``half`` on its left
side and the last frame of a recording (``n // hop``) mirrors at the right edge.  A slab of frames ``t_first .. t_last`` is
``stft`` of the samples from two frames of history on (so that the slab is longer than its own reflect padding, and the
reflection of the slab's left edge only reaches frames that are thrown away) up to the last sample the slab's last frame
needs - or to the recording's end, whose reflection is then the true one.

Synthesis: the inverse of frames ``first .. `` needs the frame before them as overlap-add partner; it is carried from slab
to slab as one enhanced frame (re, im) ``[B, F, 1]``."""
import torch

from .acoustics.feature import istft, stft


def analysis_bounds(t_first, t_last, n_samples, final, n_fft, hop):
    """(j0, a, b): ``stft`` of the samples [a, b) has the frames j0 .. of the recording; those from ``t_first`` to ``t_last``
    are exact.  ``n_samples``: samples known so far; ``final``: they are the whole recording (its right edge is real)."""
    half = n_fft // 2
    j0 = max(t_first - 2, 0)
    b = n_samples if final else max(t_last * hop + half, half + 1)
    return j0, j0 * hop, b


def analysis_slab(samples, j0, t_first, t_last, n_fft, hop):
    """samples [B, b - a] of ``analysis_bounds`` -> (mag, re, im) [B, F, t_last - t_first + 1] of frames t_first .. t_last."""
    mag, _, re, im = stft(samples.contiguous(), n_fft, hop, n_fft, return_phase=False)
    lo, hi = t_first - j0, t_last - j0 + 1
    return tuple(x[:, :, lo:hi].contiguous() for x in (mag, re, im))


def synthesis_slab(er, ei, prev, first, n_out, n_fft, hop, total_length=None):
    """Enhanced frames ``first ..`` (er, ei [B, F, k]) -> (their samples that are final and not yet emitted [B, n] or None,
    the frame to carry).  ``prev``: the carried frame ``first - 1`` (None at the start); ``n_out``: samples emitted so far;
    ``total_length``: the recording's length when these are its last frames (the tail behind the last hop follows)."""
    if prev is not None:
        er = torch.cat([prev[0], er], dim=-1)
        ei = torch.cat([prev[1], ei], dim=-1)
        first -= 1
    carry = (er[..., -1:].contiguous(), ei[..., -1:].contiguous())
    length = (er.shape[-1] - 1) * hop if total_length is None else total_length - first * hop
    if length <= 0:
        return None, carry
    y = istft((er.contiguous(), ei.contiguous()), n_fft, hop, n_fft, length=length, input_type="real_imag")
    skip = n_out - first * hop  # samples of this slab already emitted (none in steady state)
    return y[:, skip:], carry
