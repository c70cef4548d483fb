"""Recordings of any length on Fast FullSubNet: ``fast_fullsubnet.Model.enhance_long``.

``Model.enhance`` stops at 65 535 frames (17.5 minutes at hop 256 / 16 kHz, and only after the encoder has run) and its
memory grows with the recording at hidden-state width (the bottleneck's ``[Ts, B 64, 384]`` sequences, the decoder's
``[T, Bp, 512]``).  Here the model runs in segments of k steps with carried state; what lives for the whole recording are
planes of F floats per frame - magnitude, spectrum (re, im), mask - and two planes of 64 floats per step, the mel spectrum
and the encoder's output.

The shipped norm (``offline_laplace_norm``) divides by one mean per utterance and this model applies it twice, so a
recording takes three passes over its segments (libfsn_hip ``fsn_fast_segment_*``): (1) the mel spectrum and its sum, (2)
the encoder, which needs the first mean, and the sum of the down-sampled unit tensor, (3) the bottleneck and the decoder,
which need the second.  A ``cumulative_laplace_norm`` model is causal: one pass of ``fsn_fast_stream_step`` over the same
segments.  Segments, slabs, transforms and the cIRM product are the shared driver's (``long_form.run_segments``)."""
import ctypes
from functools import partial

from . import _lib
from .long_form import HOP, N_FFT, SLAB_FRAMES, SegmentPlan, cirm_mask, run_segments

OFFLINE, CUMULATIVE = _lib.NORM_TYPES["offline_laplace_norm"], _lib.NORM_TYPES["cumulative_laplace_norm"]


class FastLongPlan(SegmentPlan):
    """``SegmentPlan`` of Fast FullSubNet.  ``cfg``: the model's ``stream_cfg()`` (``_lib.FastCfg``; its norm decides the
    passes and the size queries), ``look_ahead`` the model's.  Under the offline norm ``mel`` and ``enc`` live for the whole
    recording too: 64 floats per step and padded row."""

    LINEAR = ("mag", "spec_re", "spec_im", "mask", "mel", "enc", "enhanced")

    def __init__(self, cfg, look_ahead, batch, num_samples, segment_frames=None, workspace_limit=4 << 30, slab_frames=SLAB_FRAMES):
        L, c = _lib.lib(), ctypes.byref(cfg)
        self.offline = cfg.norm == OFFLINE
        state_of, workspace_of = ((L.fsn_fast_segment_state_bytes, L.fsn_fast_segment_workspace_bytes) if self.offline else
                                  (L.fsn_fast_stream_state_bytes, L.fsn_fast_stream_workspace_bytes))
        band = 4 * ((batch + 15) // 16 * 16) * cfg.num_mels if self.offline else 0
        super().__init__(N_FFT, look_ahead, cfg.F, partial(state_of, c), partial(workspace_of, c), 1 + 2, {"mel": band, "enc": band},
                         batch, num_samples, segment_frames, workspace_limit, slab_frames)


def refuse(model, n_fft, hop_length):
    """What ``enhance_long`` does not take, as an ``FsnError`` that names the path that does; -> the model's ``FastCfg``."""
    L = _lib.lib()
    if any(b.cell != "LSTM" for b in (*model.encoder, model.bottleneck, *model.decoder_lstm)):
        raise _lib.FsnError("enhance_long is built for LSTM cells (the segment entries carry (h, c) of fsn_lstm_layer_forward_state); "
                            "use Model.enhance for a GRU model")
    if (n_fft, hop_length) != (N_FFT, HOP) or model.num_freqs != N_FFT // 2 + 1:
        raise _lib.FsnError(f"enhance_long is built for n_fft {N_FFT} / hop {HOP} ({N_FFT // 2 + 1} bins) only, got n_fft {n_fft} / "
                            f"hop {hop_length} on a model of {model.num_freqs} bins (the slabbed transforms carry half a frame); use "
                            "Model.enhance for this transform")
    cfg = model.stream_cfg()
    if cfg.norm not in (OFFLINE, CUMULATIVE):
        raise _lib.FsnError(f"enhance_long takes offline_laplace_norm or cumulative_laplace_norm, the model is built with "
                            f"{model.norm_type!r}; use Model.enhance for this norm")
    size = (L.fsn_fast_segment_state_bytes if cfg.norm == OFFLINE else L.fsn_fast_stream_state_bytes)(ctypes.byref(cfg), 1)
    if size == 0:
        raise _lib.FsnError(f"enhance_long: {L.fsn_last_error().decode()}; use Model.enhance for this configuration")
    return cfg


def _passes(model, fcfg, plan, total, mag, sargs, wargs, new, keep):
    """Three passes over the segments under the offline norm, one pass of the stream step under the causal one."""
    L, st, cfg, (B, F, Tp) = _lib.lib(), _lib.stream_ptr(mag.device), ctypes.byref(fcfg), mag.shape
    # the packing entry takes the causal norm only; the blob's layout does not depend on the norm
    packed = model.stream_packed_weights(norm=CUMULATIVE if plan.offline else None).data_ptr()
    if not plan.offline:
        for s0, k in plan.segments:
            x, c = mag[:, :, s0:s0 + k].contiguous(), new(B, 2, F, k)
            _lib.check(L.fsn_fast_stream_step(cfg, packed, *sargs, s0, _lib.dev_ptr(x, "mag"), B, k, _lib.dev_ptr(c), *wargs, st))
            keep(s0, k, c)
        return
    Bp = (B + 15) // 16 * 16
    mel, enc = new(Tp, Bp, model.num_mels), new(Tp, Bp, model.num_mels)  # time-major: a segment is a contiguous slice
    for s0, k in plan.segments:
        x = mag[:, :, s0:s0 + k].contiguous()
        _lib.check(L.fsn_fast_segment_stats(cfg, packed, *sargs, _lib.dev_ptr(x, "mag"), B, k, _lib.dev_ptr(mel[s0:s0 + k]),
                                            *wargs, st))
    for s0, k in plan.segments:
        _lib.check(L.fsn_fast_segment_encoder(cfg, packed, *sargs, s0, total.data_ptr(), _lib.dev_ptr(mel[s0:s0 + k]), B, k,
                                              _lib.dev_ptr(enc[s0:s0 + k]), *wargs, st))
    for s0, k in plan.segments:
        c = new(B, 2, F, k)
        _lib.check(L.fsn_fast_segment_decoder(cfg, packed, *sargs, s0, total.data_ptr(), _lib.dev_ptr(mel[s0:s0 + k]),
                                              _lib.dev_ptr(enc[s0:s0 + k]), B, k, _lib.dev_ptr(c), *wargs, st))
        keep(s0, k, c)


def enhance_long(model, noisy, lengths=None, segment_frames=None, workspace_limit=4 << 30, return_crm=False, poison=False,
                 n_fft=N_FFT, hop_length=HOP, slab_frames=SLAB_FRAMES):
    """See ``fast_fullsubnet.Model.enhance_long``."""
    fcfg = refuse(model, n_fft, hop_length)
    return run_segments(model, noisy, lengths, n_fft, partial(FastLongPlan, fcfg, model.look_ahead),
                        (segment_frames, workspace_limit, slab_frames), partial(_passes, model, fcfg), cirm_mask, "Model.enhance",
                        return_crm, poison)
