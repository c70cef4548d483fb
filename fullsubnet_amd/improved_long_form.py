"""Recordings of any length on Improved FullSubNet: ``improved_fullsubnet.Model.enhance_long``.

``model(y)`` keeps gate planes of hidden-state width for every frame of every band section ([T][rows][4 x 384] floats at
48 kHz): a minute of one utterance costs gigabytes, and a 10 ms hop gives 360 001 frames per hour.  Here the model runs in
segments of k frames with carried LSTM state; what lives for the whole recording are planes of F floats per frame -
magnitude, spectrum (re, im), mask - and, under the offline section norm, the full-band model's output.

The reference normalises twice with one mean per utterance: in front of the full-band model, and in front of every band
section over the section's unfolded windows of the noisy magnitude and of the full-band output.  A recording therefore
takes three passes over its segments (libfsn_hip ``fsn_improved_segment_*``): (1) the magnitude's sum, (2) the full-band
model, which needs the first mean, and the sections' sums, (3) the sections, which need those.  With ``norm_type =
"cumulative_laplace_norm"`` the reference's sections stay offline: pass 2 carries the running mean itself and pass 1 is
not run.  A model whose sections are causal too (``sb_norm_type = "cumulative_laplace_norm"``) is one pass of
``fsn_improved_stream_step`` over the same segments.  Segments, slabs and transforms are the shared driver's
(``long_form.run_segments``), at the model's own n_fft and hop = n_fft / 2 and with no look-ahead."""
import ctypes
from functools import partial

from . import _lib
from .long_form import SLAB_FRAMES, SegmentPlan, run_segments

# the passes a model's pair of norms takes: (norm_type, sb_norm_type or "offline_laplace_norm") -> name
OFFLINE, CUMULATIVE_OFFLINE, CUMULATIVE = "offline", "cumulative/offline", "cumulative"
PASSES = {("offline_laplace_norm", "offline_laplace_norm"): OFFLINE,
          ("cumulative_laplace_norm", "offline_laplace_norm"): CUMULATIVE_OFFLINE,
          ("cumulative_laplace_norm", "cumulative_laplace_norm"): CUMULATIVE}


class ImprovedLongPlan(SegmentPlan):
    """``SegmentPlan`` of Improved FullSubNet.  ``cfg``: the model's ``stream_cfg()`` (``_lib.ImprovedCfg``), ``n_fft`` its
    transform, ``passes`` one of ``PASSES``' values.  The steps are the frames.  ``fb_out`` (F - 1 floats per frame and row)
    lives for the whole recording only when a pass needs it: not for a model that is causal throughout."""

    LINEAR = ("mag", "spec_re", "spec_im", "mask", "fb_out", "enhanced")
    MASK_PLANES = 2 + 2  # no decompressed mask

    def __init__(self, cfg, n_fft, passes, batch, num_samples, segment_frames=None, workspace_limit=4 << 30,
                 slab_frames=SLAB_FRAMES):
        L, c = _lib.lib(), ctypes.byref(cfg)
        if passes not in PASSES.values():
            raise _lib.FsnError(f"enhance_long: passes {passes!r}, expected one of {sorted(PASSES.values())}")
        self.passes = passes
        super().__init__(n_fft, 0, cfg.F, partial(L.fsn_improved_stream_state_bytes, c), partial(L.fsn_improved_stream_workspace_bytes, c),
                         1 + 2, {"fb_out": 0 if passes == CUMULATIVE else 4 * batch * (cfg.F - 1)}, batch, num_samples, segment_frames,
                         workspace_limit, slab_frames)


def refuse(model, n_fft=None, hop_length=None):
    """What ``enhance_long`` does not take, as an ``FsnError`` that names the path that does; -> (the model's
    ``ImprovedCfg``, its passes).  Needs no device."""
    L = _lib.lib()
    if any(m.cell != "LSTM" for m in (model.fb_model, *model.sb_model.sb_models)):
        raise _lib.FsnError("enhance_long is built for LSTM cells (the segment entries carry (h, c) of fsn_lstm_layer_forward_state); "
                            "use model(y) for a GRU model")
    n_fft = model.n_fft if n_fft is None else n_fft
    hop_length = model.hop_length if hop_length is None else hop_length
    if (n_fft, hop_length) != (model.n_fft, model.hop_length):
        raise _lib.FsnError(f"enhance_long runs the model's own transform (n_fft {model.n_fft} / hop {model.hop_length}), got n_fft "
                            f"{n_fft} / hop {hop_length}; use model(y) of a model built for that transform")
    if 2 * model.hop_length != model.n_fft or model.win_length != model.n_fft or model.num_freqs != model.n_fft // 2 + 1:
        raise _lib.FsnError(f"enhance_long is built for hop = n_fft / 2 and win_length = n_fft (960 / 480 at 48 kHz; the slabbed "
                            f"transforms carry half a frame), the model has n_fft {model.n_fft} / hop {model.hop_length} / win_length "
                            f"{model.win_length} on {model.num_freqs} bins; use model(y) for this transform")
    norms = (model.norm_type, model.sb_norm_type or "offline_laplace_norm")
    if norms not in PASSES:
        why = ("its sections would need a mean that its full-band norm has not got yet" if norms[0] == "offline_laplace_norm"
               and norms[1] == "cumulative_laplace_norm" else "the passes carry sums, not variances")
        raise _lib.FsnError(f"enhance_long takes norm_type / sb_norm_type offline / offline (or None), cumulative / offline (or None) "
                            f"and cumulative / cumulative, the model is built with {model.norm_type!r} / {model.sb_norm_type!r} ({why}); "
                            "use model(y) for these norms")
    cfg = model.stream_cfg()
    if L.fsn_improved_stream_state_bytes(ctypes.byref(cfg), 1) == 0:
        raise _lib.FsnError(f"enhance_long: {L.fsn_last_error().decode()}; use model(y) for this configuration")
    return cfg, PASSES[norms]


def mask_parts(crm, re, im):
    """model.py:575-577: the mask multiplies real and imaginary parts separately (no decompression, no complex product)."""
    return crm[:, 0] * re, crm[:, 1] * im


def _passes(model, icfg, on_stage, plan, total, mag, sargs, wargs, new, keep):
    """One pass of the stream step for a model that is causal throughout, else (stats,) full-band model, sections."""
    L, st, cfg, (B, F, T) = _lib.lib(), _lib.stream_ptr(mag.device), ctypes.byref(icfg), mag.shape
    done = on_stage or (lambda stage: None)
    packed = model.stream_packed_weights().data_ptr()
    # a segment's frames as the entries take them; the caller holds the copy until the entry has been issued
    segment = lambda s0, k: mag[:, :, s0:s0 + k].contiguous()  # noqa: E731
    if plan.passes == CUMULATIVE:
        for s0, k in plan.segments:
            x, c = segment(s0, k), new(B, 2, F, k)
            _lib.check(L.fsn_improved_stream_step(cfg, packed, *sargs, s0, _lib.dev_ptr(x, "mag"), B, k, _lib.dev_ptr(c), *wargs, st))
            keep(s0, k, c)
        return done("stream_step")
    fb_out = new(T, B, F - 1)  # time-major: a segment is a contiguous slice
    if plan.passes == OFFLINE:
        for s0, k in plan.segments:
            x = segment(s0, k)
            _lib.check(L.fsn_improved_segment_stats(cfg, *sargs, s0, total.data_ptr(), _lib.dev_ptr(x, "mag"), B, k, st))
        done("stats")
    for s0, k in plan.segments:
        x = segment(s0, k)
        _lib.check(L.fsn_improved_segment_fullband(cfg, packed, *sargs, 0 if plan.passes == OFFLINE else 1, s0, total.data_ptr(),
                                                   _lib.dev_ptr(x, "mag"), B, k, _lib.dev_ptr(fb_out[s0:s0 + k]), *wargs, st))
    done("fullband")
    for s0, k in plan.segments:
        x, c = segment(s0, k), new(B, 2, F, k)
        _lib.check(L.fsn_improved_segment_sections(cfg, packed, *sargs, s0, total.data_ptr(), _lib.dev_ptr(x, "mag"),
                                                   _lib.dev_ptr(fb_out[s0:s0 + k]), B, k, _lib.dev_ptr(c), *wargs, st))
        keep(s0, k, c)
    done("sections")


def enhance_long(model, noisy, lengths=None, segment_frames=None, workspace_limit=4 << 30, return_crm=False, poison=False,
                 n_fft=None, hop_length=None, slab_frames=SLAB_FRAMES, on_stage=None):
    """See ``improved_fullsubnet.Model.enhance_long``.  ``on_stage`` (measurement, tools/bench_long_improved.py): called with
    the name of every stage of the run as it ends."""
    icfg, passes = refuse(model, n_fft, hop_length)
    return run_segments(model, noisy, lengths, model.n_fft, partial(ImprovedLongPlan, icfg, model.n_fft, passes),
                        (segment_frames, workspace_limit, slab_frames), partial(_passes, model, icfg, on_stage), mask_parts, "model(y)",
                        return_crm, poison, on_stage)
