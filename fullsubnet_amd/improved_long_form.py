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
``fsn_improved_stream_step`` over the same segments.  The transforms run in slabs of frames (``slabs.py``) with the model's
own n_fft and hop = n_fft / 2.

``ImprovedLongPlan`` is the host book-keeping of one run - segments, slabs and the bytes of everything the run allocates -
with no device call, like ``fast_long_form.FastLongPlan``."""
import ctypes

import torch

from . import _lib
from .long_form import MAX_SEGMENT_FRAMES, SLAB_FRAMES
from .ragged import check_lengths, frames
from .slabs import analysis_bounds, analysis_slab, synthesis_slab

# the passes a model's pair of norms takes: (norm_type, sb_norm_type or "offline_laplace_norm") -> name
OFFLINE, CUMULATIVE_OFFLINE, CUMULATIVE = "offline", "cumulative/offline", "cumulative"
PASSES = {("offline_laplace_norm", "offline_laplace_norm"): OFFLINE,
          ("cumulative_laplace_norm", "offline_laplace_norm"): CUMULATIVE_OFFLINE,
          ("cumulative_laplace_norm", "cumulative_laplace_norm"): CUMULATIVE}


class ImprovedLongPlan:
    """What ``enhance_long`` does for ``batch`` rows of up to ``num_samples`` samples, without doing it.

    ``cfg``: the model's ``stream_cfg()`` (``_lib.ImprovedCfg``), ``n_fft`` its transform (hop = n_fft / 2), ``passes`` one
    of ``PASSES``' values.  ``segments``: (first frame, k) of the model calls of every pass - the frames in order, each
    exactly once, 1 <= k <= 4096.  ``slabs``: (first frame, end frame, samples read [lo, hi), samples written [lo, hi)) of
    the transform calls; the written ranges tile [0, num_samples).  ``bytes``: name -> bytes of every allocation of the run
    (device memory); ``total_bytes`` their sum.  Only the entries of ``LINEAR`` grow with the recording: by F floats (F - 1
    for ``fb_out``, a hop of samples for ``enhanced``) per frame and row; ``fb_out`` is there only when a pass needs it
    (not for a model that is causal throughout)."""

    LINEAR = ("mag", "spec_re", "spec_im", "mask", "fb_out", "enhanced")

    def __init__(self, cfg, n_fft, passes, batch, num_samples, segment_frames=None, workspace_limit=4 << 30,
                 slab_frames=SLAB_FRAMES):
        L = _lib.lib()
        if passes not in PASSES.values():
            raise _lib.FsnError(f"enhance_long: passes {passes!r}, expected one of {sorted(PASSES.values())}")
        if batch < 1 or num_samples <= n_fft // 2:
            raise _lib.FsnError(f"enhance_long: batch {batch} / {num_samples} samples (need more than n_fft / 2 = {n_fft // 2})")
        self.batch, self.num_samples, self.passes = batch, num_samples, passes
        self.n_fft, self.hop = n_fft, n_fft // 2
        self.frames = frames(num_samples, self.hop)
        query = lambda k: L.fsn_improved_stream_workspace_bytes(ctypes.byref(cfg), batch, k)  # noqa: E731
        if segment_frames is None:
            # the workspace grows with k: the largest k under the limit, by bisection
            lo, hi = 1, min(MAX_SEGMENT_FRAMES, self.frames)
            if not 0 < query(lo) <= workspace_limit:
                raise _lib.FsnError(f"enhance_long: one frame of {batch} rows needs {query(lo)} bytes of workspace, the limit "
                                    f"is {workspace_limit} ({L.fsn_last_error().decode() if query(lo) == 0 else 'lower the batch'})")
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if query(mid) <= workspace_limit else (lo, mid - 1)
            segment_frames = lo
        segment_frames = int(segment_frames)
        if not 1 <= segment_frames <= MAX_SEGMENT_FRAMES:
            raise _lib.FsnError(f"enhance_long: segment_frames {segment_frames} outside [1, {MAX_SEGMENT_FRAMES}]")
        self.segment_frames = k = min(segment_frames, self.frames)
        self.segments = [(s, min(k, self.frames - s)) for s in range(0, self.frames, k)]
        self.slab_frames = max(2, int(slab_frames))
        self.slabs = self.slabs_of(num_samples)
        state, workspace = L.fsn_improved_stream_state_bytes(ctypes.byref(cfg), batch), query(k)
        if state == 0 or workspace == 0:
            raise _lib.FsnError(f"enhance_long: {L.fsn_last_error().decode()}")
        T, S, F = self.frames, min(self.slab_frames + 1, self.frames), cfg.F
        plane = 4 * batch * F
        self.bytes = {
            "state": state, "workspace": workspace,
            # linear in the recording: planes of F floats per frame, and the result
            "mag": plane * T, "spec_re": plane * T, "spec_im": plane * T, "mask": 2 * plane * T,
            "fb_out": 0 if passes == CUMULATIVE else 4 * batch * (F - 1) * T,
            "enhanced": 4 * batch * num_samples,
            # bounded: what one segment / one slab passes to and takes from the library
            "segment_io": (1 + 2) * plane * k,
            "slab_samples": 4 * batch * (S + 2) * self.hop, "slab_spectra": 3 * plane * (S + 2),
            "slab_enhanced": (2 + 2) * plane * S + 4 * batch * S * self.hop + 4 * batch * S * n_fft,
            "total_frames": 4 * batch,
        }
        self.total_bytes = sum(self.bytes.values())

    def slabs_of(self, n):
        """The transform calls over a row of n samples (a ragged batch transforms each row over its own length)."""
        T, out = frames(n, self.hop), []
        for t0 in range(0, T, self.slab_frames):
            t1 = min(t0 + self.slab_frames, T)
            _, a, b = analysis_bounds(t0, t1 - 1, n, t1 == T, self.n_fft, self.hop)
            out.append((t0, t1, (a, b), (max(t0 - 1, 0) * self.hop, n if t1 == T else (t1 - 1) * self.hop)))
        return out


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


@torch.no_grad()
def enhance_long(model, noisy, lengths=None, segment_frames=None, workspace_limit=4 << 30, return_crm=False, poison=False,
                 n_fft=None, hop_length=None, slab_frames=SLAB_FRAMES, on_stage=None):
    """See ``improved_fullsubnet.Model.enhance_long``.  ``on_stage`` (measurement, tools/bench_long_improved.py): called with
    the name of every stage of the run as it ends."""
    icfg, passes = refuse(model, n_fft, hop_length)
    n_fft, hop = model.n_fft, model.hop_length
    assert noisy.dim() == 2
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.FsnError("enhance_long needs the model on a ROCm device (this path has no CPU implementation); "
                            "model(y) runs a host model")
    B, Lmax = noisy.shape
    lens = [Lmax] * B if lengths is None else check_lengths(lengths, B, Lmax, n_fft)
    plan = ImprovedLongPlan(icfg, n_fft, passes, B, Lmax, segment_frames, workspace_limit, slab_frames)
    cfg, F, T = ctypes.byref(icfg), model.num_freqs, plan.frames
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    fill = float("nan") if poison else None  # test hook: whatever is read must have been written first

    def new(*shape):
        t = torch.empty(shape, dtype=torch.float32, device=dev)
        return t.fill_(fill) if poison else t

    def done(stage):
        if on_stage is not None:
            on_stage(stage)

    # rows that share a length are transformed together; a ragged batch row by row, each over its own samples
    groups = [(slice(0, B), Lmax)] if len(set(lens)) == 1 and lens[0] == Lmax else [(slice(b, b + 1), n) for b, n in enumerate(lens)]
    mag, re, im, crm = new(B, F, T), new(B, F, T), new(B, F, T), new(B, 2, F, T)

    # ---- STFT in slabs ----------------------------------------------------------------------------------------------
    for rows, n in groups:
        for t0, t1, (a, b), _ in plan.slabs_of(n):
            m, r, i = analysis_slab(noisy[rows, a:b].to(dev, torch.float32), a // hop, t0, t1 - 1, n_fft, hop)
            mag[rows, :, t0:t1], re[rows, :, t0:t1], im[rows, :, t0:t1] = m, r, i
        mag[rows, :, frames(n, hop):] = 0.0  # a shorter row's padding (the entries do not read it)
    done("stft")

    # ---- the model over the segments ----------------------------------------------------------------------------------
    state = torch.empty(plan.bytes["state"], dtype=torch.uint8, device=dev)
    if poison:
        state.view(torch.float32).fill_(fill)
    state.zero_()  # a fresh recording
    ws = _lib.workspace(plan.bytes["workspace"], dev)
    if poison:
        ws.view(torch.float32).fill_(fill)
    packed = model.stream_packed_weights().data_ptr()
    sargs, wargs = (state.data_ptr(), state.numel()), (ws.data_ptr(), ws.numel())
    # a segment's frames as the entries take them; the caller holds the copy until the entry has been issued
    segment = lambda s0, k: mag[:, :, s0:s0 + k].contiguous()  # noqa: E731

    def keep(s0, k, c):
        crm[:, :, :, s0:s0 + k] = c

    if passes == CUMULATIVE:
        for s0, k in plan.segments:
            x, c = segment(s0, k), new(B, 2, F, k)
            _lib.check(L.fsn_improved_stream_step(cfg, packed, *sargs, s0, _lib.dev_ptr(x, "mag"), B, k, _lib.dev_ptr(c), *wargs, st))
            keep(s0, k, c)
        done("stream_step")
    else:
        total = torch.tensor([frames(n, hop) for n in lens], dtype=torch.int32, device=dev)
        fb_out = new(T, B, F - 1)  # time-major: a segment is a contiguous slice
        if passes == OFFLINE:
            for s0, k in plan.segments:
                x = segment(s0, k)
                _lib.check(L.fsn_improved_segment_stats(cfg, *sargs, s0, total.data_ptr(), _lib.dev_ptr(x, "mag"), B, k, st))
            done("stats")
        for s0, k in plan.segments:
            x = segment(s0, k)
            _lib.check(L.fsn_improved_segment_fullband(cfg, packed, *sargs, 0 if passes == OFFLINE else 1, s0, total.data_ptr(),
                                                       _lib.dev_ptr(x, "mag"), B, k, _lib.dev_ptr(fb_out[s0:s0 + k]), *wargs, st))
        done("fullband")
        for s0, k in plan.segments:
            x, c = segment(s0, k), new(B, 2, F, k)
            _lib.check(L.fsn_improved_segment_sections(cfg, packed, *sargs, s0, total.data_ptr(), _lib.dev_ptr(x, "mag"),
                                                       _lib.dev_ptr(fb_out[s0:s0 + k]), B, k, _lib.dev_ptr(c), *wargs, st))
            keep(s0, k, c)
        done("sections")

    # ---- mask and iSTFT in slabs, the overlap-add half frame carried ----------------------------------------------------
    out = new(B, Lmax)
    for rows, n in groups:
        Tb = frames(n, hop)
        prev, n_out = None, 0
        for t0, t1, _, (o0, o1) in plan.slabs_of(n):
            # model.py:575-577: the mask multiplies real and imaginary parts separately (no decompression, no complex product)
            er = crm[rows, 0, :, t0:t1] * re[rows, :, t0:t1]
            ei = crm[rows, 1, :, t0:t1] * im[rows, :, t0:t1]
            y, prev = synthesis_slab(er, ei, prev, t0, n_out, n_fft, hop, n if t1 == Tb else None)
            if y is not None:
                assert (n_out, n_out + y.shape[1]) == (o0, o1)
                out[rows, o0:o1] = y
                n_out = o1
        out[rows, n:] = 0.0
        crm[rows, :, :, Tb:] = 0.0
    done("istft")
    return (out, crm) if return_crm else out
