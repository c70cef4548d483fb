"""Recordings of any length, and on the fused FullSubNet configurations: ``Model.enhance_long``.

``Model.enhance`` stops at 100 000 frames (26.7 minutes at hop 256 / 16 kHz) and its workspace grows with the recording at
hidden-state width (418 KB per frame and utterance for ONE sub-band hidden sequence).  Here the model runs in segments of k
frames with carried LSTM state (libfsn_hip ``fsn_fullsubnet_segment_*``); what lives for the whole recording are planes of F
floats per frame only - magnitude, spectrum (re, im), full-band output, mask - about 6 KB per frame and utterance.

The shipped norm (``offline_laplace_norm``) divides by one mean per utterance, so a recording takes three passes over its
segments: (1) the per-bin magnitude sums, (2) the full-band model, which needs the first mean and yields the sum of its own
output, (3) the sub-band model, which needs the second.  The sums are fp64 accumulators in the state blob.  A
``cumulative_laplace_norm`` model takes the same three loops (pass 1 has nothing to do, the entries continue the running
sums as ``fsn_fullsubnet_stream_step`` does).

The segment driver of all three models lives here: ``SegmentPlan`` (segments, slabs and the bytes of a run, with no device
call: the size queries of the library answer without one, like ``stream_pool.SessionBook``) and ``run_segments`` (the slabbed
transforms of ``slabs.py``, shared with ``StreamingEnhancer``, around a model's passes).  What a model adds - its refusals, its
plan class, its passes and its mask function - is the second half of this file for FullSubNet, and ``fast_long_form.py`` and
``improved_long_form.py`` for the other two."""
import ctypes
from functools import partial

import torch

from . import _lib
from .acoustics.mask import decompress_cIRM
from .ragged import check_lengths, frames
from .slabs import analysis_bounds, analysis_slab, synthesis_slab

N_FFT, HOP = 512, 256          # the transform the fused path is built for
MAX_SEGMENT_FRAMES = 4096      # k of the segment entries (as of the stream step)
SLAB_FRAMES = 4096             # frames per transform call


class SegmentPlan:
    """What ``enhance_long`` does for ``batch`` rows of up to ``num_samples`` samples, without doing it.

    ``segments``: (first step, k) of the model calls of every pass - the ``steps = frames + look_ahead`` model steps in
    order, each exactly once, 1 <= k <= 4096.  ``slabs``: (first frame, end frame, samples read [lo, hi), samples written
    [lo, hi)) of the transform calls over a row of ``num_samples`` samples; the written ranges tile [0, num_samples).
    ``bytes``: name -> bytes of every allocation of the run (device memory); ``total_bytes`` their sum.  Only the entries of
    ``LINEAR`` grow with the recording.  A subclass passes its transform (hop = n_fft / 2), its look-ahead and bins, its two
    size queries (``state_of(batch)``, ``workspace_of(batch, k)``), ``io_planes`` (the planes of F floats per step that a
    segment passes to and takes from the library) and ``per_step`` (name -> bytes per step of its own whole-recording planes)."""

    LINEAR = ()
    MASK_PLANES = 4 + 2 + 2  # of ``slab_enhanced``: what the mask function holds per frame of a slab, in planes of F floats

    def __init__(self, n_fft, look_ahead, F, state_of, workspace_of, io_planes, per_step, batch, num_samples, segment_frames,
                 workspace_limit, slab_frames):
        L = _lib.lib()
        if batch < 1 or num_samples <= n_fft // 2:
            raise _lib.FsnError(f"enhance_long: batch {batch} / {num_samples} samples (need more than n_fft / 2 = {n_fft // 2})")
        self.batch, self.num_samples, self.look_ahead, self.n_fft, self.hop = batch, num_samples, look_ahead, n_fft, n_fft // 2
        self.frames = frames(num_samples, self.hop)
        self.steps = self.frames + look_ahead
        query = partial(workspace_of, batch)
        if segment_frames is None:
            # the workspace grows with k: the largest k under the limit, by bisection
            lo, hi = 1, min(MAX_SEGMENT_FRAMES, self.steps)
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
        self.segment_frames = k = min(segment_frames, self.steps)
        self.segments = [(s, min(k, self.steps - s)) for s in range(0, self.steps, k)]
        self.slab_frames = max(2, int(slab_frames))
        self.slabs = self.slabs_of(num_samples)
        state, workspace = state_of(batch), query(k)
        if state == 0 or workspace == 0:
            raise _lib.FsnError(f"enhance_long: {L.fsn_last_error().decode()}")
        T, Tp, S = self.frames, self.steps, min(self.slab_frames + 1, self.frames)
        plane = 4 * batch * F
        self.bytes = {
            "state": state, "workspace": workspace,
            # linear in the recording: planes of F floats per frame, and the result
            "mag": plane * Tp, "spec_re": plane * T, "spec_im": plane * T, "mask": 2 * plane * T, "enhanced": 4 * batch * num_samples,
            **{name: n * Tp for name, n in per_step.items()},
            # bounded: what one segment / one slab passes to and takes from the library
            "segment_io": io_planes * plane * k,
            "slab_samples": 4 * batch * (S + 2) * self.hop, "slab_spectra": 3 * plane * (S + 2),
            "slab_enhanced": self.MASK_PLANES * plane * S + 4 * batch * S * self.hop + 4 * batch * S * n_fft,
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


def cirm_mask(crm, re, im):
    """The compressed cIRM [b, 2, F, t] on the spectrum (re, im) [b, F, t] -> the enhanced spectrum: a complex product."""
    dm = decompress_cIRM(crm.permute(0, 2, 3, 1).contiguous())
    return dm[..., 0] * re - dm[..., 1] * im, dm[..., 1] * re + dm[..., 0] * im


@torch.no_grad()
def run_segments(model, noisy, lengths, n_fft, plan_of, limits, passes, mask, one_call=None, return_crm=False, poison=False,
                 on_stage=None):
    """The scaffold of every ``enhance_long``, after the model's refusals: noisy [B, L] -> enhanced [B, L] (and the mask).

    ``plan_of(B, L, *limits)`` -> the model's ``SegmentPlan``.  ``passes(plan, total, mag, sargs, wargs, new, keep)`` issues the
    library calls over ``plan.segments``: ``total`` [B] holds the steps of every row, ``mag`` [B, F, steps] the magnitude (zero
    past a row's frames), ``sargs`` / ``wargs`` the (pointer, bytes) of the zeroed state and of the workspace, ``new(*shape)``
    allocates, ``keep(s0, k, c)`` stores the mask c [B, 2, F, k] of steps s0 .. s0 + k (step s is the mask of frame s -
    look_ahead).  ``mask(crm, re, im)`` -> (er, ei), the enhanced spectrum of a slab.  ``one_call`` names the model's path that
    runs on the host.  ``poison`` (test hook): every buffer starts as NaN.  ``on_stage`` (measurement): told "stft" / "istft"."""
    assert noisy.dim() == 2
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.FsnError("enhance_long needs the model on a ROCm device (this path has no CPU implementation)"
                            + (f"; {one_call} runs a host model" if one_call else ""))
    B, Lmax = noisy.shape
    lens = [Lmax] * B if lengths is None else check_lengths(lengths, B, Lmax, n_fft)
    plan = plan_of(B, Lmax, *limits)
    F, T, la, hop = model.num_freqs, plan.frames, plan.look_ahead, plan.hop
    fill = float("nan") if poison else None  # whatever is read must have been written first
    done = on_stage or (lambda stage: None)

    def new(*shape):
        t = torch.empty(shape, dtype=torch.float32, device=dev)
        return t.fill_(fill) if poison else t

    # rows that share a length are transformed together; a ragged batch row by row, each over its own samples
    groups = [(slice(0, B), Lmax)] if len(set(lens)) == 1 and lens[0] == Lmax else [(slice(b, b + 1), n) for b, n in enumerate(lens)]
    mag, re, im, crm = new(B, F, plan.steps), new(B, F, T), new(B, F, T), new(B, 2, F, T)

    # ---- STFT in slabs ----------------------------------------------------------------------------------------------
    for rows, n in groups:
        for t0, t1, (a, b), _ in plan.slabs_of(n):
            m, r, i = analysis_slab(noisy[rows, a:b].to(dev, torch.float32), a // hop, t0, t1 - 1, n_fft, hop)
            mag[rows, :, t0:t1], re[rows, :, t0:t1], im[rows, :, t0:t1] = m, r, i
        mag[rows, :, frames(n, hop):] = 0.0  # the look-ahead zero frames of the model, and a shorter row's padding
    done("stft")

    # ---- the model over the segments ----------------------------------------------------------------------------------
    state = torch.empty(plan.bytes["state"], dtype=torch.uint8, device=dev)
    if poison:
        state.view(torch.float32).fill_(fill)
    state.zero_()  # a fresh recording
    ws = _lib.workspace(plan.bytes["workspace"], dev)
    if poison:
        ws.view(torch.float32).fill_(fill)
    total = torch.tensor([frames(n, hop) + la for n in lens], dtype=torch.int32, device=dev)

    def keep(s0, k, c):
        drop = max(la - s0, 0)
        if k > drop:
            crm[:, :, :, s0 + drop - la:s0 + k - la] = c[..., drop:]

    passes(plan, total, mag, (state.data_ptr(), state.numel()), (ws.data_ptr(), ws.numel()), new, keep)

    # ---- mask and iSTFT in slabs, the overlap-add half frame carried ----------------------------------------------------
    out = new(B, Lmax)
    for rows, n in groups:
        Tb = frames(n, hop)
        prev, n_out = None, 0
        for t0, t1, _, (o0, o1) in plan.slabs_of(n):
            er, ei = mask(crm[rows, :, :, t0:t1], re[rows, :, t0:t1], im[rows, :, t0:t1])
            y, prev = synthesis_slab(er, ei, prev, t0, n_out, n_fft, hop, n if t1 == Tb else None)
            if y is not None:
                assert (n_out, n_out + y.shape[1]) == (o0, o1)
                out[rows, o0:o1] = y
                n_out = o1
        out[rows, n:] = 0.0
        crm[rows, :, :, Tb:] = 0.0
    done("istft")
    return (out, crm) if return_crm else out


# ---- FullSubNet ---------------------------------------------------------------------------------------------------------

class LongPlan(SegmentPlan):
    """``SegmentPlan`` of FullSubNet (``cfg``: the model's ``_lib.Cfg``): the full-band output ``fb_out`` lives for the whole
    recording too, F floats per step and row like ``mag``."""

    LINEAR = ("mag", "spec_re", "spec_im", "fb_out", "mask", "enhanced")

    def __init__(self, cfg, batch, num_samples, segment_frames=None, workspace_limit=4 << 30, slab_frames=SLAB_FRAMES):
        L, c = _lib.lib(), ctypes.byref(cfg)
        super().__init__(N_FFT, cfg.look_ahead, cfg.num_freqs, partial(L.fsn_fullsubnet_segment_state_bytes, c),
                         partial(L.fsn_fullsubnet_segment_workspace_bytes, c), 1 + 1 + 2, {"fb_out": 4 * batch * cfg.num_freqs},
                         batch, num_samples, segment_frames, workspace_limit, slab_frames)


def _refuse(model, n_fft, hop_length):
    if not getattr(model, "_fused", False):
        raise _lib.FsnError("enhance_long runs the fused FullSubNet configurations only (LSTM, no full-band neighbours, ReLU / "
                            "no output activation, sub-band hidden size 384, the two Laplace norms): the segment entries of "
                            "libfsn_hip carry the state of exactly those kernels; use Model.enhance for this configuration")
    if (n_fft, hop_length) != (N_FFT, HOP) or model.num_freqs != N_FFT // 2 + 1:
        raise _lib.FsnError(f"enhance_long is built for n_fft {N_FFT} / hop {HOP} ({N_FFT // 2 + 1} bins) only, got n_fft {n_fft} / "
                            f"hop {hop_length} on a model of {model.num_freqs} bins: the slabbed transforms carry half a frame")
    if model.arithmetic != "f32":
        raise _lib.FsnError(f"enhance_long is built for the fp32 arithmetic, the model is set to {model.arithmetic!r}")


def _passes(model, plan, total, mag, sargs, wargs, new, keep):
    """The three passes over the segments (either norm)."""
    L, st, cfg, (B, F, _) = _lib.lib(), _lib.stream_ptr(mag.device), ctypes.byref(model._cfg), mag.shape
    fb_out = new(B, F, plan.steps)
    packed = model.packed_weights().data_ptr()
    for s0, k in plan.segments:
        x = mag[:, :, s0:s0 + k].contiguous()
        _lib.check(L.fsn_fullsubnet_segment_stats(cfg, *sargs, _lib.dev_ptr(x, "mag"), B, k, st))
    for s0, k in plan.segments:
        x, y = mag[:, :, s0:s0 + k].contiguous(), new(B, F, k)
        _lib.check(L.fsn_fullsubnet_segment_fullband(cfg, packed, *sargs, s0, total.data_ptr(), _lib.dev_ptr(x, "mag"), B, k,
                                                     _lib.dev_ptr(y), *wargs, st))
        fb_out[:, :, s0:s0 + k] = y
    for s0, k in plan.segments:
        x, y, c = mag[:, :, s0:s0 + k].contiguous(), fb_out[:, :, s0:s0 + k].contiguous(), new(B, 2, F, k)
        _lib.check(L.fsn_fullsubnet_segment_subband(cfg, packed, *sargs, s0, total.data_ptr(), _lib.dev_ptr(x, "mag"),
                                                    _lib.dev_ptr(y, "fb_out"), B, k, _lib.dev_ptr(c), *wargs, st))
        keep(s0, k, c)


def enhance_long(model, noisy, lengths=None, segment_frames=None, workspace_limit=4 << 30, return_crm=False, poison=False,
                 n_fft=N_FFT, hop_length=HOP, slab_frames=SLAB_FRAMES):
    """See ``Model.enhance_long``."""
    _refuse(model, n_fft, hop_length)
    return run_segments(model, noisy, lengths, n_fft, partial(LongPlan, model._cfg), (segment_frames, workspace_limit, slab_frames),
                        partial(_passes, model), cirm_mask, None, return_crm, poison)
