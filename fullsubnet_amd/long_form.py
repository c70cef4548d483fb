"""Recordings of any length on the fused FullSubNet configurations: ``Model.enhance_long``.

``Model.enhance`` stops at 100 000 frames (26.7 minutes at hop 256 / 16 kHz) and its workspace grows with the recording at
hidden-state width (418 KB per frame and utterance for ONE sub-band hidden sequence).  Here the model runs in segments of k
frames with carried LSTM state (libfsn_hip ``fsn_fullsubnet_segment_*``); what lives for the whole recording are planes of F
floats per frame only - magnitude, spectrum (re, im), full-band output, mask - about 6 KB per frame and utterance.

The shipped norm (``offline_laplace_norm``) divides by one mean per utterance, so a recording takes three passes over its
segments: (1) the per-bin magnitude sums, (2) the full-band model, which needs the first mean and yields the sum of its own
output, (3) the sub-band model, which needs the second.  The sums are fp64 accumulators in the state blob.  A
``cumulative_laplace_norm`` model takes the same three loops (pass 1 has nothing to do, the entries continue the running
sums as ``fsn_fullsubnet_stream_step`` does).  The transforms run in slabs of frames (``slabs.py``, shared with
``StreamingEnhancer``); the overlap-add half frame is carried from slab to slab.

``LongPlan`` is the host book-keeping of one run - segments, slabs, and the bytes of everything the run allocates - with
no device call (the size queries of the library answer without one), like ``stream_pool.SessionBook``."""
import ctypes

import torch

from . import _lib
from .acoustics.mask import decompress_cIRM
from .ragged import check_lengths, frames
from .slabs import analysis_bounds, analysis_slab, synthesis_slab

N_FFT, HOP = 512, 256          # the transform the fused path is built for
MAX_SEGMENT_FRAMES = 4096      # k of the segment entries (as of the stream step)
SLAB_FRAMES = 4096             # frames per transform call


class LongPlan:
    """What ``enhance_long`` does for ``batch`` rows of up to ``num_samples`` samples, without doing it.

    ``segments``: (first step, k) of the model calls - the ``frames + look_ahead`` model steps in order, each exactly once,
    1 <= k <= 4096.  ``slabs``: (first frame, end frame, samples read [lo, hi), samples written [lo, hi)) of the
    transform calls over a row of ``num_samples`` samples; the written ranges tile [0, num_samples).  ``bytes``: name ->
    bytes of every allocation of the run (device memory); ``total_bytes`` their sum.  Only the entries of
    ``LINEAR`` grow with the recording, by F floats (a hop of samples for ``enhanced``) per frame and row."""

    LINEAR = ("mag", "spec_re", "spec_im", "fb_out", "mask", "enhanced")

    def __init__(self, cfg, batch, num_samples, segment_frames=None, workspace_limit=4 << 30, slab_frames=SLAB_FRAMES):
        L = _lib.lib()
        if batch < 1 or num_samples <= N_FFT // 2:
            raise _lib.FsnError(f"enhance_long: batch {batch} / {num_samples} samples (need more than n_fft / 2 = {N_FFT // 2})")
        self.batch, self.num_samples = batch, num_samples
        self.look_ahead = cfg.look_ahead
        self.frames = frames(num_samples, HOP)
        self.steps = self.frames + cfg.look_ahead
        F = cfg.num_freqs
        query = lambda k: L.fsn_fullsubnet_segment_workspace_bytes(ctypes.byref(cfg), batch, k)  # noqa: E731
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
        state = L.fsn_fullsubnet_segment_state_bytes(ctypes.byref(cfg), batch)
        workspace = query(k)
        if state == 0 or workspace == 0:
            raise _lib.FsnError(f"enhance_long: {L.fsn_last_error().decode()}")
        T, Tp, S = self.frames, self.steps, min(self.slab_frames + 1, self.frames)
        plane = 4 * batch * F
        self.bytes = {
            "state": state, "workspace": workspace,
            # linear in the recording: planes of F floats per frame, and the result
            "mag": plane * Tp, "spec_re": plane * T, "spec_im": plane * T, "fb_out": plane * Tp, "mask": 2 * plane * T,
            "enhanced": 4 * batch * num_samples,
            # bounded: what one segment / one slab passes to and takes from the library
            "segment_io": (1 + 1 + 2) * plane * k,
            "slab_samples": 4 * batch * (S + 2) * HOP, "slab_spectra": 3 * plane * (S + 2),
            "slab_enhanced": (4 + 2 + 2) * plane * S + 4 * batch * S * HOP + 4 * batch * S * N_FFT,
            "total_frames": 4 * batch,
        }
        self.total_bytes = sum(self.bytes.values())

    def slabs_of(self, n):
        """The transform calls over a row of n samples (a ragged batch transforms each row over its own length)."""
        T, out = frames(n, HOP), []
        for t0 in range(0, T, self.slab_frames):
            t1 = min(t0 + self.slab_frames, T)
            _, a, b = analysis_bounds(t0, t1 - 1, n, t1 == T, N_FFT, HOP)
            out.append((t0, t1, (a, b), (max(t0 - 1, 0) * HOP, n if t1 == T else (t1 - 1) * HOP)))
        return out


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


@torch.no_grad()
def enhance_long(model, noisy, lengths=None, segment_frames=None, workspace_limit=4 << 30, return_crm=False, poison=False,
                 n_fft=N_FFT, hop_length=HOP, slab_frames=SLAB_FRAMES):
    """See ``Model.enhance_long``."""
    _refuse(model, n_fft, hop_length)
    assert noisy.dim() == 2
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.FsnError("enhance_long needs the model on a ROCm device; this path has no CPU implementation")
    B, Lmax = noisy.shape
    lens = [Lmax] * B if lengths is None else check_lengths(lengths, B, Lmax, n_fft)
    plan = LongPlan(model._cfg, B, Lmax, segment_frames, workspace_limit, slab_frames)
    cfg, F, la, T, Tp = ctypes.byref(model._cfg), model.num_freqs, model.look_ahead, plan.frames, plan.steps
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    fill = float("nan") if poison else None  # test hook: whatever is read must have been written first

    def new(*shape):
        t = torch.empty(shape, dtype=torch.float32, device=dev)
        return t.fill_(fill) if poison else t

    # rows that share a length are transformed together; a ragged batch row by row, each over its own samples
    groups = [(slice(0, B), Lmax)] if len(set(lens)) == 1 and lens[0] == Lmax else [(slice(b, b + 1), n) for b, n in enumerate(lens)]
    mag, fb_out = new(B, F, Tp), new(B, F, Tp)
    re, im, crm = new(B, F, T), new(B, F, T), new(B, 2, F, T)

    # ---- STFT in slabs ----------------------------------------------------------------------------------------------
    for rows, n in groups:
        Tb = frames(n, hop_length)
        for t0, t1, (a, b), _ in plan.slabs_of(n):
            j0 = a // hop_length
            m, r, i = analysis_slab(noisy[rows, a:b].to(dev, torch.float32), j0, t0, t1 - 1, n_fft, hop_length)
            mag[rows, :, t0:t1], re[rows, :, t0:t1], im[rows, :, t0:t1] = m, r, i
        mag[rows, :, Tb:] = 0.0  # the look-ahead zero frames of model.py:85, and a shorter row's padding

    # ---- the model: three passes over the segments ------------------------------------------------------------------
    state = torch.empty(plan.bytes["state"], dtype=torch.uint8, device=dev)
    if poison:
        state.view(torch.float32).fill_(fill)
    state.zero_()  # a fresh recording
    ws = _lib.workspace(plan.bytes["workspace"], dev)
    if poison:
        ws.view(torch.float32).fill_(fill)
    total = torch.tensor([frames(n, hop_length) + la for n in lens], dtype=torch.int32, device=dev)
    packed = model.packed_weights().data_ptr()
    sargs = (state.data_ptr(), state.numel())
    for s0, k in plan.segments:
        x = mag[:, :, s0:s0 + k].contiguous()
        _lib.check(L.fsn_fullsubnet_segment_stats(cfg, *sargs, _lib.dev_ptr(x, "mag"), B, k, st))
    for s0, k in plan.segments:
        x, y = mag[:, :, s0:s0 + k].contiguous(), new(B, F, k)
        _lib.check(L.fsn_fullsubnet_segment_fullband(cfg, packed, *sargs, s0, total.data_ptr(), _lib.dev_ptr(x, "mag"), B, k,
                                                     _lib.dev_ptr(y), ws.data_ptr(), ws.numel(), st))
        fb_out[:, :, s0:s0 + k] = y
    for s0, k in plan.segments:
        x, y, c = mag[:, :, s0:s0 + k].contiguous(), fb_out[:, :, s0:s0 + k].contiguous(), new(B, 2, F, k)
        _lib.check(L.fsn_fullsubnet_segment_subband(cfg, packed, *sargs, s0, total.data_ptr(), _lib.dev_ptr(x, "mag"),
                                                    _lib.dev_ptr(y, "fb_out"), B, k, _lib.dev_ptr(c), ws.data_ptr(), ws.numel(),
                                                    st))
        drop = max(la - s0, 0)  # step s is the mask of frame s - look_ahead
        if k > drop:
            crm[:, :, :, s0 + drop - la:s0 + k - la] = c[..., drop:]

    # ---- mask and iSTFT in slabs, the overlap-add half frame carried ----------------------------------------------------
    out = new(B, Lmax)
    for rows, n in groups:
        Tb = frames(n, hop_length)
        prev, n_out = None, 0
        for t0, t1, _, (o0, o1) in plan.slabs_of(n):
            dm = decompress_cIRM(crm[rows, :, :, t0:t1].permute(0, 2, 3, 1).contiguous())
            r, i = re[rows, :, t0:t1], im[rows, :, t0:t1]
            er = dm[..., 0] * r - dm[..., 1] * i
            ei = dm[..., 1] * r + dm[..., 0] * i
            y, prev = synthesis_slab(er, ei, prev, t0, n_out, n_fft, hop_length, n if t1 == Tb else None)
            if y is not None:
                assert (n_out, n_out + y.shape[1]) == (o0, o1)
                out[rows, o0:o1] = y
                n_out = o1
        out[rows, n:] = 0.0
        crm[rows, :, :, Tb:] = 0.0
    return (out, crm) if return_crm else out
