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
segments.  The transforms run in slabs of frames (``slabs.py``), as in ``long_form.enhance_long``.

``FastLongPlan`` is the host book-keeping of one run - segments, slabs and the bytes of everything the run allocates -
with no device call, like ``long_form.LongPlan``."""
import ctypes

import torch

from . import _lib
from .acoustics.mask import decompress_cIRM
from .long_form import HOP, MAX_SEGMENT_FRAMES, N_FFT, SLAB_FRAMES
from .ragged import check_lengths, frames
from .slabs import analysis_bounds, analysis_slab, synthesis_slab

OFFLINE, CUMULATIVE = _lib.NORM_TYPES["offline_laplace_norm"], _lib.NORM_TYPES["cumulative_laplace_norm"]


class FastLongPlan:
    """What ``enhance_long`` does for ``batch`` rows of up to ``num_samples`` samples, without doing it.

    ``cfg``: the model's ``stream_cfg()`` (``_lib.FastCfg``; its norm decides the passes), ``look_ahead`` the model's.
    ``segments``: (first step, k) of the model calls of every pass - the ``frames + look_ahead`` model steps in order, each
    exactly once, 1 <= k <= 4096.  ``slabs``: (first frame, end frame, samples read [lo, hi), samples written [lo, hi)) of
    the transform calls; the written ranges tile [0, num_samples).  ``bytes``: name -> bytes of every allocation of the run
    (device memory); ``total_bytes`` their sum.  Only the entries of ``LINEAR`` grow with the recording: by F floats (a hop
    of samples for ``enhanced``) per frame and row, by 64 floats per step and padded row for ``mel`` and ``enc``."""

    LINEAR = ("mag", "spec_re", "spec_im", "mask", "mel", "enc", "enhanced")

    def __init__(self, cfg, look_ahead, batch, num_samples, segment_frames=None, workspace_limit=4 << 30, slab_frames=SLAB_FRAMES):
        L = _lib.lib()
        if batch < 1 or num_samples <= N_FFT // 2:
            raise _lib.FsnError(f"enhance_long: batch {batch} / {num_samples} samples (need more than n_fft / 2 = {N_FFT // 2})")
        self.batch, self.num_samples, self.look_ahead = batch, num_samples, look_ahead
        self.offline = cfg.norm == OFFLINE
        self.frames = frames(num_samples, HOP)
        self.steps = self.frames + look_ahead
        state_of, workspace_of = ((L.fsn_fast_segment_state_bytes, L.fsn_fast_segment_workspace_bytes) if self.offline else
                                  (L.fsn_fast_stream_state_bytes, L.fsn_fast_stream_workspace_bytes))
        query = lambda k: workspace_of(ctypes.byref(cfg), batch, k)  # noqa: E731
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
        state, workspace = state_of(ctypes.byref(cfg), batch), query(k)
        if state == 0 or workspace == 0:
            raise _lib.FsnError(f"enhance_long: {L.fsn_last_error().decode()}")
        T, Tp, S, F = self.frames, self.steps, min(self.slab_frames + 1, self.frames), cfg.F
        plane, band = 4 * batch * F, 4 * ((batch + 15) // 16 * 16) * cfg.num_mels
        self.bytes = {
            "state": state, "workspace": workspace,
            # linear in the recording: planes of F floats per frame, 64 floats per step, and the result
            "mag": plane * Tp, "spec_re": plane * T, "spec_im": plane * T, "mask": 2 * plane * T,
            "mel": band * Tp if self.offline else 0, "enc": band * Tp if self.offline else 0,
            "enhanced": 4 * batch * num_samples,
            # bounded: what one segment / one slab passes to and takes from the library
            "segment_io": (1 + 2) * plane * k,
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


@torch.no_grad()
def enhance_long(model, noisy, lengths=None, segment_frames=None, workspace_limit=4 << 30, return_crm=False, poison=False,
                 n_fft=N_FFT, hop_length=HOP, slab_frames=SLAB_FRAMES):
    """See ``fast_fullsubnet.Model.enhance_long``."""
    fcfg = refuse(model, n_fft, hop_length)
    assert noisy.dim() == 2
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise _lib.FsnError("enhance_long needs the model on a ROCm device (this path has no CPU implementation); "
                            "Model.enhance runs a host model")
    B, Lmax = noisy.shape
    lens = [Lmax] * B if lengths is None else check_lengths(lengths, B, Lmax, n_fft)
    la = model.look_ahead
    plan = FastLongPlan(fcfg, la, B, Lmax, segment_frames, workspace_limit, slab_frames)
    cfg, F, M, T, Tp, Bp = ctypes.byref(fcfg), model.num_freqs, model.num_mels, plan.frames, plan.steps, (B + 15) // 16 * 16
    L, st = _lib.lib(), _lib.stream_ptr(dev)
    fill = float("nan") if poison else None  # test hook: whatever is read must have been written first

    def new(*shape):
        t = torch.empty(shape, dtype=torch.float32, device=dev)
        return t.fill_(fill) if poison else t

    # rows that share a length are transformed together; a ragged batch row by row, each over its own samples
    groups = [(slice(0, B), Lmax)] if len(set(lens)) == 1 and lens[0] == Lmax else [(slice(b, b + 1), n) for b, n in enumerate(lens)]
    mag, re, im, crm = new(B, F, Tp), new(B, F, T), new(B, F, T), new(B, 2, F, T)

    # ---- STFT in slabs ----------------------------------------------------------------------------------------------
    for rows, n in groups:
        Tb = frames(n, hop_length)
        for t0, t1, (a, b), _ in plan.slabs_of(n):
            j0 = a // hop_length
            m, r, i = analysis_slab(noisy[rows, a:b].to(dev, torch.float32), j0, t0, t1 - 1, n_fft, hop_length)
            mag[rows, :, t0:t1], re[rows, :, t0:t1], im[rows, :, t0:t1] = m, r, i
        mag[rows, :, Tb:] = 0.0  # the look-ahead zero frames of model.py:161, and a shorter row's padding

    # ---- the model over the segments ----------------------------------------------------------------------------------
    state = torch.empty(plan.bytes["state"], dtype=torch.uint8, device=dev)
    if poison:
        state.view(torch.float32).fill_(fill)
    state.zero_()  # a fresh recording
    ws = _lib.workspace(plan.bytes["workspace"], dev)
    if poison:
        ws.view(torch.float32).fill_(fill)
    # the packing entry takes the causal norm only; the blob's layout does not depend on the norm
    packed = model.stream_packed_weights(norm=CUMULATIVE if plan.offline else None).data_ptr()
    sargs, wargs = (state.data_ptr(), state.numel()), (ws.data_ptr(), ws.numel())

    def keep(s0, k, c):
        drop = max(la - s0, 0)  # step s is the mask of frame s - look_ahead
        if k > drop:
            crm[:, :, :, s0 + drop - la:s0 + k - la] = c[..., drop:]

    if plan.offline:
        total = torch.tensor([frames(n, hop_length) + la for n in lens], dtype=torch.int32, device=dev)
        mel, enc = new(Tp, Bp, M), new(Tp, Bp, M)  # time-major: a segment is a contiguous slice
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
    else:
        for s0, k in plan.segments:
            x, c = mag[:, :, s0:s0 + k].contiguous(), new(B, 2, F, k)
            _lib.check(L.fsn_fast_stream_step(cfg, packed, *sargs, s0, _lib.dev_ptr(x, "mag"), B, k, _lib.dev_ptr(c), *wargs, st))
            keep(s0, k, c)

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
