"""A pool of streaming sessions that open, advance and close on their own and share ONE model step per tick.

``StreamingEnhancer`` runs a fixed batch in lockstep; a server that enhances calls has sessions that arrive and hang up
at any time, whose hops are not phase-aligned and of which only some have a frame ready on a given 16 ms tick:

    pool = StreamPool(model, capacity=64)      # fused FullSubNet config, Fast or Improved FullSubNet, cumulative norm(s)
    sid  = pool.open()                         # raises when the pool is full
    pool.push(sid, chunk)                      # 1-D samples, any length >= 0, host or device
    out  = pool.step()                         # {sid: samples}: ONE frame for every session that has one ready
    out  = pool.drain()                        # step() until no session has a frame ready; samples concatenated per sid
    tail = pool.close(sid)                     # last frame, look_ahead zero frames, OLA tail; the slot is free again

Per session, the ``drain()`` outputs followed by ``close()`` equal ``model.enhance(utterance[None])[0]``, whatever the
other sessions do.  A tick is three C calls on the list of ready slots - frame analysis (``fsn_stream_pool_analysis``), the
model step (``fsn_fullsubnet_stream_pool_step``) and frame synthesis (``fsn_stream_pool_synthesis``) - around one
``torch.stack`` of the new hops (two on a tick where a session starts: the samples its first frame reflects) and one small
host-to-device copy of the slot list.  Everything a session carries (LSTM states, norm sums, its own step count, the last
hop, the spectra waiting for their mask, the overlap-add half frame) lives in its slot of one device blob.

Sessions at another sample rate (``input_sr``, ``output_sr`` = "model" | "input" | Hz, ``resample_design``): ``push`` keeps
the raw chunk; ``step()`` first converts every session's pending input to the model's rate in ONE
``fsn_resample_stream_push`` call, runs the tick as above and sends its outputs through ONE call of a second resampler -
at most two more library calls and two small table copies per tick, whatever the number of sessions.  Both resamplers
carry their state (``stream_resample.StreamResampler``), so the model sees, bit for bit, ``resample.resample`` of the whole
utterance; ``close()`` flushes both and trims to ``out_length(n, input_sr, output_sr)`` samples in all.  The conversion adds
H / u samples of delay each way (0.625 ms at 48 <-> 16 kHz with "scipy", 2 ms with "sharp").  With the default arguments
no resampler exists and nothing here runs differently.

A ``fast_fullsubnet.Model`` (cumulative norm, LSTM cells) is served the same way through ``fsn_fast_stream_pool_*``: its sessions
stand at different phases of a down-sampling block, so the bottleneck runs on the rows that are due on a tick.  The entry wants
those rows listed first (``fast_pool_order``, on a host mirror of the slots' step counts); what differs between the two models
sits behind one small object (``_FullSubNetCalls`` / ``_FastCalls``), everything else here is shared.

An ``improved_fullsubnet.Model`` (both norms cumulative, LSTM cells, hop = n_fft / 2: 960 / 480 at 48 kHz) is served through
``fsn_improved_stream_pool_*`` (``_ImprovedCalls``): the pool's transform is then the model's own, the mask multiplies real and
imaginary parts, there is no look-ahead and rows go in any order.  Rate conversion around this pool is not built.

``SessionBook`` is the host book-keeping (which frame is next, who is ready, model steps versus output frames, the
look-ahead drop); it makes no device call, so it is tested without a GPU.
"""
import ctypes

import torch

from . import _lib
from .resample import out_length
from .stream_resample import StreamResampler

N_FFT, HOP = 512, 256
MODEL_SR = 16000  # the rate the fused FullSubNet configuration is trained at (a model may say otherwise: model.sr)


class _Session:
    __slots__ = ("slot", "n_in", "t_next", "frames_out", "frames_out_at_close", "steps", "n_out", "closing")

    def __init__(self, slot):
        self.slot = slot
        self.n_in = 0                  # samples received
        self.t_next = 0                # next frame to analyse = model steps on real frames so far
        self.frames_out = 0            # output frames synthesised (frame 0 counts: it emits no samples)
        self.frames_out_at_close = 0   # ... of which by close()
        self.steps = 0                 # model steps, the look-ahead zero frames at the end included
        self.n_out = 0                 # samples emitted
        self.closing = False


class _RateSession:
    """What a session carries when the pool converts rates: its ids in the two resamplers, the raw chunks that wait
    for the next step(), samples received at the input rate and samples emitted at the output rate."""
    __slots__ = ("down", "up", "pending", "n_in", "n_out")

    def __init__(self, down, up):
        self.down, self.up, self.pending, self.n_in, self.n_out = down, up, [], 0, 0


class SessionBook:
    """Host book-keeping of a pool of ``capacity`` slots; no device calls.

    Frame t of a session covers samples [t hop - hop, t hop + hop) (torch.stft, center=True): frame 0 reflects sample
    ``hop`` on its left, so it needs hop + 1 samples; frame t >= 1 is complete with (t + 1) hop samples.  A complete frame
    is never the utterance's last one (T - 1 = L // hop), which reflects at the right edge and is only known at close.
    Model step s of a session takes frame s and yields the mask of output frame s - look_ahead (none for the first
    look_ahead steps: the drop of ``StreamingEnhancer._advance``); output frame m >= 1 emits hop samples."""

    def __init__(self, capacity, look_ahead, hop=HOP):
        if capacity < 1:
            raise ValueError(f"capacity {capacity} < 1")
        self.capacity, self.la, self.hop = int(capacity), int(look_ahead), int(hop)
        self._free = list(range(self.capacity))  # kept sorted: lowest id first
        self._s = {}
        self._next_sid = 0

    # ---- slots --------------------------------------------------------------------------------
    def open(self):
        if not self._free:
            raise RuntimeError(f"StreamPool is full: all {self.capacity} slots hold an open session")
        sid = self._next_sid
        self._next_sid += 1
        self._s[sid] = _Session(self._free.pop(0))
        return sid

    def session(self, sid):
        try:
            return self._s[sid]
        except KeyError:
            raise KeyError(f"StreamPool: no open session {sid!r}") from None

    def slot(self, sid):
        return self.session(sid).slot

    def sids(self):
        return sorted(self._s, key=lambda i: self._s[i].slot)

    def release(self, sid):
        s = self.session(sid)
        del self._s[sid]
        self._free.append(s.slot)
        self._free.sort()
        return s.slot

    # ---- frames -------------------------------------------------------------------------------
    def push(self, sid, n):
        s = self.session(sid)
        if n < 0:
            raise ValueError("negative sample count")
        s.n_in += int(n)

    def has_frame(self, sid):
        s = self.session(sid)
        return not s.closing and s.n_in >= max((s.t_next + 1) * self.hop, self.hop + 1)

    def ready(self):
        """Sessions with a complete frame waiting, in slot order."""
        return [sid for sid in self.sids() if self.has_frame(sid)]

    def keep_from(self, sid):
        """Index of the oldest sample the session still needs: two hops of history (the last frame's right-edge
        reflection reaches one sample beyond the previous hop)."""
        return max(self.session(sid).t_next - 2, 0) * self.hop

    def take_frame(self, sid):
        """Advance the session by its next complete frame: (frame, first_frame, samples) - the frame to analyse, the
        output frame its model step yields (negative: none) and the samples that output frame emits."""
        s = self.session(sid)
        if not (self.has_frame(sid) or (s.closing and s.t_next < s.n_in // self.hop)):
            raise RuntimeError(f"session {sid}: no complete frame")
        t = s.t_next
        m = t - self.la
        n = self.hop if m >= 1 else 0
        s.t_next += 1
        s.steps += 1
        if m >= 0:
            s.frames_out += 1
            s.frames_out_at_close += int(s.closing)
        s.n_out += n
        return t, m, n

    def begin_close(self, sid):
        """End of the session's input: returns the number of complete frames still to run one by one (take_frame)
        before the last frame (take_last)."""
        s = self.session(sid)
        if s.n_in <= self.hop:
            raise _lib.FsnError(f"session shorter than n_fft / 2 + 1 = {self.hop + 1} samples (reflect padding), like torch.stft")
        s.closing = True
        return s.n_in // self.hop - s.t_next

    def take_last(self, sid):
        """The utterance's last frame T - 1 plus the look_ahead zero frames: (frame, first_frame, k, skip, tail,
        samples) - k = 1 + look_ahead model steps whose columns are output frames first_frame .., of which the first
        `skip` emit nothing (frames < 1); `tail` samples follow the last frame; `samples` is the total."""
        s = self.session(sid)
        t = s.n_in // self.hop
        if not s.closing or s.t_next != t:
            raise RuntimeError(f"session {sid}: take_last before its other frames were taken")
        k = 1 + self.la
        m0 = t - self.la
        skip = min(max(1 - m0, 0), k)
        tail = s.n_in - t * self.hop
        n = (k - skip) * self.hop + tail
        s.t_next += 1
        s.steps += k
        new = k - max(-m0, 0)
        s.frames_out += new
        s.frames_out_at_close += new
        s.n_out += n
        return t, m0, k, skip, tail, n


def _check_slots(slots, capacity):
    ids = [int(x) for x in slots]
    if not ids:
        raise ValueError("empty slot list")
    if any(i < 0 or i >= capacity for i in ids):
        raise ValueError(f"slot ids {ids} outside [0, {capacity})")
    if len(set(ids)) != len(ids):
        raise ValueError(f"slot ids {ids} are not distinct")
    return ids


def fast_pool_order(steps, k, shrink):
    """The row order ``fsn_fast_stream_pool_step`` asks for.  A slot that has taken t0 steps completes, in k more, as many
    low-rate frames as [t0, t0 + k) holds multiples of ``shrink``: lo = k // shrink or hi = ceil(k / shrink).  Returns
    (perm, n_long): the rows that complete hi first, each group in the caller's order (a stable sort), and how many they
    are - all of them when shrink divides k."""
    k, s = int(k), int(shrink)
    if k < 1 or s < 1:
        raise ValueError(f"fast_pool_order: k {k} and shrink {s} must be >= 1")
    hi = -(-k // s)
    long_rows, short_rows = [], []
    for i, t0 in enumerate(steps):
        t0 = int(t0)
        if t0 < 0:
            raise ValueError(f"fast_pool_order: negative step count {t0}")
        done = (t0 + k - 1) // s - ((t0 - 1) // s if t0 > 0 else -1)
        (long_rows if done == hi else short_rows).append(i)
    return long_rows + short_rows, len(long_rows)


class _FullSubNetCalls:
    """What StreamPool needs of the fused FullSubNet configuration: the cfg, the state size, the packed weights, the four C
    entries, the transform and the row order (any)."""
    fft = (N_FFT, HOP)

    def __init__(self, model):
        if not getattr(model, "_fused", False):
            raise NotImplementedError("StreamPool runs the fused FullSubNet configuration and Fast FullSubNet only "
                                      "(model._fused is false: use one StreamingEnhancer per stream for composed configurations)")
        self.model = model
        self.head = (ctypes.byref(model._cfg),)  # what every entry takes in front of the state
        L = _lib.lib()
        self.analysis, self.synthesis = L.fsn_stream_pool_analysis, L.fsn_stream_pool_synthesis
        self.step, self.reset = L.fsn_fullsubnet_stream_pool_step, L.fsn_fullsubnet_stream_pool_reset

    def state_bytes(self, capacity):
        nbytes = _lib.lib().fsn_fullsubnet_stream_pool_state_bytes(*self.head, capacity)
        if nbytes == 0:
            raise _lib.FsnError(_lib.lib().fsn_last_error().decode())
        return nbytes

    def workspace_bytes(self, n, k):
        return _lib.lib().fsn_fullsubnet_stream_pool_workspace_bytes(*self.head, n, k)

    def packed(self):
        return self.model.packed_weights()

    def order(self, steps, k):
        return None  # rows in any order

    def rows(self, n, n_long):
        return (n,)


class _FastCalls:
    """... of a ``fast_fullsubnet.Model``: ``fsn_fast_stream_pool_*``, which take the look-ahead beside the cfg and want the
    rows that complete the larger number of low-rate frames first (``fast_pool_order``)."""
    fft = (N_FFT, HOP)

    def __init__(self, model):
        if any(b.cell != "LSTM" for b in (*model.encoder, model.bottleneck, *model.decoder_lstm)):
            raise NotImplementedError("StreamPool runs Fast FullSubNet with LSTM cells (fsn_fast_stream_pool_step)")
        self.model = model
        self._cfg = model.stream_cfg()
        self.shrink = int(model.shrink_size)
        self.head = (ctypes.byref(self._cfg), int(model.look_ahead))
        L = _lib.lib()
        self.analysis, self.synthesis = L.fsn_fast_stream_pool_analysis, L.fsn_fast_stream_pool_synthesis
        self.step, self.reset = L.fsn_fast_stream_pool_step, L.fsn_fast_stream_pool_reset

    def state_bytes(self, capacity):
        nbytes = _lib.lib().fsn_fast_stream_pool_state_bytes(*self.head, capacity)
        if nbytes == 0:  # a configuration (or a capacity) the C entry refuses
            raise NotImplementedError(_lib.lib().fsn_last_error().decode())
        return nbytes

    def workspace_bytes(self, n, k):
        return _lib.lib().fsn_fast_stream_pool_workspace_bytes(self.head[0], n, k)

    def packed(self):
        return self.model.stream_packed_weights()

    def order(self, steps, k):
        return fast_pool_order(steps, k, self.shrink)

    def rows(self, n, n_long):
        return (n, n_long)


class _ImprovedCalls:
    """... of an ``improved_fullsubnet.Model``: ``fsn_improved_stream_pool_*`` on the model's own transform.  Its synthesis entry
    takes one frame per call and finds the frame's number in the record, so it has no k, no first frame and no workspace."""

    def __init__(self, model):
        for key in ("norm_type", "sb_norm_type"):
            if getattr(model, key) != "cumulative_laplace_norm":
                raise ValueError(f"streaming needs a causal norm in front of the full-band model and of the band sections: "
                                 f"build the model with {key} = 'cumulative_laplace_norm'")
        if model.n_fft // 2 + 1 != model.num_freqs or model.hop_length * 2 != model.n_fft or model.win_length != model.n_fft:
            raise NotImplementedError(
                f"the pool's overlap-add is written for hop = n_fft / 2 = win_length / 2 (960 / 480 at 48 kHz), not for "
                f"{model.n_fft} / {model.hop_length} / {model.win_length}: set hop_length = n_fft / 2 (the model's 16 kHz default of "
                f"512 / 128 is not served)")
        self.model = model
        self.fft = (int(model.n_fft), int(model.hop_length))
        self._cfg = model.stream_cfg()
        self.head = (ctypes.byref(self._cfg),)
        L = _lib.lib()
        self.analysis, self.synthesis = L.fsn_improved_stream_pool_analysis, L.fsn_improved_stream_pool_synthesis
        self.step, self.reset = L.fsn_improved_stream_pool_step, L.fsn_improved_stream_pool_reset

    def state_bytes(self, capacity):
        nbytes = _lib.lib().fsn_improved_stream_pool_state_bytes(*self.head, capacity)
        if nbytes == 0:  # a configuration (GRU cells: sequence_model = "LSTM" is the one served) or a capacity the C entry refuses
            raise NotImplementedError(_lib.lib().fsn_last_error().decode())
        return nbytes

    def workspace_bytes(self, n, k):
        return _lib.lib().fsn_improved_stream_pool_workspace_bytes(*self.head, n, k)

    def packed(self):
        return self.model.stream_packed_weights()

    def order(self, steps, k):
        return None  # rows in any order

    def rows(self, n, n_long):
        return (n,)


class StreamPool:
    def __init__(self, model, capacity=64, poison_buffers=False, input_sr=None, output_sr="model", resample_design="scipy",
                 record_model_rate=False):
        from .fast_fullsubnet import Model as FastModel
        from .improved_fullsubnet import Model as ImprovedModel
        self._improved = isinstance(model, ImprovedModel)
        if self._improved and (input_sr is not None or output_sr not in ("model", "input")):
            raise NotImplementedError("StreamPool(improved model) runs at the model's own rate: the model carries no sample rate and "
                                      "the rate conversion around this pool is not built (leave input_sr / output_sr at their defaults)")
        if model.norm_type != "cumulative_laplace_norm" and (isinstance(model, FastModel) or getattr(model, "_fused", False)):
            raise ValueError("streaming needs a causal norm: build the model with norm_type = 'cumulative_laplace_norm' "
                             "(fullsubnet/train_cumulativeLaplaceNorm.toml)")
        self._calls = (_ImprovedCalls(model) if self._improved else _FastCalls(model) if isinstance(model, FastModel)
                       else _FullSubNetCalls(model))
        # the transform: the model's own for Improved FullSubNet, 512 / 256 otherwise
        self.n_fft, self.hop = self._calls.fft
        self.model = model.eval()
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise _lib.FsnError("StreamPool needs the model on a ROCm device; this path has no CPU implementation")
        if not self._improved and model.num_freqs != N_FFT // 2 + 1:
            raise NotImplementedError(f"StreamPool is built for the 512 / 256 transform (num_freqs 257, got {model.num_freqs})")
        self.capacity = int(capacity)
        nbytes = self._calls.state_bytes(self.capacity)
        self.state = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self.slot_bytes = nbytes // self.capacity
        self._steps = [0] * self.capacity  # host mirror of the slots' step counts: model_step advances, reset_slots clears
        self.book = SessionBook(self.capacity, model.look_ahead, self.hop)
        self._window = torch.hann_window(self.n_fft, device=self.device)
        self.poison_buffers = bool(poison_buffers)  # debugging: NaN-fill every workspace and output before its call
        self._buf = {}   # sid -> (device samples from global index buf0 on, buf0)
        # Sessions at another rate than the model's (module docstring): two stateful resamplers around the tick.  With
        # the default arguments neither exists and no code below this block runs differently.
        self.model_sr = int(getattr(model, "sr", MODEL_SR))
        if input_sr is not None and (isinstance(input_sr, bool) or not isinstance(input_sr, int) or input_sr < 1):
            raise ValueError(f"input_sr must be a positive integer or None, got {input_sr!r}")
        self.input_sr = self.model_sr if input_sr is None else input_sr
        if output_sr == "model":
            self.output_sr = self.model_sr
        elif output_sr == "input":
            self.output_sr = self.input_sr
        elif isinstance(output_sr, bool) or not isinstance(output_sr, int) or output_sr < 1:
            raise ValueError(f'output_sr must be "model", "input" or a positive integer, got {output_sr!r}')
        else:
            self.output_sr = output_sr
        self.resample_design = resample_design
        self._down = self._up = None
        if self.input_sr != self.model_sr:
            self._down = StreamResampler(self.input_sr, self.model_sr, self.capacity, resample_design, self.device)
        if self.output_sr != self.model_sr:
            self._up = StreamResampler(self.model_sr, self.output_sr, self.capacity, resample_design, self.device)
        self.record_model_rate = bool(record_model_rate)  # debugging: keep every session's model-rate input and output
        self._recorded = {}  # sid -> ([input chunks], [output chunks]) at the model's rate; kept after close
        self._rate = {}      # sid -> _RateSession, while a resampler exists

    # ---- the three entries on a list of slots -------------------------------------------------
    def _ints(self, rows):
        return torch.tensor(rows, dtype=torch.int32, device=self.device)

    def _state_args(self):
        return (*self._calls.head, self.state.data_ptr(), self.state.numel(), self.capacity)

    def analysis(self, slots_dev, n, hops, prime, frame_no_dev):
        """hops [n, hop] (and prime [n, hop] = samples 1 .. hop of the sessions at frame 0, or None) -> mag [n, 1, F, 1]."""
        mag = torch.empty((n, 1, self.model.num_freqs, 1), dtype=torch.float32, device=self.device)
        if self.poison_buffers:
            mag.fill_(float("nan"))
        _lib.check(self._calls.analysis(
            *self._state_args(), slots_dev.data_ptr(), n, _lib.dev_ptr(hops, "hops"),
            _lib.dev_ptr(prime, "prime", allow_none=True), frame_no_dev.data_ptr(), self.n_fft, self.hop, _lib.dev_ptr(self._window),
            _lib.dev_ptr(mag), _lib.stream_ptr(self.device)))
        return mag

    def model_step(self, slots, mag, slots_dev=None):
        """Advance the listed slots (distinct ids in [0, capacity), any order) by the k frames of mag [n, 1, F, k], each
        from its own step count -> compressed cIRM [n, 2, F, k], rows in the caller's order."""
        ids = _check_slots(slots, self.capacity)
        n, k = len(ids), mag.shape[-1]
        if tuple(mag.shape) != (n, 1, self.model.num_freqs, k) or k < 1:
            raise ValueError(f"mag {tuple(mag.shape)}: need [{n}, 1, {self.model.num_freqs}, k >= 1]")
        # Fast FullSubNet: the rows that complete the larger number of low-rate frames go first (a stable sort on the host
        # mirror of the counts); the rows come back in the caller's order
        order, perm, n_long = self._calls.order([self._steps[i] for i in ids], k), None, n
        if order is not None:
            n_long = order[1]
            if order[0] != list(range(n)):
                perm = torch.tensor(order[0], dtype=torch.long, device=self.device)
                mag, slots_dev = mag.index_select(0, perm), self._ints([ids[i] for i in order[0]])
        if slots_dev is None:
            slots_dev = self._ints(ids)
        crm = torch.empty((n, 2, self.model.num_freqs, k), dtype=torch.float32, device=self.device)
        ws = _lib.workspace(self._calls.workspace_bytes(n, k), self.device)
        if self.poison_buffers:
            ws.view(torch.float32).fill_(float("nan"))
            crm.fill_(float("nan"))
        _lib.check(self._calls.step(
            *self._calls.head, self._calls.packed().data_ptr(), self.state.data_ptr(), self.state.numel(),
            self.capacity, slots_dev.data_ptr(), *self._calls.rows(n, n_long), _lib.dev_ptr(mag.contiguous(), "mag"), k,
            _lib.dev_ptr(crm), ws.data_ptr(), ws.numel(), _lib.stream_ptr(self.device)))
        for i in ids:
            self._steps[i] += k
        if perm is not None:
            crm = torch.empty_like(crm).index_copy_(0, perm, crm)
        return crm

    def synthesis(self, slots_dev, n, crm, first_frame_dev, tail_dev):
        """crm [n, 2, F, k] -> out [n, (k + 1) hop]: the hop of every column that is an output frame >= 1, then the tail."""
        k = crm.shape[-1]
        out = torch.empty((n, (k + 1) * self.hop), dtype=torch.float32, device=self.device)
        if self._improved:  # one frame per call (k = 1: no look-ahead), its number in the record, no workspace
            if self.poison_buffers:
                out.fill_(float("nan"))
            _lib.check(self._calls.synthesis(
                *self._state_args(), slots_dev.data_ptr(), n, _lib.dev_ptr(crm, "mask"), tail_dev.data_ptr(), self.n_fft, self.hop,
                _lib.dev_ptr(self._window), _lib.dev_ptr(out), _lib.stream_ptr(self.device)))
            return out
        ws = _lib.workspace(n * k * self.n_fft * 4, self.device)
        if self.poison_buffers:
            ws.view(torch.float32).fill_(float("nan"))
            out.fill_(float("nan"))
        _lib.check(self._calls.synthesis(
            *self._state_args(), slots_dev.data_ptr(), n, _lib.dev_ptr(crm, "crm"), k, first_frame_dev.data_ptr(),
            tail_dev.data_ptr(), self.n_fft, self.hop, _lib.dev_ptr(self._window), _lib.dev_ptr(out), ws.data_ptr(), ws.numel(),
            _lib.stream_ptr(self.device)))
        return out

    def reset_slots(self, slots):
        ids = _check_slots(slots, self.capacity)
        _lib.check(self._calls.reset(*self._state_args(), self._ints(ids).data_ptr(), len(ids), _lib.stream_ptr(self.device)))
        for i in ids:
            self._steps[i] = 0

    # ---- sessions -----------------------------------------------------------------------------
    def open(self):
        sid = self.book.open()
        self._buf[sid] = (torch.zeros(0, dtype=torch.float32, device=self.device), 0)
        if self._down is not None or self._up is not None:
            self._rate[sid] = _RateSession(self._down.open() if self._down is not None else None,
                                           self._up.open() if self._up is not None else None)
        if self.record_model_rate:
            self._recorded[sid] = ([], [])
        return sid

    def slot(self, sid):
        return self.book.slot(sid)

    def push(self, sid, chunk):
        s = self.book.session(sid)
        if s.closing:
            raise RuntimeError(f"session {sid} is closing")
        chunk = torch.as_tensor(chunk).to(self.device, torch.float32)
        if chunk.dim() != 1:
            raise ValueError(f"chunk must be 1-D samples, got shape {tuple(chunk.shape)}")
        if sid in self._rate:
            self._rate[sid].n_in += chunk.numel()
        if self._down is not None:  # the raw chunk waits for the next step()
            if chunk.numel():
                self._rate[sid].pending.append(chunk)
            return
        self._append(sid, chunk)

    def _append(self, sid, chunk):
        """Samples at the model's rate join the session's buffer."""
        if chunk.numel():
            buf, b0 = self._buf[sid]
            self._buf[sid] = (torch.cat([buf, chunk]), b0)
            self.book.push(sid, chunk.numel())
            if self.record_model_rate:
                self._recorded[sid][0].append(chunk)

    def recorded(self, sid):
        """(input, output) of a session at the model's rate so far (``record_model_rate=True``); kept after close."""
        x, y = self._recorded[sid]
        empty = torch.zeros(0, dtype=torch.float32, device=self.device)
        return torch.cat(x) if x else empty, torch.cat(y) if y else empty

    def _convert(self):
        """Every session's pending input to the model's rate: ONE call of the down resampler."""
        todo = {sid: r for sid, r in self._rate.items() if r.pending}
        if not todo:
            return
        got = self._down.push({r.down: torch.cat(r.pending) if len(r.pending) > 1 else r.pending[0] for r in todo.values()})
        for sid, r in todo.items():
            r.pending = []
            self._append(sid, got[r.down])

    def _emit(self, out):
        """A tick's outputs {sid: samples at the model's rate} to the output rate: ONE call of the up resampler."""
        if self.record_model_rate:
            for sid, y in out.items():
                self._recorded[sid][1].append(y)
        if self._up is None or not out:
            return out
        got = self._up.push({self._rate[sid].up: y for sid, y in out.items()})
        res = {}
        for sid in out:
            r = self._rate[sid]
            res[sid] = got[r.up]
            r.n_out += res[sid].numel()
        return res

    def _trim(self, sid):
        buf, b0 = self._buf[sid]
        keep = self.book.keep_from(sid)
        if keep > b0:
            self._buf[sid] = (buf[keep - b0:], keep)

    @torch.no_grad()
    def _tick(self, sids):
        """One frame of each listed session (all have one complete): {sid: samples}."""
        n = len(sids)
        order = self._calls.order([self._steps[self.book.slot(sid)] for sid in sids], 1)
        if order is not None:  # Fast FullSubNet: list the sessions in the order the model step wants, so that it moves no rows
            sids = [sids[i] for i in order[0]]
        hops, primes, rows = [], [], [[], [], [], []]  # slots, frame numbers, first output frames, tail samples
        counts, any_first = [], False
        for sid in sids:
            t, m, cnt = self.book.take_frame(sid)
            buf, b0 = self._buf[sid]
            hop = buf[t * self.hop - b0:(t + 1) * self.hop - b0]
            hops.append(hop)
            primes.append(buf[1 - b0:self.hop + 1 - b0] if t == 0 else hop)  # only read for frame 0
            any_first |= t == 0
            rows[0].append(self.book.slot(sid))
            rows[1].append(t)
            rows[2].append(m)
            rows[3].append(-1)
            counts.append(cnt)
        meta = self._ints(rows)
        mag = self.analysis(meta[0], n, torch.stack(hops), torch.stack(primes) if any_first else None, meta[1])
        crm = self.model_step(rows[0], mag, slots_dev=meta[0])
        out = self.synthesis(meta[0], n, crm, meta[2], meta[3])
        for sid in sids:
            self._trim(sid)
        return {sid: out[i, :cnt] for i, (sid, cnt) in enumerate(zip(sids, counts))}

    def step(self):
        """One frame for every session that has one ready: {sid: samples} (empty while the look-ahead fills)."""
        if self._down is not None:
            self._convert()
        sids = self.book.ready()
        if self._up is None and not self.record_model_rate:
            return self._tick(sids) if sids else {}
        return self._emit(self._tick(sids)) if sids else {}

    def drain(self):
        """step() until no session has a frame ready; the samples concatenated per session."""
        parts = {}
        while True:
            out = self.step()
            if not out:
                break
            for sid, y in out.items():
                parts.setdefault(sid, []).append(y)
        return {sid: torch.cat(ys) for sid, ys in parts.items()}

    def close(self, sid):
        """End of the session: its remaining samples; over drain() + close() a session of n samples at ``input_sr`` has
        returned exactly ``out_length(n, input_sr, output_sr)``."""
        if self._down is None and self._up is None and not self.record_model_rate:
            return self._close_model_rate(sid)
        r = self._rate.get(sid)
        if r is None:  # recording only
            tail = self._close_model_rate(sid)
            self._recorded[sid][1].append(tail)
            return tail
        self.book.session(sid)
        n_model = out_length(r.n_in, self.input_sr, self.model_sr)
        if n_model <= self.hop:  # before anything is flushed: the session stays as it is, like the plain pool's
            raise _lib.FsnError(f"session shorter than n_fft / 2 + 1 = {self.hop + 1} samples at the model's rate (reflect padding), "
                                f"like torch.stft: {r.n_in} samples at {self.input_sr} Hz are {n_model}")
        if self._down is not None:
            raw = torch.cat(r.pending) if r.pending else torch.zeros(0, dtype=torch.float32, device=self.device)
            r.pending = []
            self._append(sid, self._down.push({r.down: raw}, final=(r.down,))[r.down])
            self._down.close(r.down)
            assert self.book.session(sid).n_in == n_model
        tail = self._close_model_rate(sid)
        if self.record_model_rate:
            self._recorded[sid][1].append(tail)
        if self._up is not None:
            target = out_length(r.n_in, self.input_sr, self.output_sr)
            assert r.n_out <= target, (r.n_out, target)  # nothing beyond the target left before the end was known
            tail = self._up.push({r.up: tail}, final=(r.up,))[r.up]
            assert r.n_out + tail.numel() >= target
            tail = tail[:target - r.n_out]  # the round trip n -> model rate -> out can be a few samples long
            self._up.close(r.up)
        del self._rate[sid]
        return tail

    @torch.no_grad()
    def _close_model_rate(self, sid):
        """End of the session at the model's rate: its remaining samples.  Complete frames that were not stepped yet run one by one (n = 1);
        then the last frame (right-edge reflection) and the look_ahead zero frames run as ONE model call with n = 1,
        k = 1 + look_ahead, the overlap-add tail follows, and the slot is reset and freed."""
        left = self.book.begin_close(sid)
        parts = [self._tick([sid])[sid] for _ in range(left)]
        L = self.book.session(sid).n_in
        t, m0, k, skip, tail, cnt = self.book.take_last(sid)
        buf, b0 = self._buf[sid]
        j = torch.arange(t * self.hop, (t + 1) * self.hop, device=self.device)
        j = torch.where(j >= L, 2 * (L - 1) - j, j)  # torch.stft's reflect padding at the right edge
        hop = buf[j - b0][None]
        slot = self.book.slot(sid)
        meta = self._ints([[slot], [t], [m0], [tail]])
        mag = self.analysis(meta[0], 1, hop, None, meta[1])  # t = T - 1 >= 1: never a session's frame 0
        mag = torch.cat([mag, mag.new_zeros(1, 1, mag.shape[2], k - 1)], dim=-1)  # fullsubnet/model.py:85
        crm = self.model_step([slot], mag, slots_dev=meta[0])
        out = self.synthesis(meta[0], 1, crm, meta[2], meta[3])
        parts.append(out[0, skip * self.hop:skip * self.hop + cnt])
        self.reset_slots([slot])
        self.book.release(sid)
        del self._buf[sid]
        return torch.cat(parts)
