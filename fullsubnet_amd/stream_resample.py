"""Sample-rate conversion of streams on the device (libfsn_hip ``fsn_resample_stream_*``): sessions that receive their
input chunk by chunk, and whose outputs are bit for bit those of ``resample.resample`` on the whole utterance.

    rs   = StreamResampler(48000, 16000, capacity=64)
    sid  = rs.open()
    out  = rs.push({sid: chunk, other: chunk2})     # ONE library call for all listed sessions -> {sid: samples}
    tail = rs.close(sid)                            # what the end of the input releases; the slot is free again

After ``n_in`` samples a session has emitted every output whose newest input has arrived (``ResampleBook.ready``); the
delay this adds is H / u input samples (30 samples = 0.625 ms at 48 -> 16 kHz with "scipy", 2 ms with "sharp"), DESIGN 9d.
A session carries its last J - 1 input samples in its slot of one device blob; every count lives on the host.

``ResampleBook`` is that host book-keeping; it makes no device call, so it is tested without a GPU.  There is no host
fallback: a CPU tensor raises."""
import ctypes

import torch

from . import _lib
from . import resample as _rs


class _Stream:
    __slots__ = ("slot", "n_in", "n_out", "parity", "final")

    def __init__(self, slot):
        self.slot = slot
        self.n_in = 0      # samples received
        self.n_out = 0     # outputs emitted
        self.parity = 0    # the history buffer of the slot that holds the last J - 1 samples
        self.final = False


class ResampleBook:
    """Host book-keeping of ``capacity`` resampling sessions at sr_in -> sr_out; no device calls.

    ``ready(n_in)`` is the number of outputs whose newest input q(k) = (k d + H) // u lies below n_in; at the end of the
    input it is ``out_length(n_in)``.  The parity of a session flips on exactly the pushes that carry samples and are
    not final: those are the pushes after which the device has written the other history buffer."""

    def __init__(self, capacity, sr_in, sr_out, design="scipy"):
        if capacity < 1:
            raise ValueError(f"capacity {capacity} < 1")
        self.capacity = int(capacity)
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        self.zeros = _rs.design_parameters(design)[0]
        self.u, self.d = _rs.ratio(sr_in, sr_out)
        if self.u == self.d == 1:   # chunks pass through: no filter, no delay, no history
            self.H, self.J = 0, 1
        else:
            self.H = self.zeros * max(self.u, self.d)
            self.J = -(-(2 * self.H + 1) // self.u)
        self.history = self.J - 1
        self._free = list(range(self.capacity))  # kept sorted: lowest id first
        self._s = {}
        self._next_sid = 0

    # ---- arithmetic ---------------------------------------------------------------------------
    def ready(self, n_in, final=False):
        if n_in < 0:
            raise ValueError(f"n_in = {n_in}")
        if final:
            return -(-n_in * self.u // self.d)
        return 0 if n_in * self.u <= self.H else (n_in * self.u - self.H - 1) // self.d + 1

    # ---- slots --------------------------------------------------------------------------------
    def open(self):
        if not self._free:
            raise RuntimeError(f"StreamResampler is full: all {self.capacity} slots hold an open session")
        sid = self._next_sid
        self._next_sid += 1
        self._s[sid] = _Stream(self._free.pop(0))
        return sid

    def session(self, sid):
        try:
            return self._s[sid]
        except KeyError:
            raise KeyError(f"StreamResampler: no open session {sid!r}") from None

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

    def restart(self, sid):
        """The session starts over in its slot (the caller has reset the slot)."""
        self._s[sid] = _Stream(self.session(sid).slot)

    # ---- chunks -------------------------------------------------------------------------------
    def take(self, sid, n_chunk, final=False):
        """Advance the session by a chunk of ``n_chunk`` samples: the fields of its item, (slot, n_chunk, final, parity,
        n_before, k0, count, 0) - ``count`` outputs from ``k0`` on become due with it."""
        s = self.session(sid)
        n_chunk = int(n_chunk)
        if n_chunk < 0:
            raise ValueError("negative sample count")
        if s.final:
            raise RuntimeError(f"session {sid}: its input has ended")
        n_before, k0, parity = s.n_in, s.n_out, s.parity
        s.n_in += n_chunk
        s.n_out = self.ready(s.n_in, final)
        if final:
            s.final = True
        elif n_chunk > 0:
            s.parity ^= 1
        return (s.slot, n_chunk, int(bool(final)), parity, n_before, k0, s.n_out - k0, 0)


class StreamResampler:
    def __init__(self, sr_in, sr_out, capacity=64, design="scipy", device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.FsnError(f"StreamResampler needs a ROCm device (got {self.device}); this path has no CPU implementation")
        self.zeros, self.beta, self.rolloff = _rs.design_parameters(design)
        self.book = ResampleBook(capacity, sr_in, sr_out, design)
        self.sr_in, self.sr_out, self.capacity = self.book.sr_in, self.book.sr_out, self.book.capacity
        L = _lib.lib()
        nbytes = L.fsn_resample_stream_state_bytes(self.sr_in, self.sr_out, self.zeros, self.capacity)
        if nbytes == 0:
            raise _lib.FsnError(L.fsn_last_error().decode())
        with torch.cuda.device(self.device):
            self.state = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(L.fsn_resample_stream_init(*self._state_args(), self.beta, self.rolloff, _lib.stream_ptr(self.device)))
        self.calls = 0  # library calls of push(): one per call that lists a session
        self.last_rows = None

    def _state_args(self):
        return self.state.data_ptr(), self.state.numel(), self.capacity, self.sr_in, self.sr_out, self.zeros

    def slot_bytes(self, slot):
        """The bytes of one slot of the state blob (a view)."""
        n = 4 * ((max(2 * self.book.history, 1) + 63) // 64 * 64)
        first = self.state.numel() - self.capacity * n
        return self.state[first + slot * n:first + (slot + 1) * n]

    # ---- sessions -----------------------------------------------------------------------------
    def open(self):
        return self.book.open()

    def slot(self, sid):
        return self.book.slot(sid)

    def _chunk(self, sid, chunk):
        if not isinstance(chunk, torch.Tensor):
            raise _lib.FsnError(f"session {sid}: a chunk must be a tensor on a ROCm device, got {type(chunk).__name__}")
        if not chunk.is_cuda:
            raise _lib.FsnError(f"session {sid}: the chunk must live on a ROCm device (got {chunk.device}); this path has no "
                                "CPU implementation")
        if chunk.dim() != 1:
            raise ValueError(f"session {sid}: a chunk must be 1-D samples, got shape {tuple(chunk.shape)}")
        return chunk.to(self.device, torch.float32)

    def push(self, chunks, final=(), poison=False):
        """``chunks`` {sid: 1-D samples, any length >= 0} -> {sid: the outputs that became due}; the sessions in ``final``
        end with this chunk (they may be listed with an empty one) and receive their remaining outputs.  One library call
        and one small copy of the item table, no synchronisation."""
        final = set(final)
        unknown = final - set(chunks)
        if unknown:
            raise KeyError(f"final sessions {sorted(unknown)} are not among the chunks")
        if not chunks:
            return {}
        sids = list(chunks)
        rows = [self._chunk(sid, chunks[sid]) for sid in sids]
        for sid in sids:  # before any session advances
            if self.book.session(sid).final:
                raise RuntimeError(f"session {sid}: its input has ended")
        items = [self.book.take(sid, row.numel(), sid in final) for sid, row in zip(sids, rows)]
        n = len(sids)
        C = max(1, max(row.numel() for row in rows))
        O = max(1, max(item[6] for item in items))
        with torch.cuda.device(self.device):
            if n == 1 and rows[0].numel() == C:
                x = rows[0].contiguous().view(1, C)
            elif all(row.numel() == C for row in rows):
                x = torch.stack(rows)  # a tick: every chunk as long as the others, one copy kernel
            elif any(row.numel() for row in rows):
                x = torch.nn.utils.rnn.pad_sequence(rows, batch_first=True)  # [n, C], a copy per session
            else:
                x = torch.zeros((n, 1), dtype=torch.float32, device=self.device)
            table = torch.tensor(items, dtype=torch.int64, device=self.device)
            y = torch.empty((n, O), dtype=torch.float32, device=self.device)
            if poison:
                y.fill_(float("nan"))
            _lib.check(_lib.lib().fsn_resample_stream_push(*self._state_args(), table.data_ptr(), n, _lib.dev_ptr(x, "x"), C,
                                                           _lib.dev_ptr(y, "y"), O, _lib.stream_ptr(self.device)))
        self.calls += 1
        self.last_rows = y  # the whole rows of the last call (a test hook: zeros behind every count)
        return {sid: y[i, :item[6]] for i, (sid, item) in enumerate(zip(sids, items))}

    def reset(self, sid):
        """The session starts over: its slot is zeroed, its counts return to 0."""
        slot = self.book.slot(sid)
        with torch.cuda.device(self.device):
            ids = torch.tensor([slot], dtype=torch.int32, device=self.device)
            _lib.check(_lib.lib().fsn_resample_stream_reset(*self._state_args(), ids.data_ptr(), 1, _lib.stream_ptr(self.device)))
        self.book.restart(sid)

    def close(self, sid):
        """End of the session's input: its remaining outputs; the slot is reset and free again."""
        empty = torch.zeros(0, dtype=torch.float32, device=self.device)
        tail = self.push({sid: empty}, final=(sid,))[sid] if not self.book.session(sid).final else empty
        self.reset(sid)
        self.book.release(sid)
        return tail
