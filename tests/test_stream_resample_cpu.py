"""The streaming resampler's host side (fullsubnet_amd.stream_resample, fsn_resample_stream_ready) without a
GPU: which outputs are due after n_in samples, how much history they need, that a chunked evaluation in the pinned order
equals the whole-row one whatever the chunking, what the pool trims after a round trip, and the slot book-keeping."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_reference as R  # noqa: E402
from fullsubnet_amd import ResampleBook, _lib  # noqa: E402
from fullsubnet_amd.resample import out_length  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(a, b, "scipy") for a, b in R.RATIOS] + [(a, b, "sharp") for a, b in R.SHARP_RATIOS]
IDS = [f"{a}to{b}-{design}" for a, b, design in CASES]


def geometry(sr_in, sr_out, design):
    """(u, d, H, J) of DESIGN 9c, worked out here and not taken from the book; the identity has no filter."""
    u, d = R.ratio(sr_in, sr_out)
    if u == d == 1:
        return 1, 1, 0, 1
    H = R.DESIGNS[design][0] * max(u, d)
    return u, d, H, -(-(2 * H + 1) // u)


@pytest.mark.parametrize("sr_in,sr_out,design", CASES, ids=IDS)
def test_readiness_against_brute_force(sr_in, sr_out, design):
    u, d, H, J = geometry(sr_in, sr_out, design)
    book = ResampleBook(4, sr_in, sr_out, design)
    assert (book.u, book.d, book.H, book.J, book.history) == (u, d, H, J, J - 1)
    L = _lib.lib()
    zeros = R.DESIGNS[design][0]
    newest = lambda k: (k * d + H) // u
    for n_in in range(201):
        r = book.ready(n_in)
        assert r == L.fsn_resample_stream_ready(n_in, 0, sr_in, sr_out, zeros), n_in
        assert all(newest(k) < n_in for k in range(r)), n_in      # every emitted output has all its inputs
        assert newest(r) >= n_in, n_in                            # and the next one does not: nothing waits longer
        # history: the oldest sample any pending output touches is one of the last J - 1
        assert newest(r) - (J - 1) >= n_in - (J - 1)
        assert book.ready(n_in, final=True) == out_length(n_in, sr_in, sr_out) == R.out_length(n_in, sr_in, sr_out)
        assert L.fsn_resample_stream_ready(n_in, 1, sr_in, sr_out, zeros) == out_length(n_in, sr_in, sr_out)
        assert r <= book.ready(n_in, final=True)
    if u == d == 1:
        assert [book.ready(n) for n in range(5)] == list(range(5))  # no delay


def test_ready_refusals_and_bindings():
    L = _lib.lib()
    assert L.fsn_resample_stream_ready(-1, 0, 48000, 16000, 10) == -1
    assert L.fsn_resample_stream_ready(10, 0, 0, 16000, 10) == -1 and b"rates" in L.fsn_last_error()
    assert L.fsn_resample_stream_ready(10, 0, 48000, 16000, 0) == -1
    assert L.fsn_resample_stream_state_bytes(48000, 16000, 10, 0) == 0 and b"capacity" in L.fsn_last_error()
    assert L.fsn_resample_stream_state_bytes(48000, 16000, 0, 4) == 0
    assert L.fsn_resample_stream_state_bytes(48000, 48001, 10, 4) == 0  # max(u, d) past FSN_RESAMPLE_MAX_P
    one, two = (L.fsn_resample_stream_state_bytes(48000, 16000, 10, c) for c in (1, 2))
    assert 0 < one < two and (two - one) % 256 == 0 and two - one >= 2 * 20 * 4  # a slot: two histories of J - 1 = 20
    # a blob of the wrong size, n outside [1, capacity], NULL pointers: refused on the host, before any device call
    for call, args in (("init", (5.0, 1.0, None)), ("push", (1, 1, 1, 1, 1, 1, None)), ("reset", (1, 1, None))):
        fn = getattr(L, "fsn_resample_stream_" + call)
        assert fn(256, one + 256, 1, 48000, 16000, 10, *args) == -1 and b"bytes" in L.fsn_last_error(), call
        assert fn(None, one, 1, 48000, 16000, 10, *args) == -1, call
    assert L.fsn_resample_stream_push(256, two, 2, 48000, 16000, 10, 256, 3, 256, 1, 512, 1, None) == -1
    assert b"n = 3" in L.fsn_last_error()
    assert L.fsn_resample_stream_push(256, two, 2, 48000, 16000, 10, 256, 0, 256, 1, 512, 1, None) == -1
    assert L.fsn_resample_stream_reset(256, two, 2, 48000, 16000, 10, 256, 3, None) == -1
    assert L.fsn_resample_stream_init(256, two, 2, 48000, 16000, 10, 300.0, 1.0, None) == -1 and b"beta" in L.fsn_last_error()
    header = open(os.path.join(ROOT, "include", "fsn_hip.h")).read()
    for name in ("fsn_resample_stream_ready", "fsn_resample_stream_state_bytes", "fsn_resample_stream_init",
                 "fsn_resample_stream_push", "fsn_resample_stream_reset"):
        decl = re.search(r"\b%s\(([^;]*?)\);" % name, header, flags=re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert name in _lib.ADDED_IN_118


# ---- a numpy model of the stream: fp64, the sum in the pinned order -----------------------------------------------------
def pinned(ks, sample, poly, u, d, H, J):
    """y[k] = sum_j poly[phase][j] x[q - j], j = 0 .. J - 1 in that order from 0.0; ``sample(m)`` -> x[m] (vectorised)."""
    ks = np.asarray(ks, dtype=np.int64)
    c = ks * d + H
    q, phase = c // u, c % u
    acc = np.zeros(len(ks))
    for j in range(J):
        acc = acc + poly[phase, j] * sample(q - j)
    return acc


def table(sr_in, sr_out, design):
    u, d, H, J = geometry(sr_in, sr_out, design)
    if u == d == 1:
        return np.ones((1, 1))  # chunks pass through
    h = R.taps(sr_in, sr_out, design)[0]
    poly = np.zeros((u, J))
    poly[np.arange(len(h)) % u, np.arange(len(h)) // u] = h
    return poly


class NumpyStream:
    """Carries the last J - 1 samples and nothing else."""

    def __init__(self, sr_in, sr_out, design):
        self.u, self.d, self.H, self.J = geometry(sr_in, sr_out, design)
        self.poly = table(sr_in, sr_out, design)
        self.book = ResampleBook(1, sr_in, sr_out, design)
        self.sid = self.book.open()
        self.hist = np.zeros(self.J - 1)

    def push(self, chunk, final=False):
        _, n, _, _, n_before, k0, count, _ = self.book.take(self.sid, len(chunk), final)
        window = np.concatenate([self.hist, chunk])  # samples n_before - (J - 1) .. n_before + n - 1
        first = n_before - (self.J - 1)

        def sample(m):
            assert (m >= first).all(), "an output reaches behind the carried history"
            i = m - first
            inside = i < len(window)
            assert final or inside.all(), "an output was emitted before its newest input"
            return np.where(inside, window[np.minimum(i, len(window) - 1)] if len(window) else 0.0, 0.0)

        y = pinned(np.arange(k0, k0 + count), sample, self.poly, self.u, self.d, self.H, self.J)
        self.hist = window[len(window) - (self.J - 1):] if self.J > 1 else window[:0]
        return y


def schedules(n, rng):
    random = []
    while sum(random) < n:
        random.append(int(min(rng.choice([0, 1, int(rng.integers(2, 400))]), n - sum(random))))
    return [random, [0, 1, 0, 1, 1] + [n - 3], [n], [1] * 60 + [n - 60]]


@pytest.mark.parametrize("sr_in,sr_out,design", CASES, ids=IDS)
def test_any_chunking_equals_the_whole_row(sr_in, sr_out, design):
    u, d, H, J = geometry(sr_in, sr_out, design)
    n = 1500
    rng = np.random.default_rng(sr_in * 7 + sr_out)
    x = R.signal(n, seed=sr_in + 31 * sr_out).astype(np.float64)
    poly = table(sr_in, sr_out, design)
    whole = pinned(np.arange(R.out_length(n, sr_in, sr_out)), lambda m: np.where((m >= 0) & (m < n), x[np.clip(m, 0, n - 1)], 0.0),
                   poly, u, d, H, J)
    if (u, d) != (1, 1):  # the pinned order is the reference's sum up to rounding
        ref = R.resample(x, sr_in, sr_out, design)
        assert np.abs(whole - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    for sizes in schedules(n, rng):
        assert sum(sizes) == n
        s, parts, pos = NumpyStream(sr_in, sr_out, design), [], 0
        for i, c in enumerate(sizes):
            parts.append(s.push(x[pos:pos + c], final=False))
            pos += c
        parts.append(s.push(x[:0], final=True))
        got = np.concatenate(parts)
        assert got.shape == whole.shape
        assert np.array_equal(got, whole), sizes[:8]
    s = NumpyStream(sr_in, sr_out, design)  # the end of the input arriving with the last samples
    assert np.array_equal(np.concatenate([s.push(x[:700]), s.push(x[700:], final=True)]), whole)


def test_round_trip_excess_stays_below_the_up_sides_delay():
    """What StreamPool trims at close: n samples -> the model's rate -> the output rate can be a few samples more than
    out_length(n, in, out); they lie inside the up side's delay H / d, so none was emitted before the end was known."""
    worst = 0
    pairs = [(a, b) for a, b in R.RATIOS if a != b] + [(48000, 16000), (44100, 16000), (8000, 16000), (22050, 16000)]
    for zeros in (R.DESIGNS["scipy"][0], R.DESIGNS["sharp"][0]):
        for a, b in pairs:                       # a: the input rate, b: the model's
            for c in {a, 3 * b, 2 * b}:          # "input" and two other output rates
                if c == b:
                    continue
                u, d = R.ratio(b, c)
                delay = zeros * max(u, d) / d    # H / d, in output samples
                for n in range(3001):
                    excess = out_length(out_length(n, a, b), b, c) - out_length(n, a, c)
                    assert 0 <= excess < delay, (a, b, c, n)
                    worst = max(worst, excess)
    assert worst <= 3


def test_book_keeping():
    book = ResampleBook(3, 48000, 16000)
    a, b, c = book.open(), book.open(), book.open()
    assert [book.slot(s) for s in (a, b, c)] == [0, 1, 2] and book.sids() == [a, b, c]
    with pytest.raises(RuntimeError, match="full"):
        book.open()
    assert book.release(b) == 1 and book.release(a) == 0
    e = book.open()
    assert book.slot(e) == 0 and book.slot(book.open()) == 1  # lowest free slot first
    with pytest.raises(KeyError):
        book.take(b, 10)
    # items: (slot, n_chunk, final, parity, n_before, k0, count, 0); the parity flips on exactly the pushes that carry
    # samples and are not final
    assert book.take(c, 0) == (2, 0, 0, 0, 0, 0, 0, 0)
    assert book.take(c, 10) == (2, 10, 0, 0, 0, 0, 0, 0)          # 10 u <= H = 30: nothing due
    assert book.take(c, 0) == (2, 0, 0, 1, 10, 0, 0, 0)
    assert book.take(c, 20) == (2, 20, 0, 1, 10, 0, 0, 0)         # 30 samples: output 0 waits for sample H / u = 30
    assert book.take(c, 1) == (2, 1, 0, 0, 30, 0, 1, 0)           # here it is
    assert book.take(c, 768) == (2, 768, 0, 1, 31, 1, 256, 0)     # a tick: 768 in, 256 out
    assert book.take(c, 5, final=True) == (2, 5, 1, 0, 799, 257, out_length(804, 48000, 16000) - 257, 0)
    assert book.session(c).parity == 0                             # a final push writes no history
    with pytest.raises(RuntimeError, match="ended"):
        book.take(c, 1)
    with pytest.raises(ValueError):
        book.take(e, -1)
    book.restart(c)
    assert book.take(c, 3) == (2, 3, 0, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        ResampleBook(0, 48000, 16000)
