"""The streaming pool without a device: the C entries in the header / ctypes table / built library, their size queries,
and the host book-keeping (fullsubnet_amd.stream_pool.SessionBook: frames, model steps, samples, slots)."""
import ctypes
import os
import re

import numpy as np
import pytest

from fullsubnet_amd import _lib
from fullsubnet_amd.stream_pool import SessionBook

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["fsn_fullsubnet_stream_pool_state_bytes", "fsn_fullsubnet_stream_pool_workspace_bytes",
           "fsn_fullsubnet_stream_pool_reset", "fsn_fullsubnet_stream_pool_step",
           "fsn_stream_pool_analysis", "fsn_stream_pool_synthesis"]
LA, HOP = 2, 256


def cfg(norm=1):
    return _lib.Cfg(num_freqs=257, look_ahead=LA, sb_num_neighbors=15, fb_hidden=512, sb_hidden=384, norm_type=norm, arith=0)


def test_entries_are_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "fsn_hip.h")).read()
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b(int|size_t) " + name + r"\(", src), name
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert "#define FSN_ABI_VERSION 118" in src and _lib.ABI_VERSION == 118 and L.fsn_version() == 118
    # the argument counts of the declarations and of the ctypes table agree
    for name in ENTRIES:
        decl = re.search(r"\b(?:int|size_t) " + name + r"\(([^;()]*)\);", src).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_state_bytes_query():
    L = _lib.lib()
    c = cfg()
    sizes = [L.fsn_fullsubnet_stream_pool_state_bytes(ctypes.byref(c), cap) for cap in (1, 2, 3, 17, 64, 4096)]
    assert sizes[0] > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))
    # equal records, one per slot; a record holds at least (h, c) of the four layers and the two fp64 sums
    assert all(s % cap == 0 for s, cap in zip(sizes, (1, 2, 3, 17, 64, 4096))) and sizes[3] // 17 == sizes[0]
    assert sizes[0] >= 4 * (512 + 257 * 384) * 4 + 8 * (1 + 257) + 4
    assert L.fsn_fullsubnet_stream_pool_state_bytes(ctypes.byref(c), 0) == 0
    assert L.fsn_fullsubnet_stream_pool_state_bytes(ctypes.byref(c), 4097) == 0
    assert "capacity" in L.fsn_last_error().decode()
    off = cfg(norm=0)
    assert L.fsn_fullsubnet_stream_pool_state_bytes(ctypes.byref(off), 4) == 0
    assert "causal" in L.fsn_last_error().decode()


def test_workspace_bytes_query():
    L = _lib.lib()
    c = cfg()
    q = lambda n, k: L.fsn_fullsubnet_stream_pool_workspace_bytes(ctypes.byref(c), n, k)  # noqa: E731
    assert q(1, 1) > 0
    for k in (1, 3):
        row = [q(n, k) for n in (1, 2, 3, 16, 17, 64)]
        assert all(b >= a > 0 for a, b in zip(row, row[1:]))
    for n in (1, 17):
        col = [q(n, k) for k in (1, 2, 3, 8)]
        assert all(b >= a > 0 for a, b in zip(col, col[1:]))
    # at least the lockstep step's workspace plus the compact (h, c) tiles
    assert q(3, 2) >= L.fsn_fullsubnet_stream_workspace_bytes(ctypes.byref(c), 3, 2) + 4 * (16 * 512 + 784 * 384) * 4
    assert q(0, 1) == 0 and q(1, 0) == 0
    off = cfg(norm=0)
    assert L.fsn_fullsubnet_stream_pool_workspace_bytes(ctypes.byref(off), 1, 1) == 0


def chunkings(L):
    yield "hop", [HOP] * (L // HOP) + ([L % HOP] if L % HOP else [])
    yield "one", [L]
    rng = np.random.default_rng(L)
    sizes = []
    while sum(sizes) < L:
        sizes.append(int(min(rng.integers(1, 900), L - sum(sizes))))
    yield "random", sizes


def run_book(L, sizes, check_latency):
    book = SessionBook(capacity=2, look_ahead=LA)
    sid = book.open()
    for n in sizes:
        book.push(sid, n)
        while book.ready():
            assert book.ready() == [sid]
            t, m, cnt = book.take_frame(sid)
            assert m == t - LA and cnt == (HOP if m >= 1 else 0)
            assert book.keep_from(sid) <= max(t - 1, 0) * HOP  # the next frame's left half is still buffered
        s = book.session(sid)
        if check_latency:
            assert s.n_in - s.n_out <= (2 + 2) * HOP
    s = book.session(sid)
    assert s.n_in == L and s.frames_out_at_close == 0
    before = s.frames_out
    for _ in range(book.begin_close(sid)):
        book.take_frame(sid)
    t, m0, k, skip, tail, cnt = book.take_last(sid)
    T = 1 + L // HOP
    assert t == T - 1 and m0 == t - LA and k == 1 + LA and tail == L - (T - 1) * HOP
    assert 0 <= skip <= k and cnt == (k - skip) * HOP + tail
    assert before + s.frames_out_at_close == s.frames_out == T
    assert s.steps == T + LA
    assert s.n_out == L
    assert book.release(sid) == 0


def test_book_keeping_for_every_length():
    for L in range(257, 2101):
        for name, sizes in chunkings(L):
            assert sum(sizes) == L
            run_book(L, sizes, check_latency=name == "hop")


def test_book_refuses_short_sessions_and_early_frames():
    book = SessionBook(capacity=1, look_ahead=LA)
    sid = book.open()
    book.push(sid, 256)
    assert not book.ready()  # frame 0 reflects sample 256
    with pytest.raises(RuntimeError):
        book.take_frame(sid)
    with pytest.raises(_lib.FsnError, match="shorter"):
        book.begin_close(sid)
    book.push(sid, 1)
    assert book.ready() == [sid]
    with pytest.raises(ValueError):
        book.push(sid, -1)


def test_slot_allocation():
    book = SessionBook(capacity=3, look_ahead=LA)
    a, b, c = book.open(), book.open(), book.open()
    assert [book.slot(s) for s in (a, b, c)] == [0, 1, 2] and len({a, b, c}) == 3
    with pytest.raises(RuntimeError, match="full"):
        book.open()
    assert book.release(c) == 2 and book.release(a) == 0
    d = book.open()
    assert book.slot(d) == 0 and d not in (a, b, c)  # lowest free slot first; ids are never reused
    e = book.open()
    assert book.slot(e) == 2
    for bad in (a, c, 12345, "x"):
        with pytest.raises(KeyError):
            book.slot(bad)
        with pytest.raises(KeyError):
            book.push(bad, 10)
        with pytest.raises(KeyError):
            book.release(bad)
    assert book.sids() == [d, b, e]  # slot order
    with pytest.raises(ValueError):
        SessionBook(capacity=0, look_ahead=LA)
