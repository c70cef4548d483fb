"""tests/improved_pool_reference.py without a device: the checkers of the GPU sweep on a CPU pool and on wrong stand-ins, the
records through the layout hook, and the size queries, the layout and every refusal of fsn_improved_stream_pool_* through
the built library (none of them needs a device); the header's ABI number, the new names in the header and in the binding;
the host book-keeping at a hop that is not 256."""
import ctypes
import os
import re

import numpy as np
import pytest

import improved_pool_reference as P
import improved_stream_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fsn_improved_stream_pool_state_bytes", "fsn_improved_stream_pool_workspace_bytes", "fsn_improved_stream_pool_reset",
         "fsn_improved_stream_pool_step", "fsn_improved_stream_pool_analysis", "fsn_improved_stream_pool_synthesis",
         "fsn_debug_improved_stream_pool_layout")


def test_the_sweep_covers_what_it_claims():
    assert [len(v) for v in P.LISTS.values()] == [1, 1, 3, 8, 16, 17]
    for name, ids in P.LISTS.items():
        inside = [i for i in ids if 0 <= i < P.CAP]
        assert len(set(ids)) == len(ids) and len(inside) == len(ids) - (2 if name == "seventeen" else 0)
    assert P.LISTS["sixteen"] == sorted(P.LISTS["sixteen"], reverse=True) and P.LISTS["seventeenth"] == [16]
    assert P.LISTS["seventeen"][0] < 0 and P.LISTS["seventeen"][-1] == P.CAP
    assert {P.slot_count(i) for i in range(P.CAP)} == set(P.COUNTS) and P.slot_count(0) == 0
    assert len({P.slot_count(i) for i in P.LISTS["three"]}) == 3  # three different counts in one call, not in slot order


@pytest.fixture(scope="module")
def cpu_calls():
    """The right stand-in (the fp32 cell emulation as a pool) on every list x k, judged by check_call; and which (list, k) each
    wrong stand-in fails."""
    cfg = R.SMALL
    before = P.start_pool(cfg)
    quiet = lambda *a: None  # noqa: E731
    caught = {w: [] for w in P.WRONG}
    worst = 0.0
    for name, slots in P.LISTS.items():
        for k in P.KS:
            mags = P.call_mags(cfg, slots, k)
            pool = P.copy_pool(before)
            mask = P.pool_step(pool, slots, mags, k, cfg)
            worst = max(worst, *P.check_call(f"cpu-{name}-k{k}", cfg, slots, k, mask, before, pool, log=quiet))
            for wrong in P.WRONG:
                pool = P.copy_pool(before)
                mask = P.pool_step(pool, slots, mags, k, cfg, wrong=wrong)
                try:
                    P.check_call(wrong, cfg, slots, k, mask, before, pool, log=quiet)
                except AssertionError:
                    caught[wrong].append((name, k))
    return worst, caught


def test_checkers_pass_the_cpu_pool_on_every_list(cpu_calls):
    assert cpu_calls[0] <= 1.0 + 1e-9  # it is the yardstick itself


@pytest.mark.parametrize("wrong", P.WRONG)
def test_checkers_catch_the_wrong_stand_in(cpu_calls, wrong):
    assert cpu_calls[1][wrong], f"{wrong} passes check_call on every list"


def test_records_travel_through_the_layout_unchanged():
    from fullsubnet_amd import _lib
    for cfg in (R.SMALL, R.TWO_SECTIONS, R.K48):
        lay = _lib.improved_stream_pool_layout(P.c_cfg(cfg))
        pool = {i: P.start_state(cfg, i) for i in (0, 1, 4, 7)}
        blob = P.records_to_blob(lay, cfg, pool, 8)
        back = P.blob_to_records(lay, cfg, blob, 8)
        for i in range(8):
            assert P.states_equal(back[i], pool.get(i, R.new_state(1, cfg))), i
        assert not P.transform_bytes(lay, blob, 1).any()


# ---- the C entries: sizes, layout, refusals (no device) ---------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [R.SMALL, R.SMALL_FDRC1, R.TWO_SECTIONS, R.K48, R.K16], ids=lambda c: f"F{c.F}-{len(c.centers)}sec")
def test_layout_fields_are_disjoint_aligned_and_inside_the_record(cfg):
    from fullsubnet_amd import _lib
    L = _lib.lib()
    c = P.c_cfg(cfg)
    lay = _lib.improved_stream_pool_layout(c)
    P.check_layout(lay, cfg)
    F, hop = cfg.F, cfg.F - 1
    sizes = {"fb_sum": 8, "sb_sum": 8 * 8, "steps": 8, "in_tail": 4 * hop, "ola_tail": 4 * hop, "spec_re": 4 * F, "spec_im": 4 * F, "frame": 4}
    spans = [(lay[n], lay[n] + b, n) for n, b in sizes.items()]
    spans += [(lay["fb"][a], lay["fb"][a] + 4 * cfg.fb_hidden, f"fb{a}") for a in range(4)]
    for i, n in enumerate(R.num_units(cfg)):
        spans += [(lay["sb"][i][a], lay["sb"][i][a] + 4 * n * cfg.sb_hidden, f"sb{i}.{a}") for a in range(4)]
    spans.sort()
    for (a0, a1, an), (b0, _, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, f"{an} overlaps {bn}"
    assert all(a0 % 256 == 0 and a0 >= 0 for a0, _, _ in spans)
    assert spans[-1][1] <= lay["slot_bytes"] and lay["slot_bytes"] % 256 == 0
    assert min(lay[n] for n in ("in_tail", "ola_tail", "spec_re", "spec_im", "frame")) == lay["in_tail"] > lay["steps"]  # transform_bytes
    for cap in (1, 20, 4096):
        assert L.fsn_improved_stream_pool_state_bytes(ctypes.byref(c), cap) == cap * lay["slot_bytes"]
    ws = {(n, k): L.fsn_improved_stream_pool_workspace_bytes(ctypes.byref(c), n, k) for n in (1, 2, 16, 17, 64) for k in (1, 2, 9)}
    for (n, k), b in ws.items():
        assert b > L.fsn_improved_stream_workspace_bytes(ctypes.byref(c), n, k) > 0  # the lockstep entry's and the compact state
        assert all(b <= ws[m, j] for (m, j) in ws if m >= n and j >= k), (n, k)      # monotone in n and in k
    assert ws[1, 1] < ws[1, 2] < ws[1, 9] and ws[1, 1] < ws[17, 1] < ws[64, 1]


def _step(L, c, cap=20, n=1, k=2, state_bytes=1 << 40, ws_bytes=1 << 40):
    """The step with pointers that are never read: every refusal comes before a launch."""
    return L.fsn_improved_stream_pool_step(c, 1, 1, state_bytes, cap, 1, n, 1, k, 1, 1, ws_bytes, None)


@pytest.mark.parametrize("kw,text", [(dict(cell=1), b"LSTM"), (dict(fdrc=0.3), b"fdrc"), (dict(F=2), b"F 2"), (dict(num_sections=1), b"sections"),
                                     (dict(fb_hidden=96), b"hidden"), (dict(sb_activation=2), b"activations"), (dict(F=35), b"tile")])
def test_configurations_the_lockstep_entry_refuses_are_refused(kw, text):
    from fullsubnet_amd import _lib
    L = _lib.lib()
    c = ctypes.byref(P.c_cfg(**kw))
    assert L.fsn_improved_stream_state_bytes(c, 1) == 0  # check_stream refuses it
    assert L.fsn_improved_stream_pool_state_bytes(c, 20) == 0 and text in L.fsn_last_error()
    assert L.fsn_improved_stream_pool_workspace_bytes(c, 1, 1) == 0 and text in L.fsn_last_error()
    assert L.fsn_debug_improved_stream_pool_layout(c, (ctypes.c_long * 58)(), 58) == -1
    assert _step(L, c) == -1 and text in L.fsn_last_error()
    assert L.fsn_improved_stream_pool_reset(c, 1, 1 << 40, 20, 1, 1, None) == -1 and text in L.fsn_last_error()
    assert L.fsn_improved_stream_pool_analysis(c, 1, 1 << 40, 20, 1, 1, 1, None, 1, 64, 32, 1, 1, None) == -1
    assert L.fsn_improved_stream_pool_synthesis(c, 1, 1 << 40, 20, 1, 1, 1, 1, 64, 32, 1, 1, None) == -1


def test_ranges_are_refused():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    c = ctypes.byref(P.c_cfg())
    for cap in (0, -1, 4097):
        assert L.fsn_improved_stream_pool_state_bytes(c, cap) == 0 and b"capacity" in L.fsn_last_error()
        assert _step(L, c, cap=cap) == -1 and b"capacity" in L.fsn_last_error()
    assert L.fsn_improved_stream_pool_state_bytes(c, 1) > 0 and L.fsn_improved_stream_pool_state_bytes(c, 4096) > 0
    for n in (0, -1, 21):
        assert _step(L, c, n=n) == -1 and b"slots listed" in L.fsn_last_error()
    for n, k in ((0, 1), (4097, 1), (1, 0), (1, 4097)):
        assert L.fsn_improved_stream_pool_workspace_bytes(c, n, k) == 0 and b"out of range" in L.fsn_last_error()
    assert _step(L, c, k=0) == -1 and _step(L, c, k=4097) == -1
    assert L.fsn_debug_improved_stream_pool_layout(c, (ctypes.c_long * 58)(), 57) == -1
    assert L.fsn_debug_improved_stream_pool_layout(c, None, 58) == -1
    # buffers too small: FSN_ERR_WORKSPACE, still before any launch
    sb = L.fsn_improved_stream_pool_state_bytes(c, 20)
    assert _step(L, c, state_bytes=sb - 1) == -2 and b"too small" in L.fsn_last_error()
    assert _step(L, c, state_bytes=sb, ws_bytes=L.fsn_improved_stream_pool_workspace_bytes(c, 1, 2) - 1) == -2 and b"too small" in L.fsn_last_error()
    assert L.fsn_improved_stream_pool_reset(c, 1, sb - 1, 20, 1, 1, None) == -2
    # the transform: an even n_fft with hop = n_fft / 2 = F - 1 (SMALL: 64 / 32)
    for n_fft, hop in ((64, 16), (62, 31), (512, 256), (63, 32)):
        assert L.fsn_improved_stream_pool_analysis(c, 1, sb, 20, 1, 1, 1, None, 1, n_fft, hop, 1, 1, None) == -1, (n_fft, hop)
        assert L.fsn_improved_stream_pool_synthesis(c, 1, sb, 20, 1, 1, 1, 1, n_fft, hop, 1, 1, None) == -1, (n_fft, hop)
    assert L.fsn_improved_stream_pool_analysis(c, 1, sb - 1, 20, 1, 1, 1, None, 1, 64, 32, 1, 1, None) == -2
    assert L.fsn_improved_stream_pool_synthesis(c, 1, sb - 1, 20, 1, 1, 1, 1, 64, 32, 1, 1, None) == -2


def test_the_abi_number_stays_and_the_names_are_declared_and_bound():
    from fullsubnet_amd import _lib
    header = open(os.path.join(ROOT, "include", "fsn_hip.h")).read()
    assert re.search(r"#define\s+FSN_ABI_VERSION\s+118\b", header) and _lib.ABI_VERSION == 118 and _lib.lib().fsn_version() == 118
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in include/fsn_hip.h"
        assert name in _lib.SIGNATURES and name in _lib.ADDED_IN_118
        assert hasattr(_lib.lib(), name)


def test_session_book_at_another_hop():
    """SessionBook(capacity, 0, hop=32) on a short session: frames, samples and tail add up to L."""
    from fullsubnet_amd.stream_pool import SessionBook
    hop = 32
    for L in (33, 64, 95, 96, 700):
        book = SessionBook(4, 0, hop=hop)
        sid = book.open()
        frames, samples, pushed = [], 0, 0
        for n in [1, 31, 1, 40, 7] + [hop] * 40:
            n = min(n, L - pushed)
            book.push(sid, n)
            pushed += n
            while book.has_frame(sid):
                t, m, cnt = book.take_frame(sid)
                assert m == t and cnt == (hop if t >= 1 else 0)  # no look-ahead: the step's frame is the output frame
                frames.append(t)
                samples += cnt
        assert pushed == L
        for _ in range(book.begin_close(sid)):
            t, m, cnt = book.take_frame(sid)
            frames.append(t)
            samples += cnt
        t, m0, k, skip, tail, cnt = book.take_last(sid)
        assert (t, m0, k, skip) == (L // hop, L // hop, 1, 0) and tail == L - t * hop and cnt == hop + tail
        frames.append(t)
        assert frames == list(range(1 + L // hop)) and samples + cnt == L
        assert book.release(sid) == 0
