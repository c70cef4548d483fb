"""tests/fast_pool_reference.py without a device: the lo / hi claim the compaction rests on, fast_pool_order against its
definition, the checkers of the GPU sweep on a CPU pool and on wrong stand-ins, and the size queries, the layout hook and
every refusal of fsn_fast_stream_pool_* through the built library (none of them needs a device)."""
import ctypes

import numpy as np
import pytest

import fast_pool_reference as P
import fast_stream_reference as R


def test_every_window_holds_lo_or_hi_multiples():
    """A window [t0, t0 + k) holds floor(k / s) or ceil(k / s) multiples of s - by brute force; both occur unless s | k."""
    for s in range(1, 6):
        for k in range(1, 13):
            lo, hi = P.lo_hi(k, s)
            seen = set()
            for t0 in range(0, 41):
                brute = sum(1 for t in range(t0, t0 + k) if t % s == 0)
                assert brute == P.low_frames(t0, k, s) and brute in (lo, hi), (s, k, t0, brute)
                seen.add(brute)
            assert seen == {lo, hi}, (s, k, seen)
            assert (lo == hi) == (k % s == 0)


def test_fast_pool_order_is_the_stable_sort_of_its_definition():
    from fullsubnet_amd.stream_pool import fast_pool_order
    rng = np.random.default_rng(5)
    for _ in range(300):
        s, k, n = int(rng.integers(1, 6)), int(rng.integers(1, 13)), int(rng.integers(1, 40))
        steps = [int(x) for x in rng.choice([0, 1, 2, 3, 5, 7, R.LONG, R.LONG + 1, 2 ** 31 - 1 - 12], n)]
        perm, n_long = fast_pool_order(steps, k, s)
        assert sorted(perm) == list(range(n))
        assert (perm, n_long) == P.order_by_definition(steps, k, s)
        hi = P.lo_hi(k, s)[1]
        is_long = [P.low_frames(steps[i], k, s) == hi for i in perm]
        assert is_long == [True] * n_long + [False] * (n - n_long)      # the long rows are a prefix
        assert perm[:n_long] == sorted(perm[:n_long]) and perm[n_long:] == sorted(perm[n_long:])  # stable
        if k % s == 0:
            assert n_long == n
    assert fast_pool_order([], 1, 2) == ([], 0)
    for bad in (([0], 0, 2), ([0], 1, 0), ([-1], 1, 2)):
        with pytest.raises(ValueError):
            fast_pool_order(*bad)


def test_the_sweep_covers_what_it_claims():
    for cfg in (R.SHIPPED, P.SMALL):
        assert {P.slot_count(i) % cfg.shrink for i in range(P.CAP)} == set(range(cfg.shrink))
        assert {P.slot_count(i) % cfg.shrink for i in P.LISTS["three-phases"]} == set(range(min(cfg.shrink, 3)))
        assert P.not_due_list(cfg) and all(P.low_frames(P.slot_count(i), 1, cfg.shrink) == 0 for i in P.not_due_list(cfg))
        for name, ids in P.LISTS.items():
            assert len(set(ids)) == len(ids) and all(0 <= i < P.CAP for i in ids)
            for k in P.ks_of(cfg):
                rows, n_long = P.call_rows(cfg, name, k)
                assert len(rows) == len(ids) + (2 if name == "seventeen" else 0) and 0 <= n_long <= len(rows)
                hi = P.lo_hi(k, cfg.shrink)[1]
                for r, i in enumerate(rows):
                    if 0 <= i < P.CAP:
                        assert (P.low_frames(P.slot_count(i), k, cfg.shrink) == hi) == (r < n_long), (name, k, r, i)
    assert [len(v) for v in P.LISTS.values()] == [1, 1, 3, 8, 16, 15]
    rows, n_long = P.call_rows(R.SHIPPED, "seventeen", 3)
    assert rows[0] == P.OUTSIDE[0] and rows[-1] == P.OUTSIDE[1] and 1 < n_long < len(rows)  # one on each side of n_long
    assert P.ks_of(R.SHIPPED) == [1, 3, 4] and P.ks_of(P.SMALL) == [1, 2]


CASES = [(P.SMALL, [2, 0, 1, P.CAP], 1), (P.SMALL, [5, 1, 3, 2], 2)]


@pytest.mark.parametrize("cfg,slots,k", CASES, ids=["k1", "k2"])
def test_checkers_pass_the_cpu_pool_and_catch_the_wrong_ones(cfg, slots, k):
    """The fp32 cell emulation as a pool passes check_call (it is the yardstick); each wrong stand-in is caught."""
    before = {i: P.start_state(cfg, i) for i in range(8)}
    mags = [P.slot_mag(i, k) for i in slots]
    quiet = lambda *a: None  # noqa: E731
    pool = P.copy_pool(before)
    crm = P.pool_step(pool, slots, mags, k, cfg)
    worst = P.check_call("cpu", cfg, slots, k, crm, before, pool, log=quiet)
    assert max(worst) <= 1.0 + 1e-9
    caught = {}
    for wrong in P.WRONG:
        pool = P.copy_pool(before)
        crm = P.pool_step(pool, slots, mags, k, cfg, wrong=wrong)
        try:
            P.check_call(wrong, cfg, slots, k, crm, before, pool, log=quiet)
            caught[wrong] = False
        except AssertionError:
            caught[wrong] = True
    need = set(P.WRONG)
    if k == 1:  # slot 0 alone is due, from a fresh state: the bottleneck's first output is zero behind its ReLU, like the held
        need.discard("held-not-refreshed")  # output it replaces - only the k = 2 case, with due slots mid-stream, can tell
    assert all(caught[w] for w in need), caught


def test_records_travel_through_the_layout_unchanged():
    from fullsubnet_amd import _lib
    for cfg in (R.SHIPPED, P.SMALL):
        lay = _lib.fast_stream_pool_layout(P.c_cfg(cfg), cfg.la)
        pool = {i: P.start_state(cfg, i) for i in (0, 1, 4, 7)}
        blob = P.records_to_blob(lay, cfg, pool, 8)
        back = P.blob_to_records(lay, cfg, blob, 8)
        for i in range(8):
            want = pool.get(i, R.new_state(1, cfg))
            assert P.states_equal(back[i], want), i
        assert not P.transform_bytes(lay, blob, 1).any()


# ---- the C entries: sizes, layout, refusals (no device) ---------------------------------------------------------------------

@pytest.mark.parametrize("cfg", [R.SHIPPED, P.SMALL, R.Cfg(shrink=1, la=0), R.Cfg(bn_hidden=512, bn_layers=1, la=64)], ids=str)
def test_layout_fields_are_disjoint_aligned_and_inside_the_record(cfg):
    from fullsubnet_amd import _lib
    L = _lib.lib()
    c = P.c_cfg(cfg)
    lay = _lib.fast_stream_pool_layout(c, cfg.la)
    W, H, FP, Rr = R.unit_width(cfg), cfg.bn_hidden, 272, cfg.la + 1
    assert (lay["F"], lay["FP"], lay["R"], lay["bn_hidden"], lay["bn_layers"], lay["unit_width"]) == (257, FP, Rr, H, cfg.bn_layers, W)
    sizes = {"enc0_h": 384 * 4, "enc0_c": 384 * 4, "enc1_h": 320 * 4, "enc1_c": 320 * 4, "dec0_h": 512 * 4, "dec0_c": 512 * 4,
             "dec1_h": 512 * 4, "dec1_c": 512 * 4, "bn_h0": 64 * H * 4, "bn_c0": 64 * H * 4, "mel_sum": 8, "unit_sum": 64 * 8,
             "partial": 64 * W * 4, "held": 64 * 4, "steps": 4, "in_tail": 1024, "ola_tail": 1024, "ring_re": Rr * FP * 4,
             "ring_im": Rr * FP * 4}
    if cfg.bn_layers == 2:
        sizes.update(bn_h1=64 * H * 4, bn_c1=64 * H * 4)
    else:
        assert lay["bn_h1"] == lay["bn_c1"] == -1
    spans = sorted((lay[n], lay[n] + b, n) for n, b in sizes.items())
    for (a0, a1, an), (b0, _, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, f"{an} overlaps {bn}"
    assert all(a0 % 256 == 0 and a0 >= 0 for a0, _, _ in spans)
    assert spans[-1][1] <= lay["slot_bytes"] and lay["slot_bytes"] % 256 == 0
    assert min(lay[n] for n in ("in_tail", "ola_tail", "ring_re", "ring_im")) == lay["in_tail"] > lay["steps"]  # transform_bytes
    for cap in (1, 20, 4096):
        assert L.fsn_fast_stream_pool_state_bytes(ctypes.byref(c), cfg.la, cap) == cap * lay["slot_bytes"]
    w11, w18, w81 = (L.fsn_fast_stream_pool_workspace_bytes(ctypes.byref(c), n, k) for n, k in ((1, 1), (1, 8), (17, 1)))
    assert 0 < L.fsn_fast_stream_workspace_bytes(ctypes.byref(c), 1, 1) < w11 < w18 and w11 < w81


def _step(L, c, la=2, cap=20, n=1, n_long=1, k=2, state_bytes=1 << 40, ws_bytes=1 << 40):
    """The step with pointers that are never read: every refusal comes before a launch."""
    return L.fsn_fast_stream_pool_step(c, la, 1, 1, state_bytes, cap, 1, n, n_long, 1, k, 1, 1, ws_bytes, None)


@pytest.mark.parametrize("kw,text", [(dict(norm=0), b"causal norm"), (dict(shrink=0), b"shrink"), (dict(F=161), b"257"), (dict(num_mels=80), b"64"),
                                     (dict(mel_neighbors=8), b"neighbours"), (dict(bn_hidden=192), b"bottleneck"), (dict(bn_layers=3), b"bottleneck")])
def test_configurations_the_lockstep_entry_refuses_are_refused(kw, text):
    from fullsubnet_amd import _lib
    L = _lib.lib()
    c = ctypes.byref(P.c_cfg(**kw))
    assert L.fsn_fast_stream_pool_state_bytes(c, 2, 20) == 0 and text in L.fsn_last_error()
    assert L.fsn_fast_stream_pool_workspace_bytes(c, 1, 1) == 0 and text in L.fsn_last_error()
    assert L.fsn_debug_fast_stream_pool_layout(c, 2, (ctypes.c_long * 28)(), 28) == -1
    assert _step(L, c) == -1 and text in L.fsn_last_error()
    assert L.fsn_fast_stream_pool_reset(c, 2, 1, 1 << 40, 20, 1, 1, None) == -1 and text in L.fsn_last_error()
    assert L.fsn_fast_stream_pool_analysis(c, 2, 1, 1 << 40, 20, 1, 1, 1, None, 1, 512, 256, 1, 1, None) == -1
    assert L.fsn_fast_stream_pool_synthesis(c, 2, 1, 1 << 40, 20, 1, 1, 1, 1, 1, 1, 512, 256, 1, 1, 1, 1 << 40, None) == -1


def test_ranges_are_refused():
    from fullsubnet_amd import _lib
    L = _lib.lib()
    c = ctypes.byref(P.c_cfg())
    for cap in (0, -1, 4097):
        assert L.fsn_fast_stream_pool_state_bytes(c, 2, cap) == 0 and b"capacity" in L.fsn_last_error()
        assert _step(L, c, cap=cap) == -1 and b"capacity" in L.fsn_last_error()
    for la in (-1, 65):
        assert L.fsn_fast_stream_pool_state_bytes(c, la, 20) == 0 and b"look_ahead" in L.fsn_last_error()
        assert _step(L, c, la=la) == -1 and b"look_ahead" in L.fsn_last_error()
        assert L.fsn_debug_fast_stream_pool_layout(c, la, (ctypes.c_long * 28)(), 28) == -1
    assert L.fsn_fast_stream_pool_state_bytes(c, 0, 1) > 0 and L.fsn_fast_stream_pool_state_bytes(c, 64, 4096) > 0
    for n in (0, -1, 21):
        assert _step(L, c, n=n, n_long=0) == -1 and b"slots listed" in L.fsn_last_error()
    for n, k in ((0, 1), (4097, 1), (1, 0), (1, 4097)):
        assert L.fsn_fast_stream_pool_workspace_bytes(c, n, k) == 0 and b"out of range" in L.fsn_last_error()
    assert _step(L, c, k=0) == -1 and _step(L, c, k=4097) == -1
    for n_long in (-1, 4):
        assert _step(L, c, n=3, n_long=n_long, k=1) == -1 and b"n_long" in L.fsn_last_error()
    assert _step(L, c, n=3, n_long=2, k=4) == -1 and b"n_long must be n" in L.fsn_last_error()  # shrink 2 divides k = 4
    assert L.fsn_debug_fast_stream_pool_layout(c, 2, (ctypes.c_long * 28)(), 27) == -1
    assert L.fsn_debug_fast_stream_pool_layout(c, 2, None, 28) == -1
    # buffers too small: FSN_ERR_WORKSPACE, still before any launch
    sb = L.fsn_fast_stream_pool_state_bytes(c, 2, 20)
    assert _step(L, c, state_bytes=sb - 1) == -2 and b"too small" in L.fsn_last_error()
    assert _step(L, c, state_bytes=sb, ws_bytes=L.fsn_fast_stream_pool_workspace_bytes(c, 1, 2) - 1) == -2
    assert L.fsn_fast_stream_pool_reset(c, 2, 1, sb - 1, 20, 1, 1, None) == -2
    assert L.fsn_fast_stream_pool_analysis(c, 2, 1, sb, 20, 1, 1, 1, None, 1, 400, 200, 1, 1, None) == -1 and b"512" in L.fsn_last_error()
    assert L.fsn_fast_stream_pool_synthesis(c, 2, 1, sb, 20, 1, 1, 1, 1, 1, 1, 512, 256, 1, 1, 1, 511, None) == -2
