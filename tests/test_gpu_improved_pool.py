"""fsn_improved_stream_pool_* and StreamPool(improved_model) on the device: the step over every slot list of
tests/improved_pool_reference.py against each session's own fp64 step, a schedule of sessions that join and leave, the step
beside the lockstep entry, the frame transforms at 64 / 32 and 960 / 480 against the oracle's STFT and masked iSTFT, the pool
end to end against the whole-utterance model, and the refusals.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import improved_pool_reference as P
import improved_stream_reference as R
from oracle import fullsubnet_oracle as O
from test_gpu_improved_stream import model_of, run_stream, uneven_sizes, write_state
from test_gpu_transform_sweep import Guarded, check_istft, istft_bound, window_of

pytestmark = pytest.mark.gpu
CAUSAL = dict(norm_type="cumulative_laplace_norm", sb_norm_type="cumulative_laplace_norm")


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()  # raises if libfsn_hip.so is missing: no fallback
    return fullsubnet_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pool_call(fsn, model, blob, cap, slots, mags, k):
    """fsn_improved_stream_pool_step on `blob` (updated in place): mags [n, 1, F, k] -> mask [n, 2, F, k] (numpy).  The mask
    starts as NaN and the workspace as 0xFF: nothing of either may be read before the call wrote it."""
    L, lib = fsn._lib.lib(), fsn._lib
    cfg = model.stream_cfg()
    c = ctypes.byref(cfg)
    n = len(slots)
    sd = torch.tensor(slots, dtype=torch.int32, device="cuda")
    x = dev(np.asarray(mags, dtype=np.float32))
    assert tuple(x.shape) == (n, 1, cfg.F, k)
    mask = torch.full((n, 2, cfg.F, k), float("nan"), dtype=torch.float32, device="cuda")
    ws = lib.workspace(L.fsn_improved_stream_pool_workspace_bytes(c, n, k), sd.device)
    ws.fill_(0xFF)
    lib.check(L.fsn_improved_stream_pool_step(c, model.stream_packed_weights().data_ptr(), blob.data_ptr(), blob.numel(), cap,
                                              sd.data_ptr(), n, lib.dev_ptr(x, "mag"), k, lib.dev_ptr(mask), ws.data_ptr(), ws.numel(),
                                              lib.stream_ptr(sd.device)))
    torch.cuda.synchronize()
    return mask.cpu().numpy()


def start_blob(fsn, model, cfg, cap=P.CAP):
    """(layout, the blob of the reference's start pool with every transform field 0xFF)."""
    lay = fsn._lib.improved_stream_pool_layout(model.stream_cfg())
    host = P.records_to_blob(lay, cfg, P.start_pool(cfg, cap), cap)
    for i in range(cap):
        P.transform_bytes(lay, host, i)[...] = 0xFF
    return lay, host


# ---- 1. the sweep -------------------------------------------------------------------------------------------------------------

SWEEP = [(R.SMALL, name, k) for name in P.LISTS for k in P.KS] + [(R.K48, "three", 1), (R.TWO_SECTIONS, "odd", 1)]


@pytest.mark.parametrize("cfg,name,k", SWEEP, ids=[f"F{c.F}-{len(c.centers)}sec-{n}-k{k}" for c, n, k in SWEEP])
def test_pool_step_sweep(fsn, cfg, name, k):
    """Every list x k on a blob of CAP records written from the reference's start pool, by check_call: masks and listed
    records against each session's own fp64 step, unlisted records bit-identical, counts advanced by k, rows of outside ids
    finite; no transform field of any record is touched."""
    model = model_of(cfg, **CAUSAL)
    lay, host = start_blob(fsn, model, cfg)
    blob = dev(host)
    slots = P.LISTS[name]
    mask = pool_call(fsn, model, blob, P.CAP, slots, P.call_mags(cfg, slots, k), k)
    got = blob.cpu().numpy()
    worst = P.check_call(f"F{cfg.F}-{name}-k{k}", cfg, slots, k, mask, P.start_pool(cfg), P.blob_to_records(lay, cfg, got, P.CAP))
    for i in range(P.CAP):
        assert (P.transform_bytes(lay, got, i) == 0xFF).all(), f"slot {i}: a transform field was written by the step"
    print(f"[ipool] F{cfg.F} {name} k{k}: mask worst (frob, max, tile) = ({worst[0]:.2f}, {worst[1]:.2f}, {worst[2]:.2f}) x")


# ---- 2. a sequence ------------------------------------------------------------------------------------------------------------

TICKS = 21
JOIN = {"a": (0, 0), "b": (1, 1), "c": (2, 2), "d": (5, 3), "e": (12, 1)}  # session: (first tick, slot); e takes b's slot
LEAVE = {"b": 9}                                                           # b's last tick is 8; its slot is reset at tick 9


def _schedule():
    """[(tick, [sessions in the call's row order])]: the open sessions, rotated by the tick so that the row order changes."""
    out = []
    for t in range(TICKS):
        live = [s for s, (t0, _) in JOIN.items() if t0 <= t < LEAVE.get(s, TICKS)]
        r = t % len(live)
        out.append((t, live[r:] + live[:r]))
    return out


def _play(fsn, model, cfg, mags):
    """The schedule on a fresh blob of 4 records -> ({session: [mask per call]}, the blob)."""
    L, lib = fsn._lib.lib(), fsn._lib
    c = model.stream_cfg()
    blob = torch.zeros(L.fsn_improved_stream_pool_state_bytes(ctypes.byref(c), 4), dtype=torch.uint8, device="cuda")
    done = {s: 0 for s in JOIN}
    masks = {s: [] for s in JOIN}
    for t, live in _schedule():
        for s, t_end in LEAVE.items():
            if t == t_end:
                sd = torch.tensor([JOIN[s][1]], dtype=torch.int32, device="cuda")
                lib.check(L.fsn_improved_stream_pool_reset(ctypes.byref(c), blob.data_ptr(), blob.numel(), 4, sd.data_ptr(), 1,
                                                           lib.stream_ptr(sd.device)))
        x = np.stack([mags[s][:, :, done[s]:done[s] + 1] for s in live])
        m = pool_call(fsn, model, blob, 4, [JOIN[s][1] for s in live], x, 1)
        for row, s in enumerate(live):
            masks[s].append(m[row:row + 1])
            done[s] += 1
    return masks, blob


def test_sessions_join_leave_and_are_reset(fsn):
    """A pool of 4: sessions join at ticks 0, 1, 2 and 5, one leaves and its slot is reset at tick 9 (and taken again at tick
    12); 21 ticks of k = 1.  Each session's masks call by call, and the open ones' records, against their own fp64 run; the
    same schedule replayed on a fresh blob gives the same blob and masks bit for bit."""
    cfg = R.SMALL
    model = model_of(cfg, **CAUSAL)
    lay = fsn._lib.improved_stream_pool_layout(model.stream_cfg())
    frames = {s: sum(1 for _, live in _schedule() if s in live) for s in JOIN}
    assert frames == {"a": 21, "b": 8, "c": 19, "d": 16, "e": 9}
    mags = {s: R.make_mag(1, cfg.F, frames[s], seed=40 + i) for i, s in enumerate(JOIN)}
    masks, blob = _play(fsn, model, cfg, mags)
    records = P.blob_to_records(lay, cfg, blob.cpu().numpy(), 4)
    for s in JOIN:
        ref = P.Ref()
        ref.mask, ref.state, ref.state0 = {}, {}, R.new_state(1, cfg)
        for m, dtype, act in P.MODES:
            ref.mask[m], ref.state[m] = R.run_chunked(mags[s], P.params_of(cfg), cfg, (1,) * frames[s], dtype, act)
        row = P.Row(f"session-{s}", cfg, frames[s])
        worst = R.check_calls(row, ref, masks[s])
        if s not in LEAVE:  # still open: its record is the state after its last call, its count the frames it has had
            R.check_state(row, ref, records[JOIN[s][1]])
        print(f"[ipool] session {s}: {frames[s]} calls, mask worst (frob, max, tile) = ({worst[0]:.2f}, {worst[1]:.2f}, {worst[2]:.2f}) x")
    masks_b, blob_b = _play(fsn, model, cfg, mags)
    assert torch.equal(blob, blob_b)
    assert all(a.tobytes() == b.tobytes() for s in JOIN for a, b in zip(masks[s], masks_b[s]))


# ---- 3. beside the lockstep entry ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k", [("three", 2), ("seventeen", 1)])
def test_pool_rows_beside_the_lockstep_entry(fsn, name, k):
    """Each listed slot beside fsn_improved_stream_step at B = 1 from the same state and count: the Frobenius difference
    within 2 x SHARP x the yardstick (both are within SHARP x of the fp64 step; the recurrent kernels are chosen by the row
    count, so the bits may differ).  Bit equality is counted and printed, not required."""
    L, lib = fsn._lib.lib(), fsn._lib
    cfg = R.SMALL
    model = model_of(cfg, **CAUSAL)
    c = model.stream_cfg()
    lay, host = start_blob(fsn, model, cfg)
    slots = P.LISTS[name]
    mags = P.call_mags(cfg, slots, k)
    mask = pool_call(fsn, model, dev(host), P.CAP, slots, mags, k)
    lay1 = lib.improved_stream_state_layout(c, 1)
    equal = total = 0
    for row, i in enumerate(slots):
        if not 0 <= i < P.CAP:
            continue
        st = P.start_state(cfg, i)
        blob = write_state(lay1, cfg, 1, st, torch.device("cuda"))
        x = dev(mags[row])
        lock = torch.full((1, 2, cfg.F, k), float("nan"), dtype=torch.float32, device="cuda")
        ws = lib.workspace(L.fsn_improved_stream_workspace_bytes(ctypes.byref(c), 1, k), x.device)
        lib.check(L.fsn_improved_stream_step(ctypes.byref(c), model.stream_packed_weights().data_ptr(), blob.data_ptr(), blob.numel(),
                                             st["steps"], lib.dev_ptr(x, "mag"), 1, k, lib.dev_ptr(lock), ws.data_ptr(), ws.numel(),
                                             lib.stream_ptr(x.device)))
        torch.cuda.synchronize()
        lock = lock.cpu().numpy()
        ref = P.slot_reference(cfg, i, k)
        yard = R.frob(ref["c32"][0].astype(np.float64), ref["64"][0])
        diff = R.frob(mask[row:row + 1].astype(np.float64), lock.astype(np.float64))
        assert diff <= 2 * R.SHARP * yard, f"{name} slot {i}: {diff:.3e} from the lockstep entry, the yardstick is {yard:.3e}"
        equal += int(mask[row:row + 1].tobytes() == lock.tobytes())
        total += 1
    print(f"[ipool] {name} k{k}: {equal} of {total} rows bit-equal to fsn_improved_stream_step at B = 1")


# ---- 4. the transforms --------------------------------------------------------------------------------------------------------

POOL_T = 5  # frames 0 .. 4 of every session
# 62 = 2 x 31 does not split: the transforms take the direct form (64 = 8 x 8 and 960 = 30 x 32 take the two-level one)
DIRECT = R.SMALL._replace(F=32, centers=(1, 2, 3))


def _pool_run(fsn, pool, slots, utts, masks, tails):
    """Every session frame by frame as StreamPool does: analysis of frame t, then synthesis of the same frame, the last one
    with tail_samples.  -> mags [n, F, T], outs: [n, 2 hop] per frame."""
    lib = fsn._lib
    n, N, hop = len(slots), pool.n_fft, pool.hop
    F = hop + 1
    args = pool._state_args()
    sd = torch.tensor(slots, dtype=torch.int32, device="cuda")
    win = dev(window_of(N))
    mags, outs = [], []
    for t in range(POOL_T):
        hops = np.stack([np.pad(u, (0, hop), mode="reflect")[hop * t: hop * (t + 1)] if t == POOL_T - 1 else u[hop * t: hop * (t + 1)]
                         for u in utts]).astype(np.float32)
        prime = dev(np.stack([u[1:hop + 1] for u in utts])) if t == 0 else None
        fno = torch.full((n,), t, dtype=torch.int32, device="cuda")
        g = Guarded((n, F))
        lib.check(lib.lib().fsn_improved_stream_pool_analysis(*args, sd.data_ptr(), n, lib.dev_ptr(dev(hops)),
                                                              lib.dev_ptr(prime, "prime", allow_none=True), fno.data_ptr(), N, hop,
                                                              lib.dev_ptr(win), lib.dev_ptr(g.t), lib.stream_ptr(sd.device)))
        mags.append(g.numpy(f"pool analysis frame {t}"))
        m = dev(np.stack([x[:, :, t:t + 1] for x in masks]))
        tl = torch.tensor(tails if t == POOL_T - 1 else [-1] * n, dtype=torch.int32, device="cuda")
        go = Guarded((n, 2 * hop))
        lib.check(lib.lib().fsn_improved_stream_pool_synthesis(*args, sd.data_ptr(), n, lib.dev_ptr(m), tl.data_ptr(), N, hop,
                                                               lib.dev_ptr(win), lib.dev_ptr(go.t), lib.stream_ptr(sd.device)))
        outs.append(go.numpy(f"pool synthesis frame {t}"))
    return np.stack(mags, axis=-1), outs


@pytest.mark.parametrize("case", ["odd-count", "partner-outside-the-pool"])
@pytest.mark.parametrize("cfg", [R.SMALL, R.K48, DIRECT], ids=["64-32", "960-480", "62-31"])
def test_pool_transforms(fsn, cfg, case):
    """fsn_improved_stream_pool_analysis / _synthesis hop by hop against the oracle's STFT and the fp64 iSTFT of mask[0] re,
    mask[1] im of the whole utterance, in both forms of the transform: n = 3, frame 0 from `prime`, every kind of tail_samples; a slot id outside the pool
    yields zero rows and touches no record; idle records stay as they were; two runs give the same bits."""
    hop = cfg.F - 1
    N = 2 * hop
    slots, tails = {"odd-count": ([2, 0, 3], [0, 1, hop - 1]), "partner-outside-the-pool": ([2, 9, 0], [hop, 5, 1])}[case]
    win = window_of(N)
    capacity = 4
    pool = fsn.StreamPool(model_of(cfg, **CAUSAL), capacity=capacity)
    assert (pool.n_fft, pool.hop) == (N, hop)
    n = len(slots)
    utts = [O.make_noisy(1, hop * (POOL_T - 1) + hop * 100 // 256 + 3 * i, seed=90 + i)[0] for i in range(n)]
    rng = np.random.default_rng(20)
    masks = [rng.standard_normal((2, cfg.F, POOL_T)).astype(np.float32) for _ in range(n)]
    live = [0 <= s < capacity for s in slots]
    idle = [s for s in range(capacity) if s not in slots]
    sb = pool.slot_bytes
    runs = []
    for _ in range(2):
        pool.state.fill_(0xFF)  # every record NaN: the idle ones must stay so, the listed ones are reset
        pool.reset_slots([s for s in slots if 0 <= s < capacity])
        runs.append(_pool_run(fsn, pool, slots, utts, masks, tails))
        for s in idle:
            assert bool((pool.state[s * sb:(s + 1) * sb] == 0xFF).all()), f"record of idle slot {s} was written"
    (mags, outs), (mags2, outs2) = runs
    assert mags.tobytes() == mags2.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(outs, outs2)), "two runs differ"
    for i in range(n):
        if not live[i]:
            assert not mags[i].any() and not any(o[i].any() for o in outs), "a skipped row must be zeros"
            continue
        omag, _, ore, oim = O.stft(utts[i][None], N, hop, N, window=win)
        assert omag.shape[-1] == POOL_T
        mb = 4.0 * float(np.spacing(np.float32(omag.max())))
        mu = float(np.abs(mags[i].astype(np.float64) - omag[0]).max()) / mb
        assert mu <= 1.0, f"session {i}: mag off by {mu:.3g} x (4 ULP of the largest magnitude)"
        er = masks[i][None, 0].astype(np.float64) * ore.astype(np.float64)
        ei = masks[i][None, 1].astype(np.float64) * oim.astype(np.float64)
        tail = max(tails[i], 0)
        n_out = hop * (POOL_T - 1) + tail
        ref = O.istft(er, ei, N, hop, N, length=n_out, window=win, dtype=np.float64)
        assert not outs[0][i].any(), f"session {i}: frame 0 emits nothing"
        for t in range(POOL_T - 1):
            assert not outs[t][i, hop:].any(), "tail column of a frame without tail_samples"
        got = np.concatenate([outs[t][i, :hop] for t in range(1, POOL_T)] + [outs[-1][i, hop:hop + tail]])[None]
        assert not outs[-1][i, hop + tail:].any(), "past tail_samples"
        bound, complete = istft_bound(er, ei, N, hop, win, n_out, ref)
        rc, rd = check_istft(got, ref, bound, complete, f"session {i} tail {tails[i]}")
        print(f"\n[ipool] {N}/{hop} session {i} (slot {slots[i]}, tail {tails[i]}): mag {mu:.2f} of 4 ULP, out {rc:.3f} of 2e-6 max|ref|, "
              f"{rd:.3f} of the derived bound", end="")


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------

def _serve(fsn, model, utts, joins, top, **kw):
    """Sessions that join at round joins[i], push uneven chunks round by round and close when their samples are through (the
    shortest one early, while the others go on): drain() after every round, close() at the end -> [samples per session]."""
    pool = fsn.StreamPool(model, capacity=4, **kw)
    n = len(utts)
    sizes = [uneven_sizes(len(u), 5 + i, top) for i, u in enumerate(utts)]
    pos, sid, out, done = [0] * n, [None] * n, [[] for _ in range(n)], [False] * n
    r = 0
    while not all(done):
        for i in range(n):
            if r < joins[i] or done[i]:
                continue
            if sid[i] is None:
                sid[i] = pool.open()
            if sizes[i]:
                m = sizes[i].pop(0)
                pool.push(sid[i], utts[i][pos[i]:pos[i] + m])
                pos[i] += m
        for s, y in pool.drain().items():
            out[sid.index(s)].append(y)
        for i in range(n):
            if sid[i] is not None and not done[i] and not sizes[i]:
                out[i].append(pool.close(sid[i]))
                done[i] = True
        r += 1
    assert not pool.book.sids()
    return [torch.cat(o) for o in out]


def _offline(model, y):
    with torch.no_grad():
        return model(y[None])[:, 0][0]


def test_stream_pool_end_to_end_small(fsn):
    """Three sessions of 5003 / 3000 / 700 samples at 64 / 32, pushed in uneven chunks, joining at different rounds, the
    shortest closing early: drain + close of each = model(y) of its utterance within 1e-4 of its peak (the bound of
    test_streaming_enhancer_equals_the_whole_utterance_at_48k), exactly L samples; the same schedule with poison_buffers gives
    the same bits; a session alone against StreamingEnhancer is printed."""
    model = model_of(R.SMALL, **CAUSAL)
    utts = [torch.from_numpy(O.make_noisy(1, L, seed=60 + i)[0]).cuda() for i, L in enumerate((5003, 3000, 700))]
    joins = (0, 3, 7)
    outs = _serve(fsn, model, utts, joins, 40)
    for i, (u, y) in enumerate(zip(utts, outs)):
        assert y.shape == u.shape and torch.isfinite(y).all()
        off = _offline(model, u)
        scale, err = off.abs().max().item(), (y - off).abs().max().item()
        print(f"[ipool] 64/32 session {i} ({u.numel()} samples): pool against the whole utterance {err:.3e}, peak {scale:.3e} ({err / scale:.2e} of it)")
        assert scale > 0 and err <= 1e-4 * scale
    poisoned = _serve(fsn, model, utts, joins, 40, poison_buffers=True)
    assert all(torch.equal(a, b) for a, b in zip(outs, poisoned))
    alone = _serve(fsn, model, utts[2:], (0,), 40)[0]
    enh, _, _ = run_stream(model, utts[2][None], uneven_sizes(700, 5, 40))
    print(f"[ipool] 64/32 session 2 alone: {(alone - outs[2]).abs().max().item():.3e} from its run among the others, "
          f"{(alone - enh[0]).abs().max().item():.3e} from StreamingEnhancer")
    assert alone.shape == enh[0].shape


def test_stream_pool_end_to_end_at_48k(fsn):
    """One session of 9611 samples through the shipped 48 kHz configuration (960 / 480), held the same way."""
    model = model_of(R.K48, **CAUSAL)
    u = torch.from_numpy(O.make_noisy(1, 9611, seed=17)[0]).cuda()
    y = _serve(fsn, model, [u], (0,), 900)[0]
    assert y.shape == u.shape and torch.isfinite(y).all()
    off = _offline(model, u)
    scale, err = off.abs().max().item(), (y - off).abs().max().item()
    print(f"[ipool] 48 kHz: pool against the whole utterance {err:.3e}, peak {scale:.3e} ({err / scale:.2e} of it)")
    assert scale > 0 and err <= 1e-4 * scale
    assert torch.equal(y, _serve(fsn, model, [u], (0,), 900, poison_buffers=True)[0])


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals(fsn):
    from fullsubnet_amd.improved_fullsubnet import Model
    from oracle import model_family_oracle as MF
    with pytest.raises(ValueError, match="norm_type = 'cumulative_laplace_norm'"):
        fsn.StreamPool(model_of(R.SMALL))
    with pytest.raises(ValueError, match="sb_norm_type = 'cumulative_laplace_norm'"):
        fsn.StreamPool(model_of(R.SMALL, norm_type="cumulative_laplace_norm"))
    with pytest.raises(NotImplementedError, match="512 / 128"):
        fsn.StreamPool(Model(**dict(MF.IMPROVED_16K, **CAUSAL)).cuda())
    with pytest.raises(NotImplementedError, match="LSTM"):
        fsn.StreamPool(Model(**dict(R.as_dict(R.SMALL), sequence_model="GRU", **CAUSAL)).cuda())
    with pytest.raises(NotImplementedError, match="capacity"):
        fsn.StreamPool(model_of(R.SMALL, **CAUSAL), capacity=4097)
    with pytest.raises(NotImplementedError, match="input_sr"):
        fsn.StreamPool(model_of(R.SMALL, **CAUSAL), input_sr=16000)
    with pytest.raises(NotImplementedError, match="output_sr"):
        fsn.StreamPool(model_of(R.SMALL, **CAUSAL), output_sr=16000)
    pool = fsn.StreamPool(model_of(R.SMALL, **CAUSAL), capacity=4)
    assert (pool.n_fft, pool.hop, pool.book.hop, pool.book.la) == (64, 32, 32, 0)
    mag = torch.ones((2, 1, R.SMALL.F, 1), device="cuda")
    state0 = pool.state.clone()
    for bad in ([1, 1], [0, 4], [-1, 2]):
        with pytest.raises(ValueError):
            pool.model_step(bad, mag)
    assert torch.equal(pool.state, state0) and pool._steps == [0, 0, 0, 0]


def test_step_refuses_short_buffers_before_anything_is_launched(fsn):
    """A short state or workspace buffer: FSN_ERR_WORKSPACE, the records, the mask and the guard bytes around them untouched."""
    L, lib = fsn._lib.lib(), fsn._lib
    model = model_of(R.SMALL, **CAUSAL)
    c = ctypes.byref(model.stream_cfg())
    cap = 4
    nbytes = L.fsn_improved_stream_pool_state_bytes(c, cap)
    guard = 4096
    buf = torch.full((nbytes + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda")
    blob = buf[guard:guard + nbytes]
    blob.zero_()
    before = buf.clone()
    sd = torch.tensor([1, 3], dtype=torch.int32, device="cuda")
    mag = torch.ones((2, 1, R.SMALL.F, 1), device="cuda")
    mask = Guarded((2, 2, R.SMALL.F, 1))
    wb = L.fsn_improved_stream_pool_workspace_bytes(c, 2, 1)
    ws = torch.full((wb + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda")
    ws0 = ws.clone()
    args = lambda sbytes, wbytes: (c, model.stream_packed_weights().data_ptr(), blob.data_ptr(), sbytes, cap, sd.data_ptr(), 2,  # noqa: E731
                                   lib.dev_ptr(mag), 1, lib.dev_ptr(mask.t), ws[guard:].data_ptr(), wbytes, lib.stream_ptr(sd.device))
    assert L.fsn_improved_stream_pool_step(*args(nbytes - 1, wb)) == -2 and b"too small" in L.fsn_last_error()
    assert L.fsn_improved_stream_pool_step(*args(nbytes, wb - 1)) == -2 and b"too small" in L.fsn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and torch.equal(ws, ws0) and np.isnan(mask.numpy("refused step")).all()  # nothing was launched
    # ... and with both sizes right the same call runs inside its buffers
    assert L.fsn_improved_stream_pool_step(*args(nbytes, wb)) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf[:guard], before[:guard]) and torch.equal(buf[guard + nbytes:], before[guard + nbytes:])
    assert torch.equal(ws[:guard], ws0[:guard]) and torch.equal(ws[guard + wb:], ws0[guard + wb:])
    assert np.isfinite(mask.numpy("step")).all()
