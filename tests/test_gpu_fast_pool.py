"""fsn_fast_stream_pool_* and StreamPool(fast_model): sessions at their own phases of a down-sampling block, each held to the
fp64 per-session step of tests/fast_stream_reference.py by the checkers of tests/fast_pool_reference.py - records written
through the layout hook at counts 0, 1, 2, 5, 100 000 and 100 001, slot lists at the tile edges, k = 1, the close call, a mixed
call and one with s | k; sequences in which the due set changes every tick; the pool beside the lockstep entry; a wrong
n_long; the Python pool end to end against the whole-utterance model.
Needs a real MI355X:  python -m pytest tests -m gpu"""
import ctypes

import numpy as np
import pytest
import torch

import fast_pool_reference as P
import fast_stream_reference as R
from oracle import fullsubnet_oracle as O
from test_gpu_core_sweep import SHARP, frob

pytestmark = pytest.mark.gpu

CFGS = [R.SHIPPED, P.SMALL]
HOP = 256


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()  # raises if libfsn_hip.so is missing: no fallback
    return fullsubnet_amd


_MODELS = {}


def model_of(cfg, norm="cumulative_laplace_norm", cell="LSTM"):
    from fullsubnet_amd.fast_fullsubnet import Model
    key = (cfg, norm, cell)
    if key not in _MODELS:
        m = Model(look_ahead=cfg.la, shrink_size=cfg.shrink, sequence_model=cell, num_mels=R.M, encoder_input_size=R.F,
                  bottleneck_hidden_size=cfg.bn_hidden, bottleneck_num_layers=cfg.bn_layers, noisy_input_num_neighbors=cfg.n_mel,
                  encoder_output_num_neighbors=cfg.n_enc, norm_type=norm)
        if cell == "LSTM":
            m.load_state_dict({k: torch.from_numpy(v) for k, v in R.make_params(cfg).items()}, strict=True)
        _MODELS[key] = m.cuda().eval()
    return _MODELS[key]


# ---- the C entry on a blob --------------------------------------------------------------------------------------------------

class CPool:
    """A blob of `cap` records and the calls on it; every call runs with NaN-filled workspace and output."""

    def __init__(self, fsn, cfg, cap=P.CAP, records=None):
        self.fsn, self.cfg, self.cap, self.model = fsn, cfg, cap, model_of(cfg)
        self.L, self.lib = fsn._lib.lib(), fsn._lib
        self.c = self.model.stream_cfg()
        self.lay = fsn._lib.fast_stream_pool_layout(self.c, cfg.la)
        host = P.records_to_blob(self.lay, cfg, records or {}, cap)
        assert host.size == self.L.fsn_fast_stream_pool_state_bytes(ctypes.byref(self.c), cfg.la, cap)
        self.blob = torch.from_numpy(host).cuda()
        self.dev = self.blob.device

    def step(self, rows, n_long, mags, k):
        n = len(rows)
        mag = torch.from_numpy(np.concatenate(mags)).to(self.dev).contiguous()
        assert tuple(mag.shape) == (n, 1, R.F, k)
        slots = torch.tensor(rows, dtype=torch.int32, device=self.dev)
        crm = torch.full((n, 2, R.F, k), float("nan"), dtype=torch.float32, device=self.dev)
        ws = self.lib.workspace(self.L.fsn_fast_stream_pool_workspace_bytes(ctypes.byref(self.c), n, k), self.dev)
        ws.view(torch.float32).fill_(float("nan"))
        rc = self.L.fsn_fast_stream_pool_step(ctypes.byref(self.c), self.cfg.la, self.model.stream_packed_weights().data_ptr(),
                                              self.blob.data_ptr(), self.blob.numel(), self.cap, slots.data_ptr(), n, n_long,
                                              self.lib.dev_ptr(mag, "mag"), k, self.lib.dev_ptr(crm), ws.data_ptr(), ws.numel(),
                                              self.lib.stream_ptr(self.dev))
        torch.cuda.synchronize()
        return rc, crm

    def reset(self, rows):
        slots = torch.tensor(rows, dtype=torch.int32, device=self.dev)
        self.lib.check(self.L.fsn_fast_stream_pool_reset(ctypes.byref(self.c), self.cfg.la, self.blob.data_ptr(), self.blob.numel(),
                                                         self.cap, slots.data_ptr(), len(rows), self.lib.stream_ptr(self.dev)))

    def records(self):
        return P.blob_to_records(self.lay, self.cfg, self.blob.cpu().numpy(), self.cap)


def mags_of(rows, k):
    return [P.slot_mag(i, k) if 0 <= i < P.CAP else np.ones((1, 1, R.F, k), dtype=np.float32) for i in rows]


def sweep_call(fsn, cfg, what, rows, n_long, k):
    before = P.start_pool(cfg)
    pool = CPool(fsn, cfg, records=before)
    blob0 = pool.blob.cpu().numpy().copy()
    rc, crm = pool.step(rows, n_long, mags_of(rows, k), k)
    assert rc == 0, fsn._lib.lib().fsn_last_error()
    blob1 = pool.blob.cpu().numpy()
    for i in range(P.CAP):  # the transform fields are not the step's
        assert np.array_equal(P.transform_bytes(pool.lay, blob0, i), P.transform_bytes(pool.lay, blob1, i)), i
    sb = pool.lay["slot_bytes"]
    for i in range(P.CAP):  # an unlisted record: every byte
        if i not in rows:
            assert np.array_equal(blob0[i * sb:(i + 1) * sb], blob1[i * sb:(i + 1) * sb]), f"{what}: record {i} is not listed and changed"
    worst = P.check_call(what, cfg, rows, k, crm.cpu().numpy(), before, pool.records())
    print(f"[fpool] {what}: crm worst (frob, max, tile) = ({worst[0]:.2f}, {worst[1]:.2f}, {worst[2]:.2f}) x")
    return pool, crm


SWEEP = [(cfg, name, k) for cfg in CFGS for name in P.LISTS for k in P.ks_of(cfg)]


@pytest.mark.parametrize("cfg,name,k", SWEEP, ids=lambda v: str(v) if not isinstance(v, tuple) else f"s{v.shrink}la{v.la}")
def test_pool_step_sweep(fsn, cfg, name, k):
    """One call on the sweep's pool, by fast_pool_reference.check_call: masks and states against the per-session fp64 step at
    SHARP x the fp32 yardstick's own error, unlisted records bit-identical, every listed count advanced by k, a slot that is
    not due with its bottleneck fields bit-identical, ids outside the pool skipped on either side of n_long."""
    rows, n_long = P.call_rows(cfg, name, k)
    sweep_call(fsn, cfg, f"{name}-s{cfg.shrink}-k{k}", rows, n_long, k)


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_a_call_that_lists_only_slots_that_are_not_due(fsn, cfg):
    """k = 1, n_long = 0: the bottleneck does not run; every listed record's bottleneck (h, c), unit sums and held output are
    bit-identical (check_call), the masks finite from the held output, the other fields moved."""
    rows = P.not_due_list(cfg)
    pool, crm = sweep_call(fsn, cfg, f"not-due-s{cfg.shrink}", rows, 0, 1)
    before, after = P.start_pool(cfg), pool.records()
    for i in rows:
        assert P.bottleneck_untouched(before[i], after[i])
        assert not np.array_equal(before[i]["enc0"][0][0], after[i]["enc0"][0][0]) and after[i]["mel_sum"][0] > before[i]["mel_sum"][0]


# ---- sequences: the due set changes every tick --------------------------------------------------------------------------------

JOIN = {3: 0, 0: 1, 2: 2, 1: 5}  # slot: the tick it joins at
LEAVES = (0, 9)                  # slot 0 leaves before tick 9
TICKS = 21


def run_sequence(fsn, cfg, mags):
    """21 ticks of k = 1 on a fresh pool of 4 -> ({slot: [crm per tick]}, the pool)."""
    from fullsubnet_amd.stream_pool import fast_pool_order
    pool = CPool(fsn, cfg, cap=4)
    counts, got = {}, {s: [] for s in JOIN}
    for t in range(TICKS):
        for s, t_join in JOIN.items():
            if t_join == t:
                counts[s] = 0
        if t == LEAVES[1]:
            del counts[LEAVES[0]]
            pool.reset([LEAVES[0]])
        ids = sorted(counts)
        perm, n_long = fast_pool_order([counts[s] for s in ids], 1, cfg.shrink)
        rows = [ids[j] for j in perm]
        rc, crm = pool.step(rows, n_long, [mags[s][..., counts[s]:counts[s] + 1] for s in rows], 1)
        assert rc == 0
        for r, s in enumerate(rows):
            got[s].append(crm[r:r + 1])
            counts[s] += 1
    return got, pool, counts


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_sequences_hold_each_session_to_its_own_reference(fsn, cfg):
    """Sessions join at ticks 0, 1, 2 and 5 and one leaves at tick 9: each session's masks, call by call, and the states of
    the ones still open against their own fp64 step; the same schedule replayed in a fresh blob repeats itself bit for bit."""
    mags = {s: R.make_mag(1, TICKS, seed=300 + s) for s in JOIN}
    got, pool, counts = run_sequence(fsn, cfg, mags)
    after = pool.records()
    assert not pool.blob.view(4, -1)[LEAVES[0]].any()  # reset after it left, never listed again
    for s, t_join in JOIN.items():
        T = (LEAVES[1] if s == LEAVES[0] else TICKS) - t_join
        assert len(got[s]) == T
        ref, row = P.Ref(), P.Row(f"sequence-s{cfg.shrink}-slot{s}", cfg, T)
        ref.crm, ref.state, ref.state0 = {}, {}, R.new_state(1, cfg)
        for m, dtype, act in P.MODES:
            ref.crm[m], ref.state[m] = R.run_chunked(mags[s][..., :T], P.params_of(cfg), cfg, (1,) * T, dtype, act)
        worst = R.check_calls(row, ref, [g.cpu().numpy() for g in got[s]])
        print(f"[fpool] {row.id}: crm worst (frob, max, tile) = ({worst[0]:.2f}, {worst[1]:.2f}, {worst[2]:.2f}) x")
        if s != LEAVES[0]:
            assert after[s]["steps"] == T == counts[s]
            R.check_state(row, ref, dict(after[s], steps=None))
    again, pool2, _ = run_sequence(fsn, cfg, mags)
    assert torch.equal(pool.blob, pool2.blob)
    for s in JOIN:
        assert all(torch.equal(a, b) for a, b in zip(got[s], again[s])), s


# ---- the pool beside the lockstep entry -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg,name,k", [(R.SHIPPED, "odd", 3), (R.SHIPPED, "seventeen", 1), (P.SMALL, "three-phases", 2)],
                         ids=lambda v: str(v) if not isinstance(v, tuple) else f"s{v.shrink}")
def test_pool_beside_the_lockstep_entry(fsn, cfg, name, k):
    """Each listed slot beside fsn_fast_stream_step at B = 1 from the same state and count.  The recurrent step kernels are
    chosen by the call's row count, so bit equality is not required: the difference is printed and held within the sum of the
    two runs' bounds to the fp64 reference (Frobenius, 2 x SHARP x the yardstick's own error)."""
    from test_gpu_fast_stream import run_calls, write_state
    rows, n_long = P.call_rows(cfg, name, k)
    pool, crm = sweep_call(fsn, cfg, f"beside-{name}-s{cfg.shrink}-k{k}", rows, n_long, k)
    model = model_of(cfg)
    lay1 = fsn._lib.fast_stream_state_layout(model.stream_cfg(), 1)
    equal = 0
    for r, i in enumerate(rows):
        if not 0 <= i < P.CAP:
            continue
        blob = write_state(lay1, cfg, 1, P.start_state(cfg, i), torch.device("cuda"))
        lock, _, _ = run_calls(fsn, model, 1, (k,), P.slot_mag(i, k), blob, P.slot_count(i))
        a, b = crm[r:r + 1].cpu().numpy().astype(np.float64), lock[0].cpu().numpy().astype(np.float64)
        ref = P.slot_reference(cfg, i, k)
        yard = frob(ref["c32"][0].astype(np.float64), ref["64"][0])
        d = frob(a, b)
        equal += int(np.array_equal(a, b))
        print(f"[fpool] {name} k={k} slot {i}: pool against lockstep {d:.3e} (max {np.abs(a - b).max():.3e}), yardstick {yard:.3e}, "
              f"bit-equal {np.array_equal(a, b)}")
        assert d <= 2 * SHARP * yard, (i, d, yard)
    print(f"[fpool] {name} k={k}: {equal} of {sum(0 <= i < P.CAP for i in rows)} rows bit-equal to the lockstep entry")


def test_a_wrong_n_long_poisons_the_masks(fsn):
    """Rows in the right order but n_long one short: the order check raises the call's status word, crm_out is all NaN, the
    call returns FSN_OK (the host does not wait) and the stream's status record is raised until it is cleared."""
    cfg, k = R.SHIPPED, 1
    rows, n_long = P.call_rows(cfg, "three-phases", k)
    assert n_long == 2
    pool = CPool(fsn, cfg, records=P.start_pool(cfg))
    try:
        rc, crm = pool.step(rows, n_long - 1, mags_of(rows, k), k)
        assert rc == 0
        assert torch.isnan(crm).all()
        status, events = fsn._lib.stream_status(raise_on_timeout=False)
        assert status != 0 and events >= 1
    finally:
        fsn._lib.stream_status_clear()
    assert fsn._lib.stream_status(raise_on_timeout=False)[0] == 0
    # the same rows with the right n_long on a fresh copy: served
    rc, crm = CPool(fsn, cfg, records=P.start_pool(cfg)).step(rows, n_long, mags_of(rows, k), k)
    assert rc == 0 and torch.isfinite(crm).all()


# ---- StreamPool(fast_model) -------------------------------------------------------------------------------------------------
# the staggered A / B / C schedule of tests/test_gpu_stream_pool.py (helpers copied from there)

LEN = {"A": 5003, "B": 3000, "C": 700}


def utterances():
    return {name: torch.from_numpy(O.make_noisy(1, L, seed=40 + i)[0]).cuda() for i, (name, L) in enumerate(LEN.items())}


def chunks_of(name):
    L = LEN[name]
    if name == "A":
        return [HOP] * (L // HOP) + [L % HOP]
    if name == "B":
        rng = np.random.default_rng(3)
        sizes = []
        while sum(sizes) < L:
            sizes.append(int(min(rng.integers(1, 900), L - sum(sizes))))
        return sizes
    return [100, 1, 155, 1, 443]


class Feeder:
    def __init__(self, pool, name, y):
        self.pool, self.y, self.sizes, self.pos = pool, y, list(chunks_of(name)), 0
        self.sid = pool.open()
        self.out, self.lat = [], []

    def push(self):
        n = self.sizes.pop(0)
        self.pool.push(self.sid, self.y[self.pos:self.pos + n])
        self.pos += n

    def close(self):
        assert not self.sizes and self.pos == self.y.numel()
        self.out.append(self.pool.close(self.sid))
        return torch.cat(self.out)


def drain(pool, feeders):
    got = pool.drain()
    for f in feeders:
        if f.sid in got:
            f.out.append(got[f.sid])
        f.lat.append(f.pos - sum(o.numel() for o in f.out))  # samples in and not out yet


def run_schedule(fsn, model, utts, poison=False):
    """A opens; B opens after A has pushed 1500 samples and pushes a chunk every third round; A closes while B is
    mid-stream; C opens afterwards, into A's freed slot, and runs beside the rest of B."""
    pool = fsn.StreamPool(model, capacity=4, poison_buffers=poison)
    res, lat = {}, []
    a = Feeder(pool, "A", utts["A"])
    while a.pos < 1500:
        a.push()
        drain(pool, [a])
    b = Feeder(pool, "B", utts["B"])
    assert (pool.slot(a.sid), pool.slot(b.sid)) == (0, 1)
    r = 0
    while a.sizes:
        a.push()
        if r % 3 == 0:
            b.push()
        drain(pool, [a, b])
        r += 1
    assert 0 < b.pos < LEN["B"] and b.sizes  # B is mid-stream
    res["A"] = a.close()
    c = Feeder(pool, "C", utts["C"])
    assert pool.slot(c.sid) == 0  # A's slot
    while c.sizes or b.sizes:
        if c.sizes:
            c.push()
        if b.sizes:
            b.push()
        drain(pool, [b, c])
    res["C"] = c.close()
    res["B"] = b.close()
    assert not pool.book.sids() and not any(pool._steps)
    for f in (a, b, c):
        lat += f.lat
    return res, max(lat)


def run_alone(pool, name, y):
    f = Feeder(pool, name, y)
    while f.sizes:
        f.push()
        drain(pool, [f])
    return f.close()


@pytest.fixture(scope="module")
def schedule(fsn):
    utts = utterances()
    return utts, {cfg: run_schedule(fsn, model_of(cfg), utts) for cfg in CFGS}


@pytest.mark.parametrize("cfg", CFGS, ids=str)
def test_staggered_sessions_equal_the_whole_utterance(fsn, schedule, cfg):
    """Each session's drain() + close() has its utterance's length and is model.enhance of the whole utterance to 1e-4 of its
    peak (the bound of test_streaming_enhancer_equals_the_whole_utterance); no sample leaves later than (look_ahead + 2) hops
    after it came in."""
    utts, runs = schedule
    res, lat = runs[cfg]
    model = model_of(cfg)
    for name in LEN:
        y, got = utts[name], res[name]
        assert got.shape == y.shape and torch.isfinite(got).all()
        offline = model.enhance(y[None])[0]
        scale, err = offline.abs().max().item(), (got - offline).abs().max().item()
        print(f"[fpool] {cfg} {name}: pool against the whole utterance {err:.3e}, peak {scale:.3e} ({err / scale:.2e} of it)")
        assert scale > 0 and err <= 1e-4 * scale
    print(f"[fpool] {cfg}: largest backlog {lat} samples")
    assert lat <= (cfg.la + 2) * HOP


def test_sessions_beside_others_and_poison_proof(fsn, schedule):
    """A beside B and C compared with A alone (printed; the rows batch differently, so the kernels may differ); the schedule
    replayed with every workspace and output NaN-filled is finite and repeats the first run bit for bit."""
    utts, runs = schedule
    cfg = R.SHIPPED
    res, _ = runs[cfg]
    alone = run_alone(fsn.StreamPool(model_of(cfg), capacity=4), "A", utts["A"])
    d = (res["A"] - alone).abs().max().item()
    print(f"[fpool] A in the schedule vs alone: {d:.3e} of {alone.abs().max().item():.3e}")
    assert d <= 1e-4 * alone.abs().max().item()  # both are within that of the whole-utterance result
    again, _ = run_schedule(fsn, model_of(cfg), utts, poison=True)
    for name in LEN:
        assert torch.isfinite(again[name]).all()
        assert torch.equal(again[name], res[name]), name


def test_model_step_sorts_and_returns_rows_in_the_callers_order(fsn):
    """StreamPool.model_step takes the slots in any order: the same call on the C entry, rows compared in the caller's order;
    the host mirror of the counts follows, and reset_slots clears it."""
    cfg, k = R.SHIPPED, 3
    pool = fsn.StreamPool(model_of(cfg), capacity=P.CAP, poison_buffers=True)
    ref = CPool(fsn, cfg, records=P.start_pool(cfg))
    assert pool.state.numel() == ref.blob.numel()
    pool.state.copy_(ref.blob)
    pool._steps = [P.slot_count(i) for i in range(P.CAP)]
    ids = [1, 2, 5, 4, 0, 3]  # counts 1, 2, 100001, 100000, 0, 5: long (even) and short rows interleaved
    perm, n_long = P.order_by_definition([P.slot_count(i) for i in ids], k, cfg.shrink)
    assert 0 < n_long < len(ids) and perm != list(range(len(ids)))
    mag = torch.from_numpy(np.concatenate(mags_of(ids, k))).cuda()
    crm = pool.model_step(ids, mag)
    rc, want = ref.step([ids[j] for j in perm], n_long, [P.slot_mag(ids[j], k) for j in perm], k)
    assert rc == 0 and torch.isfinite(crm).all()
    for r, j in enumerate(perm):
        assert torch.equal(crm[j], want[r]), (r, j)
    assert torch.equal(pool.state, ref.blob)
    assert [pool._steps[i] for i in ids] == [P.slot_count(i) + k for i in ids]
    pool.reset_slots([5, 0])
    assert pool._steps[5] == pool._steps[0] == 0 and pool._steps[1] == 1 + k
    assert not pool.state.view(P.CAP, -1)[5].any()


def test_one_session_at_48_khz(fsn):
    """input_sr = 48000, output_sr = "input": what the model received is resample(x, 48000, 16000) bit for bit and the output
    has out_length(n, 48000, 48000) = n samples."""
    rs = fsn.resample
    n = 13807
    x = torch.from_numpy(O.make_noisy(1, n, seed=50)[0]).cuda()
    pool = fsn.StreamPool(model_of(R.SHIPPED), capacity=2, input_sr=48000, output_sr="input", record_model_rate=True)
    sid, pos, outs = pool.open(), 0, []
    rng = np.random.default_rng(8)
    while pos < n:
        c = int(min(rng.integers(0, 2000), n - pos))
        pool.push(sid, x[pos:pos + c])
        pos += c
        outs.append(pool.drain().get(sid, x[:0]))
    outs.append(pool.close(sid))
    got = torch.cat(outs)
    model_in, _ = pool.recorded(sid)
    assert torch.equal(model_in, rs.resample(x, 48000, 16000)[0])
    assert got.numel() == rs.out_length(n, 48000, 48000) == n and torch.isfinite(got).all()


def test_refusals(fsn):
    with pytest.raises(ValueError, match="causal"):
        fsn.StreamPool(model_of(R.SHIPPED, norm="offline_laplace_norm"))
    with pytest.raises(NotImplementedError, match="LSTM"):
        fsn.StreamPool(model_of(R.SHIPPED, cell="GRU"))
    with pytest.raises(NotImplementedError, match="capacity"):
        fsn.StreamPool(model_of(R.SHIPPED), capacity=4097)
    pool = fsn.StreamPool(model_of(R.SHIPPED), capacity=4)
    mag = torch.ones((2, 1, R.F, 1), device="cuda")
    pool.model_step([0, 1], mag)
    state0, steps0 = pool.state.clone(), list(pool._steps)
    for bad in ([1, 1], [0, 4], [-1, 2]):
        with pytest.raises(ValueError):
            pool.model_step(bad, mag)
    assert torch.equal(pool.state, state0) and pool._steps == steps0 == [1, 1, 0, 0]
