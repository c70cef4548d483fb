"""The model entries that carry state between calls, held to an fp64 step of the model.  Needs an MI355X:
python -m pytest tests/test_gpu_stream_sweep.py -m gpu -s

fsn_fullsubnet_stream_step (the lockstep streaming step), fsn_fullsubnet_stream_pool_step (the same step over a list of pool
slots: gather, scatter, pool_den_fb_kernel, pool_den_sb_kernel of csrc/stream_pool_kernels.hip) and the three passes of
enhance_long (fsn_fullsubnet_segment_stats / _fullband / _divisors / _subband) all go through stream_fullband and
stream_subband of csrc/fsn_api_fullsubnet.hip: fsn_launch_lstm_wavefront2 in its continuation form, gemm_a_fullband and
sb_input_model with per-frame or per-row divisors, the cumulative-norm kernels with a carried fp64 sum and a step offset.
tests/stream_reference.py has the table (one Row per line, named after the edge it is there for), the stateful fp64 step with
its two fp32 yardsticks and the checkers; tests/test_stream_sweep_cpu.py tries all of that on the CPU, wrong stand-ins included.
The entries are called through fullsubnet_amd._lib directly; the opaque states are written and read through
fsn_debug_stream_state_layout / fsn_debug_stream_pool_layout.

Every row runs a sequence of calls on one state.  Held: every call's crm (the segment rows' fb_out too) against the fp64 step
with check_tensor of the core sweep at SHARP = 4 x the fp32 yardstick - whole tensor (Frobenius and max), per frame, per
16-row tile against the yardstick's worst tile - call by call and over all calls; after the last call h and c of the four
layers at SHARP x the cell emulation's own state error (Frobenius, per array; pad rows finite), the step counts exactly, and
the two norm carries by a derived bound: an fp64 sum of positive fp32 terms is within (terms + 2) 2^-53 of the exact sum in
any order (sb_sum, which holds the device's own fb_out, + frames x SHARP x max|fb_t32 - fb64|).  A carry kept in fp32 misses
that by four decades.  Besides, in every row: outputs behind the NaN sentinel with GUARD elements that survive and every
declared element written; workspaces exactly the queried size and filled with 0xFF; the state exactly the queried size with
a guard behind it; the sequence run twice from the same initial state bit-identical; the stream status clean.

Pool rows: all 19 records are written with their own h, c, sums and step counts (slot i at 3 i frames, slot 18 at 100 000; the
transform parts random bytes).  Listed records are held to the fp64 step of their slot and must advance by exactly k; every
byte of every unlisted record, of the listed records' transform parts and of the guard must be unchanged; ids outside
[0, capacity) give finite rows and write nothing.  Every listed slot is also compared, bit for bit, with a lockstep B = 1
call on that slot's numbers.  Segment rows: the offline norm at ragged totals with look-ahead 2; the divisors within one
np.spacing of the fp32 of the exact mean; the cumulative norm through the segment entries bit-equal to the lockstep entry.

Seen on an MI355X, all 25 tests, 7 s: no row above the margin, no state mismatch, no byte written outside a listed record, no
bug found - the candidates by reading (pad rows of the last tile under a carried h at B F % 16 = 1 .. 15, den of skipped rows
in the [k][Npad] layout, masked_sum_accumulate at a row that ends on a segment edge, the step count of a slot listed last in
a permuted list) all hold.  Worst hip / yardstick ratio of the relative Frobenius error (max-error ratio, worst 16-row tile
against the yardstick's worst tile):
lockstep crm - 1.11 - 1.49 x (1.63 x, 1.51 x) from zero states, 1.60 x (3.17 x on its one-frame first call, 1.59 x) resumed at
100 000 frames; h and c <= 1.40 x; fb_sum equal to the exact sum, sb_sum <= 0.34 of its bound.
pool crm - 1.64 - 1.74 x (2.60 x, 1.92 x) on the lists, 1.91 x (3.29 x, 2.61 x) on slot 18 alone at k = 1; h and c <= 1.30 x; sb_sum
<= 0.26 of its bound; steps exactly + 4.
segment crm - 1.29 - 1.47 x (2.12 x, 1.43 x); fb_out against torch's fp32 1.67 - 2.11 x (3.46 x on the one-frame segment (0, 1): 514
elements, the largest of the module; 2.11 x); h and c <= 1.31 x; den_fb and den_sb equal to the fp32 of the exact mean (0.00 ulp).
Bit-equalities, all holding: the sequence twice from one state (every row); six frames one by one against one call of six
(crm and state, max|a - b| = 0); every listed slot of every pool list against the lockstep B = 1 entry at k = 1 and k = 3 (112
slot calls); the cumulative norm through the segment entries against the lockstep entry on 1, 4, 1, 2 frames (crm of every
call and the state).
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import stream_reference as R
from test_gpu_core_sweep import packed_weights
from test_gpu_recurrent_sweep import GUARD, Out

pytestmark = pytest.mark.gpu

HS = 384
PAD_BYTE = 0xA5
ARRAYS = ("h0", "h1", "c0", "c1")


@pytest.fixture(scope="module")
def fsn():
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a ROCm device")
    import fullsubnet_amd
    fullsubnet_amd._lib.lib()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return fullsubnet_amd


# ---- states on the device, through the layout queries --------------------------------------------------------------------

def _arr(buf, off, count, dtype):
    return buf[off:off + count * torch.empty((), dtype=dtype).element_size()].view(dtype)


def _guarded(dev, nbytes):
    buf = torch.full((nbytes + 4 * GUARD,), PAD_BYTE, dtype=torch.uint8, device=dev)
    buf[:nbytes].zero_()
    return buf


def _guard_ok(buf, nbytes, what):
    assert bool((buf[nbytes:] == PAD_BYTE).all()), f"{what}: written behind the state"


def stream_state(lib, row, cfg, st, dev, pad_seed=None):
    """The blob of the row's entry at batch B holding the state `st` of its B rows (R.take_state's layout); pad rows zero, or
    finite random numbers with pad_seed.  Returns (guarded buffer, bytes, layout)."""
    L, c = lib.lib(), ctypes.byref(cfg)
    nbytes = (L.fsn_fullsubnet_segment_state_bytes if row.entry == "segment" else L.fsn_fullsubnet_stream_state_bytes)(c, row.B)
    lay = lib.stream_state_layout(cfg, row.B)
    assert nbytes >= lay["bytes"] > 0
    buf = _guarded(dev, nbytes)
    rng = np.random.default_rng(pad_seed)
    for key, H, npad in (("fb", row.Hf, lay["npad_fb"]), ("sb", HS, lay["npad_sb"])):
        for a, name in enumerate(ARRAYS):
            full = np.zeros((npad, H), dtype=np.float32) if pad_seed is None else rng.uniform(-0.9, 0.9, (npad, H)).astype(np.float32)
            full[:st[key][a].shape[0]] = st[key][a]
            _arr(buf, lay[f"{key}_{name}"], npad * H, torch.float32).copy_(torch.from_numpy(full.reshape(-1)))
    _arr(buf, lay["fb_sum"], row.B, torch.float64).copy_(torch.from_numpy(np.ascontiguousarray(st["fb_sum"])))
    _arr(buf, lay["sb_sum"], row.B * row.F, torch.float64).copy_(torch.from_numpy(np.ascontiguousarray(st["sb_sum"]).reshape(-1)))
    return buf, nbytes, lay


def read_stream_state(row, buf, lay, steps):
    host = buf.cpu()
    st = {"fb": [], "sb": [], "steps": np.full(row.B, steps, dtype=np.int64)}
    for key, H, npad, n in (("fb", row.Hf, lay["npad_fb"], row.B), ("sb", HS, lay["npad_sb"], row.B * row.F)):
        for name in ARRAYS:
            full = _arr(host, lay[f"{key}_{name}"], npad * H, torch.float32).view(npad, H).numpy()
            assert np.isfinite(full[n:]).all(), f"{row.id} state {key}_{name}: pad rows not finite"
            st[key].append(full[:n].copy())
    st["fb_sum"] = _arr(host, lay["fb_sum"], row.B, torch.float64).numpy().copy()
    st["sb_sum"] = _arr(host, lay["sb_sum"], row.B * row.F, torch.float64).view(row.B, row.F).numpy().copy()
    return st


def pool_state(lib, row, cfg, st, dev):
    """A pool of R.CAPACITY records: random bytes, then every slot's own h, c, sums and step count from `st`."""
    L = lib.lib()
    lay = lib.stream_pool_layout(cfg)
    nbytes = L.fsn_fullsubnet_stream_pool_state_bytes(ctypes.byref(cfg), R.CAPACITY)
    assert nbytes == R.CAPACITY * lay["slot_bytes"] > 0
    host = torch.full((nbytes + 4 * GUARD,), PAD_BYTE, dtype=torch.uint8)
    host[:nbytes] = torch.from_numpy(np.random.default_rng(5).integers(0, 256, nbytes, dtype=np.uint8))
    F = row.F
    for s in range(R.CAPACITY):
        rec = host[s * lay["slot_bytes"]:(s + 1) * lay["slot_bytes"]]
        for a, name in enumerate(ARRAYS):
            _arr(rec, lay[f"fb_{name}"], row.Hf, torch.float32).copy_(torch.from_numpy(st["fb"][a][s]))
            _arr(rec, lay[f"sb_{name}"], F * HS, torch.float32).copy_(torch.from_numpy(st["sb"][a][s * F:(s + 1) * F].reshape(-1)))
        _arr(rec, lay["fb_sum"], 1, torch.float64)[0] = float(st["fb_sum"][s])
        _arr(rec, lay["sb_sum"], F, torch.float64).copy_(torch.from_numpy(np.ascontiguousarray(st["sb_sum"][s])))
        _arr(rec, lay["steps"], 1, torch.int32)[0] = int(st["steps"][s])
    return host.to(dev), nbytes, lay


def read_pool_records(row, buf, lay, slots):
    host = buf.cpu()
    F = row.F
    st = {"fb": [[] for _ in ARRAYS], "sb": [[] for _ in ARRAYS], "fb_sum": [], "sb_sum": [], "steps": []}
    for s in slots:
        rec = host[s * lay["slot_bytes"]:(s + 1) * lay["slot_bytes"]]
        for a, name in enumerate(ARRAYS):
            st["fb"][a].append(_arr(rec, lay[f"fb_{name}"], row.Hf, torch.float32).numpy().copy())
            st["sb"][a].append(_arr(rec, lay[f"sb_{name}"], F * HS, torch.float32).view(F, HS).numpy().copy())
        st["fb_sum"].append(float(_arr(rec, lay["fb_sum"], 1, torch.float64)[0]))
        st["sb_sum"].append(_arr(rec, lay["sb_sum"], F, torch.float64).numpy().copy())
        st["steps"].append(int(_arr(rec, lay["steps"], 1, torch.int32)[0]))
    return {"fb": [np.stack(a) for a in st["fb"]], "sb": [np.concatenate(a) for a in st["sb"]], "fb_sum": np.asarray(st["fb_sum"]),
            "sb_sum": np.stack(st["sb_sum"]), "steps": np.asarray(st["steps"], dtype=np.int64)}


# ---- the entries --------------------------------------------------------------------------------------------------------

def _ws(lib, nbytes, dev):
    return lib.workspace(nbytes, dev).fill_(0xFF)


def stream_calls(lib, row, cfg, packed, mags, buf, nbytes, steps0):
    """The row's calls of fsn_fullsubnet_stream_step on the state in buf; returns the crm of every call (on the device)."""
    L, c, dev = lib.lib(), ctypes.byref(cfg), buf.device
    out, done = [], steps0
    for i, mag in enumerate(mags):
        B, k = mag.shape[0], mag.shape[-1]
        ws = _ws(lib, L.fsn_fullsubnet_stream_workspace_bytes(c, B, k), dev)
        o = Out(dev, (B, 2, row.F, k))
        lib.check(L.fsn_fullsubnet_stream_step(c, packed.data_ptr(), buf.data_ptr(), nbytes, done, lib.dev_ptr(mag), B, k, lib.dev_ptr(o.f),
                                               ws.data_ptr(), ws.numel(), lib.stream_ptr(dev)))
        out.append(o.take(f"{row.id} call {i} crm"))
        done += k
    _guard_ok(buf, nbytes, row.id)
    return out


def pool_calls(lib, row, cfg, packed, mags, buf, nbytes):
    L, c, dev = lib.lib(), ctypes.byref(cfg), buf.device
    slots = torch.tensor(row.slots, dtype=torch.int32, device=dev)
    out = []
    for i, mag in enumerate(mags):
        n, k = mag.shape[0], mag.shape[-1]
        ws = _ws(lib, L.fsn_fullsubnet_stream_pool_workspace_bytes(c, n, k), dev)
        o = Out(dev, (n, 2, row.F, k))
        lib.check(L.fsn_fullsubnet_stream_pool_step(c, packed.data_ptr(), buf.data_ptr(), nbytes, R.CAPACITY, slots.data_ptr(), n,
                                                    lib.dev_ptr(mag), k, lib.dev_ptr(o.f), ws.data_ptr(), ws.numel(), lib.stream_ptr(dev)))
        out.append(o.take(f"{row.id} call {i} crm"))
    _guard_ok(buf, nbytes, row.id)
    return out


def segment_calls(lib, row, cfg, packed, mags, buf, nbytes, totals):
    """stats over all segments, fullband over all, the divisors, subband over all (enhance_long's order).  Returns (crm per
    segment, fb_out per segment, den_fb, den_sb)."""
    L, c, dev = lib.lib(), ctypes.byref(cfg), buf.device
    st, sargs, B, F = lib.stream_ptr(dev), (buf.data_ptr(), nbytes), row.B, row.F
    total = torch.tensor(totals, dtype=torch.int32, device=dev)
    flat = [m[:, 0].contiguous() for m in mags]  # [B, F, k]
    for (s0, k), x in zip(row.segments, flat):
        lib.check(L.fsn_fullsubnet_segment_stats(c, *sargs, lib.dev_ptr(x), B, k, st))
    fbs, crms = [], []
    for i, ((s0, k), x) in enumerate(zip(row.segments, flat)):
        ws = _ws(lib, L.fsn_fullsubnet_segment_workspace_bytes(c, B, k), dev)
        o = Out(dev, (B, F, k))
        lib.check(L.fsn_fullsubnet_segment_fullband(c, packed.data_ptr(), *sargs, s0, total.data_ptr(), lib.dev_ptr(x), B, k, lib.dev_ptr(o.f),
                                                    ws.data_ptr(), ws.numel(), st))
        fbs.append(o.take(f"{row.id} call {i} fb_out"))
    den_fb = den_sb = None
    if row.norm == "offline":
        dens = Out(dev, (2, B))
        lib.check(L.fsn_fullsubnet_segment_divisors(c, *sargs, total.data_ptr(), B, lib.dev_ptr(dens.f[:B]), lib.dev_ptr(dens.f[B:2 * B]), st))
        den_fb, den_sb = dens.take(f"{row.id} divisors").cpu().numpy()
    for i, ((s0, k), x, y) in enumerate(zip(row.segments, flat, fbs)):
        ws = _ws(lib, L.fsn_fullsubnet_segment_workspace_bytes(c, B, k), dev)
        o = Out(dev, (B, 2, F, k))
        lib.check(L.fsn_fullsubnet_segment_subband(c, packed.data_ptr(), *sargs, s0, total.data_ptr(), lib.dev_ptr(x), lib.dev_ptr(y), B, k,
                                                   lib.dev_ptr(o.f), ws.data_ptr(), ws.numel(), st))
        crms.append(o.take(f"{row.id} call {i} crm"))
    _guard_ok(buf, nbytes, row.id)
    return crms, fbs, den_fb, den_sb


def _device_mags(row, ref, dev):
    return [torch.from_numpy(np.ascontiguousarray(m[row.sel])).to(dev) for m in ref.mags]


def _twice(row, run):
    """The sequence from the same initial state, twice: (outputs, final state buffer) of the first, bit-equal to the second."""
    try:
        a, b = run(), run()
        torch.cuda.synchronize()
    except RuntimeError as e:  # a launch or the device failed: nothing more may run on it in this session
        pytest.exit(f"{row.id}: the device call failed, stopping the sweep: {e}", returncode=3)
    for x, y in zip(a[0], b[0]):
        assert x is None and y is None or all(torch.equal(p, q) for p, q in zip(x, y)), f"{row.id}: two runs from the same state differ in an output"
    assert torch.equal(a[1], b[1]), f"{row.id}: two runs from the same state leave different states"
    return a


def _line(row, worst, ws, t0, extra=""):
    parts = [f"{what} {r[0]:.2f} x (max {r[1]:.2f} x, tile {r[2]:.2f} x)" for what, r in worst.items()]
    state = max(ws[n] for n in R.STATE_ARRAYS)
    sums = f", fb_sum {ws['fb_sum']:.3f} / sb_sum {ws['sb_sum']:.3f} of the bound" if "fb_sum" in ws else ""
    print(f"[ssweep] {row.id}: {', '.join(parts)}; state worst {state:.2f} x{sums}{extra}; {time.time() - t0:.1f} s")


ROWS = {e: [r for r in R.TABLE if r.entry == e] for e in ("stream", "pool", "segment")}


def _setup(fsn, row):
    lib, dev = fsn._lib, torch.device("cuda:0")
    cfg = row.cfg(lib)
    R.check_duplication(row)
    ref = R.reference_of(row)
    return lib, dev, cfg, ref, packed_weights(lib, row, cfg, ref.params, dev), _device_mags(row, ref, dev)


@pytest.mark.parametrize("row", ROWS["stream"], ids=[r.id for r in ROWS["stream"]])
def test_stream_sweep(fsn, row):
    t0 = time.time()
    lib, dev, cfg, ref, packed, mags = _setup(fsn, row)
    st0 = R.take_state(ref.state0, row.sel, row.F)
    steps0 = int(st0["steps"][0])

    def run():
        buf, nbytes, lay = stream_state(lib, row, cfg, st0, dev, pad_seed=13 if row.resumed else None)
        return (stream_calls(lib, row, cfg, packed, mags, buf, nbytes, steps0),), buf, lay

    (crm,), buf, lay = _twice(row, run)
    assert lib.stream_status(dev) == (0, 0), "the stream carries a timeout record"
    lib.check_canaries()
    worst = R.check_calls(row, ref, [c.cpu().numpy() for c in crm])
    ws = R.check_state(row, ref, read_stream_state(row, buf, lay, steps0 + row.T))
    _line(row, worst, ws, t0)


def test_chunkings_of_the_same_frames(fsn):
    """Rows 1 and 2 of the lockstep table cover the same six frames, one by one and in one call.  Both are held to fp64 by
    test_stream_sweep; here the two are compared with each other."""
    a, b = ROWS["stream"][:2]
    assert (a.split, b.split, a.B, b.B) == ((1,) * 6, (6,), 1, 1)
    outs, states = [], []
    for row in (a, b):
        lib, dev, cfg, ref, packed, mags = _setup(fsn, row)
        buf, nbytes, lay = stream_state(lib, row, cfg, R.take_state(ref.state0, row.sel, row.F), dev)
        outs.append(torch.cat(stream_calls(lib, row, cfg, packed, mags, buf, nbytes, 0), dim=-1))
        states.append(buf[:lay["bytes"]].clone())
    d = (outs[0] - outs[1]).abs().max().item()
    same, same_state = torch.equal(outs[0], outs[1]), torch.equal(states[0], states[1])
    print(f"[ssweep] six frames one by one vs in one call: max|a - b| = {d:.3e} of {outs[1].abs().max().item():.3e}, crm bit-equal: {same}, "
          f"state bit-equal: {same_state}")
    assert same and same_state  # seen to hold on the MI355X: a frame's arithmetic does not depend on the call it arrives in


_LOCKSTEP = {}


def lockstep_of_slot(lib, row, cfg, packed, ref, slot, dev):
    """The lockstep B = 1 entry on the slot's numbers: crm of the k = 1 and the k = 3 call (cached: it does not depend on the list)."""
    if slot not in _LOCKSTEP:
        one = R.Row("slot", "stream", 1, row.split, F=row.F, Hf=row.Hf, nb=row.nb)
        st0 = R.take_state(ref.state0, np.asarray([slot]), row.F)
        buf, nbytes, _ = stream_state(lib, one, cfg, st0, dev)
        mags = [torch.from_numpy(np.ascontiguousarray(m[slot:slot + 1])).to(dev) for m in ref.mags]
        _LOCKSTEP[slot] = stream_calls(lib, one, cfg, packed, mags, buf, nbytes, int(st0["steps"][0]))
    return _LOCKSTEP[slot]


@pytest.mark.parametrize("row", ROWS["pool"], ids=[r.id for r in ROWS["pool"]])
def test_pool_sweep(fsn, row):
    t0 = time.time()
    lib, dev, cfg, ref, packed, mags = _setup(fsn, row)
    listed = [row.slots[i] for i in row.held]
    buf0, nbytes, lay = pool_state(lib, row, cfg, ref.state0, dev)

    def run():
        buf = buf0.clone()
        return (pool_calls(lib, row, cfg, packed, mags, buf, nbytes),), buf

    (crm,), buf = _twice(row, run)
    assert lib.stream_status(dev) == (0, 0), "the stream carries a timeout record"
    lib.check_canaries()
    # nothing but the listed records' model parts may change
    before, after = buf0[:nbytes].view(R.CAPACITY, -1), buf[:nbytes].view(R.CAPACITY, -1)
    for s in range(R.CAPACITY):
        if s in listed:
            assert torch.equal(before[s, lay["in_tail"]:], after[s, lay["in_tail"]:]), f"{row.id}: the transform part of record {s} was written"
        else:
            assert torch.equal(before[s], after[s]), f"{row.id}: record {s} is not listed and was written"
    worst = R.check_calls(row, ref, [c.cpu().numpy() for c in crm])
    got = read_pool_records(row, buf, lay, listed)
    assert got["steps"].tolist() == [int(ref.state0["steps"][s]) + row.T for s in listed], f"{row.id}: the listed slots' step counts did not advance by {row.T}"
    ws = R.check_state(row, ref, got)
    # the pool against the lockstep entry on each listed slot's numbers, bit for bit
    equal = 0
    for i in row.held:
        want = lockstep_of_slot(lib, row, cfg, packed, ref, row.slots[i], dev)
        for c, (p, q) in enumerate(zip(crm, want)):
            d = (p[i:i + 1] - q).abs().max().item()
            assert torch.equal(p[i:i + 1], q), f"{row.id} call {c}: slot {row.slots[i]} differs from the lockstep entry by {d:.3e}"
            equal += 1
    _line(row, worst, ws, t0, extra=f"; {equal} slot calls bit-equal to the lockstep entry")


@pytest.mark.parametrize("row", ROWS["segment"], ids=[r.id for r in ROWS["segment"]])
def test_segment_sweep(fsn, row):
    t0 = time.time()
    lib, dev, cfg, ref, packed, mags = _setup(fsn, row)
    st0 = R.take_state(ref.state0, row.sel, row.F)
    totals = [int(n) for n in row.totals]

    def run():
        buf, nbytes, lay = stream_state(lib, row, cfg, st0, dev)
        crm, fb, den_fb, den_sb = segment_calls(lib, row, cfg, packed, mags, buf, nbytes, totals)
        return (crm, fb), buf, lay, den_fb, den_sb

    (crm, fb), buf, lay, den_fb, den_sb = _twice(row, run)
    assert lib.stream_status(dev) == (0, 0), "the stream carries a timeout record"
    lib.check_canaries()
    extra = ""
    if row.norm == "cumulative":  # the same launches as the lockstep entry: the same bits
        twin = next(r for r in ROWS["stream"] if (r.B, r.split, r.F, r.Hf, r.nb, r.resumed) == (row.B, row.split, row.F, row.Hf, row.nb, False))
        sbuf, sbytes, slay = stream_state(lib, twin, cfg, st0, dev)
        want = stream_calls(lib, twin, cfg, packed, mags, sbuf, sbytes, 0)
        same = [torch.equal(p, q) for p, q in zip(crm, want)]
        same_state = torch.equal(buf[:slay["bytes"]], sbuf[:slay["bytes"]])
        d = max((p - q).abs().max().item() for p, q in zip(crm, want))
        extra = f"; segment entries vs the lockstep entry: max|a - b| = {d:.3e}, crm bit-equal per call {same}, state bit-equal {same_state}"
        assert all(same) and same_state, f"{row.id}: the segment entries differ from the lockstep entry{extra}"
    worst = R.check_calls(row, ref, [c.cpu().numpy() for c in crm], [f.cpu().numpy() for f in fb])
    ws = R.check_state(row, ref, read_stream_state(row, buf, lay, row.T))
    if row.norm == "offline":
        ulp = R.check_divisors(row, ref, den_fb, den_sb, torch.cat(fb, dim=-1).cpu().numpy())
        extra = f"; divisors within {ulp:.2f} ulp"
    _line(row, worst, ws, t0, extra=extra)
