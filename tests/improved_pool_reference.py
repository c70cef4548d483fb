"""The reference, the slot lists and the checkers of tests/test_gpu_improved_pool.py; importable without a device
(tests/test_improved_pool_cpu.py runs all of it on the CPU).

The pool's reference is no new arithmetic: ONE improved_stream_reference.step state per session (U = 1), advanced with that
session's own rows from its own step count.  What the pool adds - whose count a row's divisors are taken from, in what order
the rows travel, whose record is written - is held by the checkers below, and tests/test_improved_pool_cpu.py shows on wrong
stand-ins (WRONG) that each of them bites.

A pool here is {slot: state}: an improved_stream_reference state of one stream whose "steps" is the slot's own count.
`records_to_blob` / `blob_to_records` move such a pool to and from the device's blob through the layout hook (a dict of byte
offsets, fullsubnet_amd._lib.improved_stream_pool_layout), so the same checkers read the device's records.
"""
import functools

import numpy as np

import improved_stream_reference as R

CAP = 20
COUNTS = (0, 1, 2, 5, R.LONG, R.LONG + 1)  # 0 is a fresh slot; the long ones hold the sums and divisors of 100 000 steps
MODES = (("64", np.float64, "torch"), ("c32", np.float32, "cell"), ("t32", np.float32, "torch"))
OUTSIDE = (-3, CAP)  # ids outside the pool: one goes in front of "seventeen", one at its end


def c_cfg(cfg=R.SMALL, **kw):
    """fsn_improved_cfg of a table configuration (fields overridden by kw), for the queries that need no model."""
    from fullsubnet_amd import _lib
    f = dict(F=cfg.F, fdrc=cfg.fdrc, num_sections=len(cfg.centers), fb_hidden=cfg.fb_hidden, sb_hidden=cfg.sb_hidden, cell=0,
             fb_activation=0, sb_activation=0)
    f.update(kw)
    c = _lib.ImprovedCfg(f["F"], float(f["fdrc"]), f["num_sections"], f["fb_hidden"], f["sb_hidden"], f["cell"], f["fb_activation"],
                         f["sb_activation"])
    for i, ((lower, upper), n) in enumerate(zip(R.bands(cfg), cfg.centers)):
        c.sec[i] = _lib.ImprovedSection(lower, upper, n, cfg.sb_n[i], n, cfg.fb_n[i])
    return c


# ---- the slots of the sweep: count, start state and input of each --------------------------------------------------------------

def slot_count(i):
    return COUNTS[i % len(COUNTS)]


@functools.lru_cache(maxsize=None)
def params_of(cfg):
    return R.make_params(cfg)


def start_state(cfg, i):
    """Slot i of the sweep's pool before a call: fresh at count 0, else a state no short history reaches."""
    c = slot_count(i)
    return R.new_state(1, cfg) if c == 0 else R.random_state(1, cfg, c, R.LEVEL, seed=100 + i)


def start_pool(cfg, cap=CAP):
    return {i: start_state(cfg, i) for i in range(cap)}


def slot_mag(cfg, i, k):
    """[1, F, k]: the frames slot i gets in a call of k steps."""
    return R.make_mag(1, cfg.F, k, seed=7000 + 31 * i + k)


@functools.lru_cache(maxsize=None)
def slot_reference(cfg, i, k):
    """{mode: (mask [1, 2, F, k], state after)} of k steps of slot i from its start state, in the three runs of
    improved_stream_reference.  Computed once per (cfg, slot, k) and shared by every list the slot is part of."""
    out = {}
    for m, dtype, act in MODES:
        st = R.copy_state(start_state(cfg, i))
        out[m] = (R.step(st, slot_mag(cfg, i, k), params_of(cfg), cfg, dtype, act), st)
    return out


LISTS = {"first": [0], "seventeenth": [16], "three": [2, 0, 1], "odd": list(range(1, 16, 2)), "sixteen": list(range(17, 1, -1)),
         "seventeen": [OUTSIDE[0]] + list(range(3, 18)) + [OUTSIDE[1]]}  # "seventeen": 15 slots and the two ids of OUTSIDE
KS = (1, 3)


def call_mags(cfg, slots, k):
    """mag [n, 1, F, k] of a call: every row its slot's own frames (an id outside the pool gets frames too: they are not used)."""
    return np.stack([slot_mag(cfg, i, k) for i in slots])


# ---- a pool on the CPU: the stand-in the checkers are tried on -------------------------------------------------------------

WRONG = ("count-from-the-position", "divisor-count-of-the-first-row", "section-sums-to-the-neighbouring-slot",
         "count-advanced-for-an-unlisted-slot", "rows-in-sorted-order")


def pool_step(pool, slots, mags, k, cfg, dtype=np.float32, act="cell", wrong=None):
    """One call on {slot: state} (updated in place): `slots` in the caller's order (ids outside the pool are skipped: a zero
    row), mags [n, 1, F, k] -> mask [n, 2, F, k] in the caller's order.  wrong: one of WRONG."""
    assert wrong is None or wrong in WRONG
    params = params_of(cfg)
    valid = [i for i in slots if i in pool]
    mask = np.zeros((len(slots), 2, cfg.F, k), dtype=np.float32)
    first = pool[valid[0]]["steps"] if valid else 0
    for row, i in enumerate(slots):
        if i not in pool:
            continue
        st = pool[i]
        t0 = st["steps"]
        sums0 = np.array(st["sb_sum"], copy=True)
        if wrong == "count-from-the-position":  # the row's place in the list instead of the record's count
            st["steps"] = row
        if wrong == "divisor-count-of-the-first-row":  # the call's first row decides the divisors for everybody
            st["steps"] = first
        mask[row] = R.step(st, np.asarray(mags[row]), params, cfg, dtype, act)[0]
        st["steps"] = t0 + k
        if wrong == "section-sums-to-the-neighbouring-slot":
            other = pool.get(i + 1)
            if other is not None:
                other["sb_sum"], st["sb_sum"] = st["sb_sum"], sums0
    if wrong == "rows-in-sorted-order":
        mask = mask[np.argsort(np.asarray(slots), kind="stable")]
    if wrong == "count-advanced-for-an-unlisted-slot":
        other = [i for i in sorted(pool) if i not in slots]
        if other:
            pool[other[0]]["steps"] += k
    return mask


def copy_pool(pool):
    return {i: R.copy_state(st) for i, st in pool.items()}


# ---- the blob through the layout hook ---------------------------------------------------------------------------------------

def _record_fields(lay, cfg):
    """(byte offset in the record, dtype, shape, path into the state)."""
    out = []
    for a in range(4):
        out.append((lay["fb"][a], np.float32, (1, cfg.fb_hidden), ("fb", a // 2, a % 2)))
    for i, n in enumerate(R.num_units(cfg)):
        for a in range(4):
            out.append((lay["sb"][i][a], np.float32, (n, cfg.sb_hidden), ("sb", i, a // 2, a % 2)))
    return out


def _view(rec, off, dtype, shape):
    return rec[off:off + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)


def check_layout(lay, cfg):
    """The record the hook describes is the one this configuration needs."""
    assert lay["sections"] == len(cfg.centers) and list(lay["units"]) == R.num_units(cfg)
    assert (lay["F"], lay["hop"], lay["fb_hidden"], lay["sb_hidden"]) == (cfg.F, cfg.F - 1, cfg.fb_hidden, cfg.sb_hidden)


def records_to_blob(lay, cfg, pool, cap):
    """{slot: state} -> the pool's blob as a uint8 array (slots without a state stay all zeros: fresh)."""
    check_layout(lay, cfg)
    sb, S = lay["slot_bytes"], len(cfg.centers)
    blob = np.zeros(cap * sb, dtype=np.uint8)
    for i, st in pool.items():
        rec = blob[i * sb:(i + 1) * sb]
        for off, dtype, shape, path in _record_fields(lay, cfg):
            a = st
            for p in path:
                a = a[p]
            _view(rec, off, dtype, shape)[...] = np.asarray(a).reshape(shape)
        _view(rec, lay["fb_sum"], np.float64, (1,))[...] = st["fb_sum"]
        _view(rec, lay["sb_sum"], np.float64, (S,))[...] = np.asarray(st["sb_sum"])[:, 0]
        _view(rec, lay["steps"], np.int64, (1,))[0] = st["steps"]
    return blob


def blob_to_records(lay, cfg, blob, cap):
    """The blob (uint8 array) -> {slot: state}, "steps" the record's own count."""
    check_layout(lay, cfg)
    sb, S = lay["slot_bytes"], len(cfg.centers)
    pool = {}
    for i in range(cap):
        rec = blob[i * sb:(i + 1) * sb]
        st = R.new_state(1, cfg)
        for off, dtype, shape, path in _record_fields(lay, cfg):
            a = st
            for p in path[:-1]:
                a = a[p]
            a[path[-1]] = _view(rec, off, dtype, shape).copy()
        st["fb_sum"] = _view(rec, lay["fb_sum"], np.float64, (1,)).copy()
        st["sb_sum"] = _view(rec, lay["sb_sum"], np.float64, (S,)).copy()[:, None]
        st["steps"] = int(_view(rec, lay["steps"], np.int64, (1,))[0])
        pool[i] = st
    return pool


def transform_bytes(lay, blob, i):
    """The transform fields of record i (in_tail .. the end of the record)."""
    sb = lay["slot_bytes"]
    return blob[i * sb + lay["in_tail"]:(i + 1) * sb]


# ---- the checkers -----------------------------------------------------------------------------------------------------------

class Row:
    def __init__(self, id_, cfg, T):
        self.id, self.cfg, self.T = id_, cfg, T


class Ref:
    pass


def join_states(states):
    """States of one stream each -> one state of U streams (steps: None, the slots have their own)."""
    out = {"steps": None}
    out["fb"] = [[np.concatenate([np.asarray(st["fb"][l][j]) for st in states]) for j in range(2)] for l in range(2)]
    out["sb"] = [[[np.concatenate([np.asarray(st["sb"][i][l][j]) for st in states]) for j in range(2)] for l in range(2)]
                 for i in range(len(states[0]["sb"]))]
    out["fb_sum"] = np.concatenate([np.asarray(st["fb_sum"], dtype=np.float64) for st in states])
    out["sb_sum"] = np.concatenate([np.asarray(st["sb_sum"], dtype=np.float64) for st in states], axis=1)
    return out


def states_equal(a, b):
    """Bit for bit, the count included."""
    if a["steps"] != b["steps"]:
        return False
    x, y = R.state_arrays(a), R.state_arrays(b)
    return (all(np.array_equal(x[n], y[n]) for n in x) and np.array_equal(a["fb_sum"], b["fb_sum"]) and
            np.array_equal(a["sb_sum"], b["sb_sum"]))


def reference_of_call(cfg, valid, k, refs=None, starts=None):
    """The Ref of improved_stream_reference's checkers for the rows `valid` of one call: refs(cfg, slot, k) as slot_reference
    gives it, starts(cfg, slot) the slot's state before the call."""
    refs, starts = refs or slot_reference, starts or start_state
    per = [refs(cfg, i, k) for i in valid]
    ref = Ref()
    ref.mask = {m: [np.concatenate([p[m][0] for p in per])] for m, _, _ in MODES}
    ref.state = {m: join_states([p[m][1] for p in per]) for m, _, _ in MODES}
    ref.state0 = join_states([starts(cfg, i) for i in valid])
    return ref


def check_call(what, cfg, slots, k, mask, before, after, log=print, refs=None, starts=None):
    """One call on the sweep's pool, by what it left behind.  slots: the rows as the entry got them; mask [n, 2, F, k] in that
    order; before / after: {slot: state} of the whole pool.
      - every listed count advanced by exactly k, every unlisted record bit-identical;
      - every row finite, those of ids outside the pool included (what they hold is not specified);
      - the masks by improved_stream_reference.check_calls, the listed records by its check_state (check_sums included), against
        each session's own fp64 step at SHARP x the c32 run's error.
    Returns the worst (Frobenius, max, tile) ratios of the masks."""
    valid = [i for i in slots if i in before]
    assert len(set(valid)) == len(valid)
    for i in before:
        if i in valid:
            assert after[i]["steps"] == before[i]["steps"] + k, f"{what}: slot {i} went from {before[i]['steps']} to {after[i]['steps']} steps, k = {k}"
        else:
            assert states_equal(before[i], after[i]), f"{what}: slot {i} is not listed, but its record changed"
    mask = np.asarray(mask)
    assert mask.shape == (len(slots), 2, cfg.F, k) and np.isfinite(mask).all(), f"{what}: masks {mask.shape}, finite {np.isfinite(mask).all()}"
    rows = [row for row, i in enumerate(slots) if i in before]
    ref = reference_of_call(cfg, valid, k, refs, starts)
    row_ = Row(what, cfg, k)
    worst = R.check_calls(row_, ref, [mask[rows]], log=log)
    R.check_state(row_, ref, join_states([after[i] for i in valid]), log=log)
    return worst
