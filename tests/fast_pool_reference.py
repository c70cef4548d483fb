"""The reference, the schedules and the checkers of tests/test_gpu_fast_pool.py; importable without a device
(tests/test_fast_pool_cpu.py runs all of it on the CPU).

The pool's reference is no new arithmetic: ONE fast_stream_reference.step state per session (U = 1), advanced with that
session's own rows from its own step count.  What the pool adds - which slots are due, in what order the rows travel, whose
count moves - is held by the checkers below, and tests/test_fast_pool_cpu.py shows on wrong stand-ins (WRONG) that each of them
bites.

A pool here is {slot: state}: a fast_stream_reference state of one stream whose "steps" is the slot's own count.  `records_to_blob`
/ `blob_to_records` move such a pool to and from the device's blob through the layout hook (a dict of byte offsets), so the
same checkers read the device's records.
"""
import functools

import numpy as np

import fast_stream_reference as R

CAP = 20
COUNTS = (0, 1, 2, 5, R.LONG, R.LONG + 1)  # every phase of a block of 2 and of 3; 0 is a fresh slot
SMALL = R.Cfg(shrink=3, la=1, n_mel=2, n_enc=1, bn_hidden=128, bn_layers=1)
MODES = (("64", np.float64, "torch"), ("c32", np.float32, "cell"), ("t32", np.float32, "torch"))
OUTSIDE = (-3, CAP)  # ids outside the pool: one goes in front of the long rows, one behind the short ones


def c_cfg(cfg=R.SHIPPED, **kw):
    """fsn_fast_cfg of a table configuration (fields overridden by kw)."""
    from fullsubnet_amd import _lib
    f = dict(F=257, num_mels=64, shrink=cfg.shrink, mel_neighbors=cfg.n_mel, enc_neighbors=cfg.n_enc, bn_hidden=cfg.bn_hidden,
             bn_layers=cfg.bn_layers, norm=_lib.NORM_TYPES["cumulative_laplace_norm"])
    f.update(kw)
    return _lib.FastCfg(**f)


def low_frames(t0, k, s):
    """Multiples of s in [t0, t0 + k): the low-rate frames a slot at count t0 completes in k more steps."""
    return (t0 + k - 1) // s - ((t0 - 1) // s if t0 > 0 else -1)


def lo_hi(k, s):
    return k // s, -(-k // s)


def order_by_definition(steps, k, s):
    """fast_pool_order from its definition: the rows that complete hi frames, then the others, each in the given order."""
    hi = lo_hi(k, s)[1]
    long_rows = [i for i, t0 in enumerate(steps) if low_frames(t0, k, s) == hi]
    return long_rows + [i for i in range(len(steps)) if i not in long_rows], len(long_rows)


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


def slot_mag(i, k):
    return R.make_mag(1, k, seed=7000 + 31 * i + k)


@functools.lru_cache(maxsize=None)
def slot_reference(cfg, i, k):
    """{mode: (crm [1, 2, F, k], state after)} of k steps of slot i from its start state, in the three runs of
    fast_stream_reference.  Computed once per (cfg, slot, k) and shared by every list the slot is part of."""
    out = {}
    for m, dtype, act in MODES:
        st = R.copy_state(start_state(cfg, i))
        out[m] = (R.step(st, slot_mag(i, k), params_of(cfg), cfg, dtype, act), st)
    return out


LISTS = {"first": [0], "seventeenth": [16], "three-phases": [2, 0, 1], "odd": list(range(1, 16, 2)), "sixteen": list(range(17, 1, -1)),
         "seventeen": list(range(3, 18))}  # "seventeen": 15 slots and the two ids of OUTSIDE


def ks_of(cfg):
    """k = 1, the close call k = 1 + look_ahead, and at shrink 2 a mixed call (k = 3: lo 1, hi 2) and one with s | k (4)."""
    return sorted({1, 1 + cfg.la} | ({3, 4} if cfg.shrink == 2 else set()))


def call_rows(cfg, name, k):
    """(slots in the order the entry wants, n_long) of list `name`: the long rows first by the definition; "seventeen" gets one
    id outside the pool in front (a long row's place) and one at the end (a short row's, unless s | k)."""
    ids = LISTS[name]
    perm, n_long = order_by_definition([slot_count(i) for i in ids], k, cfg.shrink)
    rows = [ids[j] for j in perm]
    if name == "seventeen":
        rows = [OUTSIDE[0]] + rows + [OUTSIDE[1]]
        n_long = len(rows) if k % cfg.shrink == 0 else n_long + 1
    return rows, n_long


def not_due_list(cfg, cap=CAP):
    """The slots of the pool that complete no low-rate frame in a k = 1 call."""
    return [i for i in range(cap) if slot_count(i) % cfg.shrink]


# ---- a pool on the CPU: the stand-in the checkers are tried on -------------------------------------------------------------

WRONG = ("bottleneck-stepped-when-not-due", "held-not-refreshed", "count-from-the-position", "rows-in-sorted-order",
         "count-advanced-for-an-unlisted-slot")


def pool_step(pool, slots, mags, k, cfg, dtype=np.float32, act="cell", wrong=None):
    """One call on {slot: state} (updated in place): `slots` in the caller's order (ids outside the pool are skipped: a zero
    row), mags[row] [1, 1, F, k] -> crm [n, 2, F, k] in the caller's order.  wrong: one of WRONG."""
    assert wrong is None or wrong in WRONG
    params = params_of(cfg)
    valid = [i for i in slots if i in pool]
    crm = np.zeros((len(slots), 2, R.F, k), dtype=np.float32)
    first = pool[valid[0]]["steps"] if valid else 0
    for row, i in enumerate(slots):
        if i not in pool:
            continue
        st = pool[i]
        t0 = st["steps"]
        held0 = np.array(st["held"], copy=True)
        if wrong == "count-from-the-position":  # the call's first row decides the count for everybody
            st["steps"] = first
        crm[row] = R.step(st, mags[row], params, cfg, dtype, act)[0]
        st["steps"] = t0 + k
        due = low_frames(t0, k, cfg.shrink) > 0
        if wrong == "bottleneck-stepped-when-not-due" and not due:
            W = R.unit_width(cfg)
            R._block(np.ones((R.M, W, 1), dtype=dtype), params, "bottleneck", cfg.bn_layers, True, True, dtype, act, st["bn"])
        if wrong == "held-not-refreshed" and due:
            st["held"] = held0
    if wrong == "rows-in-sorted-order":
        perm, _ = order_by_definition([pool[i]["steps"] - k if i in pool else 0 for i in slots], k, cfg.shrink)
        crm = crm[perm]
    if wrong == "count-advanced-for-an-unlisted-slot":
        other = [i for i in sorted(pool) if i not in slots]
        if other:
            pool[other[0]]["steps"] += k
    return crm


def copy_pool(pool):
    return {i: R.copy_state(st) for i, st in pool.items()}


# ---- the blob through the layout hook ---------------------------------------------------------------------------------------

def _record_fields(lay, cfg):
    """(name in the layout, dtype, shape in the record, (key, layer, index) or key of the state, valid extent)."""
    H, W = cfg.bn_hidden, lay["unit_width"]
    out = []
    for key, width, real in (("enc0", 384, 384), ("enc1", 320, 257), ("dec0", 512, 512), ("dec1", 512, 512)):
        for j, hc in enumerate("hc"):
            out.append((f"{key}_{hc}", np.float32, (1, width), (key, 0, j), (1, real)))
    for l in range(cfg.bn_layers):
        for j, hc in enumerate("hc"):
            out.append((f"bn_{hc}{l}", np.float32, (R.M, H), ("bn", l, j), (R.M, H)))
    out += [("mel_sum", np.float64, (1,), "mel_sum", (1,)), ("unit_sum", np.float64, (1, R.M), "unit_sum", (1, R.M)),
            ("partial", np.float32, (1, R.M, W), "partial", (1, R.M, W)), ("held", np.float32, (1, R.M), "held", (1, R.M))]
    return out


def _view(rec, lay, name, dtype, shape):
    return rec[lay[name]:lay[name] + int(np.prod(shape)) * np.dtype(dtype).itemsize].view(dtype).reshape(shape)


def records_to_blob(lay, cfg, pool, cap):
    """{slot: state} -> the pool's blob as a uint8 array (slots without a state stay all zeros: fresh)."""
    sb = lay["slot_bytes"]
    blob = np.zeros(cap * sb, dtype=np.uint8)
    for i, st in pool.items():
        rec = blob[i * sb:(i + 1) * sb]
        for name, dtype, shape, src, valid in _record_fields(lay, cfg):
            a = st[src[0]][src[1]][src[2]] if isinstance(src, tuple) else st[src]
            _view(rec, lay, name, dtype, shape)[tuple(slice(0, n) for n in valid)] = np.asarray(a).reshape(valid)
        _view(rec, lay, "steps", np.int32, (1,))[0] = st["steps"]
    return blob


def blob_to_records(lay, cfg, blob, cap):
    """The blob (uint8 array) -> {slot: state}, "steps" the record's own count."""
    sb = lay["slot_bytes"]
    pool = {}
    for i in range(cap):
        rec = blob[i * sb:(i + 1) * sb]
        st = R.new_state(1, cfg)
        for name, dtype, shape, src, valid in _record_fields(lay, cfg):
            view = _view(rec, lay, name, dtype, shape)
            a = view[tuple(slice(0, n) for n in valid)].copy()
            if isinstance(src, tuple):
                st[src[0]][src[1]][src[2]] = a
                if name.startswith("enc1"):
                    assert not view[:, 257:].any(), f"slot {i} {name}: a padded unit left zero"
            else:
                st[src] = a
        st["steps"] = int(_view(rec, lay, "steps", np.int32, (1,))[0])
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
    for key, _, _ in R.BLOCKS:
        out[key] = [[np.concatenate([np.asarray(st[key][l][j]) for st in states]) for j in range(2)] for l in range(len(states[0][key]))]
    for key in ("mel_sum", "unit_sum", "partial", "held"):
        out[key] = np.concatenate([np.asarray(st[key]) for st in states])
    return out


def states_equal(a, b):
    """Bit for bit, the count included."""
    if a["steps"] != b["steps"]:
        return False
    x, y = R.state_arrays(a), R.state_arrays(b)
    return (all(np.array_equal(x[n], y[n]) for n in x) and np.array_equal(a["mel_sum"], b["mel_sum"]) and
            np.array_equal(a["unit_sum"], b["unit_sum"]))


def bottleneck_untouched(a, b):
    """The fields a call in which the slot completes no low-rate frame must leave alone."""
    return (all(np.array_equal(a["bn"][l][j], b["bn"][l][j]) for l in range(len(a["bn"])) for j in range(2)) and
            np.array_equal(a["unit_sum"], b["unit_sum"]) and np.array_equal(a["held"], b["held"]))


def check_call(what, cfg, slots, k, crm, before, after, log=print, refs=slot_reference):
    """One call on the sweep's pool, by what it left behind.  slots: the rows as the entry got them (or, for a pool that sorts
    by itself, as its caller gave them); crm [n, 2, F, k] in that order; before / after: {slot: state} of the whole pool.
      - every listed count advanced by exactly k, every unlisted record bit-identical;
      - every row finite, those of ids outside the pool included (what they hold is not specified);
      - a slot that completes no low-rate frame: its bottleneck (h, c), unit sums and held output bit-identical;
      - the masks by fast_stream_reference.check_calls, the states by its check_state (check_sums included), against the
        per-session fp64 reference.
    Returns the worst (Frobenius, max, tile) ratios of the masks."""
    valid = [i for i in slots if i in before]
    assert len(set(valid)) == len(valid)
    for i in before:
        if i in valid:
            assert after[i]["steps"] == before[i]["steps"] + k, f"{what}: slot {i} went from {before[i]['steps']} to {after[i]['steps']} steps, k = {k}"
            if low_frames(before[i]["steps"], k, cfg.shrink) == 0:
                assert bottleneck_untouched(before[i], after[i]), f"{what}: slot {i} completes no low-rate frame, but its bottleneck fields moved"
        else:
            assert states_equal(before[i], after[i]), f"{what}: slot {i} is not listed, but its record changed"
    crm = np.asarray(crm)
    assert crm.shape == (len(slots), 2, R.F, k) and np.isfinite(crm).all(), f"{what}: masks {crm.shape}, finite {np.isfinite(crm).all()}"
    rows = [row for row, i in enumerate(slots) if i in before]
    ref = Ref()
    per = [refs(cfg, i, k) for i in valid]
    ref.crm = {m: [np.concatenate([p[m][0] for p in per])] for m, _, _ in MODES}
    ref.state = {m: join_states([p[m][1] for p in per]) for m, _, _ in MODES}
    ref.state0 = join_states([start_state(cfg, i) for i in valid])
    row_ = Row(what, cfg, k)
    worst = R.check_calls(row_, ref, [crm[rows]], log=log)
    R.check_state(row_, ref, join_states([after[i] for i in valid]), log=log)
    return worst
