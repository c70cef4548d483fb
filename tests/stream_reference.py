"""The stateful reference, the table and the checkers of tests/test_gpu_stream_sweep.py; importable without a device
(tests/test_stream_sweep_cpu.py runs all of it on the CPU).

The model entries that carry state between calls - fsn_fullsubnet_stream_step, fsn_fullsubnet_stream_pool_step and the
fsn_fullsubnet_segment_* passes - hand back EVERY model step (look-ahead 0 semantics; the caller matches step s to frame
s - look_ahead), so the reference is one step function, `step`: k more frames of the model on a state.  It is built on the
pieces of tests/test_gpu_core_sweep.py (subband_units, rows_to_mask, lstm_layer, make_inputs' recipe) and the oracle's
norms; tests/test_stream_sweep_cpu.py holds it, chunked as the table chunks it, to the whole-sequence `model` of the core
sweep to 1e-12.

State (`new_state`): (h0, h1, c0, c1) of the full-band layers [U, Hf] and of the sub-band layers [U F, Hs], the running
sums fb_sum [U] and sb_sum [U, F] of the cumulative norm (fp64, as the oracle sums), and steps [U] - per row, so that the
pool's per-slot counts and the lockstep entry's single steps_done are the same code.  Under the offline norm the divisors
are arguments, one per row, as fsn_fullsubnet_segment_divisors yields them (`offline_divisors`).

Three runs, as in the core sweep: fp64 with torch's activations (the reference), fp32 with lstm_cell.h's formulas
(act="cell": the yardstick of the masks and of h and c), fp32 with torch's activations (the yardstick of fb_out).
"""
import functools
import math

import numpy as np
import torch

from oracle import fullsubnet_oracle as O
from test_gpu_core_sweep import SHARP, check_tensor, frob, lstm_layer, rows_to_mask, subband_units

LEVEL = 0.05 + math.sqrt(2.0 / math.pi)  # the mean of |N(0, 1)| + 0.05, the inputs' level
LONG = 100000                            # frames of a long stream
U53 = 2.0 ** -53
CAPACITY = 19


# ---- the stateful step ------------------------------------------------------------------------------------------------

def new_state(U, F, Hf, Hs=384):
    z = lambda *s: np.zeros(s, dtype=np.float32)  # noqa: E731
    return {"fb": [z(U, Hf) for _ in range(4)], "sb": [z(U * F, Hs) for _ in range(4)], "fb_sum": np.zeros(U), "sb_sum": np.zeros((U, F)),
            "steps": np.zeros(U, dtype=np.int64)}


def random_state(U, F, Hf, steps, level, seed, Hs=384, nb=15):
    """A state no short history reaches: h uniform in (-0.9, 0.9), c in (-2, 2) (fp32 values, so every run starts from the
    same numbers), the sums of `steps[u]` frames at the inputs' level (sb_sum a little different per bin)."""
    rng = np.random.default_rng(seed)
    st = new_state(U, F, Hf, Hs)
    for key in ("fb", "sb"):
        for a in range(4):
            lim = 0.9 if a < 2 else 2.0
            st[key][a] = rng.uniform(-lim, lim, st[key][a].shape).astype(np.float32)
    st["steps"] = np.asarray(steps, dtype=np.int64).copy()
    st["fb_sum"] = st["steps"] * float(F) * np.asarray(level, dtype=np.float64)
    st["sb_sum"] = (st["steps"] * float(2 * nb + 2) * np.asarray(level, dtype=np.float64))[:, None] * (1.0 + 0.1 * rng.uniform(-1, 1, (U, F)))
    return st


def copy_state(st):
    return {k: [a.copy() for a in v] if isinstance(v, list) else v.copy() for k, v in st.items()}


def take_state(st, sel, F):
    """The state of the utterances `sel` (an index array), in that order."""
    rows = (np.asarray(sel)[:, None] * F + np.arange(F)[None, :]).reshape(-1)
    return {"fb": [a[sel] for a in st["fb"]], "sb": [a[rows] for a in st["sb"]], "fb_sum": st["fb_sum"][sel], "sb_sum": st["sb_sum"][sel],
            "steps": st["steps"][sel]}


def _seq_state(x, params, prefix, dtype, act, relu, hc):
    """_seq of the core sweep from a given state: x [N, I, k] -> [N, out, k]; hc = [h0, h1, c0, c1] is replaced."""
    td = torch.float64 if dtype == np.float64 else torch.float32
    o = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype).transpose(2, 0, 1)))  # [k, N, I]
    for l in range(2):
        g = lambda n: torch.from_numpy(np.asarray(params[f"{prefix}.sequence_model.{n}_l{l}"], dtype=dtype))  # noqa: E731
        h, c = (torch.from_numpy(np.asarray(hc[a], dtype=dtype)).to(td) for a in (l, 2 + l))
        o, h, c = lstm_layer(o, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"), h, c, act=act)
        hc[l], hc[2 + l] = h.numpy(), c.numpy()
    w = torch.from_numpy(np.asarray(params[f"{prefix}.fc_output_layer.weight"], dtype=dtype))
    b = torch.from_numpy(np.asarray(params[f"{prefix}.fc_output_layer.bias"], dtype=dtype))
    o = o @ w.t() + b
    return (torch.relu(o) if relu else o).numpy().transpose(1, 2, 0)


def _cumulative(x, run0, steps, carry_dtype):
    """cumulative_laplace_norm of the oracle on x [n, C, k] continued from the running sums run0 [n] after steps [n] frames:
    (normalised x, new running sums).  carry_dtype=float32 is the deliberately wrong carry of the CPU self-test."""
    dtype = x.dtype.type
    n, C, k = x.shape
    run = np.empty((n, k), dtype=carry_dtype)
    acc = np.asarray(run0, dtype=carry_dtype).copy()
    step_sum = x.sum(axis=1, dtype=np.float64)
    for t in range(k):
        acc = (acc + step_sum[:, t].astype(carry_dtype)).astype(carry_dtype)
        run[:, t] = acc
    count = float(C) * (np.asarray(steps, dtype=np.float64)[:, None] + np.arange(1, k + 1)[None, :])
    mean = (run.astype(np.float64) / count).astype(dtype)[:, None, :]
    return (x / (mean + dtype(O.EPSILON))).astype(dtype), run[:, -1].astype(np.float64)


def fullband_step(state, mag, params, norm, dtype, act, den_fb=None, carry_dtype=np.float64):
    """k more frames of the full-band model: mag [U, 1, F, k] -> fb_out [U, F, k]; updates state["fb"] and fb_sum (not steps)."""
    x = np.asarray(mag, dtype=dtype)[:, 0]
    if norm == "cumulative":
        xn, state["fb_sum"] = _cumulative(x, state["fb_sum"], state["steps"], carry_dtype)
    else:
        xn = (x / np.asarray(den_fb, dtype=dtype)[:, None, None]).astype(dtype)
    return _seq_state(xn, params, "fb_model", dtype, act, True, state["fb"])


def subband_step(state, mag, fb_out, params, nb, norm, dtype, act, den_sb=None, carry_dtype=np.float64):
    """k more frames of the sub-band model on mag [U, 1, F, k] and fb_out [U, F, k] -> crm [U, 2, F, k]; updates state["sb"],
    sb_sum and steps."""
    x = np.asarray(mag, dtype=dtype)
    U, _, F, k = x.shape
    units = subband_units(x, np.asarray(fb_out, dtype=dtype)[:, None], nb).reshape(U * F, 2 * nb + 2, k)
    if norm == "cumulative":
        un, run = _cumulative(units, state["sb_sum"].reshape(-1), np.repeat(state["steps"], F), carry_dtype)
        state["sb_sum"] = run.reshape(U, F)
    else:
        un = (units / np.repeat(np.asarray(den_sb, dtype=dtype), F)[:, None, None]).astype(dtype)
    rows = _seq_state(un, params, "sb_model", dtype, act, False, state["sb"])
    state["steps"] = state["steps"] + k
    return rows_to_mask(rows, U)


def step(state, mag, params, nb, norm, dtype, act, den=None, carry_dtype=np.float64):
    """One call of the model step on `state` (updated in place): mag [U, 1, F, k] -> (crm [U, 2, F, k], fb_out [U, F, k], state)."""
    den_fb, den_sb = den if den is not None else (None, None)
    fb = fullband_step(state, mag, params, norm, dtype, act, den_fb, carry_dtype)
    crm = subband_step(state, mag, fb, params, nb, norm, dtype, act, den_sb, carry_dtype)
    return crm, fb, state


def offline_divisors(mag, fb_out, nb, totals, dtype):
    """(den_fb [U], den_sb [U]) of offline_laplace_norm over each row's own total frames: mag [U, 1, F, Tp] (zero beyond a
    row's frames), fb_out [U, F, Tp] or None (then den_sb is None)."""
    den_fb, den_sb = [], []
    for u, n in enumerate(totals):
        x = np.asarray(mag[u:u + 1, :, :, :n], dtype=dtype)
        den_fb.append(x.mean(dtype=np.float64).astype(dtype) + dtype(1e-5))
        if fb_out is not None:
            units = subband_units(x, np.asarray(fb_out[u:u + 1, None, :, :n], dtype=dtype), nb)
            den_sb.append(units.mean(dtype=np.float64).astype(dtype) + dtype(1e-5))
    return np.asarray(den_fb, dtype=dtype), (np.asarray(den_sb, dtype=dtype) if fb_out is not None else None)


def crm_rows(crm):
    """[U, 2, F, k] -> rows [U F, 2, k]."""
    U, _, F, k = crm.shape
    return np.ascontiguousarray(crm.transpose(0, 2, 1, 3)).reshape(U * F, 2, k)


# ---- the table --------------------------------------------------------------------------------------------------------

class Row:
    """One line of the sweep.  entry "stream": split = the frames of the calls on one state, B utterances in lockstep;
    "pool": slots = the list, the calls are k = 1 then k = 3 on a pool of CAPACITY records; "segment": totals = frames of
    each row (look-ahead zeros included), segments = (first step, steps)."""

    def __init__(self, why, entry, B=None, split=None, F=257, Hf=512, nb=15, norm="cumulative", resumed=False, slots=None, totals=None,
                 segments=None, la=2):
        self.why, self.entry, self.F, self.Hf, self.nb, self.norm, self.resumed, self.la = why, entry, F, Hf, nb, norm, resumed, la
        self.slots, self.totals, self.gain = slots, totals, 2.0
        if entry == "pool":
            B, split = len(slots), (1, 3)
        if entry == "segment" and segments is not None:
            split = tuple(k for _, k in segments)
        self.B, self.split = B, tuple(split)
        self.T = sum(self.split)
        self.segments = [(sum(self.split[:c]), k) for c, k in enumerate(self.split)]  # (steps done before the call, frames)
        assert segments is None or list(segments) == self.segments
        # distinct utterances computed on the CPU: the pool's slots are all distinct, a batch above 3 repeats 3 (b -> base[b % k])
        self.k = CAPACITY if entry == "pool" else min(B, 3)

    @property
    def id(self):
        what = "s" + "_".join(map(str, self.slots)) if self.entry == "pool" else f"B{self.B}-" + "_".join(map(str, self.split))
        return f"{self.why}-{self.entry}-{what}" + (f"-nb{self.nb}" if self.nb != 15 else "") + (f"-F{self.F}" if self.F != 257 else "") + \
            (f"-Hf{self.Hf}" if self.Hf != 512 else "") + ("-offline" if self.norm == "offline" else "")

    @property
    def sel(self):
        """The reference utterance behind each row of a call."""
        valid = [s if 0 <= s < CAPACITY else 0 for s in self.slots] if self.entry == "pool" else None
        return np.asarray(valid) if self.entry == "pool" else np.arange(self.B) % self.k

    @property
    def held(self):
        """Rows of a call that are held to fp64 (all but the ids outside the pool)."""
        return [i for i, s in enumerate(self.slots) if 0 <= s < CAPACITY] if self.entry == "pool" else list(range(self.B))

    def cfg(self, lib):
        return lib.Cfg(self.F, self.la, self.nb, self.Hf, 384, lib.NORM_TYPES[f"{self.norm}_laplace_norm"], 0)


def pool_steps():
    """Slot i sits at 3 i frames, the last one at LONG."""
    return np.asarray([3 * i for i in range(CAPACITY - 1)] + [LONG], dtype=np.int64)


def _table():
    rows = []
    S = lambda why, B, split, **kw: rows.append(Row(why, "stream", B, split, **kw))  # noqa: E731
    # ---- the lockstep entry; steps_done is the running total ----
    S("frame-by-frame", 1, (1, 1, 1, 1, 1, 1))  # the production regime; 17 sub-band tiles, 15 pad rows
    S("one-call", 1, (6,))                      # the same frames in one call
    S("uneven-chunks", 2, (1, 4, 1, 2))         # 514 rows, 14 pad rows
    S("pad13", 3, (3, 5))                       # 771 rows
    S("pad1", 15, (2, 1))                       # 3855 rows
    S("pad0-fb-one-tile", 16, (2, 1))           # 4112 rows; the full-band model exactly one tile
    S("fb-second-tile", 17, (1, 2))             # the full-band model's second tile with 15 pad rows
    S("fpad-5-tiles", 1, (1, 1, 3), F=65, Hf=384)
    S("fpad-325-rows", 5, (4,), F=65, Hf=384)
    S("fb-h-below-sb", 2, (2, 3), Hf=256)       # the full-band H0 smaller than the sub-band's 384
    S("kin16", 2, (2, 3), nb=7)                 # 16 sub-band input columns (sb_kin_pad)
    S("kin2", 2, (2, 3), nb=0)                  # 2
    S("resumed", 2, (1, 3), resumed=True)       # from a written state at 100 000 frames
    # ---- the pool: every record written, one call at k = 1 and one at k = 3 ----
    P = lambda why, slots: rows.append(Row(why, "pool", slots=list(slots)))  # noqa: E731
    P("long-slot-alone", [18])
    P("unordered", [16, 0, 7])
    P("unordered-reversed", [7, 0, 16])
    P("descending", range(18, -1, -1))
    P("permutation", np.random.default_rng(19).permutation(CAPACITY).tolist())
    P("odd-reversed", range(17, 0, -2))
    P("ids-outside", [3, -1, 5, 19])            # C level: an id outside [0, capacity) is skipped by every kernel
    # ---- the segment passes, offline norm with look-ahead 2 (the caller appends the zero frames) ----
    G = lambda why, totals, segments, **kw: rows.append(Row(why, "segment", len(totals), None, norm="offline", totals=totals,  # noqa: E731
                                                            segments=segments, **kw))
    G("ends-inside-last", (12, 9), ((0, 1), (1, 7), (8, 4)))
    G("ends-on-edge", (12, 8, 3), ((0, 4), (4, 4), (8, 4)))  # row 1 ends exactly on a segment edge, row 2 inside the first
    G("one-segment", (12,), ((0, 12),))
    rows.append(Row("as-lockstep", "segment", 2, (1, 4, 1, 2), totals=(8, 8)))  # the cumulative norm through the segment entries
    return rows


TABLE = _table()


def check_duplication(row):
    """b -> base[b % k] cannot hide a mix-up of rows: no two copies of an utterance lie a whole number of 16-row tiles apart."""
    for j in range(1, -(-row.B // row.k)):
        assert (j * row.k * row.F) % 16 != 0, f"{row.id}: copies {j} periods apart lie a whole number of row tiles apart"


# ---- the reference of a row ---------------------------------------------------------------------------------------------

def make_inputs(F, nb, Hf, T, k):
    """The core sweep's recipe: |N(0, 1)| + 0.05 magnitudes, O.make_params(gain=2, mask_gain=24)."""
    params = O.make_params(seed=3, num_freqs=F, fb_hidden=Hf, sb_num_neighbors=nb, gain=2.0, mask_gain=24.0)
    rng = np.random.default_rng(1000 * T + 10 * F + k)
    return params, (np.abs(rng.standard_normal((k, 1, F, T))) + 0.05).astype(np.float32)


def _sums(state0, mags, fbs, nb):
    """The running sums after the calls, summed in extended precision from the fp32 inputs (and the given full-band outputs)."""
    assert np.finfo(np.longdouble).nmant >= 63
    ld = np.longdouble
    fb_sum, sb_sum = state0["fb_sum"].astype(ld), state0["sb_sum"].astype(ld)
    for mag, fb in zip(mags, fbs):
        fb_sum = fb_sum + mag.astype(ld).sum(axis=(1, 2, 3))
        sb_sum = sb_sum + subband_units(mag.astype(ld), fb[:, None].astype(ld), nb).sum(axis=(2, 3))
    return fb_sum, sb_sum


class Ref:
    """The row's calls through the fp64 step and the two fp32 yardsticks on its k distinct utterances: crm[m][call] [k, 2, F,
    frames], fb[m][call] [k, F, frames] and the final state[m] for m in "64", "c32", "t32" (t32: the full-band half only)."""

    def __init__(self, entry, k, split, F, Hf, nb, norm, resumed, totals, la):
        self.F, self.nb, self.k, self.split, self.norm = F, nb, k, split, norm
        T = sum(split)
        self.params, mag = make_inputs(F, nb, Hf, T, k)
        if totals is not None and norm == "offline":  # frames from a row's own end on are zero: its look-ahead frames, then padding
            self.totals = [totals[u % len(totals)] for u in range(k)]
            for u, n in enumerate(self.totals):
                mag[u, :, :, n - la:] = 0.0
        self.mag = mag
        edges = np.concatenate([[0], np.cumsum(split)])
        self.mags = [mag[..., a:b] for a, b in zip(edges[:-1], edges[1:])]
        level = mag.mean(axis=(1, 2, 3), dtype=np.float64)
        if entry == "pool":
            self.state0 = random_state(k, F, Hf, pool_steps(), level, seed=7, nb=nb)
            self.state0["fb_sum"][0], self.state0["sb_sum"][0] = 0.0, 0.0
        elif resumed:
            self.state0 = random_state(k, F, Hf, [LONG] * k, level, seed=11, nb=nb)
        else:
            self.state0 = new_state(k, F, Hf)
        self.crm, self.fb, self.state, self.den = {}, {}, {}, {}
        for m, dtype, act in (("64", np.float64, "torch"), ("c32", np.float32, "cell"), ("t32", np.float32, "torch")):
            self.crm[m], self.fb[m], self.state[m], self.den[m] = self.run(dtype, act, fb_only=m == "t32")
        self.fb_exact, self.sb_exact = _sums(self.state0, self.mags, self.fb["64"], nb)
        self.fb_gap = np.max([np.abs(a.astype(np.float64) - b).max(axis=(1, 2)) for a, b in zip(self.fb["t32"], self.fb["64"])], axis=0)  # [k]

    def run(self, dtype, act, fb_only=False, tamper=None, carry_dtype=np.float64, totals=None):
        """The calls of the row in `dtype`; tamper(call index, state) may change the state before a call (the wrong stand-ins
        of the CPU self-test).  Offline: all full-band calls, the divisors, then all sub-band calls, as the entries run."""
        st = copy_state(self.state0)
        tamper = tamper or (lambda c, s: None)
        kw = dict(carry_dtype=carry_dtype)
        crm, fb, den = [], [], (None, None)
        if self.norm == "cumulative":
            for c, x in enumerate(self.mags):
                tamper(c, st)
                fb.append(fullband_step(st, x, self.params, "cumulative", dtype, act, **kw))
                if fb_only:
                    st["steps"] = st["steps"] + x.shape[-1]
                else:
                    crm.append(subband_step(st, x, fb[-1], self.params, self.nb, "cumulative", dtype, act, **kw))
            return crm, fb, st, den
        totals = totals or self.totals
        den_fb, _ = offline_divisors(self.mag, None, self.nb, totals, dtype)
        for c, x in enumerate(self.mags):
            fb.append(fullband_step(st, x, self.params, "offline", dtype, act, den_fb))
        den = offline_divisors(self.mag, np.concatenate(fb, axis=-1), self.nb, totals, dtype)
        if not fb_only:
            for c, x in enumerate(self.mags):
                tamper(c, st)
                crm.append(subband_step(st, x, fb[c], self.params, self.nb, "offline", dtype, act, den[1]))
        return crm, fb, st, den


@functools.lru_cache(maxsize=8)
def _reference(entry, k, split, F, Hf, nb, norm, resumed, totals, la):
    return Ref(entry, k, split, F, Hf, nb, norm, resumed, totals, la)


def reference_of(row):
    """Shared between the rows that run the same calls on the same utterances (all pool lists; a row and its second run)."""
    totals = tuple(row.totals) if row.totals is not None and row.norm == "offline" else None
    return _reference("pool" if row.entry == "pool" else "seq", row.k, row.split, row.F, row.Hf, row.nb, row.norm, row.resumed, totals, row.la)


# ---- the checkers -------------------------------------------------------------------------------------------------------

def frames_held(row, ref, c, u):
    """The frames of call c that are held for reference utterance u: all, or those below the row's own total."""
    k = row.split[c]
    if row.norm != "offline":
        return k
    return int(np.clip(ref.totals[u] - sum(row.split[:c]), 0, k))


def check_calls(row, ref, got_crm, got_fb=None, log=print):
    """got_crm[call] [B, 2, F, k] (and got_fb[call] [B, F, k]) against the fp64 step at SHARP x the fp32 yardsticks: every call
    on its own, then all calls together.  Returns the worst (Frobenius, max, tile) ratios per output."""
    sel, held, F = row.sel, row.held, row.F
    worst = {}

    def hold(name, what, got, yard, r64, who):
        res = check_tensor(f"{row.id} {name} {what}", got, yard, r64, log=log, who=who)
        worst[what] = tuple(max(a, b) for a, b in zip(worst.get(what, (0.0, 0.0, 0.0)), res))

    ragged = row.norm == "offline" and len(set(ref.totals)) > 1
    for what, got_calls, yard_m, rows_of, who in (("crm", got_crm, "c32", crm_rows, "the fp32 cell emulation"),
                                                 ("fb_out", got_fb, "t32", lambda a: a, "torch's fp32")):
        if got_calls is None:
            continue
        per_call, per_utterance = [], {}
        for c, got in enumerate(got_calls):
            g = rows_of(np.asarray(got)[held])
            y = rows_of((ref.crm if what == "crm" else ref.fb)[yard_m][c][sel[held]])
            r = rows_of((ref.crm if what == "crm" else ref.fb)["64"][c][sel[held]])
            per = F if what == "crm" else 1
            if what == "crm" and ragged:  # each utterance over its own frames
                for i, b in enumerate(held):
                    n = frames_held(row, ref, c, sel[b])
                    if n > 0:
                        s = slice(i * per, (i + 1) * per)
                        hold(f"call {c} utterance {b}", what, g[s, ..., :n], y[s, ..., :n], r[s, ..., :n], who)
                        per_utterance.setdefault(b, []).append((g[s, ..., :n], y[s, ..., :n], r[s, ..., :n]))
                continue
            n = frames_held(row, ref, c, sel[held[0]]) if what == "crm" else row.split[c]
            if n > 0:
                hold(f"call {c}", what, g[..., :n], y[..., :n], r[..., :n], who)
                per_call.append((g[..., :n], y[..., :n], r[..., :n]))
        if len(per_call) > 1:
            hold("all calls", what, *(np.concatenate(parts, axis=-1) for parts in zip(*per_call)), who)
        for b, calls in per_utterance.items():
            if len(calls) > 1:
                hold(f"all calls utterance {b}", what, *(np.concatenate(parts, axis=-1) for parts in zip(*calls)), who)
    return worst


STATE_ARRAYS = ("fb_h0", "fb_h1", "fb_c0", "fb_c1", "sb_h0", "sb_h1", "sb_c0", "sb_c1")


def check_state(row, ref, got, log=print, after="the last call"):
    """got: a state dict of the held rows in call order (take_state's layout).  h and c of the four layers against the fp64
    state at SHARP x the cell emulation's own state error (Frobenius, per array); the steps exactly; the two sums by the
    derived bounds.  Returns the worst ratios."""
    sel = row.sel[row.held]
    r64, c32 = take_state(ref.state["64"], sel, row.F), take_state(ref.state["c32"], sel, row.F)
    worst = {}
    for i, name in enumerate(STATE_ARRAYS):
        key, a = name[:2], "h0 h1 c0 c1".split().index(name[3:])
        g = np.asarray(got[key][a], dtype=np.float64)
        assert np.isfinite(g).all(), f"{row.id} state {name} after {after}: not finite"
        fg, fy = frob(g, r64[key][a]), frob(c32[key][a].astype(np.float64), r64[key][a])
        worst[name] = fg / fy if fy > 0 else float("inf") if fg > 0 else 0.0
        log(f"[ssweep] {row.id} state {name} after {after}: frob hip {fg:.3e} yardstick {fy:.3e} ({worst[name]:.2f} x)")
        assert fg <= SHARP * fy, (f"{row.id} state {name} after {after}: Frobenius error {fg:.3e} of the device against {fy:.3e} of the fp32 "
                                  f"cell emulation on the CPU ({worst[name]:.2f} x, allowed {SHARP:g} x)")
    assert np.array_equal(np.asarray(got["steps"]), r64["steps"]), \
        f"{row.id} after {after}: step counts {np.asarray(got['steps']).tolist()}, expected {r64['steps'].tolist()}"
    if row.norm == "cumulative":
        worst.update(check_sums(row, ref, got, log, after))
    return worst


def check_sums(row, ref, got, log=print, after="the last call", hold=True):
    """The carries are fp64 sums of positive fp32 terms: |sum - exact| <= (terms added + 2) 2^-53 exact, whatever the order;
    sb_sum also holds the device's own fb_out: + frames SHARP max|fb_t32 - fb64| (the full-band rule's own margin).
    hold=False: only the ratios error / bound are returned."""
    sel = row.sel[row.held]
    ld = np.longdouble
    frames = row.T
    fb_exact, sb_exact = ref.fb_exact[sel], ref.sb_exact[sel]
    fb_err = np.abs(np.asarray(got["fb_sum"]).astype(ld) - fb_exact).astype(np.float64)
    fb_bound = ((frames * row.F + 2) * U53 * fb_exact).astype(np.float64)
    sb_err = np.abs(np.asarray(got["sb_sum"]).astype(ld) - sb_exact).astype(np.float64)
    sb_round = ((frames * (2 * row.nb + 2) + 2) * U53 * sb_exact).astype(np.float64)
    sb_bound = sb_round + frames * SHARP * ref.fb_gap[sel][:, None]
    out = {"fb_sum": float((fb_err / fb_bound).max()), "sb_sum": float((sb_err / sb_bound).max()),
           "sb_sum rounding": float((sb_err / sb_round).max())}
    log(f"[ssweep] {row.id} sums after {after}: fb_sum error {out['fb_sum']:.3f} of its bound ({fb_err.max():.3e}), sb_sum "
        f"{out['sb_sum']:.3f} of its bound ({sb_err.max():.3e}; rounding part {sb_round.max():.3e})")
    for name, err, bound in (("fb_sum", fb_err, fb_bound), ("sb_sum", sb_err, sb_bound)) if hold else ():
        bad = np.argwhere(err > bound)
        assert bad.size == 0, (f"{row.id} {name} after {after}: at {tuple(bad[0])} of the held rows the carry is {err[tuple(bad[0])]:.3e} from the exact "
                               f"sum, the bound of an fp64 sum is {bound[tuple(bad[0])]:.3e}")
    return out


def check_divisors(row, ref, got_fb, got_sb, fb_device, log=print):
    """den_fb / den_sb [B] of fsn_fullsubnet_segment_divisors: within one np.spacing of the fp32 of the exact fp64 mean + 1e-5
    (tests/test_gpu_long.py::test_divisors_are_fp64_sums), over each row's own total frames; the sub-band mean is over the
    device's own fb_out [B, F, Tp]."""
    sel = row.sel
    worst = 0.0
    for b in range(row.B):
        n = ref.totals[sel[b]]
        x = ref.mag[sel[b]:sel[b] + 1, :, :, :n].astype(np.float64)
        units = subband_units(x, np.asarray(fb_device, dtype=np.float64)[b:b + 1, None, :, :n], row.nb)
        for name, got, mean in (("den_fb", got_fb[b], x.mean()), ("den_sb", got_sb[b], units.mean())):
            want = np.float32(np.float32(mean) + np.float32(1e-5))
            ulp = abs(np.float64(got) - np.float64(want)) / np.float64(np.spacing(want))
            worst = max(worst, float(ulp))
            log(f"[ssweep] {row.id} {name} row {b}: {float(got)!r} vs {float(want)!r}, {ulp:.2f} ulp")
            assert ulp <= 1.0, f"{row.id} {name} row {b} (after the divisors call): {float(got)!r}, the fp32 of the exact mean is {float(want)!r} ({ulp:.2f} ulp)"
    return worst
