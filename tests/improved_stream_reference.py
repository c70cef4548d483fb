"""The reference, the table and the checkers of tests/test_gpu_improved_stream.py; importable without a device
(tests/test_improved_stream_cpu.py runs all of it on the CPU).

fsn_improved_stream_step hands back the mask of k more frames of Improved FullSubNet (no look-ahead) under the cumulative
norm in front of the full-band model and of every band section.  The reference is built from the oracle's pieces -
model_family_oracle.banded_unfold / sequence_block and the norms:

  (i)   `forward`: the whole-sequence model from the magnitudes to the mask, with both norms as arguments.  Under the
        reference's norms (offline, eps = fp32 epsilon, in both places) it is model_family_oracle.improved_fullsubnet_forward
        operation for operation (that one is held to the reference's goldens).  The sections' cumulative norm is the one the
        issue defines: cumulative_laplace_norm of the section input [B, N, 1, W, T] seen as [B, 1, N W, T];
  (ii)  `step`: the stateful form over the fields of the device's state blob.  tests/test_improved_stream_cpu.py holds it,
        in every chunking of the table, to (i) under the cumulative norms to 1e-12;
  (iii) `TABLE`: the GPU rows;
  (iv)  the checkers, by the rule of tests/stream_reference.py and tests/fast_stream_reference.py.  Three runs of `step`:
        fp64 with torch's activations (the reference), fp32 with lstm_cell.h's formulas and every product summed in k order
        as the device sums it ("c32": the yardstick) and fp32 with torch's activations and BLAS products ("t32": logged
        beside it).  A device mask's error against fp64 may be SHARP = 4 x the c32 run's own error - per whole tensor, per
        frame and per 16-row tile (check_tensor of the core sweep, on every call and on all calls together); carried (h, c)
        at 4 x the c32 run's own state error; the fp64 sums by the bound of an fp64 sum (`check_sums`).

State (`new_state`), U streams: "fb" [[h, c], [h, c]] of the two full-band layers [U, H_fb]; "sb"[i] the same of section i
[U N_i, H_sb]; fb_sum [U] and sb_sum [sections, U] (fp64); steps (one int: the streams run in lockstep).
"""
import collections
import functools
import math

import numpy as np

from fast_stream_reference import _block, _cumulative
from oracle import fullsubnet_oracle as O
from oracle import model_family_oracle as MF
from test_gpu_core_sweep import SHARP, check_tensor, frob

LONG = 100000  # steps of a long stream
U53 = 2.0 ** -53

Cfg = collections.namedtuple("Cfg", "F cuts centers sb_n fb_n fb_hidden sb_hidden fdrc")


def as_dict(cfg):
    """The constructor arguments of improved_fullsubnet.Model / the configuration dict of the oracle."""
    return dict(n_fft=2 * (cfg.F - 1), hop_length=cfg.F - 1, win_length=2 * (cfg.F - 1), fdrc=cfg.fdrc, num_freqs=cfg.F,
                freq_cutoffs=list(cfg.cuts), sb_num_center_freqs=list(cfg.centers), sb_num_neighbor_freqs=list(cfg.sb_n),
                fb_num_center_freqs=list(cfg.centers), fb_num_neighbor_freqs=list(cfg.fb_n), fb_hidden_size=cfg.fb_hidden,
                sb_hidden_size=cfg.sb_hidden)


def of_dict(d):
    assert d["sb_num_center_freqs"] == d["fb_num_center_freqs"]
    return Cfg(d["num_freqs"], tuple(d["freq_cutoffs"]), tuple(d["sb_num_center_freqs"]), tuple(d["sb_num_neighbor_freqs"]),
               tuple(d["fb_num_neighbor_freqs"]), d["fb_hidden_size"], d["sb_hidden_size"], d["fdrc"])


def bands(cfg):
    """(lower, upper) of every section on the F - 1 bins the model runs on."""
    edges = (0, *cfg.cuts, cfg.F - 1)
    return list(zip(edges[:-1], edges[1:]))


def num_units(cfg):
    return [(hi - lo) // c for (lo, hi), c in zip(bands(cfg), cfg.centers)]


def widths(cfg):
    return [2 * c + 2 * sn + 2 * fn for c, sn, fn in zip(cfg.centers, cfg.sb_n, cfg.fb_n)]


def make_params(cfg, seed=3):
    return MF.make_improved_params(as_dict(cfg), seed=seed)


def make_mag(U, F, T, seed):
    rng = np.random.default_rng(seed)
    return (np.abs(rng.standard_normal((U, F, T))) + 0.05).astype(np.float32)


def compress(mag, cfg, dtype):
    """model.py:565-566: mag ** fdrc without the last bin, [U, F, k] -> [U, F - 1, k] (0.5 is a square root on the device and
    in torch.pow)."""
    x = np.asarray(mag, dtype=dtype)[:, :-1]
    return np.sqrt(x) if cfg.fdrc == 0.5 else x if cfg.fdrc == 1.0 else (x ** dtype(cfg.fdrc)).astype(dtype)


def wrap(o, U, N):
    """[U N, 2 c, T] of a section's block -> [U, 2, N c, T] (SubBandSequenceWrapper.forward, model.py:238-245)."""
    T = o.shape[-1]
    return o.reshape(U, N, 2, -1, T).transpose(0, 2, 1, 3, 4).reshape(U, 2, -1, T)


# ---- (i) the whole-sequence model -----------------------------------------------------------------------------------------

def section_cumulative(s, dtype):
    """The issue's definition: [B, N, 1, W, T] through the reference's cumulative_laplace_norm as [B, 1, N W, T]."""
    B, N, _, W, T = s.shape
    return O.cumulative_laplace_norm(s.reshape(B, 1, N * W, T), dtype).reshape(B, N, 1, W, T)


def forward(mag, params, cfg, norm, sb_norm, dtype=np.float32):
    """improved_fullsubnet/model.py:565-575 between the transforms, with `norm` / `sb_norm` = "offline" / "cumulative" in
    front of the full-band model / the sections: mag [B, F, T] -> the mask [B, 2, F, T], last bin zero."""
    fb_norm = {"offline": MF._norm_eps32, "cumulative": O.cumulative_laplace_norm}[norm]
    sec_norm = {"offline": MF._norm_eps32, "cumulative": section_cumulative}[sb_norm]
    x = (np.asarray(mag, dtype=dtype)[:, None] ** dtype(cfg.fdrc)).astype(dtype)[:, :, :-1, :]
    B, _, Fm, T = x.shape
    fb = MF.sequence_block(fb_norm(x, dtype).reshape(B, Fm, T), params, "fb_model", 2, True, None, dtype).reshape(B, 1, Fm, T)
    sections = []
    for i, (lower, upper) in enumerate(bands(cfg)):
        a = MF.banded_unfold(x, lower, upper, cfg.centers[i], cfg.sb_n[i])
        b = MF.banded_unfold(fb, lower, upper, cfg.centers[i], cfg.fb_n[i])
        s = sec_norm(np.concatenate([a, b], axis=-2), dtype)
        N, K = s.shape[1], s.shape[3]
        o = MF.sequence_block(s.reshape(B * N, K, T), params, f"sb_model.sb_models.{i}", 2, True, None, dtype)
        sections.append(o.reshape(B, N, 2, -1, T).transpose(0, 2, 1, 3, 4).reshape(B, 2, -1, T))
    crm = np.concatenate(sections, axis=-2)
    return np.pad(crm, [(0, 0), (0, 0), (0, 1), (0, 0)])


# ---- (ii) the stateful step -----------------------------------------------------------------------------------------------

def new_state(U, cfg):
    z = lambda *s: np.zeros(s, dtype=np.float32)  # noqa: E731
    return dict(fb=[[z(U, cfg.fb_hidden), z(U, cfg.fb_hidden)] for _ in range(2)],
                sb=[[[z(U * n, cfg.sb_hidden), z(U * n, cfg.sb_hidden)] for _ in range(2)] for n in num_units(cfg)],
                fb_sum=np.zeros(U), sb_sum=np.zeros((len(cfg.centers), U)), steps=0)


def blocks(st):
    """(name, [[h, c], [h, c]]) of every block of a state."""
    return [("fb", st["fb"])] + [(f"sb{i}", hcs) for i, hcs in enumerate(st["sb"])]


def random_state(U, cfg, steps, level, seed):
    """A state no short history reaches: h uniform in (-0.9, 0.9), c in (-2, 2), the sums of `steps` steps at the inputs'
    level - fp32 values in (h, c), so that every run starts from the same numbers."""
    rng = np.random.default_rng(seed)
    st = new_state(U, cfg)
    for _, hcs in blocks(st):
        for hc in hcs:
            hc[0] = rng.uniform(-0.9, 0.9, hc[0].shape).astype(np.float32)
            hc[1] = rng.uniform(-2.0, 2.0, hc[1].shape).astype(np.float32)
    st["steps"] = int(steps)
    st["fb_sum"] = steps * float(cfg.F - 1) * level * (1.0 + 0.1 * rng.uniform(-1, 1, U))
    per_step = np.array([n * w for n, w in zip(num_units(cfg), widths(cfg))], dtype=np.float64)
    st["sb_sum"] = steps * per_step[:, None] * level * (1.0 + 0.1 * rng.uniform(-1, 1, (len(per_step), U)))
    return st


def copy_state(st):
    return dict(fb=[[a.copy() for a in hc] for hc in st["fb"]], sb=[[[a.copy() for a in hc] for hc in hcs] for hcs in st["sb"]],
                fb_sum=st["fb_sum"].copy(), sb_sum=st["sb_sum"].copy(), steps=st["steps"])


WRONG = ("section-sum-not-carried", "count-of-the-wrong-section", "reflection-off-by-one-at-the-top", "last-bin-not-zero",
         "unit-major-concat", "fullband-sum-not-carried", "count-from-the-call")
MASK_ONLY = ("last-bin-not-zero", "unit-major-concat")  # mistakes in the mask's assembly: no state field can show them


def _unfold_top_off_by_one(x, lower, upper, centers, neighbors):
    """banded_unfold with the mirror at the top of the spectrum one bin off (the edge bin repeated)."""
    B, _, F, T = x.shape
    units = (upper - lower) // centers
    out = np.empty((B, units, 1, centers + 2 * neighbors, T), dtype=x.dtype)
    for u in range(units):
        for k in range(centers + 2 * neighbors):
            j = abs(lower + u * centers + k - neighbors)
            out[:, u, 0, k, :] = x[:, 0, 2 * (F - 1) - j + 1 if j > F - 1 else j, :]
    return out


def step(st, mag, params, cfg, dtype, act, wrong=None):
    """One call of the model step on `st` (updated in place): mag [U, F, k] -> mask [U, 2, F, k].  wrong: one of WRONG, the
    deliberately wrong stand-ins of the CPU self-test."""
    assert wrong is None or wrong in WRONG
    U, _, k = mag.shape
    Fm, t0 = cfg.F - 1, st["steps"]
    unfold = _unfold_top_off_by_one if wrong == "reflection-off-by-one-at-the-top" else MF.banded_unfold
    t_seen = 0 if wrong == "count-from-the-call" else t0
    comp = np.ascontiguousarray(compress(mag, cfg, dtype))
    fb_in, st["fb_sum"] = _cumulative(comp, 0.0 * st["fb_sum"] if wrong == "fullband-sum-not-carried" else st["fb_sum"], Fm * t_seen, Fm)
    fb = _block(fb_in, params, "fb_model", 2, True, False, dtype, act, st["fb"])  # [U, Fm, k]
    sums = np.array(st["sb_sum"], dtype=np.float64)
    per_step = [n * w for n, w in zip(num_units(cfg), widths(cfg))]
    parts = []
    for i, (lower, upper) in enumerate(bands(cfg)):
        c, N, W = cfg.centers[i], num_units(cfg)[i], widths(cfg)[i]
        a = unfold(comp[:, None], lower, upper, c, cfg.sb_n[i])
        b = unfold(np.ascontiguousarray(fb)[:, None], lower, upper, c, cfg.fb_n[i])
        s = np.concatenate([a, b], axis=-2).reshape(U, N * W, k)
        entries = per_step[(i + 1) % len(per_step)] if wrong == "count-of-the-wrong-section" else N * W
        run0 = 0.0 * sums[i] if wrong == "section-sum-not-carried" else sums[i]
        s, sums[i] = _cumulative(s, run0, entries * t_seen, entries)
        o = _block(s.reshape(U * N, W, k), params, f"sb_model.sb_models.{i}", 2, True, False, dtype, act, st["sb"][i])  # [U N, 2 c, k]
        parts.append(o.reshape(U, 2, N * c, k) if wrong == "unit-major-concat" else wrap(o, U, N))
    st["sb_sum"], st["steps"] = sums, t0 + k
    mask = np.concatenate(parts, axis=-2)
    last = mask[:, :, -1:] if wrong == "last-bin-not-zero" else np.zeros_like(mask[:, :, -1:])
    return np.ascontiguousarray(np.concatenate([mask, last], axis=-2))


def run_chunked(mag, params, cfg, split, dtype, act, state0=None, wrong=None):
    """The calls `split` of `step` on mag [U, F, sum(split)] -> ([mask per call], final state)."""
    st = copy_state(state0) if state0 is not None else new_state(mag.shape[0], cfg)
    edges = np.concatenate([[0], np.cumsum(split)])
    return [step(st, mag[..., a:b], params, cfg, dtype, act, wrong) for a, b in zip(edges[:-1], edges[1:])], st


# ---- (iii) the table ------------------------------------------------------------------------------------------------------

# 33 bins (32 used): 8 + 4 + 4 units per stream, windows of 14 columns; fb hidden 64 / 128 and sb hidden 64 are the smallest
# the stateful layer entry runs unpadded
SMALL = Cfg(33, (8, 16), (1, 2, 4), (3, 3, 3), (3, 3, 3), 64, 64, 0.5)
SMALL_FDRC1 = SMALL._replace(fb_hidden=128, fdrc=1.0)
OTHER_NEIGHBOURS = SMALL._replace(sb_n=(3, 2, 1), fb_n=(1, 3, 2))  # sb / fb neighbour counts differ: windows of 10, 14, 14
TWO_SECTIONS = Cfg(33, (8,), (1, 4), (3, 3), (3, 3), 64, 64, 0.5)   # 8 + 6 units
K48 = of_dict(MF.IMPROVED_48K)  # 481 bins, 512 / 384 units, 20 + 25 + 6 + 4 units per stream
K16 = of_dict(MF.IMPROVED_16K)  # 257 bins, 20 + 15 + 22 units per stream
ONES = (1,) * 7


class Row:
    def __init__(self, why, B, cfg, split, resumed=None):
        self.why, self.B, self.cfg, self.split, self.resumed = why, B, cfg, tuple(split), resumed
        self.T = sum(self.split)

    @property
    def id(self):
        c = self.cfg
        return (f"{self.why}-B{self.B}-F{c.F}-{len(c.centers)}sec-h{c.fb_hidden}_{c.sb_hidden}-fdrc{c.fdrc:g}-" + "_".join(map(str, self.split)) +
                (f"-from{self.resumed}" if self.resumed is not None else ""))


def _table():
    return [
        Row("frame-by-frame", 1, SMALL, ONES),               # the production regime; 8 / 4 / 4 rows: every tile is mostly padding
        Row("mixed", 3, SMALL, (3, 4)),                      # 24 / 12 / 12 rows: section 0 crosses a tile
        Row("one-call", 17, SMALL, (7,)),                    # 136 / 68 / 68 rows: several tiles per section, each with padding
        Row("fdrc-1", 3, SMALL_FDRC1, (2, 1, 1, 2, 1)),      # no square root, fb hidden 128
        Row("fdrc-1-ones", 17, SMALL_FDRC1, ONES),
        Row("other-neighbours", 17, OTHER_NEIGHBOURS, (3, 4)),
        Row("other-neighbours-ones", 1, OTHER_NEIGHBOURS, ONES),
        Row("two-sections", 3, TWO_SECTIONS, (1, 2, 1, 2, 1)),
        Row("long", 3, SMALL, (3, 4), resumed=LONG),         # the sums and the divisors' counts at 100 000 steps
        Row("many-rows", 128, SMALL, (2, 1)),                # 1024 rows = 64 row tiles in section 0: the per-section launch is another
                                                             # step kernel there, and a call with such a section runs the chains
        Row("shipped-48k", 2, K48, (1, 2, 3)),               # the 48 kHz configuration: 40 / 50 / 12 / 8 rows
        Row("bins-257", 1, K16, (2, 1)),                     # the 16 kHz bins: 20 / 15 / 22 rows
    ]


TABLE = _table()


# ---- (iv) the reference of a row and the checkers ---------------------------------------------------------------------------

class Ref:
    """The row's calls on its B streams in the three runs: mask[m][call] [B, 2, F, k] and state[m] for m in "64", "c32",
    "t32"."""

    def __init__(self, B, cfg, split, resumed):
        self.cfg, self.split = cfg, split
        self.params = make_params(cfg)
        self.mag = make_mag(B, cfg.F, sum(split), seed=1000 * sum(split) + B)
        level = float(compress(self.mag, cfg, np.float64).mean())
        self.state0 = new_state(B, cfg) if resumed is None else random_state(B, cfg, resumed, level, seed=11)
        self.mask, self.state = {}, {}
        for m, dtype, act in (("64", np.float64, "torch"), ("c32", np.float32, "cell"), ("t32", np.float32, "torch")):
            self.mask[m], self.state[m] = run_chunked(self.mag, self.params, cfg, split, dtype, act, self.state0)


@functools.lru_cache(maxsize=4)
def _reference(B, cfg, split, resumed):
    return Ref(B, cfg, split, resumed)


def reference_of(row):
    return _reference(row.B, row.cfg, row.split, row.resumed)


def mask_rows(mask):
    """[U, 2, F, k] -> rows [U F, 2, k]."""
    U, _, F, k = mask.shape
    return np.ascontiguousarray(mask.transpose(0, 2, 1, 3)).reshape(U * F, 2, k)


def check_calls(row, ref, got, log=print):
    """got[call] [B, 2, F, k] against the fp64 step at SHARP x the fp32 yardstick run: every call on its own - whole tensor in
    the Frobenius norm and in the max error, per frame, per 16-row tile - then all calls together the same way; and the last
    bin an exact zero.  Returns the worst (Frobenius, max, tile) ratios."""
    worst = (0.0, 0.0, 0.0)
    parts = []
    for c, g in enumerate(got):
        g = np.asarray(g)
        assert g.shape == ref.mask["64"][c].shape, f"{row.id} mask call {c} : shape {g.shape}, expected {ref.mask['64'][c].shape}"
        assert not g[:, :, -1].any(), f"{row.id} mask call {c} : the last bin is not an exact zero"
        g, y, r, t = (mask_rows(np.asarray(a)) for a in (g, ref.mask["c32"][c], ref.mask["64"][c], ref.mask["t32"][c]))
        log(f"[isweep] {row.id} call {c}: yardsticks cell {frob(y.astype(np.float64), r):.3e} / torch {frob(t.astype(np.float64), r):.3e}")
        worst = tuple(max(a, b) for a, b in zip(worst, check_tensor(f"{row.id} mask call {c} ", g, y, r, log=log)))
        parts.append((g, y, r))
    if len(parts) > 1:
        worst = tuple(max(a, b) for a, b in zip(worst, check_tensor(f"{row.id} mask all calls", *(np.concatenate(p, axis=-1) for p in zip(*parts)), log=log)))
    return worst


def state_arrays(st):
    """The float fields of a state as {name: array}: h / c per block and layer."""
    out = {}
    for key, hcs in blocks(st):
        for l, (h, c) in enumerate(hcs):
            out[f"{key}_h{l}"], out[f"{key}_c{l}"] = h, c
    return out


def check_state(row, ref, got, log=print, after="the last call"):
    """got: a state dict as new_state lays it out.  h and c of every layer against the fp64 state at SHARP x the cell
    emulation's own state error (Frobenius, per array); the sums by `check_sums`; the step count where `got` carries one.
    Returns the worst ratios."""
    r64, c32 = state_arrays(ref.state["64"]), state_arrays(ref.state["c32"])
    worst = {}
    for name, g in state_arrays(got).items():
        g = np.asarray(g, dtype=np.float64)
        assert g.shape == r64[name].shape, f"{row.id} state {name}: shape {g.shape}, expected {r64[name].shape}"
        assert np.isfinite(g).all(), f"{row.id} state {name} after {after}: not finite"
        fg, fy = frob(g, r64[name]), frob(c32[name].astype(np.float64), r64[name])
        worst[name] = fg / fy if fy > 0 else float("inf") if fg > 0 else 0.0
        log(f"[isweep] {row.id} state {name} after {after}: frob hip {fg:.3e} yardstick {fy:.3e} ({worst[name]:.2f} x)")
        assert fg <= SHARP * fy, (f"{row.id} state {name} after {after}: Frobenius error {fg:.3e} of the device against {fy:.3e} of the fp32 "
                                  f"cell emulation on the CPU ({worst[name]:.2f} x, allowed {SHARP:g} x)")
    if got.get("steps") is not None:
        assert got["steps"] == ref.state["64"]["steps"], f"{row.id} after {after}: {got['steps']} steps, expected {ref.state['64']['steps']}"
    worst.update(check_sums(row, ref, got, log, after))
    return worst


def check_sums(row, ref, got, log=print, after="the last call"):
    """The carries are fp64 sums of non-negative fp32 terms on top of the fp64 start values.  Against the fp64 run's own sums
    the device may differ by the rounding of an fp64 sum - (terms + 2) 2^-53 sum, whatever the order - and by what its fp32
    terms differ from the fp64 run's:
      fb_sum   a term is the fp32 square root of an input (or the input itself: exact), within 2^-24 of the fp64 run's term
               where the root is correctly rounded; 2 x that much of the sum added in this row's calls is allowed;
      sb_sum   its terms are those values and the full-band block's outputs, fp32 results of an LSTM block with no bound of
               that kind: the array [sections, U] is held like any tensor, at SHARP x the c32 run's own error in the
               Frobenius norm."""
    out = {}
    cfg = row.cfg
    r, g = ref.state["64"]["fb_sum"], np.asarray(got["fb_sum"], dtype=np.float64)
    assert g.shape == r.shape, f"{row.id} fb_sum: shape {g.shape}, expected {r.shape}"
    err = np.abs(g - r)
    bound = (row.T * (cfg.F - 1) + 2) * U53 * np.abs(r) + 2.0 * 2.0 ** -24 * (r - ref.state0["fb_sum"])
    out["fb_sum"] = float((err / bound).max())
    log(f"[isweep] {row.id} fb_sum after {after}: error {err.max():.3e}, {out['fb_sum']:.3f} of its bound")
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (f"{row.id} fb_sum after {after}: stream {tuple(bad[0])} carries {g[tuple(bad[0])]!r}, the fp64 run "
                           f"{r[tuple(bad[0])]!r}: {err[tuple(bad[0])]:.3e} apart, the bound is {bound[tuple(bad[0])]:.3e}")
    r, y, g = ref.state["64"]["sb_sum"], ref.state["c32"]["sb_sum"], np.asarray(got["sb_sum"], dtype=np.float64)
    assert g.shape == r.shape, f"{row.id} sb_sum: shape {g.shape}, expected {r.shape}"
    terms = row.T * max(n * w for n, w in zip(num_units(cfg), widths(cfg)))
    rounding = (terms + 2) * U53 * float(np.sqrt((r * r).sum()))
    eg, ey = float(np.sqrt(((g - r) ** 2).sum())), float(np.sqrt(((y - r) ** 2).sum()))
    out["sb_sum"] = eg / (SHARP * ey + rounding)
    log(f"[isweep] {row.id} sb_sum after {after}: error {eg:.3e} against {ey:.3e} of the c32 run ({out['sb_sum']:.3f} of its bound)")
    assert eg <= SHARP * ey + rounding, (f"{row.id} sb_sum after {after}: {eg:.3e} from the fp64 run's in the Frobenius norm, the fp32 cell "
                                         f"emulation {ey:.3e} (allowed {SHARP:g} x + {rounding:.1e} of rounding)")
    return out


LEVEL = math.sqrt(0.05 + math.sqrt(2.0 / math.pi))  # about the level of the compressed inputs
