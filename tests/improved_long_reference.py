"""The reference and the checkers of tests/test_gpu_improved_long.py; importable without a device
(tests/test_improved_long_cpu.py runs all of it on the CPU).

Improved FullSubNet under the reference's norms divides by one mean per utterance in front of the full-band model and by one
per section in front of the sections (model.py:124-150, 402-440, 565-567), so a recording in segments takes three passes
(include/fsn_hip.h, fsn_improved_segment_*).  Here they are as three stateful functions over the state dict of
improved_stream_reference.new_state, built from that file's pieces (`compress`, `_block`, `_cumulative`, `wrap`) with the
arithmetic switches of its `step` (dtype fp64 / fp32, act "torch" / "cell"):

  `stats`     mag [U, F, k] -> every frame's sum of mag ** fdrc over the first F - 1 bins joins st["fb_sum"], in frame order
  `fullband`  comp / den_fb (fb_norm "offline": the finished mean; "cumulative": the running one, carried here) through the
              full-band block from the carried (h, c) -> fb [U, F - 1, k]; every section's sum over all units and window
              columns of the noisy AND the fb windows joins st["sb_sum"][i]
  `sections`  every section's windows / den_sb[i] through the sections' blocks from their carried (h, c) -> mask [U, 2, F, k]
  `run`       the passes over a split of the frames

total[b] = T_b is row b's own frame count: a frame at or past it adds nothing to a sum and its compressed magnitude counts
as zero (whatever `mag` holds there); what the blocks make of it is finite and never compared.
tests/test_improved_long_cpu.py holds `run` in fp64 to improved_stream_reference.forward of each row alone to 1e-12 in every
segmentation.  `WRONG` lists deliberately wrong stand-ins, each of which the checkers below must catch.

The checkers follow improved_stream_reference's rule (iv) and are its own functions on a `Ref` of the three runs ("64" the
truth, "c32" the yardstick, "t32" logged beside it): `check_mask` (the device mask against fp64 at SHARP x the c32 run's
error per whole tensor, per frame and per 16-row tile, over each row's own frames), `check_state` ((h, c) at SHARP x the c32
state error, the fp64 sums by the bound of an fp64 sum) and `check_divisors` (one fp32 ulp of the fp64 value)."""
import collections
import functools

import numpy as np

import improved_stream_reference as R
from oracle import fullsubnet_oracle as O
from oracle import model_family_oracle as MF

WRONG = ("section-sum-restarts-per-segment", "divisor-over-the-longest-row", "section-sum-over-noisy-windows-only",
         "frames-past-the-end-counted", "fullband-state-reset-per-segment", "mirror-off-by-one-at-the-top")

Result = collections.namedtuple("Result", "mask fb den_fb den_sb state")


def ragged_mag(totals, cfg, seed):
    """[U, F, max(totals)]: random over every frame - what lies past a row's T_b = totals[b] frames must not matter."""
    return R.make_mag(len(totals), cfg.F, max(totals), seed)


def inside(t0, k, total):
    """[U, k]: whether frame t0 + t lies inside row b."""
    return (t0 + np.arange(k))[None, :] < np.asarray(total)[:, None]


def comp_of(mag, t0, total, cfg, dtype, wrong=None):
    """mag ** fdrc without the last bin, zero past each row's end: [U, F - 1, k]."""
    c = R.compress(mag, cfg, dtype)
    if wrong != "frames-past-the-end-counted":
        c = np.where(inside(t0, mag.shape[-1], total)[:, None, :], c, dtype(0))
    return np.ascontiguousarray(c.astype(dtype))


def per_frame_entries(cfg):
    return np.array([n * w for n, w in zip(R.num_units(cfg), R.widths(cfg))], dtype=np.float64)


def divisors(st, total, cfg, dtype, wrong=None):
    """(den_fb [U], den_sb [sections, U]) from the sums: float(sum / count) + fp32 epsilon in `dtype`."""
    tot = np.maximum(np.asarray(total, dtype=np.float64), 1.0)
    if wrong == "divisor-over-the-longest-row":
        tot = np.full_like(tot, tot.max())
    eps = dtype(O.EPSILON)
    den_fb = (st["fb_sum"] / (float(cfg.F - 1) * tot)).astype(dtype) + eps
    den_sb = (st["sb_sum"] / (per_frame_entries(cfg)[:, None] * tot[None, :])).astype(dtype) + eps
    return den_fb.astype(dtype), den_sb.astype(dtype)


def stats(st, mag, t0, total, cfg, dtype, wrong=None):
    c = comp_of(mag, t0, total, cfg, dtype, wrong)
    for t in range(c.shape[-1]):
        st["fb_sum"] = st["fb_sum"] + c[..., t].sum(axis=1, dtype=np.float64)


def _unfold(wrong):
    return R._unfold_top_off_by_one if wrong == "mirror-off-by-one-at-the-top" else MF.banded_unfold


def fullband(st, mag, t0, total, params, cfg, dtype, act, fb_norm="offline", wrong=None):
    U, _, k = mag.shape
    Fm = cfg.F - 1
    comp = comp_of(mag, t0, total, cfg, dtype, wrong)
    if fb_norm == "offline":
        fb_in = (comp / divisors(st, total, cfg, dtype, wrong)[0][:, None, None]).astype(dtype)
    else:  # the running mean of improved_stream_reference.step: a frame past the end adds zeros
        fb_in, st["fb_sum"] = R._cumulative(comp, st["fb_sum"], Fm * t0, Fm)
    if wrong == "fullband-state-reset-per-segment":
        st["fb"] = R.new_state(U, cfg)["fb"]
    fb = np.ascontiguousarray(R._block(fb_in, params, "fb_model", 2, True, False, dtype, act, st["fb"]))  # [U, Fm, k]
    sums = np.array(st["sb_sum"], dtype=np.float64)
    if wrong == "section-sum-restarts-per-segment":
        sums[:] = 0.0
    counted = inside(t0, k, total) | (wrong == "frames-past-the-end-counted")
    for i, (lower, upper) in enumerate(R.bands(cfg)):
        s = _unfold(wrong)(comp[:, None], lower, upper, cfg.centers[i], cfg.sb_n[i])
        if wrong != "section-sum-over-noisy-windows-only":
            s = np.concatenate([s, _unfold(wrong)(fb[:, None], lower, upper, cfg.centers[i], cfg.fb_n[i])], axis=-2)
        frame_sum = np.where(counted, s.reshape(U, -1, k).sum(axis=1, dtype=np.float64), 0.0)
        for t in range(k):  # frame order
            sums[i] = sums[i] + frame_sum[:, t]
    st["sb_sum"], st["steps"] = sums, t0 + k
    return fb


def sections(st, mag, fb, t0, total, params, cfg, dtype, act, wrong=None):
    U, _, k = mag.shape
    comp = comp_of(mag, t0, total, cfg, dtype, wrong)
    den = divisors(st, total, cfg, dtype, wrong)[1]
    parts = []
    for i, (lower, upper) in enumerate(R.bands(cfg)):
        c, N, W = cfg.centers[i], R.num_units(cfg)[i], R.widths(cfg)[i]
        a = _unfold(wrong)(comp[:, None], lower, upper, c, cfg.sb_n[i])
        b = _unfold(wrong)(np.ascontiguousarray(np.asarray(fb, dtype=dtype))[:, None], lower, upper, c, cfg.fb_n[i])
        s = (np.concatenate([a, b], axis=-2).reshape(U, N * W, k) / den[i][:, None, None]).astype(dtype)
        o = R._block(s.reshape(U * N, W, k), params, f"sb_model.sb_models.{i}", 2, True, False, dtype, act, st["sb"][i])
        parts.append(R.wrap(o, U, N))
    mask = np.concatenate(parts, axis=-2)
    return np.ascontiguousarray(np.concatenate([mask, np.zeros_like(mask[:, :, -1:])], axis=-2))


def run(mag, total, params, cfg, split, norm="offline", dtype=np.float64, act="torch", wrong=None):
    """The passes over the calls `split` (sum(split) = max(total) frames) on mag [U, F, max(total)] with `norm` = "offline" /
    "cumulative" in front of the full-band model (the sections' norm is offline) -> Result: the mask [U, 2, F, frames], the
    full-band output [U, F - 1, frames], the divisors, the final state."""
    assert wrong is None or wrong in WRONG
    assert sum(split) == max(total) == mag.shape[-1]
    st = R.new_state(mag.shape[0], cfg)
    edges = np.concatenate([[0], np.cumsum(split)])
    calls = [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
    if norm == "offline":
        for a, b in calls:
            stats(st, mag[..., a:b], a, total, cfg, dtype, wrong)
    fb = np.concatenate([fullband(st, mag[..., a:b], a, total, params, cfg, dtype, act, norm, wrong) for a, b in calls], axis=-1)
    den_fb, den_sb = divisors(st, total, cfg, dtype, wrong)
    mask = np.concatenate([sections(st, mag[..., a:b], fb[..., a:b], a, total, params, cfg, dtype, act, wrong) for a, b in calls],
                          axis=-1)
    return Result(mask, fb, den_fb, den_sb, st)


def rows_alone(mag, total, params, cfg, norm="offline", dtype=np.float64):
    """improved_stream_reference.forward (the sections' norm offline) of each row alone over its own T_b frames: a list of
    [2, F, T_b]."""
    return [R.forward(mag[b:b + 1, :, :n], params, cfg, norm, "offline", dtype)[0] for b, n in enumerate(total)]


def trim(mask, total):
    """A copy of mask [U, 2, F, >= max T_b] with everything past each row's end zero: what is compared."""
    out = np.array(mask[..., :max(total)], copy=True)
    for b, n in enumerate(total):
        out[b, ..., n:] = 0
    return out


# ---- the reference of a case and the checkers ---------------------------------------------------------------------------------

class Case:
    """What improved_stream_reference's checkers read of a table row."""

    def __init__(self, why, cfg, total, norm="offline"):
        self.why, self.cfg, self.total, self.norm = why, cfg, tuple(int(n) for n in total), norm
        self.B, self.T = len(self.total), max(self.total)
        self.id = f"{why}-B{self.B}-F{cfg.F}-{len(cfg.centers)}sec-{norm}-T" + "_".join(map(str, self.total))


class Ref:
    """The case's recording in the three runs, each in one segment (no run depends on its segments): mask[m] = [the trimmed
    mask], state[m], and the fp64 run's Result."""

    def __init__(self, case, mag, params=None):
        cfg = case.cfg
        self.cfg, self.mag = cfg, np.asarray(mag, dtype=np.float32)
        self.params = R.make_params(cfg) if params is None else params
        self.state0 = R.new_state(case.B, cfg)
        self.mask, self.state, self.result = {}, {}, {}
        for m, dtype, act in (("64", np.float64, "torch"), ("c32", np.float32, "cell"), ("t32", np.float32, "torch")):
            r = run(self.mag, case.total, self.params, cfg, (case.T,), case.norm, dtype, act)
            self.mask[m], self.state[m], self.result[m] = [trim(r.mask, case.total)], r.state, r


@functools.lru_cache(maxsize=8)
def reference_of(why, cfg, total, norm="offline", seed=7):
    case = Case(why, cfg, total, norm)
    return case, Ref(case, ragged_mag(case.total, cfg, seed))


def check_mask(case, ref, mask, log=print):
    """mask [U, 2, F, >= T]: finite over each row's own frames, the last bin an exact zero, and within the rule of the fp64
    run.  Returns the worst (Frobenius, max, tile) ratios."""
    mask = np.asarray(mask)
    for b, n in enumerate(case.total):
        assert np.isfinite(mask[b, ..., :n]).all(), f"{case.id} mask row {b}: not finite"
    return R.check_calls(case, ref, [trim(mask, case.total)], log=log)


def check_state(case, ref, state, log=print):
    """state: a dict as new_state lays it out (the final one: every row has run to the longest row's end).  (h, c) and the
    step count by improved_stream_reference.check_state, the sums by `check_sums` below."""
    bare = dict(state, fb_sum=ref.state["64"]["fb_sum"], sb_sum=ref.state["64"]["sb_sum"])  # the sums are held below
    worst = R.check_state(case, ref, bare, log=log, after="the last segment")
    worst.update(check_sums(case, ref, state, log))
    return worst


def check_sums(case, ref, state, log=print):
    """improved_stream_reference.check_sums with every row's own term count: row b's sums have T_b frames' terms, not the
    longest row's.
      fb_sum[b]     T_b (F - 1) non-negative fp32 terms in an fp64 sum: (terms + 2) 2^-53 of the sum for its rounding, whatever
                    the order, and 2 x 2^-24 of it for the fp32 square roots (exact terms under fdrc 1 keep the allowance);
      sb_sum[i][b]  T_b N_i W_i terms, among them the full-band block's fp32 outputs, which have no bound of that kind: the
                    array is held at SHARP x the c32 run's own error in the Frobenius norm, plus the rounding of every
                    element's own fp64 sum."""
    cfg, out = case.cfg, {}
    tot = np.asarray(case.total, dtype=np.float64)
    r, g = ref.state["64"]["fb_sum"], np.asarray(state["fb_sum"], dtype=np.float64)
    assert g.shape == r.shape, f"{case.id} fb_sum: shape {g.shape}, expected {r.shape}"
    err = np.abs(g - r)
    bound = (tot * (cfg.F - 1) + 2) * R.U53 * np.abs(r) + 2.0 * 2.0 ** -24 * r
    out["fb_sum"] = float((err / bound).max())
    log(f"[ilong] {case.id} fb_sum: error {err.max():.3e}, {out['fb_sum']:.3f} of its bound")
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (f"{case.id} fb_sum: row {tuple(bad[0])} carries {g[tuple(bad[0])]!r}, the fp64 run {r[tuple(bad[0])]!r}: "
                           f"{err[tuple(bad[0])]:.3e} apart, the bound is {bound[tuple(bad[0])]:.3e}")
    r, y, g = ref.state["64"]["sb_sum"], ref.state["c32"]["sb_sum"], np.asarray(state["sb_sum"], dtype=np.float64)
    assert g.shape == r.shape, f"{case.id} sb_sum: shape {g.shape}, expected {r.shape}"
    terms = per_frame_entries(cfg)[:, None] * tot[None, :]
    rounding = float(np.sqrt((((terms + 2) * R.U53 * r) ** 2).sum()))
    eg, ey = float(np.sqrt(((g - r) ** 2).sum())), float(np.sqrt(((y - r) ** 2).sum()))
    out["sb_sum"] = eg / (R.SHARP * ey + rounding)
    log(f"[ilong] {case.id} sb_sum: error {eg:.3e} against {ey:.3e} of the c32 run ({out['sb_sum']:.3f} of its bound)")
    assert eg <= R.SHARP * ey + rounding, (f"{case.id} sb_sum: {eg:.3e} from the fp64 run's in the Frobenius norm, the fp32 cell "
                                           f"emulation {ey:.3e} (allowed {R.SHARP:g} x + {rounding:.1e} of rounding)")
    return out


def expected_divisors(state, total, cfg):
    """float32(float32(sum / count) + eps) with the quotient formed in fp64 from the sums `state` carries."""
    return divisors(state, total, cfg, np.float32)


def check_divisors(den_fb, den_sb, state, total, cfg, log=print):
    """Each divisor within one fp32 ulp of expected_divisors.  Returns the worst distance in ulps."""
    worst = 0.0
    for name, got, want in zip(("den_fb", "den_sb"), (den_fb, den_sb), expected_divisors(state, total, cfg)):
        got = np.asarray(got, dtype=np.float32)
        assert got.shape == want.shape, f"{name}: shape {got.shape}, expected {want.shape}"
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(want).astype(np.float64)
        log(f"[ilong] {name} at totals {tuple(total)}: worst {ulps.max():.2f} ulp")
        assert ulps.max() <= 1.0, f"{name} at totals {tuple(total)}: {got!r}, expected {want!r} ({ulps.max():.1f} ulp apart)"
        worst = max(worst, float(ulps.max()))
    return worst
