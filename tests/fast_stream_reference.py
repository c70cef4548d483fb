"""The reference, the table and the checkers of tests/test_gpu_fast_stream.py; importable without a device
(tests/test_fast_stream_cpu.py runs all of it on the CPU).

fsn_fast_stream_step hands back EVERY model step of Fast FullSubNet (look-ahead 0 semantics; the caller matches step t to
frame t - look_ahead), so the reference is one step function, `step`: k more frames of the model on a state.  It is built
from the oracle's pieces - model_family_oracle.sequence_block / real_time_downsampling / real_time_upsampling,
fullsubnet_oracle.freq_unfold and the norms:

  (i)   `forward`: the whole-sequence model with the norm as an argument.  Under the offline norm it is
        model_family_oracle.fast_fullsubnet_forward operation for operation (that one is held to the reference's goldens);
  (ii)  `step`: the stateful form over the fields of the device's state blob.  tests/test_fast_stream_cpu.py holds it, in
        every chunking of the table, to (i) under the cumulative norm to 1e-12;
  (iii) `TABLE`: the GPU rows;
  (iv)  the checkers, by the rule of tests/stream_reference.py.  Three runs of `step`: fp64 with torch's activations (the
        reference), fp32 with lstm_cell.h's formulas and every product summed in k order as the device sums it
        (`kmatmul`; "c32": the yardstick - the device's arithmetic as far as the CPU restates it) and fp32 with torch's
        activations and BLAS products ("t32": logged beside it).  A device tensor's error
        against fp64 may be SHARP = 4 x the c32 run's own error - per whole tensor, per frame and per 16-row tile
        (check_tensor of the core sweep, its max-error form included, on every call and on all calls together); carried (h, c), the
        held bottleneck output and the open block's partial sum at 4 x the c32 run's own state error; the fp64 sums by the
        bound of an fp64 sum (`check_sums`).

State (`new_state`), per stream u: [h, c] of encoder.0 [U, 384], encoder.1 [U, 257], the bottleneck's layers [U 64, H],
decoder_lstm.0 / .1 [U, 512]; mel_sum [U] and unit_sum [U, 64] (fp64); partial [U, 64, W] (the open block's sum, added in
frame order, zero while no block is open); held [U, 64]; steps (one int: the streams run in lockstep).
"""
import collections
import functools
import math

import numpy as np
import torch

from oracle import fullsubnet_oracle as O
from oracle import model_family_oracle as MF
from test_gpu_core_sweep import ACTS, SHARP, check_tensor, frob, lstm_layer

LEVEL = 0.05 + math.sqrt(2.0 / math.pi)  # the mean of |N(0, 1)| + 0.05, the inputs' level (the stream sweep's)
LONG = 100000                            # steps of a long stream
U53 = 2.0 ** -53
M, F = 64, 257                           # the reference's literals
BLOCKS = (("enc0", "encoder.0", 1), ("enc1", "encoder.1", 1), ("bn", "bottleneck", None), ("dec0", "decoder_lstm.0", 1),
          ("dec1", "decoder_lstm.1", 1))

Cfg = collections.namedtuple("Cfg", "shrink la n_mel n_enc bn_hidden bn_layers", defaults=(2, 2, 5, 0, 384, 2))


def unit_width(cfg):
    return 2 * cfg.n_mel + 1 + 2 * cfg.n_enc + 1


def make_params(cfg, seed=3):
    """Random weights at the oracle's gains (fsn_synthetic.make_fast_params) and the HTK filterbank."""
    p = MF.make_fast_params(seed=seed, bottleneck_hidden=cfg.bn_hidden, bottleneck_layers=cfg.bn_layers, nn_noisy=cfg.n_mel, nn_enc=cfg.n_enc)
    p["mel_scale.fb"] = MF.melscale_fbanks().astype(np.float32)
    return p


def make_mag(U, T, seed):
    rng = np.random.default_rng(seed)
    return (np.abs(rng.standard_normal((U, 1, F, T))) + 0.05).astype(np.float32)


# ---- (i) the whole-sequence model -----------------------------------------------------------------------------------------

def units_of(mel, enc_out, cfg):
    """[B, 1, M, T] x 2 -> the unit tensor [B, M, W, T] (model.py:163-172)."""
    B, _, _, T = mel.shape
    nu = O.freq_unfold(mel, cfg.n_mel).reshape(B, M, 2 * cfg.n_mel + 1, T)
    eu = O.freq_unfold(enc_out, cfg.n_enc).reshape(B, M, 2 * cfg.n_enc + 1, T)
    return np.concatenate([nu, eu], axis=2)


def forward(mix_mag, params, cfg, norm, dtype=np.float32):
    """fast_fullsubnet/model.py:143-202 with `norm` = "offline" / "cumulative" (norm_type, a constructor option of the
    reference): mix_mag [B, 1, F, T] -> [B, 2, F, T]."""
    fn = {"offline": O.offline_laplace_norm, "cumulative": O.cumulative_laplace_norm}[norm]
    x = np.asarray(mix_mag, dtype=dtype)
    x = np.pad(x, [(0, 0), (0, 0), (0, 0), (0, cfg.la)])
    B, C, _, T = x.shape
    fb = np.asarray(params["mel_scale.fb"], dtype=dtype)
    mel = (x.transpose(0, 1, 3, 2) @ fb).transpose(0, 1, 3, 2).astype(dtype)  # [B, 1, M, T]
    enc_in = fn(mel, dtype).reshape(B, -1, T)
    e = MF.sequence_block(enc_in, params, "encoder.0", 1, False, None, dtype)
    e = MF.sequence_block(e, params, "encoder.1", 1, True, "ReLU", dtype)
    enc_out = e.reshape(B, C, -1, T)
    bn_in = units_of(mel, enc_out, cfg)
    K = bn_in.shape[2]
    bn_s = fn(MF.real_time_downsampling(bn_in, cfg.shrink), dtype)
    bn_s = bn_s.reshape(B * M, K, -1)
    bo = MF.sequence_block(bn_s, params, "bottleneck", cfg.bn_layers, True, "ReLU", dtype)
    bo = bo.reshape(B, M, 1, -1).transpose(0, 2, 1, 3)
    bn_out = MF.real_time_upsampling(bo, cfg.shrink, T)
    dec_in = np.concatenate([enc_out, bn_out], axis=2).reshape(B, -1, T)
    d = MF.sequence_block(dec_in, params, "decoder_lstm.0", 1, False, None, dtype)
    d = MF.sequence_block(d, params, "decoder_lstm.1", 1, True, None, dtype)
    return np.ascontiguousarray(d.reshape(B, 2, F, T)[..., cfg.la:])


# ---- (ii) the stateful step -----------------------------------------------------------------------------------------------

def hidden_sizes(cfg):
    return {"enc0": 384, "enc1": 257, "bn": cfg.bn_hidden, "dec0": 512, "dec1": 512}


def new_state(U, cfg):
    z = lambda *s: np.zeros(s, dtype=np.float32)  # noqa: E731
    st = {key: [[z(U * (M if key == "bn" else 1), H), z(U * (M if key == "bn" else 1), H)] for _ in range(cfg.bn_layers if key == "bn" else 1)]
          for key, H in hidden_sizes(cfg).items()}
    st.update(mel_sum=np.zeros(U), unit_sum=np.zeros((U, M)), partial=z(U, M, unit_width(cfg)), held=z(U, M), steps=0)
    return st


def open_frames(steps, shrink):
    """The frames of the open down-sampling block after `steps` steps (0: no block is open)."""
    return (steps - 1) % shrink if steps >= 1 else 0


def random_state(U, cfg, steps, level, seed):
    """A state no short history reaches: h uniform in (-0.9, 0.9), c in (-2, 2), the sums of `steps` steps at the inputs'
    level, the open block's sum of open_frames(steps) frames, a held output in (0, 1) - fp32 values, so that every run starts
    from the same numbers."""
    rng = np.random.default_rng(seed)
    st = new_state(U, cfg)
    for key in hidden_sizes(cfg):
        for hc in st[key]:
            hc[0] = rng.uniform(-0.9, 0.9, hc[0].shape).astype(np.float32)
            hc[1] = rng.uniform(-2.0, 2.0, hc[1].shape).astype(np.float32)
    W = unit_width(cfg)
    mel_level = float(level) * 4.0  # (about the filterbank's column sum)
    st["steps"] = int(steps)
    st["mel_sum"] = steps * float(M) * mel_level * (1.0 + 0.1 * rng.uniform(-1, 1, U))
    st["unit_sum"] = ((steps - 1) // cfg.shrink + 1) * float(W) * mel_level * (1.0 + 0.1 * rng.uniform(-1, 1, (U, M)))
    st["partial"] = (open_frames(steps, cfg.shrink) * mel_level * rng.uniform(0.5, 1.5, (U, M, W))).astype(np.float32)
    st["held"] = rng.uniform(0.0, 1.0, (U, M)).astype(np.float32)
    return st


def copy_state(st):
    return {k: [[a.copy() for a in hc] for hc in v] if isinstance(v, list) else (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def kmatmul(a, w, acc=None):
    """a [R, K] @ w [O, K]^T (+ acc) in fp32, summed in k order in blocks of 4: the order of the device's products, which are
    chains of 16 x 16 x 4 matrix-core instructions along k (fsn_common.h mfma16; the projection and output-layer GEMMs start the
    chain from zero, the recurrent step from the stored projection).  Not bit for bit the device's sum - the four products inside
    a block are summed as the BLAS pleases - but its error grows with K as the device's does, which a blocked BLAS sum's does not."""
    wt = w.t().contiguous()
    out = torch.zeros((a.shape[0], w.shape[0]), dtype=torch.float32) if acc is None else acc.clone()
    for k in range(0, a.shape[1], 4):
        out += a[:, k:k + 4] @ wt[k:k + 4]
    return out


def lstm_cell_run(x, w_ih, w_hh, b_ih, b_hh, h, c):
    """lstm_layer of the recurrent sweep with act="cell" and every product through kmatmul: x [T, N, I] -> (hseq, h, c)."""
    sig, tanh = ACTS["cell"]
    T, N, _ = x.shape
    gx = (kmatmul(x.reshape(T * N, -1), w_ih) + (b_ih + b_hh)).reshape(T, N, -1)
    ys = []
    for t in range(T):
        i, f, g, o = kmatmul(h, w_hh, gx[t]).chunk(4, -1)
        c = sig(f) * c + sig(i) * tanh(g)
        h = sig(o) * tanh(c)
        ys.append(h)
    return torch.stack(ys), h, c


def _block(x, params, prefix, layers, has_fc, relu, dtype, act, hcs):
    """SequenceModel.forward for k more frames from the state hcs = [[h, c] per layer] (replaced): x [N, I, k] -> [N, O, k].
    act = "cell" is the yardstick run: lstm_cell.h's formulas and the device's summation order (kmatmul)."""
    td = torch.float64 if dtype == np.float64 else torch.float32
    o = torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dtype).transpose(2, 0, 1)))
    for l in range(layers):
        g = lambda n: torch.from_numpy(np.asarray(params[f"{prefix}.sequence_model.{n}_l{l}"], dtype=dtype))  # noqa: E731
        h, c = (torch.from_numpy(np.asarray(a, dtype=dtype)).to(td) for a in hcs[l])
        if act == "cell":
            o, h, c = lstm_cell_run(o, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"), h, c)
        else:
            o, h, c = lstm_layer(o, g("weight_ih"), g("weight_hh"), g("bias_ih"), g("bias_hh"), h, c, act=act)
        hcs[l] = [h.numpy(), c.numpy()]
    if has_fc:
        w = torch.from_numpy(np.asarray(params[f"{prefix}.fc_output_layer.weight"], dtype=dtype))
        b = torch.from_numpy(np.asarray(params[f"{prefix}.fc_output_layer.bias"], dtype=dtype))
        o = (kmatmul(o.reshape(-1, o.shape[-1]), w).reshape(*o.shape[:-1], -1) if act == "cell" else o @ w.t()) + b
    return (torch.relu(o) if relu else o).numpy().transpose(1, 2, 0)


def _cumulative(x, run0, count0, per_step):
    """cumulative_laplace_norm of the oracle on x [n, C, k] continued from the running sums run0 [n] (fp64) of count0 values:
    step t is divided by the mean of the count0 + per_step (t + 1) values so far.  -> (normalised x, new sums)."""
    dtype = x.dtype.type
    run = np.asarray(run0, dtype=np.float64)[:, None] + np.cumsum(x.sum(axis=1, dtype=np.float64), axis=-1)
    count = float(count0) + float(per_step) * np.arange(1, x.shape[-1] + 1, dtype=np.float64)[None, :]
    mean = (run / count).astype(dtype)[:, None, :]
    return (x / (mean + dtype(O.EPSILON))).astype(dtype), run[:, -1].copy()


WRONG = ("short-block-in-sum", "upsampling-off-by-one", "count-W-j", "block-mean-of-the-call", "held-not-carried")


def step(st, mag, params, cfg, dtype, act, wrong=None):
    """One call of the model step on `st` (updated in place): mag [U, 1, F, k] -> crm [U, 2, F, k].  wrong: one of WRONG, the
    deliberately wrong stand-ins of the CPU self-test."""
    assert wrong is None or wrong in WRONG
    x = np.asarray(mag, dtype=dtype)
    U, _, _, k = x.shape
    s, W, t0 = cfg.shrink, unit_width(cfg), st["steps"]
    eps = dtype(O.EPSILON)
    fb = np.asarray(params["mel_scale.fb"], dtype=dtype)
    if act == "cell":
        rows = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 1, 3, 2))).reshape(-1, x.shape[2])
        mel = kmatmul(rows, torch.from_numpy(np.ascontiguousarray(fb.T))).numpy().reshape(U, 1, k, M).transpose(0, 1, 3, 2)
    else:
        mel = (x.transpose(0, 1, 3, 2) @ fb).transpose(0, 1, 3, 2).astype(dtype)  # [U, 1, M, k]
    enc_in, st["mel_sum"] = _cumulative(mel[:, 0], st["mel_sum"], M * t0, M)
    e = _block(enc_in, params, "encoder.0", 1, False, False, dtype, act, st["enc0"])
    e = _block(e, params, "encoder.1", 1, True, True, dtype, act, st["enc1"])  # [U, M, k]
    units = units_of(mel, e[:, None], cfg)  # [U, M, W, k]
    partial = np.asarray(st["partial"], dtype=dtype)
    held = np.asarray(st["held"], dtype=dtype)
    if wrong == "block-mean-of-the-call":
        partial, in_call = np.zeros_like(partial), 0
    if wrong == "held-not-carried":
        held = np.zeros_like(held)
    low = []
    for t in range(k):
        T = t0 + t
        partial = (partial + units[..., t]).astype(dtype)  # frame order
        if wrong == "block-mean-of-the-call":
            in_call += 1
        if T % s:
            continue
        n = in_call if wrong == "block-mean-of-the-call" else s
        v = (partial / dtype(n)).astype(dtype) if T > 0 and n > 1 else partial
        j = T // s
        st["unit_sum"] = st["unit_sum"] + v.sum(axis=2, dtype=np.float64)
        count = W * j if wrong == "count-W-j" and j > 0 else W * (j + 1)
        mean = (st["unit_sum"] / float(count)).astype(dtype)
        low.append((v / (mean[..., None] + eps)).astype(dtype))
        partial = np.zeros_like(partial)
        if wrong == "block-mean-of-the-call":
            in_call = 0
    if wrong == "short-block-in-sum" and open_frames(t0 + k, s):  # the call's end taken for the stream's: the short block's mean joins the sum
        st["unit_sum"] = st["unit_sum"] + (partial / dtype(open_frames(t0 + k, s))).sum(axis=2, dtype=np.float64)
    slow = None
    if low:
        bn_in = np.stack(low, axis=-1).reshape(U * M, W, len(low))
        slow = _block(bn_in, params, "bottleneck", cfg.bn_layers, True, True, dtype, act, st["bn"]).reshape(U, M, len(low))
    j0 = -(-t0 // s)  # the first low-rate frame that completes in this call
    gain = np.empty((U, M, k), dtype=dtype)
    for t in range(k):
        T = t0 + t - (1 if wrong == "upsampling-off-by-one" and t0 + t > 0 else 0)
        j = T // s - j0
        gain[..., t] = slow[..., j] if j >= 0 else held
    if low:
        held = slow[..., -1]
    dec_in = np.concatenate([e, gain], axis=1)
    d = _block(dec_in, params, "decoder_lstm.0", 1, False, False, dtype, act, st["dec0"])
    d = _block(d, params, "decoder_lstm.1", 1, True, False, dtype, act, st["dec1"])
    st["partial"], st["held"], st["steps"] = partial, np.ascontiguousarray(held), t0 + k
    return np.ascontiguousarray(d.reshape(U, 2, F, k))


def run_chunked(mag, params, cfg, split, dtype, act, state0=None, wrong=None):
    """The calls `split` of `step` on mag [U, 1, F, sum(split)] -> ([crm per call], final state)."""
    st = copy_state(state0) if state0 is not None else new_state(mag.shape[0], cfg)
    edges = np.concatenate([[0], np.cumsum(split)])
    return [step(st, mag[..., a:b], params, cfg, dtype, act, wrong) for a, b in zip(edges[:-1], edges[1:])], st


# ---- (iii) the table ------------------------------------------------------------------------------------------------------

SHIPPED = Cfg()
ONES = (1,) * 14
MIXED = (1, 2, 3, 5, 1, 4, 2, 3)  # 21 steps: calls begin at every phase of a block of 2, 3 or 4 and span several blocks


class Row:
    def __init__(self, why, B, cfg, split, resumed=None):
        self.why, self.B, self.cfg, self.split, self.resumed = why, B, cfg, tuple(split), resumed
        self.T = sum(self.split)
        assert 13 <= self.T <= 25

    @property
    def id(self):
        c = self.cfg
        return (f"{self.why}-B{self.B}-s{c.shrink}la{c.la}-n{c.n_mel}_{c.n_enc}-bn{c.bn_hidden}x{c.bn_layers}-" + "_".join(map(str, self.split)) +
                (f"-from{self.resumed}" if self.resumed is not None else ""))


def _table():
    small = dict(n_mel=2, n_enc=1, bn_hidden=128, bn_layers=1)
    return [
        Row("frame-by-frame", 1, SHIPPED, ONES),             # the production regime; at shrink 2 every other call has n_low = 0
        Row("mixed", 3, SHIPPED, MIXED),                     # 13 pad rows
        Row("one-call", 16, SHIPPED, (21,)),                 # exactly one row tile
        Row("second-tile", 17, SHIPPED, MIXED),              # a second row tile with 15 pad rows
        Row("no-down-sampling", 3, Cfg(shrink=1, la=0), MIXED),
        Row("no-down-sampling-ones", 1, Cfg(shrink=1, la=0, **small), ONES),
        Row("shrink3", 3, Cfg(shrink=3, la=1, **small), MIXED),
        Row("shrink3-ones", 1, Cfg(shrink=3, la=1), ONES),
        Row("shrink4", 17, Cfg(shrink=4, la=2, **small), MIXED),
        Row("shrink4-one-call", 1, Cfg(shrink=4, la=2, n_mel=2, n_enc=1), (21,)),
        Row("small-bottleneck", 3, Cfg(bn_hidden=128, bn_layers=1), MIXED),
        Row("bottleneck-256x2", 3, Cfg(bn_hidden=256, bn_layers=2), MIXED),
        Row("bottleneck-512x1", 1, Cfg(bn_hidden=512, bn_layers=1, n_mel=2, n_enc=1), ONES),
        Row("other-neighbours", 16, Cfg(n_mel=2, n_enc=1), ONES),
        Row("widest-window", 1, Cfg(n_mel=7, n_enc=7), MIXED),
        Row("long-open-block", 3, SHIPPED, (1, 3, 2, 5, 2), resumed=LONG),       # a block is open at 100 000 steps
        Row("long-closed-block", 3, SHIPPED, (1, 3, 2, 5, 2), resumed=LONG + 1),  # ... and whole at 100 001
    ]


TABLE = _table()


# ---- (iv) the reference of a row and the checkers ---------------------------------------------------------------------------

class Ref:
    """The row's calls on its B utterances in the three runs: crm[m][call] [B, 2, F, k] and state[m] for m in "64", "c32",
    "t32"; the exact sums of the fp64 run in extended precision."""

    def __init__(self, B, cfg, split, resumed):
        self.cfg, self.split = cfg, split
        self.params = make_params(cfg)
        self.mag = make_mag(B, sum(split), seed=1000 * sum(split) + B)
        level = self.mag.mean(dtype=np.float64)
        self.state0 = new_state(B, cfg) if resumed is None else random_state(B, cfg, resumed, level, seed=11)
        self.crm, self.state = {}, {}
        for m, dtype, act in (("64", np.float64, "torch"), ("c32", np.float32, "cell"), ("t32", np.float32, "torch")):
            self.crm[m], self.state[m] = run_chunked(self.mag, self.params, cfg, split, dtype, act, self.state0)


@functools.lru_cache(maxsize=4)
def _reference(B, cfg, split, resumed):
    return Ref(B, cfg, split, resumed)


def reference_of(row):
    return _reference(row.B, row.cfg, row.split, row.resumed)


def crm_rows(crm):
    """[U, 2, F, k] -> rows [U F, 2, k]."""
    U, _, _, k = crm.shape
    return np.ascontiguousarray(crm.transpose(0, 2, 1, 3)).reshape(U * F, 2, k)


def check_calls(row, ref, got_crm, log=print):
    """got_crm[call] [B, 2, F, k] against the fp64 step at SHARP x the fp32 yardstick run, as check_calls of
    tests/stream_reference.py holds FullSubNet's: every call on its own - whole tensor in the Frobenius norm and in the max
    error, per frame, per 16-row tile - then all calls together the same way.  Returns the worst (Frobenius, max, tile)
    ratios."""
    worst = (0.0, 0.0, 0.0)
    parts = []
    for c, got in enumerate(got_crm):
        g, y, r, t = (crm_rows(np.asarray(a)) for a in (got, ref.crm["c32"][c], ref.crm["64"][c], ref.crm["t32"][c]))
        log(f"[fsweep] {row.id} call {c}: yardsticks cell {frob(y.astype(np.float64), r):.3e} / torch {frob(t.astype(np.float64), r):.3e}")
        worst = tuple(max(a, b) for a, b in zip(worst, check_tensor(f"{row.id} crm call {c}", g, y, r, log=log)))
        parts.append((g, y, r))
    if len(parts) > 1:
        worst = tuple(max(a, b) for a, b in zip(worst, check_tensor(f"{row.id} crm all calls", *(np.concatenate(p, axis=-1) for p in zip(*parts)), log=log)))
    return worst


def state_arrays(st):
    """The float fields of a state as {name: array}: h / c per layer, held, partial."""
    out = {}
    for key, _, _ in BLOCKS:
        for l, (h, c) in enumerate(st[key]):
            out[f"{key}_h{l}"], out[f"{key}_c{l}"] = h, c
    out["held"], out["partial"] = st["held"], st["partial"]
    return out


def check_state(row, ref, got, log=print, after="the last call"):
    """got: a state dict as new_state lays it out.  h and c of every layer, the held output and the open block's partial sum
    against the fp64 state at SHARP x the cell emulation's own state error (Frobenius, per array); the two
    sums by `check_sums`.  The step count is no field of the device's blob - it is an argument of the entry, kept by the caller -
    so it is compared only where `got` carries one (the CPU runs); on the device it is held through what depends on it: the
    divisors' counts and the block phase decide every mask and both sums.  Returns the worst ratios."""
    r64, c32 = state_arrays(ref.state["64"]), state_arrays(ref.state["c32"])
    worst = {}
    for name, g in state_arrays(got).items():
        g = np.asarray(g, dtype=np.float64)
        assert g.shape == r64[name].shape, f"{row.id} state {name}: shape {g.shape}, expected {r64[name].shape}"
        assert np.isfinite(g).all(), f"{row.id} state {name} after {after}: not finite"
        fg, fy = frob(g, r64[name]), frob(c32[name].astype(np.float64), r64[name])
        worst[name] = fg / fy if fy > 0 else float("inf") if fg > 0 else 0.0
        log(f"[fsweep] {row.id} state {name} after {after}: frob hip {fg:.3e} yardstick {fy:.3e} ({worst[name]:.2f} x)")
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
      mel_sum   a term is an fp32 dot product of F non-negative products, which any summation order gets to (F + 2) 2^-24 of
                its value (products and additions round once each), so the terms added in this row's calls to that much of
                their sum;
      unit_sum  its terms are those mel values and encoder outputs, fp32 results of the LSTM blocks with no bound of that
                kind: the array [U, 64] is held like any tensor, at SHARP x the c32 run's own error in the Frobenius norm."""
    out = {}
    r, g = ref.state["64"]["mel_sum"], np.asarray(got["mel_sum"], dtype=np.float64)
    assert g.shape == r.shape, f"{row.id} mel_sum: shape {g.shape}, expected {r.shape}"
    err = np.abs(g - r)
    bound = (row.T * M + 2) * U53 * np.abs(r) + (F + 2) * 2.0 ** -24 * (r - ref.state0["mel_sum"])
    out["mel_sum"] = float((err / bound).max())
    log(f"[fsweep] {row.id} mel_sum after {after}: error {err.max():.3e}, {out['mel_sum']:.3f} of its bound")
    bad = np.argwhere(err > bound)
    assert bad.size == 0, (f"{row.id} mel_sum after {after}: stream {tuple(bad[0])} carries {g[tuple(bad[0])]!r}, the fp64 run "
                           f"{r[tuple(bad[0])]!r}: {err[tuple(bad[0])]:.3e} apart, the bound is {bound[tuple(bad[0])]:.3e}")
    r, y, g = ref.state["64"]["unit_sum"], ref.state["c32"]["unit_sum"], np.asarray(got["unit_sum"], dtype=np.float64)
    assert g.shape == r.shape, f"{row.id} unit_sum: shape {g.shape}, expected {r.shape}"
    rounding = (row.T * unit_width(row.cfg) + 2) * U53 * float(np.sqrt((r * r).sum()))
    eg, ey = float(np.sqrt(((g - r) ** 2).sum())), float(np.sqrt(((y - r) ** 2).sum()))
    out["unit_sum"] = eg / (SHARP * ey + rounding)
    log(f"[fsweep] {row.id} unit_sum after {after}: error {eg:.3e} against {ey:.3e} of the c32 run ({out['unit_sum']:.3f} of its bound)")
    assert eg <= SHARP * ey + rounding, (f"{row.id} unit_sum after {after}: {eg:.3e} from the fp64 run's in the Frobenius norm, the fp32 cell "
                                         f"emulation {ey:.3e} (allowed {SHARP:g} x + {rounding:.1e} of rounding)")
    return out
