"""A bidirectional nn.LSTM / nn.GRU written out on the CPU, and the rows / checker of tests/test_gpu_birnn.py.

Reference: `lstm_layer` / `gru_layer` of tests/test_gpu_recurrent_sweep.py (the recurrences the unidirectional entries are held
to), run on x and on x.flip(0), the second result flipped back, the two concatenated: torch's output layout [T][N][2H].  Stacked
for blocks of several layers.  tests/test_birnn_cpu.py pins it to torch.nn.LSTM / nn.GRU(bidirectional=True) in fp64.

Checker: the sweep's, unchanged - `Stat`, `SHARP`, `yardstick_of`, the operand recipe of `make_operands` (one draw per
direction).  Gradients are named per direction (dw_ih_f, dw_ih_r, ...) so that the sweep's gate blocks apply to each.
"""
import torch

import test_gpu_recurrent_sweep as S


def bilayer(cell, x, wf, wr, act="torch"):
    """One bidirectional layer.  x [T][N][I]; wf / wr = (w_ih, w_hh, b_ih, b_hh) of the forward / reverse direction."""
    def run(xs, w):
        z = torch.zeros(xs.shape[1], w[1].shape[1], dtype=xs.dtype)
        return S.lstm_layer(xs, *w, z, z, act)[0] if cell == "lstm" else S.gru_layer(xs, *w, z, act)[0]
    return torch.cat((run(x, wf), run(x.flip(0), wr).flip(0)), -1)


def stack(cell, x, layers, act="torch"):
    """layers: [(wf, wr)] bottom up."""
    for wf, wr in layers:
        x = bilayer(cell, x, wf, wr, act)
    return x


class BiRow:
    """One line of the entry-level table of tests/test_gpu_birnn.py: a single bidirectional layer, forward with saves + BPTT."""

    def __init__(self, cell, T, N, I, H, gain=2.0, Hreal=None):
        self.cell, self.T, self.n, self.I, self.H, self.gain, self.Hreal = cell, T, N, I, H, gain, Hreal or H
        # the sweep's row of one direction: its operand recipe and its yardstick rule
        self.base = S.Row("bilayer", "step" if cell == "lstm" else "gru_step", "layer_train" if cell == "lstm" else "gru_train", T,
                          N // 16, I, S.ru16(I), H, gain=gain, Hreal=Hreal)

    @property
    def G(self):
        return 4 if self.cell == "lstm" else 3

    @property
    def id(self):
        return f"bi{self.cell}-T{self.T}-N{self.n}-I{self.I}-H{self.H}" + (f"-real{self.Hreal}" if self.Hreal != self.H else "") + \
            (f"-g{self.gain:g}" if self.gain != 2.0 else "")

    def draws(self):
        return max(1, -(-S.POOL_ELEMS // (self.G * self.H)))


def make_operands(row, draw):
    """fp32 operands: x [T][N][I], dy [T][N][2H] and the two directions' tensors, each direction one draw of the sweep's recipe
    (uniform +- gain / sqrt(H); units beyond Hreal all zero and their dy zero)."""
    a, b = S.make_operands(row.base, row.n, 2 * draw), S.make_operands(row.base, row.n, 2 * draw + 1)
    return dict(x=a["x"], dy=torch.cat((a["dy"], b["dy"]), -1), wf=a["layers"][0], wr=b["layers"][0])


def grad_names(cell):
    return ("dw_ih", "dw_hh", "db") if cell == "lstm" else ("dw_ih", "dw_hh", "db_ih", "db_hh")


def reference(row, ops, dtype, act="torch"):
    """y, dx and each direction's parameter gradients of sum(y * dy), in `dtype` on the CPU."""
    with torch.enable_grad():
        x = ops["x"].to(dtype).requires_grad_(True)
        wf, wr = ([p.to(dtype).requires_grad_(True) for p in ops[k]] for k in ("wf", "wr"))
        y = bilayer(row.cell, x, wf, wr, act)
        grads = torch.autograd.grad((y * ops["dy"].to(dtype)).sum(), [x] + wf + wr)
    out = {"y": y, "dx": grads[0]}
    for d, sfx in enumerate(("_f", "_r")):
        gw = grads[1 + 4 * d:5 + 4 * d]
        out["dw_ih" + sfx], out["dw_hh" + sfx] = gw[0], gw[1]
        if row.cell == "lstm":
            out["db" + sfx] = gw[2]
        else:
            out["db_ih" + sfx], out["db_hh" + sfx] = gw[2], gw[3]
    return {k: v.detach() for k, v in out.items()}


def check(row, stats, ops, outs, cpu32=None):
    """Accumulate `outs` (name -> CPU fp32 tensor) against the fp64 reference into `stats`, beside the two fp32 yardsticks
    (cpu32: the fp32 stand-in for torch's run; the written-out recurrence in fp32 when None)."""
    ref64 = reference(row, ops, torch.float64)
    cpu32 = reference(row, ops, torch.float32) if cpu32 is None else cpu32
    emu32 = reference(row, ops, torch.float32, act="cell")
    assert set(outs) == set(ref64), f"outputs {sorted(outs)} against the reference's {sorted(ref64)}"
    for k, v in outs.items():
        assert v.shape == ref64[k].shape, f"{k}: shape {tuple(v.shape)} against {tuple(ref64[k].shape)}"
        stats.setdefault(k, S.Stat(k)).add(row, v, cpu32[k], ref64[k], emu32[k])


def assert_stats(row, stats, log=print):
    """The sweep's rule: both statistics of the whole tensor and the Frobenius one of every block at most SHARP x those of the
    fp32 run yardstick_of chooses (the cell emulation for hidden outputs at I <= 48 and for gradients at T <= 2)."""
    for s in stats.values():
        rf, rm = s.ratios()
        lb, wb = s.worst_block()
        log(f"[birnn] {row.id} {s.name} [{S.yardstick_of(row, s.name)}]: frob hip {s.frob('hip'):.3e} cpu {s.frob('cpu'):.3e} "
            f"({rf:.2f} x) max hip {s.maxrel('hip'):.3e} cpu {s.maxrel('cpu'):.3e} ({rm:.2f} x) worst block {lb} {wb:.2f} x")
    for s in stats.values():
        s.assert_sharp(S.yardstick_of(row, s.name))


# ---- module level: SequenceModel(.., bidirectional=True) --------------------------------------------------------------------
def module_reference(cell, sd, x, num_layers, dy=None, dtype=torch.float64):
    """tanh(fc(stack(x))) of a bidirectional block from its state dict (torch's names), x [B][F][T] -> [B][O][T]; with dy also
    the gradient of sum(out * dy) for every parameter, by name."""
    with torch.set_grad_enabled(dy is not None):
        p = {k: v.detach().to("cpu", dtype).requires_grad_(dy is not None) for k, v in sd.items()}
        layers = [tuple([p[f"sequence_model.{n}_l{k}{sfx}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
                        for sfx in ("", "_reverse")) for k in range(num_layers)]
        h = stack(cell, x.to(dtype).permute(2, 0, 1), layers)
        out = torch.tanh(h @ p["fc_output_layer.weight"].t() + p["fc_output_layer.bias"]).permute(1, 2, 0)
        if dy is None:
            return out.detach(), None
        names = sorted(p)
        grads = torch.autograd.grad((out * dy.to(dtype)).sum(), [p[n] for n in names])
    return out.detach(), dict(zip(names, (g.detach() for g in grads)))


class ModuleRow:
    """What Stat / yardstick_of read of a row, for the module-level cases (input width 257: held to torch's fp32)."""

    def __init__(self, cell, T, I):
        self.cell, self.T, self.I = cell, T, I


def grad_key(name):
    """A parameter's gradient under a name the sweep's block rule reads: gate blocks for the rnn tensors, none for the fc."""
    return ("d" + name.split(".", 1)[1]) if name.startswith("sequence_model.") else name.replace(".", "_") + "_grad"
