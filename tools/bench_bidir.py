"""Time per bidirectional layer call, inference, T = 190: the one-launch-per-step entries (fsn_lstm_bilayer_forward /
fsn_gru_bilayer_forward, birnn_step_kernels.hip) against the composition the unidirectional entries offer - flip, two
fsn_*_layer_forward calls, flip back, concatenate.  The two forms alternate in one process, both are warmed, every window is at
least 0.5 s of calls ending in a synchronise, the composition is timed twice (its own spread) and the largest difference
between the two forms' outputs is printed.  Needs an MI355X.  usage: bench_bidir.py [--write]  (--write: profiles/bidir_layer.md)"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fullsubnet_amd  # noqa: E402,F401
from fullsubnet_amd import sequence_model as SM  # noqa: E402

T = 190
SHAPES = [(16, 257, 512, "few rows"), (64, 257, 512, "few rows"), (64, 1024, 512, "few rows"), (4096, 32, 384, "many rows")]
WINDOW_S = 0.5


def window(fn):
    """Mean time of a call in ms over a window of at least WINDOW_S seconds that ends in a synchronise."""
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        for _ in range(5):
            fn()
        calls += 5
        if time.perf_counter() - t0 >= WINDOW_S:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls * 1e3


def bench(cell, N, I, H):
    g = 4 if cell == "LSTM" else 3
    gen = torch.Generator().manual_seed(N + I + H)
    a = 2.0 / H ** 0.5
    w = [((torch.rand(s, generator=gen) * 2 - 1) * a).cuda() for s in ((2, g * H, I), (2, g * H, H), (2, g * H), (2, g * H))]
    Ip = (I + 15) // 16 * 16
    x = torch.zeros(T, N, Ip)
    x[..., :I] = torch.randn(T, N, I, generator=gen)
    x = x.cuda()
    layer = SM.lstm_layer_infer if cell == "LSTM" else SM.gru_layer_infer
    fwd, rev = [t[0].contiguous() for t in w], [t[1].contiguous() for t in w]

    def one_launch():
        return SM.bilayer_infer(cell, x, *w)

    def composed():
        yr = layer(x.flip(0).contiguous(), *rev).flip(0)
        return torch.cat((layer(x, *fwd), yr), dim=2)

    with torch.no_grad():
        for _ in range(3):  # warm both
            ya, yb = one_launch(), composed()
        diff = float((ya - yb).abs().max())
        c1 = window(composed)
        o1 = window(one_launch)
        c2 = window(composed)
        o2 = window(one_launch)
    return dict(one=min(o1, o2), one_runs=(o1, o2), comp=(c1, c2), diff=diff)


def main():
    lines = ["# Bidirectional layer: one launch per step against the composition of unidirectional entries", "",
             f"Inference, T = {T}, one MI355X, `tools/bench_bidir.py`: ms per layer call (host clock over windows of at least "
             f"{WINDOW_S} s ending in a synchronise; the two forms alternate in one process, both warmed).  composed = flip, two "
             "`fsn_*_layer_forward` calls, flip back, concatenate, timed twice; spread = the difference between its two runs.", "",
             "| cell | N | I | H | regime | one launch: run 1 / run 2 | composed: run 1 / run 2 | spread | composed / one launch | max abs diff |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for cell in ("LSTM", "GRU"):
        for N, I, H, regime in SHAPES:
            r = bench(cell, N, I, H)
            spread = abs(r["comp"][0] - r["comp"][1])
            ratio = min(r["comp"]) / r["one"]
            lines.append(f"| {cell} | {N} | {I} | {H} | {regime} | {r['one_runs'][0]:.3f} / {r['one_runs'][1]:.3f} | {r['comp'][0]:.3f} / "
                         f"{r['comp'][1]:.3f} | {spread:.3f} | {ratio:.2f} | {r['diff']:.1e} |")
            slower_by = r["one"] - min(r["comp"])
            verdicts.append((cell, N, I, H, regime, slower_by, spread))
            print(lines[-1], flush=True)
    lines += ["", "The one-launch form against the faster of the composition's two runs:"]
    for cell, N, I, H, regime, slower_by, spread in verdicts:
        what = "not slower" if slower_by <= 0 else (f"slower by {slower_by:.3f} ms, within the composition's spread of {spread:.3f} ms"
                                                    if slower_by <= spread else f"SLOWER by {slower_by:.3f} ms (spread {spread:.3f} ms)")
        lines.append(f"* {cell} N {N} I {I} H {H} ({regime}): {what}")
    lines += ["", "The many-row shape is reported for honesty: there a step is bound by its matrix work, not by the launch chain, and the "
              "per-CU step form (`lstm_step_cu_kernel`'s shape with both directions' jobs) is the later change."]
    text = "\n".join(lines) + "\n"
    print(text)
    if "--write" in sys.argv:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "bidir_layer.md"), "w") as f:
            f.write(text)


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("bench_bidir.py measures on the GPU; there is none here")
    main()
