"""Improved FullSubNet ragged batches vs the one-utterance loop (profiles/ragged_batch_improved.md).

64 seeded utterances, lengths uniform in [2 s, 4 s] at 48 kHz (BASELINE config 5: n_fft 960 / hop 480, 481 bins), weights
from ``fsn_synthetic.make_improved_params``, enhanced three ways in ONE process, the variants alternating round by round
(warm-up rounds first, a device sync around every timed call):
  (a) loop     - one ``Model.forward`` per utterance, what a caller without ``lengths`` has to do;
  (b) ragged G - the 64 utterances as 64 / G ragged calls of G (``forward(y, lengths=...)``), G = 8, 16, 32;
  (c) uniform  - the 64 x L_max batch without lengths (every utterance as long as the longest; forward chunks it).
Prints one JSON object; ``--write`` also writes profiles/ragged_batch_improved.md from it.  The loop variant uses nothing
of the ragged path, so the same script's loop figure on the parent tree (``--loop-only``) is the figure to compare with:
pass it as ``--parent-loop-ms``.

usage: python tools/bench_ragged_improved.py [--rounds 5] [--warmup 2] [--seed 0] [--write] [--parent-loop-ms MS]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fullsubnet_amd.improved_fullsubnet import Model  # noqa: E402
from fullsubnet_amd.ragged import frames as n_frames, pad_utterances  # noqa: E402
from fsn_synthetic import IMPROVED_48K, make_improved_params, make_noisy  # noqa: E402

SR, N_UTT, GROUPS = 48000, 64, (8, 16, 32)
HOP = IMPROVED_48K["hop_length"]


def frames(n):
    return n_frames(n, HOP)


def report(res):
    v = res["variants"]
    lo, hi = res["lengths_s"]
    rows = [("(a) loop", f"{N_UTT} x `Model.forward(y[None, :L_b])`", "loop")]
    rows += [(f"(b) ragged {g}", f"{N_UTT // g} ragged calls of {g} (`forward(y, lengths=...)`)", f"ragged_{g}") for g in GROUPS]
    rows += [(f"(c) uniform {N_UTT}", f"the {N_UTT} x L_max batch without `lengths` (forward runs it as chunks)", f"uniform_{N_UTT}")]
    out = ["# Improved FullSubNet ragged batches: utterances of different lengths in one call (one MI355X)", "",
           f"`python tools/bench_ragged_improved.py --write` (seed {res['seed']}, {res['warmup']} warm-up rounds, {res['rounds']} timed "
           "rounds, the variants alternating round by round in one process, a device sync around every timed call).  Improved "
           "FullSubNet (BASELINE config 5: 48 kHz, n_fft 960 / hop 480, 481 bins, `offline_laplace_norm`, fp32), weights from "
           f"`fsn_synthetic.make_improved_params(IMPROVED_48K, seed=5)`.  {N_UTT} seeded utterances with lengths uniform in "
           f"[2 s, 4 s] (drawn: {lo:.3f} - {hi:.3f} s).  Medians of the timed rounds; no time or ratio is a target here - this "
           "file records what the run gave.", "",
           f"| variant | what runs | ms for the {N_UTT} utterances | fastest round | utterances / s | padded frames |",
           "|---|---|---|---|---|---|"]
    for name, what, key in rows:
        r = v[key]
        out.append(f"| {name} | {what} | {r['ms']:.1f} | {r['ms_min']:.1f} | {r['utt_per_s']:.0f} | {100 * r['padded_frame_share']:.1f} % |")
    out += [""] + [f"* Ragged {g} vs the loop: {res[f'ragged_{g}_vs_loop']:.2f}x the loop's utterances per second." for g in GROUPS]
    out.append(f"* Ragged 32 vs uniform {N_UTT} x L_max: {res[f'ragged_32_vs_uniform_{N_UTT}']:.3f}x the time.")
    if res.get("parent_loop_ms") is not None:
        out.append(f"* The parent commit's loop (`--loop-only` on its tree, same GPU, same seeds): {res['parent_loop_ms']:.1f} ms "
                   f"for the {N_UTT} utterances - the figure a caller had before `lengths`; this tree's loop: {v['loop']['ms']:.1f} ms.")
    else:
        out.append("* The parent commit's loop figure was not measured in this run.")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--loop-only", action="store_true", help="time variant (a) alone (runs on a tree without `lengths`)")
    ap.add_argument("--parent-loop-ms", type=float, default=None, help="the parent commit's --loop-only median, for the report")
    ap.add_argument("--write", action="store_true", help="write profiles/ragged_batch_improved.md")
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    m = Model(**IMPROVED_48K)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_improved_params(IMPROVED_48K, seed=5).items()}, strict=True)
    m = m.to(dev).eval()

    rng = np.random.default_rng(args.seed)
    lengths = [int(v) for v in rng.integers(2 * SR, 4 * SR + 1, size=N_UTT)]
    full = make_noisy(N_UTT, max(lengths), seed=args.seed + 1)
    utts = [torch.from_numpy(full[b, :n].copy()).to(dev) for b, n in enumerate(lengths)]
    singles = [u[None] for u in utts]
    variants = {"loop": lambda: [m(x) for x in singles]}
    groups = {}
    if not args.loop_only:
        groups = {g: [pad_utterances(utts[i:i + g], device=dev) for i in range(0, N_UTT, g)] for g in GROUPS}
        uniform = torch.from_numpy(full).to(dev)
        for g, gs in groups.items():
            variants[f"ragged_{g}"] = (lambda gs=gs: [m(y, lengths=l) for y, l in gs])
        variants[f"uniform_{N_UTT}"] = lambda: m(uniform)

    def pad_share(gs):
        tot = sum(len(l) * frames(y.shape[1]) for y, l in gs)
        return 1.0 - sum(frames(x) for _, l in gs for x in l) / tot

    times = {k: [] for k in variants}
    with torch.no_grad():
        for r in range(args.warmup + args.rounds):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if r >= args.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)

    res = {"model": "improved_fullsubnet_48k", "utterances": N_UTT, "lengths_s": [min(lengths) / SR, max(lengths) / SR],
           "seed": args.seed, "rounds": args.rounds, "warmup": args.warmup, "parent_loop_ms": args.parent_loop_ms, "variants": {}}
    for k, ts in times.items():
        ms = statistics.median(ts)
        share = (pad_share(groups[int(k.split("_")[1])]) if k.startswith("ragged")
                 else 1.0 - sum(frames(n) for n in lengths) / (N_UTT * frames(max(lengths))) if k.startswith("uniform")
                 else 0.0)
        res["variants"][k] = {"ms": round(ms, 2), "ms_min": round(min(ts), 2), "utt_per_s": round(N_UTT / ms * 1e3, 1),
                              "padded_frame_share": round(share, 4)}
    if not args.loop_only:
        loop = res["variants"]["loop"]["utt_per_s"]
        for g in GROUPS:
            res[f"ragged_{g}_vs_loop"] = round(res["variants"][f"ragged_{g}"]["utt_per_s"] / loop, 3)
        res[f"ragged_32_vs_uniform_{N_UTT}"] = round(res["variants"]["ragged_32"]["ms"] / res["variants"][f"uniform_{N_UTT}"]["ms"], 4)
        if args.write:
            with open(os.path.join(ROOT, "profiles", "ragged_batch_improved.md"), "w") as f:
                f.write(report(res))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
