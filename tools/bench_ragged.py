"""Ragged batches vs the one-utterance loop (profiles/ragged_batch.md).

64 seeded utterances, lengths uniform in [2 s, 4 s] at 16 kHz, enhanced three ways in ONE process, the variants
alternating round by round (warm-up rounds first, a device sync around every timed call):
  (a) loop     - one ``Model.enhance`` per utterance, what ``Inferencer.__call__`` does with the default batch_size;
  (b) ragged G - the 64 utterances as 64 / G ragged calls of G (``enhance(noisy, lengths=...)``), G = 16, 32, 64;
  (c) uniform  - one 64 x L_max batch without lengths (every utterance as long as the longest).
Then the ``stft`` and ``mask_istft`` stage times (libfsn_hip's per-stage events) of a 64 x 3 s batch with and without
``lengths`` (all equal).  Prints one JSON object.

usage: python tools/bench_ragged.py [--rounds 5] [--warmup 2] [--seed 0]"""
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

import fullsubnet_amd  # noqa: E402
from fullsubnet_amd import _lib  # noqa: E402
from fullsubnet_amd.ragged import pad_utterances  # noqa: E402
from fsn_synthetic import make_noisy, make_params  # noqa: E402

SR, N_UTT = 16000, 64


def frames(n):
    return 1 + n // 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    m = fullsubnet_amd.Model(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0,
                             sb_num_neighbors=15, fb_output_activate_function="ReLU", sb_output_activate_function=False,
                             fb_model_hidden_size=512, sb_model_hidden_size=384, norm_type="offline_laplace_norm",
                             num_groups_in_drop_band=1, weight_init=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(seed=3).items()})
    m = m.to(dev).eval()

    rng = np.random.default_rng(args.seed)
    lengths = [int(v) for v in rng.integers(2 * SR, 4 * SR + 1, size=N_UTT)]
    full = make_noisy(N_UTT, max(lengths), seed=args.seed + 1)
    utts = [torch.from_numpy(full[b, :n].copy()).to(dev) for b, n in enumerate(lengths)]
    singles = [u[None] for u in utts]

    def ragged_groups(g):
        out = []
        for i in range(0, N_UTT, g):
            noisy, lens = pad_utterances(utts[i:i + g], device=dev)
            out.append((noisy, lens))
        return out

    groups = {g: ragged_groups(g) for g in (16, 32, 64)}
    uniform = torch.from_numpy(full).to(dev)

    def pad_share(gs):
        tot = sum(len(l) * frames(n.shape[1]) for n, l in gs)
        return 1.0 - sum(frames(x) for _, l in gs for x in l) / tot

    variants = {"loop": lambda: [m.enhance(x) for x in singles]}
    for g, gs in groups.items():
        variants[f"ragged_{g}"] = (lambda gs=gs: [m.enhance(n, lengths=l) for n, l in gs])
    variants["uniform_64"] = lambda: m.enhance(uniform)

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

    res = {"utterances": N_UTT, "lengths_s": [min(lengths) / SR, max(lengths) / SR], "rounds": args.rounds,
           "variants": {}}
    for k, ts in times.items():
        ms = statistics.median(ts)
        share = (pad_share(groups[int(k.split("_")[1])]) if k.startswith("ragged")
                 else 1.0 - sum(frames(n) for n in lengths) / (N_UTT * frames(max(lengths))) if k == "uniform_64" else 0.0)
        res["variants"][k] = {"ms": round(ms, 2), "ms_min": round(min(ts), 2), "utt_per_s": round(N_UTT / ms * 1e3, 1),
                              "padded_frame_share": round(share, 4)}
    loop = res["variants"]["loop"]["utt_per_s"]
    res["ragged_64_vs_loop"] = round(res["variants"]["ragged_64"]["utt_per_s"] / loop, 3)
    res["ragged_64_vs_uniform_64"] = round(res["variants"]["ragged_64"]["ms"] / res["variants"]["uniform_64"]["ms"], 4)

    # stage times at 64 x 3 s with and without lengths (all equal), alternating
    x = torch.from_numpy(make_noisy(N_UTT, 3 * SR, seed=args.seed + 2)).to(dev)
    eq = [3 * SR] * N_UTT
    stages = {"plain": {"stft": [], "mask_istft": []}, "lengths": {"stft": [], "mask_istft": []}}
    _lib.profile_enable(True, dev)
    try:
        with torch.no_grad():
            for r in range(args.warmup + 3 * args.rounds):
                for k in ("plain", "lengths"):
                    m.enhance(x) if k == "plain" else m.enhance(x, lengths=eq)
                    torch.cuda.synchronize()
                    st = _lib.profile_read(dev)
                    if r >= args.warmup:
                        for s in ("stft", "mask_istft"):
                            stages[k][s].append(st[s] * 1e3)
    finally:
        _lib.profile_enable(False, dev)
    res["stages_64x3s_us"] = {k: {s: round(statistics.median(v), 1) for s, v in d.items()} for k, d in stages.items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
