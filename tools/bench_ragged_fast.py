"""Fast FullSubNet ragged batches vs the one-utterance loop (profiles/ragged_batch_fast.md).

256 seeded utterances, lengths uniform in [2 s, 4 s] at 16 kHz, weights from ``fsn_synthetic.make_fast_params``, enhanced
three ways in ONE process, the variants alternating round by round (warm-up rounds first, a device sync around every timed
call):
  (a) loop     - one ``Model.enhance`` per utterance, what ``Inferencer.__call__`` does with the default batch_size;
  (b) ragged G - the 256 utterances as 256 / G ragged calls of G (``enhance(noisy, lengths=...)``), G = 64, 128, 256;
  (c) uniform  - one 256 x L_max batch without lengths (every utterance as long as the longest).
Prints one JSON object.

usage: python tools/bench_ragged_fast.py [--rounds 5] [--warmup 2] [--seed 0]"""
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

from fullsubnet_amd.fast_fullsubnet import Model  # noqa: E402
from fullsubnet_amd.ragged import pad_utterances  # noqa: E402
from fsn_synthetic import make_fast_params, make_noisy  # noqa: E402

SR, N_UTT = 16000, 256
FAST_KW = dict(look_ahead=2, shrink_size=2, sequence_model="LSTM", num_mels=64, encoder_input_size=257,
               bottleneck_hidden_size=384, bottleneck_num_layers=2, noisy_input_num_neighbors=5,
               encoder_output_num_neighbors=0, norm_type="offline_laplace_norm", weight_init=False)


def frames(n):
    return 1 + n // 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    dev = torch.device("cuda:0")
    m = Model(**FAST_KW)
    sd = {k: torch.from_numpy(v) for k, v in make_fast_params(seed=3).items()}
    sd["mel_scale.fb"] = m.mel_scale.fb.clone()
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()

    rng = np.random.default_rng(args.seed)
    lengths = [int(v) for v in rng.integers(2 * SR, 4 * SR + 1, size=N_UTT)]
    full = make_noisy(N_UTT, max(lengths), seed=args.seed + 1)
    utts = [torch.from_numpy(full[b, :n].copy()).to(dev) for b, n in enumerate(lengths)]
    singles = [u[None] for u in utts]
    groups = {g: [pad_utterances(utts[i:i + g], device=dev) for i in range(0, N_UTT, g)] for g in (64, 128, 256)}
    uniform = torch.from_numpy(full).to(dev)

    def pad_share(gs):
        tot = sum(len(l) * frames(n.shape[1]) for n, l in gs)
        return 1.0 - sum(frames(x) for _, l in gs for x in l) / tot

    variants = {"loop": lambda: [m.enhance(x) for x in singles]}
    for g, gs in groups.items():
        variants[f"ragged_{g}"] = (lambda gs=gs: [m.enhance(n, lengths=l) for n, l in gs])
    variants["uniform_256"] = lambda: m.enhance(uniform)

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

    res = {"model": "fast_fullsubnet", "utterances": N_UTT, "lengths_s": [min(lengths) / SR, max(lengths) / SR],
           "rounds": args.rounds, "variants": {}}
    for k, ts in times.items():
        ms = statistics.median(ts)
        share = (pad_share(groups[int(k.split("_")[1])]) if k.startswith("ragged")
                 else 1.0 - sum(frames(n) for n in lengths) / (N_UTT * frames(max(lengths))) if k.startswith("uniform")
                 else 0.0)
        res["variants"][k] = {"ms": round(ms, 2), "ms_min": round(min(ts), 2), "utt_per_s": round(N_UTT / ms * 1e3, 1),
                              "padded_frame_share": round(share, 4)}
    loop = res["variants"]["loop"]["utt_per_s"]
    for g in (64, 128, 256):
        res[f"ragged_{g}_vs_loop"] = round(res["variants"][f"ragged_{g}"]["utt_per_s"] / loop, 3)
    res["ragged_256_vs_uniform_256"] = round(res["variants"]["ragged_256"]["ms"] / res["variants"]["uniform_256"]["ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
