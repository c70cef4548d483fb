"""Golden vectors of the training-pair mixing, produced by running the REFERENCE's own
recipes/dns_interspeech_2020/dataset_train.py:Dataset.__getitem__ and Dataset.snr_mix (scipy fftconvolve, numpy) on tiny
preloaded lists in the authoring container.  Run from the repo root:   python tests/golden/make_golden_mix.py

  mix_sources.npz   the preloaded lists (16-bit PCM, so one file serves both slab formats), the dataset arguments
  mix_items.npz     a dozen items of __getitem__ at L = 4096 under recorded seeds: every random call the reference made
                    (function, arguments, result - the log draw_item must reproduce) and the (noisy, clean) it returned;
                    direct snr_mix calls for the cases a dozen draws need not hit: both clip branches, a 2-D response

The lists hold one clean file shorter than the crop, one spiky clean file (clipping needs a crest factor above 5.6 at
-15 dBFS), noise files short enough that rows are stitched from several with 0.2 s silences, and one 2-D response.
`librosa` is stubbed (feature.py:3 imports it; preloaded lists never reach it).
"""
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.modules.setdefault("librosa", types.ModuleType("librosa"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, "/root/reference/recipes/dns_interspeech_2020")

from dataset_train import Dataset  # noqa: E402

import mix_reference as R  # noqa: E402

SR, SUB, SILENCE = 2048, 2.0, 0.2  # silences of 409 samples: rows are stitched from several noise files at L = 4096
L = int(SUB * SR)
assert L == 4096
ARGS = dict(sr=SR, sub_sample_length=SUB, silence_length=SILENCE, snr_range=[-5, 20], reverb_proportion=0.75,
            target_dB_FS=-25, target_dB_FS_floating_value=10)
N_ITEMS = 12


def sources(seed=2020):
    rng = np.random.default_rng(seed)
    clean = []
    for i in range(N_ITEMS):
        n = [6000, 4096, 5200, 3000, 4097, 7000][i % 6]  # longer, equal, shorter than the crop
        t = np.arange(n)
        clean.append(R.pcm(0.25 * rng.standard_normal(n) * (0.5 + 0.5 * np.sin(2 * np.pi * t / (900.0 + 50 * i)))))
    spiky = np.zeros(4500)
    spiky[::640] = 0.9 * rng.choice([-1.0, 1.0], len(spiky[::640]))
    clean[7] = R.pcm(spiky + 1e-3 * rng.standard_normal(4500))
    noise = [R.pcm(0.05 * rng.standard_normal(n)) for n in (9000, 1500, 700, 2600, 5000)]
    rir = []
    for n, tau in ((1200, 150.0), (300, 30.0), (5000, 500.0)):  # the last one longer than the crop
        r = rng.standard_normal(n) * np.exp(-np.arange(n) / tau)
        rir.append(R.pcm(0.8 * r / np.abs(r).max()))
    r = rng.standard_normal((3, 400)) * np.exp(-np.arange(400) / 50.0)
    rir.append(R.pcm(0.8 * r / np.abs(r).max()))
    return clean, noise, rir


def dataset(clean, noise, rir):
    d = Dataset.__new__(Dataset)  # __init__ reads file lists from disk; these are its attributes for preloaded lists
    d.sr, d.num_workers = SR, 1
    d.clean_dataset_list = [(f"clean_{i}", w) for i, w in enumerate(clean)]
    d.noise_dataset_list = [(f"noise_{i}", w) for i, w in enumerate(noise)]
    d.rir_dataset_list = [(f"rir_{i}", w) for i, w in enumerate(rir)]
    d.snr_list = d._parse_snr_range(ARGS["snr_range"])
    d.reverb_proportion, d.silence_length = ARGS["reverb_proportion"], ARGS["silence_length"]
    d.target_dB_FS, d.target_dB_FS_floating_value = ARGS["target_dB_FS"], ARGS["target_dB_FS_floating_value"]
    d.sub_sample_length, d.length = SUB, len(clean)
    return d


class Recorder:
    """Logs every random call the reference makes, without changing what it returns."""

    def __enter__(self):
        self.log = []
        self.saved = (random.choice, np.random.randint, np.random.random)
        choice, randint, rand = self.saved

        def rec_choice(seq):
            r = choice(seq)
            pos = next(i for i, e in enumerate(seq) if e is r or (isinstance(e, int) and e == r))
            self.log.append(["choice", len(seq), pos])
            return r

        def rec_randint(*a):
            r = randint(*a)
            self.log.append(["randint", [int(v) for v in a], int(r)])
            return r

        def rec_random(*a):
            r = rand(*a)
            self.log.append(["random", float(np.ravel(r)[0])])
            return r

        random.choice, np.random.randint, np.random.random = rec_choice, rec_randint, rec_random
        return self

    def __exit__(self, *exc):
        random.choice, np.random.randint, np.random.random = self.saved


def main():
    clean, noise, rir = sources()
    as_i16 = lambda w: np.rint(np.asarray(w, np.float64) * 32768.0).astype(np.int16)  # noqa: E731
    src = {f"clean_{i}": as_i16(w) for i, w in enumerate(clean)}
    src.update({f"noise_{i}": as_i16(w) for i, w in enumerate(noise)})
    src.update({f"rir_{i}": as_i16(w) for i, w in enumerate(rir)})
    src["meta"] = np.array(json.dumps(dict(args=ARGS, L=L, n_clean=len(clean), n_noise=len(noise), n_rir=len(rir),
                                           numpy=np.__version__)))
    path = os.path.join(HERE, "mix_sources.npz")
    np.savez_compressed(path, **src)
    print(f"mix_sources: {os.path.getsize(path) / 1024:.0f} KiB")

    d = dataset(clean, noise, rir)
    logs, seeds, noisy, cleans = [], [], [], []
    for i in range(N_ITEMS):
        seed = (100 + i, 200 + i)
        random.seed(seed[0])
        np.random.seed(seed[1])
        with Recorder() as rec:
            n, c = d[i]
        assert n.dtype == np.float32 and n.shape == (L,)
        logs.append(rec.log)
        seeds.append(seed)
        noisy.append(n)
        cleans.append(c)
    reverb = sum(any(e[0] == "choice" and e[1] == len(rir) for e in lg[-3:]) for lg in logs)
    print(f"items: {N_ITEMS}, with reverb: {reverb}, clipped: {sum(float(np.abs(n).max()) > 0.9895 for n in noisy)}")

    # direct snr_mix calls: (clean index, start, len, noise index, noise start, snr, rir index or -1, numpy seed)
    direct = [(7, 0, 4096, 0, 50, 20, -1, 7), (7, 100, 4096, 0, 0, 18, 1, 8), (0, 1000, 4096, 4, 300, 3, 3, 9),
              (2, 0, 4096, 4, 0, -5, 2, 10), (3, 0, 3000, 0, 4000, 10, -1, 11)]
    d_desc, d_noisy, d_clean = [], [], []
    for ci, cs, cl, ni, ns, snr, ri, seed in direct:
        c = np.zeros(L, np.float32)
        c[:cl] = clean[ci][cs:cs + cl]
        nz = noise[ni][ns:ns + L].copy()
        assert len(nz) == L
        np.random.seed(seed)
        with Recorder() as rec:
            n, c_out = Dataset.snr_mix(c, nz, snr, ARGS["target_dB_FS"], ARGS["target_dB_FS_floating_value"],
                                       rir=None if ri < 0 else rir[ri])
        draws = [e[2] for e in rec.log if e[0] == "randint"]
        row = draws[0] if len(draws) == 2 else 0
        d_desc.append(dict(clean_index=ci, clean_start=cs, clean_len=cl, noise_index=ni, noise_start=ns, snr=snr, rir_index=ri,
                           rir_row=row, noisy_target_dB_FS=draws[-1], clipped=bool(np.abs(n).max() > 0.9895)))
        d_noisy.append(n.astype(np.float32))
        d_clean.append(c_out.astype(np.float32))
    print("direct:", [(x["rir_index"], x["rir_row"], x["noisy_target_dB_FS"], x["clipped"]) for x in d_desc])
    assert {x["clipped"] for x in d_desc} == {True, False}
    path = os.path.join(HERE, "mix_items.npz")
    np.savez_compressed(path, noisy=np.stack(noisy), clean=np.stack(cleans), seeds=np.asarray(seeds),
                        logs=np.array(json.dumps(logs)), direct=np.array(json.dumps(d_desc)), direct_noisy=np.stack(d_noisy),
                        direct_clean=np.stack(d_clean))
    print(f"mix_items: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
