"""Golden vectors of the reverberation-time-shortening target, produced by running the REFERENCE's own
audio_zen/acoustics/rvb.py:reverberation_time_shortening on synthetic responses in the authoring container:

    python tests/golden/make_golden_rts.py <reference checkout>      -> tests/golden/rts_windows.npz

rvb.py does not import as it stands (its return annotation calls `tuple` with two arguments), so the file is compiled
with postponed annotations (`__future__.annotations.compiler_flag`) and the function is called from the resulting
namespace: its arithmetic is untouched.  The responses are 16-bit PCM values (v / 32768, exact in fp32), so one array
serves both slab formats of the library.  Cases: lengths 1, 2, 33, 513, 4097 and 6000; a negative peak; a peak at index 0
and one at the last sample; two equal peaks (np.argmax takes the first); a peak at 5000 of 6000 (beyond the 4097 samples
the mixing tests convolve); N1 >= len; 0.6 -> 0.15 s at 16 kHz and 1.2 -> 0.3 s at 48 kHz; one pair whose q is so large
that the window runs through the fp32 denormals to zero.
"""
import __future__

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import mix_reference as R  # noqa: E402


def reference_function(checkout):
    path = os.path.join(checkout, "audio_zen", "acoustics", "rvb.py")
    ns = {"__name__": "rvb"}
    exec(compile(open(path).read(), path, "exec", flags=__future__.annotations.compiler_flag), ns)
    return ns["reverberation_time_shortening"]


def decaying(rng, n, tau, peak_at=None, peak=0.9):
    """Decaying noise below 0.5, with one sample of `peak` at peak_at."""
    h = 0.45 * rng.standard_normal(n) * np.exp(-np.arange(n) / tau)
    h = np.clip(h, -0.5, 0.5)
    if peak_at is not None:
        h[peak_at] = peak
    return R.pcm(h)


def cases():
    rng = np.random.default_rng(2204)
    A, Bk = dict(original_T60=0.6, target_T60=0.15, sr=16000), dict(original_T60=1.2, target_T60=0.3, sr=48000)
    two = decaying(rng, 4097, 700.0)
    two[100], two[2000] = 0.75, -0.75  # equal magnitudes: the first wins
    out = [
        ("len1", R.pcm([0.5]), A),
        ("len2_negative_peak", R.pcm([0.25, -0.75]), A),
        ("len33_peak_at_0", decaying(rng, 33, 10.0, 0), A),                 # N1 = 32: one windowed sample
        ("len33_n1_past_the_end", decaying(rng, 33, 10.0, 5), A),           # N1 = 37 >= len
        ("len513_peak_at_last", decaying(rng, 513, 100.0, 512, -0.9), Bk),
        ("len4097_two_equal_peaks", two, Bk),
        ("len4097_speechlike", decaying(rng, 4097, 900.0, 37), A),
        ("len6000_peak_at_5000", decaying(rng, 6000, 4000.0, 5000), A),
        # q = 3 / 8 - 3 / 9600 per sample: 10^(-q n) reaches the denormals near n = 101 and zero near n = 120
        ("len6000_huge_q", decaying(rng, 6000, 3000.0, 64), dict(original_T60=0.6, target_T60=0.0005, sr=16000)),
    ]
    return [(name, h, dict(kw, time_after_max=0.002)) for name, h, kw in out]


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    fn = reference_function(sys.argv[1])
    arrays, meta = {}, []
    for name, h, kw in cases():
        assert h.dtype == np.float32 and np.array_equal(h, R.pcm(h))
        rir, win = fn(h.copy(), **kw)
        assert rir.dtype == np.float32 and win.dtype == np.float32 and rir.shape == win.shape == h.shape
        arrays[f"{name}_h"], arrays[f"{name}_rir"], arrays[f"{name}_win"] = h, rir, win
        meta.append(dict(name=name, **kw))
        tiny = np.float32(2.0 ** -126)
        print(f"{name}: {len(h)} taps, argmax {int(np.argmax(np.abs(h)))}, window != 1 on {int((win != 1).sum())}, "
              f"denormal on {int(((win > 0) & (win < tiny)).sum())}, zero on {int((win == 0).sum())}")
    arrays["meta"] = np.asarray(json.dumps(meta))
    path = os.path.join(HERE, "rts_windows.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
