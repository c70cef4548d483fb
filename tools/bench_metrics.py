"""Time of one fsn_stoi / fsn_si_sdr call (validation metrics on the device) on one MI355X, next to the host reference:

    python tools/bench_metrics.py [--iters 20] [--commit SHA] [--write] [--out profiles/stoi_device.md]

Two shapes: 150 pairs x 10 s at 16 kHz (150 is taken as the size of one DNS validation subset; that figure is not checked
here) and 32 pairs x 10 s at 48 kHz.  Clean rows are the speech-like signals of tests/stoi_reference.py (eight distinct
ones, cycled), estimates the clean row plus white noise at 0 .. 20 dB.  The call is `metrics.stoi` / `metrics.si_sdr`
(workspace from the size query + the entry); timed with device events around `--iters` calls after a warm-up, three
windows, the median window reported.  The per-kernel split comes from torch.profiler's device activity over ten further
calls in a pass of its own ("not measured" if the profiler reports no kernels).  The host figure is the fp64 numpy
reference (tests/stoi_reference.py) on one pair in this process - numpy's convolve, rfft and elementwise paths, one
thread - taken before the device is touched.  The error table is the worst |device - reference| per sample rate over the
fixture table of tests/test_gpu_metrics.py, run through the test's own runners, plus two rows of each timed batch.
`--write` puts everything into profiles/stoi_device.md (or --out)."""
import argparse
import datetime
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ((150, 10, 16000), (32, 10, 48000))
KERNELS = ("stoi_taps_kernel", "stoi_resample_kernel", "stoi_energy_kernel", "stoi_keep_kernel", "stoi_band_kernel",
           "stoi_corr_kernel", "stoi_finish_kernel", "si_sdr_kernel")


def batch(B, seconds, sr, seed=1):
    import stoi_reference as R
    n = seconds * sr
    rng = np.random.default_rng(seed)
    voices = [R.speech_like(n, sr, rng) for _ in range(8)]
    clean = np.stack([voices[b % 8] * (0.5 + 0.5 * (b % 5) / 4) for b in range(B)]).astype(np.float32)
    est = np.stack([R.add_noise(clean[b].astype(np.float64), 5.0 * (b % 5), rng) for b in range(B)]).astype(np.float32)
    return clean, est


def host_ms(clean, est, sr, repeats=3):
    import stoi_reference as R
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        R.stoi(clean, est, sr)
        times.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(times)


def event_ms(fn, iters):
    import torch
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        windows.append(a.elapsed_time(b) / iters)
    return statistics.median(windows), min(windows), max(windows)


def kernel_split(fn, calls=10):
    """{kernel: us per call} from torch.profiler's device activity; {} when it reports none of the kernels."""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for k in KERNELS:
                if k in ev.key:
                    us = getattr(ev, "device_time_total", None)
                    if us is None:
                        us = getattr(ev, "cuda_time_total", 0.0)
                    out[k] = out.get(k, 0.0) + us / calls
        return out
    except Exception as e:  # the split is an extra: the call times stand without it
        print(f"kernel split not measured: {type(e).__name__}: {e}", file=sys.stderr)
        return {}


def fixture_errors():
    """{tag: worst |d_device - d_reference| over the rows that are not exact by construction}, worst SI-SDR difference."""
    import stoi_reference as R
    import test_gpu_metrics as T
    worst = {}
    for tag in R.fixture_table():
        sr, L, rows, clean, est, lengths = T.batch_of(tag)
        d = T.run_stoi(clean, est, lengths, sr)
        worst[tag] = (sr, max(abs(d[b] - row["d"]) for b, row in enumerate(rows) if row["exact"] is None), len(rows))
    clean, est, lengths, want, _ = T.sdr_batch()
    return worst, float(np.max(np.abs(T.run_si_sdr(clean, est, lengths) - want)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--commit", default="")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi_device.md"))
    args = ap.parse_args()

    import stoi_reference as R
    data, host = {}, {}
    for B, seconds, sr in SHAPES:
        data[sr] = batch(B, seconds, sr)
        host[sr] = host_ms(data[sr][0][0], data[sr][1][0], sr)
        print(f"host fp64 reference, one thread: {seconds} s pair at {sr} Hz: {host[sr]:.1f} ms", flush=True)

    import torch
    import fullsubnet_amd as fsn
    from fullsubnet_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on the device: no ROCm device here")
    lib = _lib.lib()
    lines, split_lines, big_lines = [], [], []
    for B, seconds, sr in SHAPES:
        clean, est = (torch.from_numpy(a).cuda() for a in data[sr])
        L = clean.shape[1]
        stoi_call = lambda: fsn.metrics.stoi(clean, est, sr)  # noqa: E731
        sdr_call = lambda: fsn.metrics.si_sdr(clean, est)  # noqa: E731
        med, lo, hi = event_ms(stoi_call, args.iters)
        smed, _, _ = event_ms(sdr_call, args.iters)
        ws = lib.fsn_stoi_workspace_bytes(B, L, sr)
        lines.append(f"| {B} | {seconds} | {sr} | {med:.3f} | {lo:.3f} - {hi:.3f} | {1e3 * med / B:.1f} | {smed:.3f} | "
                     f"{ws / 2 ** 20:.0f} | {host[sr]:.1f} | {host[sr] * B / med:.0f} x |")
        print(lines[-1], flush=True)
        both = lambda: (stoi_call(), sdr_call())  # noqa: E731
        split = kernel_split(both)
        total = sum(split.get(k, 0.0) for k in KERNELS if k != "si_sdr_kernel")
        for k in KERNELS:
            if k in split:
                share = f"{100 * split[k] / total:.1f} %" if total and k != "si_sdr_kernel" else "-"
                split_lines.append(f"| {B} x {seconds} s, {sr} Hz | {k} | {split[k]:.1f} | {share} |")
        if not split:
            split_lines.append(f"| {B} x {seconds} s, {sr} Hz | not measured | - | - |")
        d = stoi_call().cpu().numpy()
        for b in (0, B - 1):
            want = R.stoi(data[sr][0][b], data[sr][1][b], sr)
            big_lines.append(f"| {B} x {seconds} s, {sr} Hz | row {b} | {d[b]:.15f} | {abs(d[b] - want):.2e} |")
            print(big_lines[-1], flush=True)
    worst, sdr_worst = fixture_errors()
    err_lines = [f"| {tag} | {sr} | {n} | {w:.2e} | {w / 5e-11:.1e} |" for tag, (sr, w, n) in worst.items()]
    for line in split_lines + err_lines:
        print(line)
    print(f"SI-SDR: worst difference {sdr_worst:.2e} dB of 1e-8")
    if not args.write:
        return
    with open(args.out, "w") as f:
        f.write(f"""# Validation metrics on the device: fsn_stoi / fsn_si_sdr

Written by `tools/bench_metrics.py --write` on {datetime.date.today().isoformat()}{f' at commit {args.commit}' if args.commit else ''},
one MI355X, device {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Method: the tool's docstring.  150 pairs
is taken as the size of one DNS validation subset; that figure is not checked here.

## One call (device events, median of three windows of {args.iters} calls)

| pairs | seconds | Hz | fsn_stoi ms | windows | us per pair | fsn_si_sdr ms | workspace MiB | host reference ms per pair, one thread | host / device, per batch |
|---|---|---|---|---|---|---|---|---|---|
""" + "\n".join(lines) + """

The host column is the fp64 numpy reference of tests/stoi_reference.py on the host CPU of the box the tool ran on, not pystoi (which is on
no machine this project has); the last column compares one thread scoring the batch pair by pair with one device call.

## Per kernel (torch.profiler device activity, ten calls, a pass of its own)

| shape | kernel | us per call | share of fsn_stoi |
|---|---|---|---|
""" + "\n".join(split_lines) + """

## Error against the fp64 reference

Fixture table of tests/test_gpu_metrics.py (rows that are exact by construction - 1e-5, 0 - agree to the bit and are left
out); the bound is 5e-11.

| batch | Hz | rows | worst abs(d_device - d_reference) | share of the bound |
|---|---|---|---|---|
""" + "\n".join(err_lines) + f"""

SI-SDR, the same ragged rows at -5 .. 60 dB: worst difference {sdr_worst:.2e} dB (bound 1e-8 dB).

Two rows of each timed batch against the reference:

| shape | row | d (device) | abs(d_device - d_reference) |
|---|---|---|---|
""" + "\n".join(big_lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
