"""Time of one fsn_resample call (sample-rate conversion on the device) on one MI355X, next to a host resampler:

    python tools/bench_resample.py [--iters 20] [--commit SHA] [--write] [--out profiles/resample_device.md]

Cases: 64 rows x 3 s at 48 -> 16 kHz and 16 -> 48 kHz, 64 x 3 s at 44.1 -> 16 kHz in both designs, one row of 60 min at
44.1 -> 16 kHz.  Rows are unit-variance noise made on the device.  The call is `fsn_resample` through the binding into
buffers allocated once (taps kernel + resampling kernel), timed with device events around `--iters` calls after a
warm-up, three windows, the median window reported; `fsn_resample_taps` alone the same way.  Bytes moved are
4 x (input + output samples) over the call's time, shown beside the float4 copy rate of an MI355X as the guide measured it
(6.29 TB/s); the tool does not measure that rate itself.  The per-kernel split comes from torch.profiler's device
activity over ten further calls in a pass of its own ("not measured" if the profiler reports no kernels).  The host
figure is `scipy.signal.resample_poly` (the same filter; "sharp": its taps passed as the window) on the whole batch in
this process, fp32 rows, taken once per case; without scipy it is the numpy reference of tests/resample_reference.py on
ONE row of the case, and the table says which.  End to end: `Inferencer.enhance_utterances` of 64 x 3 s at 48 kHz with
`sr=48000, output_sr="input"` beside the plain call on 64 x 3 s at 16 kHz, FullSubNet with seeded weights.  The error
table runs the cases of tests/test_gpu_resample.py through the test's own runner and reports the worst |y - r| as a
fraction of its derived bound.  `--write` puts everything into profiles/resample_device.md (or --out)."""
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
COPY_TBS = 6.29  # float4 copy on an MI355X, as measured by the microarchitecture guide this project follows
# (rows, seconds, sr_in, sr_out, design)
CASES = ((64, 3, 48000, 16000, "scipy"), (64, 3, 16000, 48000, "scipy"), (64, 3, 44100, 16000, "scipy"),
         (64, 3, 44100, 16000, "sharp"), (1, 3600, 44100, 16000, "scipy"))
KERNELS = ("resample_taps_kernel", "resample_kernel", "resample_copy_kernel")


def event_ms(fn, iters):
    import torch
    for _ in range(3):
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
                if k + "(" in ev.key or k + "<" in ev.key or ev.key.endswith(k):
                    us = getattr(ev, "device_time_total", None)
                    if us is None:
                        us = getattr(ev, "cuda_time_total", 0.0)
                    out[k] = out.get(k, 0.0) + us / calls
        return out
    except Exception as e:  # the split is an extra: the call times stand without it
        print(f"kernel split not measured: {type(e).__name__}: {e}", file=sys.stderr)
        return {}


def host_ms(x, sr_in, sr_out, design):
    """(ms, what was timed) of the host resampler on the rows x [B, n] (numpy fp32)."""
    import resample_reference as R
    u, d = R.ratio(sr_in, sr_out)
    try:
        from scipy.signal import resample_poly
    except ImportError:
        t0 = time.perf_counter()
        R.resample(x[0], sr_in, sr_out, design)
        return 1e3 * (time.perf_counter() - t0), "numpy reference, ONE row"
    window = ("kaiser", 5.0) if design == "scipy" else R.taps(sr_in, sr_out, design)[0] / u
    t0 = time.perf_counter()
    resample_poly(x, u, d, axis=1, window=window)
    return 1e3 * (time.perf_counter() - t0), "scipy.signal.resample_poly, the whole batch"


def error_table():
    """[(design, rates, lengths, worst fraction of the bound)] over the cases of tests/test_gpu_resample.py."""
    import resample_reference as R
    import test_gpu_resample as T
    import fullsubnet_amd as fsn
    rows = {}
    for sr_in, sr_out, design, n, seed in T.sweep_cases(fsn):
        x = R.signal(n, seed)
        y, _ = T.run(x[None], None, sr_in, sr_out, design)
        r = R.resample(x, sr_in, sr_out, design)
        limit = R.bound(r, R.resample(x, sr_in, sr_out, design, absolute=True))
        frac = float(np.max(np.abs(y[0].astype(np.float64) - r) / limit))
        key = (design, (sr_in, sr_out))
        rows[key] = (rows.get(key, (0, 0.0))[0] + 1, max(rows.get(key, (0, 0.0))[1], frac))
    return [(design, rates, count, worst) for (design, rates), (count, worst) in rows.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--commit", default="")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_device.md"))
    ap.add_argument("--skip-long-host", action="store_true", help="do not time the host resampler on the 60 min row")
    args = ap.parse_args()

    import torch
    import fullsubnet_amd as fsn
    import resample_reference as R
    from fullsubnet_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the device: no ROCm device here")
    lib = _lib.lib()
    lines, split_lines = [], []
    for B, seconds, sr_in, sr_out, design in CASES:
        n = seconds * sr_in
        zeros, beta, rolloff = R.DESIGNS[design]
        torch.manual_seed(seconds + sr_in)
        x = torch.randn(B, n, device="cuda")
        L_out = R.out_length(n, sr_in, sr_out)
        out = torch.empty(B, L_out, device="cuda")
        out_len = torch.empty(B, dtype=torch.int32, device="cuda")
        nbytes = lib.fsn_resample_workspace_bytes(sr_in, sr_out, zeros, beta, rolloff)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        n_taps = 2 * zeros * max(R.ratio(sr_in, sr_out)) + 1
        h = torch.empty(n_taps, dtype=torch.float64, device="cuda")

        def call():
            _lib.check(lib.fsn_resample(x.data_ptr(), None, B, n, sr_in, sr_out, zeros, beta, rolloff, out.data_ptr(), L_out,
                                        out_len.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr()))

        def taps_call():
            _lib.check(lib.fsn_resample_taps(sr_in, sr_out, zeros, beta, rolloff, h.data_ptr(), n_taps, _lib.stream_ptr()))

        iters = args.iters if seconds < 60 else max(3, args.iters // 5)
        med, lo, hi = event_ms(call, iters)
        tmed, _, _ = event_ms(taps_call, args.iters)
        moved = 4.0 * B * (n + L_out)
        tbs = moved / (med * 1e-3) / 1e12
        if seconds >= 60 and args.skip_long_host:
            host, what = None, "not measured"
        else:
            host, what = host_ms(x.cpu().numpy(), sr_in, sr_out, design)
        tag = f"{B} x {seconds} s, {sr_in} -> {sr_out}, {design}"
        lines.append(f"| {tag} | {n_taps} | {fsn.resample.plan(sr_in, sr_out, design)['taps_in_lds']} | {med:.3f} | {lo:.3f} - {hi:.3f} | "
                     f"{tmed * 1e3:.1f} | {moved / 1e6:.1f} | {tbs:.3f} | {100 * tbs / COPY_TBS:.1f} % | "
                     f"{'-' if host is None else f'{host:.0f}'} | {what} | {'-' if host is None else f'{host / med:.0f} x'} |")
        print(lines[-1], flush=True)
        split = kernel_split(call)
        for k in KERNELS:
            if k in split:
                split_lines.append(f"| {tag} | {k} | {split[k]:.1f} |")
        if not split:
            split_lines.append(f"| {tag} | not measured | - |")
        print("\n".join(split_lines[-2:]), flush=True)
        del x, out, ws

    # end to end: 64 x 3 s through the Inferencer, at 48 kHz with the round trip and at the model's rate without
    from oracle import fullsubnet_oracle as O
    params = O.make_params(seed=5, gain=2.0, mask_gain=24.0)
    model = fsn.Model(norm_type="offline_laplace_norm", num_groups_in_drop_band=1, num_freqs=257, look_ahead=2,
                      sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15, fb_output_activate_function="ReLU",
                      sb_output_activate_function=False, fb_model_hidden_size=512, sb_model_hidden_size=384, weight_init=False)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    inf = fsn.Inferencer(dict(inferencer=dict(type="full_band_crm_mask", args={}),
                              acoustics=dict(n_fft=512, hop_length=256, win_length=512, sr=16000)), model=model.cuda().eval())
    torch.manual_seed(9)
    at48 = [0.1 * torch.randn(3 * 48000, device="cuda") for _ in range(64)]
    at16 = [0.1 * torch.randn(3 * 16000, device="cuda") for _ in range(64)]
    e2e = {}
    for name, fn in (("plain enhance_utterances, 64 x 3 s at 16 kHz", lambda: inf.enhance_utterances(at16)),
                     ('enhance_utterances(sr=48000, output_sr="input"), 64 x 3 s at 48 kHz',
                      lambda: inf.enhance_utterances(at48, sr=48000, output_sr="input")),
                     ('enhance_utterances(sr=48000, output_sr="input", design="sharp")',
                      lambda: inf.enhance_utterances(at48, sr=48000, output_sr="input", design="sharp"))):
        e2e[name] = event_ms(fn, max(3, args.iters // 4))
        print(f"{name}: {e2e[name][0]:.2f} ms", flush=True)
    errors = error_table()
    err_lines = [f"| {design} | {a} -> {b} | {count} | {worst:.4f} |" for design, (a, b), count, worst in errors]
    print("\n".join(err_lines))
    if not args.write:
        return
    base = e2e["plain enhance_utterances, 64 x 3 s at 16 kHz"][0]
    with open(args.out, "w") as f:
        f.write(f"""# Sample-rate conversion on the device: fsn_resample

Written by `tools/bench_resample.py --write` on {datetime.date.today().isoformat()}{f' at commit {args.commit}' if args.commit else ''},
one MI355X, device {torch.cuda.get_device_name(0)}, torch {torch.__version__}.  Method: the tool's docstring.

## One call (device events, median of three windows)

Bytes moved are 4 x (input + output samples).  The copy rate beside them, {COPY_TBS} TB/s, is the float4 copy of an MI355X as
the microarchitecture guide measured it; this tool did not measure it.  The call forms its taps on the device every time
(`fsn_resample_taps alone` is that kernel through its own entry) and then runs the resampling kernel.

| case | taps | table in LDS | fsn_resample ms | windows | fsn_resample_taps alone us | MB moved | TB/s | of the copy rate | host ms | host resampler | host / device |
|---|---|---|---|---|---|---|---|---|---|---|---|
""" + "\n".join(lines) + """

The host column is one process on the host CPU of the box the tool ran on, fp32 rows, timed once.

## Per kernel (torch.profiler device activity, ten calls, a pass of its own)

| case | kernel | us per call |
|---|---|---|
""" + "\n".join(split_lines) + f"""

## End to end through the Inferencer (FullSubNet, seeded weights, 64 utterances of 3 s)

| call | ms | windows | beside the plain call |
|---|---|---|---|
""" + "\n".join(f"| {name} | {m:.2f} | {lo:.2f} - {hi:.2f} | {m / base:.3f} x |" for name, (m, lo, hi) in e2e.items()) + """

## Error against the fp64 reference

The cases of tests/test_gpu_resample.py (rows of 1, 2, H / u, the inputs of one workgroup - 1, + 0, + 1, 4099 samples),
every output sample; the bound is 2^-24 abs(r) + 2^-40 sum abs(h) abs(x), 1.0 below is that bound.  Its first term is the one
fp32 rounding, which alone reaches 0.995 of it on these cases (tests/test_resample_cpu.py): figures near 1 are that rounding.

| design | ratio | rows | worst abs(y - r) / bound |
|---|---|---|---|
""" + "\n".join(err_lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
