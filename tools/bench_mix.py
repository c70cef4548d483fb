"""Time of one fsn_mix_pairs / fsn_mix_pairs_target call (training pairs mixed on the device) on one MI355X, next to the
host baseline:

    python tools/bench_mix.py [--batches 16 32 48] [--taps 16000 64000] [--iters 50] [--commit SHA] [--write]

For every batch size, response length and slab format: B rows of L = 49 152 samples, three quarters of them with a room
impulse response (exactly: round(0.75 B) rows), descriptors drawn by `draw_item` from a synthetic bank.  The call is
`mix_batch` (descriptor upload + fsn_mix_pairs); timed with device events around `--iters` calls after a warm-up, three
windows, the median window reported, and `fsn_conv_rows` alone on the same rows the same way.  The per-kernel split comes
from torch.profiler's device activity over ten further calls ("not measured" if the profiler reports no kernels).  Bytes per
stage are what the stage must move once (inputs read once, outputs written once) from the shapes, with the time they take
at 6.3 TB/s.  The host baseline is the fp32 numpy port (tests/mix_reference.py: snr_mix in fp32, convolution through
np.fft) of the same items on 16 worker processes, started before the device is touched.  The error ratios are the worst
error / allowance of the sweeps of tests/test_gpu_mix.py, run here through the tests' own runners.  The same batches
with a dereverberation target on every reverberant row (response shortened to a T60 of 0.15 s) go through
`fsn_mix_pairs_target`, timed in the same run next to `fsn_mix_pairs` on the same descriptors, with its own kernel split
and the worst error / allowance of the target rows of tests/test_gpu_mix_target.py.  `--write` puts everything into
profiles/mix_pairs.md."""
import argparse
import datetime
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
L = 49152
HBM = 6.3e12  # measured streaming rate of the box (README)
STEP_MS = {16: 12.4, 32: 24.0, 48: 35.0}  # README: train_step_amp_shipped_batches
KERNELS = ("mix_gather_kernel", "conv_cols_fwd_kernel", "conv_rows_kernel", "conv_cols_inv_kernel", "mix_level_kernel")
TARGET_KERNELS = KERNELS + ("rir_shorten_kernel",)
TARGET_T60 = 0.15


def sources(taps, seed=1):
    import mix_reference as R
    rng = np.random.default_rng(seed)
    clean = [R.pcm(0.2 * rng.standard_normal(int(n))) for n in rng.integers(4 * 16000, 6 * 16000, 64)]
    noise = [R.pcm(0.05 * rng.standard_normal(int(n))) for n in rng.integers(2 * 16000, 10 * 16000, 16)]
    rir = []
    for _ in range(8):
        r = rng.standard_normal(taps) * np.exp(-np.arange(taps) / (taps / 7.0))
        rir.append(R.pcm(0.8 * r / np.abs(r).max()))
    return clean, noise, rir


def draw(B, lists, seed=2):
    import random
    import mix_reference as R
    from fullsubnet_amd.mix import MixConfig, draw_item
    cfg = MixConfig(reverb_proportion=1.0)
    assert cfg.samples == L
    tables = R.HostTables(*lists)
    py, npr = random.Random(seed), np.random.RandomState(seed)
    items = [draw_item(i % len(lists[0]), tables, cfg, py, npr) for i in range(B)]
    for it in items[round(0.75 * B):]:
        it.rir_index = -1
    # the target descriptors (read by fsn_mix_pairs_target alone): the responses of `sources` decay by e every taps / 7
    # samples, a T60 of taps ln(1000) / 7 samples
    from fullsubnet_amd.mix import shortening_q
    taps = len(lists[2][0])
    for it in items[:round(0.75 * B)]:
        it.target_mode, it.target_after_max = 1, int(0.002 * cfg.sr)
        it.target_q = shortening_q(taps * np.log(1000.0) / 7.0 / cfg.sr, TARGET_T60, cfg.sr)
        assert it.target_q > 0
    return items


_LISTS = None  # the source lists of the host baseline: set before the workers fork, so that only descriptors travel


def _host_item(it):
    import mix_reference as R
    return R.mix_item(it, *_LISTS, L, np.float32)[2]


def host_baseline(B, lists, items, workers=16, repeats=5):
    """ms per batch of the fp32 numpy port on `workers` processes (the sources are already in the workers' memory)."""
    global _LISTS
    _LISTS = lists
    with multiprocessing.get_context("fork").Pool(workers) as pool:
        pool.map(_host_item, items[:workers], chunksize=1)  # warm the workers
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            pool.map(_host_item, items, chunksize=1)
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


def kernel_split(fn, calls=10, kernels=KERNELS):
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
            for k in kernels:
                if k in ev.key:
                    us = getattr(ev, "device_time_total", None)
                    if us is None:
                        us = getattr(ev, "cuda_time_total", 0.0)
                    out[k] = out.get(k, 0.0) + us / calls
        return out
    except Exception as e:  # the split is an extra: the call times above stand without it
        print(f"kernel split not measured: {type(e).__name__}: {e}", file=sys.stderr)
        return {}


def stage_bytes(B, items, bank, log_n):
    """Bytes each stage must move once, from the shapes."""
    sb = 4 if bank.fmt == "f32" else 2
    rows = [it for it in items if it.rir_index >= 0]
    R_, N = len(rows), 1 << log_n
    taps = sum(min(int(bank.rir_len[bank.rir_first_row[it.rir_index] + it.rir_row]), L) for it in rows)
    src = sum(it.clean_len + sum(s[3] for s in it.segments) for it in items)
    return {"mix_gather_kernel": src * sb + 2 * B * L * 4,
            "conv_cols_fwd_kernel": R_ * L * 4 + taps * sb + R_ * N * 16,
            "conv_rows_kernel": 2 * R_ * N * 16,
            "conv_cols_inv_kernel": R_ * N * 16 + (B - R_) * L * 4 + B * L * 4,
            "mix_level_kernel": 4 * B * L * 4}


def log_n_of(taps):
    k = 2
    while (1 << k) < L + min(taps, L) - 1:
        k += 1
    return k


def error_ratios():
    import mix_reference as R
    import test_gpu_mix as T
    import fullsubnet_amd as fsn
    conv = [r for Lc in R.CONV_L for r in R.run_conv_sweep(T.conv_rows, Lc)]
    lists = R.mix_sources()
    cases = R.mix_cases()
    items = [it for _, it, _ in cases]
    out = T.mix_poisoned(fsn.MixBank(*lists, "cuda", fmt="f32"), items, R.MIX_L)
    mix = R.run_mix_rows(out, items, *lists, R.MIX_L)
    worst = lambda rows: max(rows, key=lambda r: r[1] / r[2])  # noqa: E731
    return worst(conv), len(conv), worst(mix), len(mix)


def target_error_ratios():
    """(worst error / allowance, its row, rows) of the shortened and early rows of tests/test_gpu_mix_target.py's sweep, and
    the taps of the golden responses that are not bit-equal to the reference's (of how many)."""
    import mix_reference as R
    import mix_target_reference as T
    import test_gpu_mix_target as TT
    import fullsubnet_amd as fsn
    lists = R.mix_sources()
    items = T.sweep_items()
    _, _, target = TT.pairs_target(fsn.MixBank(*lists, "cuda", fmt="f32"), [it for _, it in items])
    ratios = {}
    for b, (name, it) in enumerate(items):
        _, _, t64, allow, mode = T.target_rows(it, *lists, R.MIX_L)
        if mode != 0 and t64.any():
            ratios[name] = T.check_target(name, target[b], t64, allow)
    name = max(ratios, key=ratios.get)
    cases = T.golden_cases(os.path.join(ROOT, "tests", "golden"))
    out, win, idx = TT.rir_shorten([c["h"] for c in cases], [(c["q"], c["after_max"], 1) for c in cases], "f32", 6000)
    differ = sum(T.check_shorten(c, out[b], win[b], idx[b]) for b, c in enumerate(cases))
    return ratios[name], name, len(ratios), differ, 2 * sum(len(c["h"]) for c in cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 32, 48])
    ap.add_argument("--taps", type=int, nargs="+", default=[16000, 64000])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--commit", default="")
    ap.add_argument("--write", action="store_true")
    args = ap.parse_args()

    work = {}
    host = {}
    for taps in args.taps:
        lists = sources(taps)
        for B in args.batches:
            work[(taps, B)] = (lists, draw(B, lists))
            host[(taps, B)] = host_baseline(B, lists, work[(taps, B)][1])
            print(f"host fp32 port, 16 processes: taps {taps} B {B}: {host[(taps, B)]:.1f} ms per batch", flush=True)

    import torch
    import fullsubnet_amd as fsn
    from fullsubnet_amd import _lib, mix
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix.py measures on the device: no ROCm device here")
    lines, split_lines, target_lines, target_split_lines = [], [], [], []
    for taps in args.taps:
        for fmt in ("f32", "i16"):
            bank = fsn.MixBank(*work[(taps, args.batches[0])][0], "cuda", fmt=fmt)
            for B in args.batches:
                items = work[(taps, B)][1]
                out = (torch.empty(B, L, device="cuda"), torch.empty(B, L, device="cuda"))
                call = lambda: mix.mix_batch(bank, items, L, out=out, target=False)  # noqa: E731
                med, lo, hi = event_ms(call, args.iters)
                tcall = lambda: mix.mix_batch(bank, items, L, out=out, target=True)  # noqa: E731
                tmed, tlo, thi = event_ms(tcall, args.iters)
                target_lines.append(f"| {B} | {taps} | {fmt} | {tmed:.3f} | {tlo:.3f} - {thi:.3f} | {med:.3f} | {tmed / med:.2f} x |")
                print(target_lines[-1], flush=True)
                # the convolution alone, on the rows of the same batch
                tab, _, _, longest = mix.pack_items(bank, items, L)
                x = torch.randn(B, L, device="cuda") * 0.1
                y = torch.empty_like(x)
                off = torch.from_numpy(np.ascontiguousarray(tab["rir_off"])).cuda()
                ln = torch.from_numpy(np.ascontiguousarray(tab["rir_len"])).cuda()
                lib = _lib.lib()
                ws = _lib.workspace(lib.fsn_conv_rows_workspace_bytes(B, L, longest), "cuda")
                conv = lambda: _lib.check(lib.fsn_conv_rows(x.data_ptr(), B, L, bank.slabs["rir"].data_ptr(), bank.slab_format,  # noqa: E731
                                                            off.data_ptr(), ln.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(),
                                                            _lib.stream_ptr()))
                cmed, _, _ = event_ms(conv, args.iters)
                step = STEP_MS.get(B)
                share = f"{100 * med / step:.1f} %" if step else "-"
                lines.append(f"| {B} | {taps} | {fmt} | {med:.3f} | {lo:.3f} - {hi:.3f} | {cmed:.3f} | {host[(taps, B)]:.1f} | "
                             f"{host[(taps, B)] / med:.0f} x | {step if step else '-'} | {share} |")
                print(lines[-1], flush=True)
                if B == 32:
                    split = kernel_split(call)
                    nbytes = stage_bytes(B, items, bank, log_n_of(longest))
                    for k in KERNELS:
                        t = f"{split[k]:.1f}" if k in split else "not measured"
                        split_lines.append(f"| {taps} | {fmt} | `{k}` | {t} | {nbytes[k] / 1e6:.1f} | {1e6 * nbytes[k] / HBM:.1f} |")
                        print(split_lines[-1], flush=True)
                    split = kernel_split(tcall, kernels=TARGET_KERNELS)
                    for k in TARGET_KERNELS:
                        t = f"{split[k]:.1f}" if k in split else "not measured"
                        target_split_lines.append(f"| {taps} | {fmt} | `{k}` | {t} |")
                        print(target_split_lines[-1], flush=True)
            del bank
    (cw, cn, mw, mn) = error_ratios()
    ratios = [f"* convolution sweep ({cn} rows, L = 1 ... 131072, both slab formats): worst error / allowance "
              f"**{cw[1] / cw[2]:.3f}** ({cw[0]}: {cw[1]:.3e} of the peak of |h| * |x|, allowance {cw[2]:.3e})",
              f"* mix sweep ({mn} outputs at L = {4097}): worst error / allowance **{mw[1] / mw[2]:.3f}** "
              f"({mw[0]}: {mw[1]:.3e} of the row's peak, allowance {mw[2]:.3e})"]
    tw, tname, tn, differ, of = target_error_ratios()
    target_ratios = [f"* target rows ({tn} shortened and early rows at L = {4097}): worst error / allowance **{tw:.3f}** ({tname}); "
                     "allowance: what the mix sweep allows `clean` on the row plus 2^-22 s conv(|x|, |h_s|)[n]",
                     f"* `fsn_rir_shorten` on the reference's own responses (`tests/golden/rts_windows.npz`): {differ} of {of} "
                     "values of `out` and `win` are not bit-equal to the reference's (allowed: 2^-22 |ref| + 2^-126 each)"]
    print("\n".join(ratios + target_ratios))
    if args.write:
        stamp = datetime.date.today().isoformat()
        doc = [
            "# Training pairs mixed on the device: time per `fsn_mix_pairs` call", "",
            f"{stamp}, commit {args.commit or '(this change)'}, one MI355X; `tools/bench_mix.py`.  L = 49 152 samples, round(0.75 B) "
            "rows with a room impulse response, descriptors drawn by `draw_item`.  `call`: `mix_batch` = descriptor upload + "
            f"`fsn_mix_pairs`, device events around {args.iters} calls, the median of three windows (and their range); `conv`: "
            "`fsn_conv_rows` alone on the same rows.  `host`: the fp32 numpy port of the same items on 16 worker processes of "
            "the same box (no file I/O).  `step`: the README's AMP training-step time at that batch; `share`: call / step.", "",
            "| B | RIR taps | slab | call (ms) | windows | conv (ms) | host (ms) | host / call | step (ms) | share of a step |",
            "|---|---|---|---|---|---|---|---|---|---|"] + lines + [
            "", "## Per kernel at B = 32", "",
            "Device time per call from torch.profiler over ten calls; bytes: what the stage must move once (inputs read once, "
            "outputs written once), and the time those bytes take at the measured 6.3 TB/s.  The transform's rows are fp64 "
            "complex (16 bytes a point), N = 2^16 for 16 000 taps and 2^17 for 64 000 (min(taps, L) = L).", "",
            "| RIR taps | slab | kernel | us per call | MB | us at 6.3 TB/s |", "|---|---|---|---|---|---|"] + split_lines + [
            "", "The sub-transforms are radix-2 passes in LDS on fp64 data; the radix-8 wave-level passes of `fft_kernels.hip` "
            "were not ported to this plan and have no measured time here.", "",
            "## Error against the fp64 port", ""] + ratios + [
            "", "## Dereverberation targets: time per `fsn_mix_pairs_target` call", "",
            "The same batches, every reverberant row with a target: its response shortened to a T60 of "
            f"{TARGET_T60} s from 2 ms behind its peak on.  `target call`: `mix_batch(target=True)` = descriptor upload + "
            "`fsn_mix_pairs_target` (three rows levelled, `clean` not written); `pairs call`: `fsn_mix_pairs` on the same "
            "descriptors in the same run, the `call` column above.  The second convolution runs the four-step plan a second "
            "time on the shortened taps; a variant that shares transform work between the two convolutions was not built, so "
            "there is no figure for it.", "",
            "| B | RIR taps | slab | target call (ms) | windows | pairs call (ms) | target / pairs |", "|---|---|---|---|---|---|---|"] + target_lines + [
            "", "Per kernel at B = 32 (the three convolution kernels run twice per call and are summed):", "",
            "| RIR taps | slab | kernel | us per call |", "|---|---|---|---|"] + target_split_lines + [""] + target_ratios + [""]
        path = os.path.join(ROOT, "profiles", "mix_pairs.md")
        with open(path, "w") as f:
            f.write("\n".join(doc))
        print(f"wrote {path}")


if __name__ == "__main__":
    main()
