"""Time per frame and peak memory of long recordings on Fast FullSubNet at B = 1 on one MI355X, through the one call
(``Model.enhance``) and through segments with carried state (``Model.enhance_long``), in the form of tools/bench_long.py:

    python tools/bench_long_fast.py [--minutes 2 10] [--segments 256 1024 4096] [--long-minutes 60] [--commit SHA] --write

For every recording length: ``enhance`` and ``enhance_long`` at each ``segment_frames``; for ``--long-minutes`` (beyond the
65 535 frames ``enhance`` takes) ``enhance_long`` alone, at the segment its default workspace limit picks - the only run that
crosses 65 535 frames on the device (no test does).  A run is one child process under a time limit: the call is warmed first
(on the recording itself up to ten minutes, so that the allocator already holds its buffers; on a 20-second recording
beyond), then the whole call is timed on the host clock, a device synchronise at both ends; recordings of up to two minutes
take the median of three calls, longer ones are timed once.  Peak memory is PyTorch's peak allocated bytes over the timed
call, the recording itself ([1, L] floats on the device) included.  The parent never opens the device and stops at the first
child that fails.  ``--write`` puts the table into profiles/long_recording_fast.md."""
import argparse
import datetime
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HOP, SR = 256, 16000
ONE_CALL_FRAMES = 65535  # fsn_fast_decoder_input's limit
CHILD_LIMIT_S = 380
FAST_KW = dict(look_ahead=2, shrink_size=2, sequence_model="LSTM", num_mels=64, encoder_input_size=257, bottleneck_hidden_size=384,
               bottleneck_num_layers=2, noisy_input_num_neighbors=5, encoder_output_num_neighbors=0,
               norm_type="offline_laplace_norm", weight_init=False)  # BASELINE config 4


def measure(minutes, segment_frames):
    """segment_frames: 0 = Model.enhance, -1 = enhance_long at its default workspace limit, else enhance_long at that k."""
    import torch
    from fullsubnet_amd.fast_fullsubnet import Model
    from fullsubnet_amd.fast_long_form import FastLongPlan
    from fsn_synthetic import make_fast_params, make_noisy

    model = Model(**FAST_KW)
    sd = {k: torch.from_numpy(v) for k, v in make_fast_params(seed=3).items()}
    sd["mel_scale.fb"] = model.mel_scale.fb.clone()
    model.load_state_dict(sd, strict=True)
    model = model.cuda().eval()
    L = int(minutes * 60 * SR)
    # one seeded minute, repeated (an hour of fresh noise is minutes of host time): the model's cost does not depend on the samples
    base = torch.from_numpy(make_noisy(1, min(L, 60 * SR), seed=1))
    noisy = base.repeat(1, -(-L // base.shape[1]))[:, :L].contiguous().cuda()
    k = None if segment_frames < 0 else segment_frames
    run = (lambda x: model.enhance(x)) if segment_frames == 0 else (lambda x: model.enhance_long(x, segment_frames=k))
    run(noisy if minutes <= 10 else noisy[:, :20 * SR])  # warm-up: kernels loaded, the allocator holding the call's buffers
    torch.cuda.synchronize()
    times = []
    torch.cuda.reset_peak_memory_stats()
    for _ in range(3 if minutes <= 2 else 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = run(noisy)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    peak = torch.cuda.max_memory_allocated()
    assert out.shape == noisy.shape and bool(torch.isfinite(out).all())
    frames = 1 + L // HOP
    used = 0 if segment_frames == 0 else FastLongPlan(model.stream_cfg(), model.look_ahead, 1, L, k).segment_frames
    return {"minutes": minutes, "frames": frames, "segment_frames": used, "default_k": segment_frames < 0,
            "seconds": sorted(times)[len(times) // 2], "calls": len(times), "peak_bytes": peak}


def table(rows, commit, long_minutes):
    out = ["# Fast FullSubNet, long recordings: time per frame and peak memory, B = 1", "",
           f"{datetime.date.today().isoformat()}, commit {commit}, one MI355X; `tools/bench_long_fast.py`: the shipped Fast FullSubNet "
           "configuration (BASELINE config 4: shrink 2, look-ahead 2, offline_laplace_norm, fp32), 16 kHz, hop 256.  Host clock "
           "around the whole call with a device synchronise at both ends, after one warm-up call (on the recording itself up to "
           "ten minutes, on a 20-second one beyond); up to two minutes the median of three calls, longer recordings one call.  "
           "Peak memory: PyTorch's peak allocated bytes over the call, the recording on the device included.", "",
           "| recording | frames | path | seconds | us per frame | x real time | vs one call | peak memory (MB) | MB per 1000 frames |",
           "|---|---|---|---|---|---|---|---|---|"]
    one_call = {r["minutes"]: r["seconds"] for r in rows if r["segment_frames"] == 0}
    for r in rows:
        path = "`enhance` (one call)" if r["segment_frames"] == 0 else (
            f"`enhance_long`, segment_frames {r['segment_frames']}" + (" (default: 4 GiB workspace limit)" if r["default_k"] else ""))
        ref = one_call.get(r["minutes"])
        rel = "-" if r["segment_frames"] == 0 or ref is None else f"{r['seconds'] / ref:.2f} x"
        out.append(f"| {r['minutes']:g} min | {r['frames']} | {path} | {r['seconds']:.3f} | {r['seconds'] / r['frames'] * 1e6:.1f} | "
                   f"{r['minutes'] * 60 / r['seconds']:.0f} | {rel} | {r['peak_bytes'] / 1e6:.0f} | "
                   f"{r['peak_bytes'] / 1e6 / r['frames'] * 1000:.1f} |")
    crossed = [r for r in rows if r["frames"] > ONE_CALL_FRAMES]
    out += ["",
            "`vs one call`: the segment path's time over `enhance` on the same recording (above 1: slower, below 1: faster).  "
            "The segment path makes three passes over the recording (the model divides by two utterance means) where the one "
            "call makes one, and runs every recurrence as per-step launches on carried state (four layers per step and the "
            "bottleneck's per low-rate frame), where the one call runs the encoder pair and the decoder pair as one chain-kernel "
            "launch each: per frame the segment path is the slower one wherever both run, by the same factor at every "
            "`segment_frames`.  What it buys is the recording's length and its memory.  Larger batches, where the one call "
            "moves to persistent kernels the segment path does not use, are not measured here - so `[inferencer] "
            f"segment_frames` stays an explicit key and not a heuristic.  Recordings beyond {ONE_CALL_FRAMES} frames (17.5 "
            "minutes) have no one-call row: `enhance` refuses them.", "",
            (f"The {crossed[-1]['minutes']:g}-minute row ran: {crossed[-1]['frames']} frames, the only run of the project that crosses "
             f"{ONE_CALL_FRAMES} frames of this model on the device (its output was checked for shape and finiteness only)."
             if crossed else
             f"No row beyond {ONE_CALL_FRAMES} frames ran (--long-minutes {long_minutes:g}): crossing that count on the device is unmeasured.")]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, nargs="+", default=[2, 10])
    ap.add_argument("--segments", type=int, nargs="+", default=[256, 1024, 4096])
    ap.add_argument("--long-minutes", type=float, default=60)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--write", action="store_true", help="write profiles/long_recording_fast.md")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_recording_fast.md"))
    ap.add_argument("--one", type=float, nargs=2, metavar=("MINUTES", "SEGMENT"), help="(child) one run, one JSON line")
    args = ap.parse_args()
    if args.one:
        print("RESULT " + json.dumps(measure(args.one[0], int(args.one[1]))), flush=True)
        return 0
    runs = [(m, k) for m in args.minutes for k in [0] + args.segments]
    if args.long_minutes > 0:
        runs.append((args.long_minutes, -1))
    rows = []
    for m, k in runs:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(m), str(k)], capture_output=True,
                               text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"{m} min / {k}: no result within {CHILD_LIMIT_S} s; stopping", file=sys.stderr)
            return 1
        res = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not res:
            print(f"{m} min / {k}: child failed ({p.returncode}); stopping\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        rows.append(json.loads(res[-1][len("RESULT "):]))
        print(rows[-1], flush=True)
    text = table(rows, args.commit, args.long_minutes)
    print(text)
    if args.write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
