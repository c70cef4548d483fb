"""Time per frame tick of Fast FullSubNet as a stream, beside FullSubNet's, on one MI355X:

    python tools/bench_fast_stream.py [--streams 1 8 32 64] [--commit SHA] [--write]

For B streams in lockstep at the shipped configuration (shrink 2, look-ahead 2, neighbours (5, 0), bottleneck 384 x 2), k = 1:
  fast step, bottleneck   fsn_fast_stream_step at a step t % shrink == 0: a low-rate frame completes, the bottleneck runs
  fast step, held         ... at a step t % shrink != 0: no frame completes, the held output serves (n_low = 0)
  fullsubnet step         fsn_fullsubnet_stream_step at the same B (the existing code: the comparison)
  fast tick / fsn tick    StreamingEnhancer(model, batch_size=B).process(one hop): STFT slab, model step, mask, overlap-add
Each figure is the median over REPEATS blocks of TICKS calls, timed with device events around the block (one synchronise per
block) after WARMUP calls of the same shape.  --write puts the table into profiles/fast_stream.md."""
import argparse
import ctypes
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, TICKS, REPEATS, HOP = 20, 200, 7, 256
HOP_MS = 16.0


def timed(call):
    """ms per call(i): median over REPEATS event-timed blocks of TICKS calls, i counting on from the warm-up."""
    import torch
    i = 0
    for _ in range(WARMUP):
        call(i)
        i += 1
    torch.cuda.synchronize()
    blocks = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(TICKS):
            call(i)
            i += 1
        b.record()
        b.synchronize()
        blocks.append(a.elapsed_time(b) / TICKS)
    blocks.sort()
    return blocks[len(blocks) // 2]


def models():
    import torch
    import fullsubnet_amd
    from fullsubnet_amd.fast_fullsubnet import Model as FastModel
    from fsn_synthetic import make_fast_params, make_params
    fast = FastModel(look_ahead=2, shrink_size=2, sequence_model="LSTM", num_mels=64, encoder_input_size=257, bottleneck_hidden_size=384,
                     bottleneck_num_layers=2, noisy_input_num_neighbors=5, encoder_output_num_neighbors=0,
                     norm_type="cumulative_laplace_norm")
    sd = {k: torch.from_numpy(v) for k, v in make_fast_params(seed=3).items()}
    sd["mel_scale.fb"] = fast.mel_scale.fb.clone()
    fast.load_state_dict(sd, strict=True)
    full = fullsubnet_amd.Model(num_freqs=257, look_ahead=2, sequence_model="LSTM", fb_num_neighbors=0, sb_num_neighbors=15,
                                fb_output_activate_function="ReLU", sb_output_activate_function=False, fb_model_hidden_size=512,
                                sb_model_hidden_size=384, norm_type="cumulative_laplace_norm", num_groups_in_drop_band=1, weight_init=False)
    full.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(seed=3).items()})
    return fast.cuda().eval(), full.cuda().eval()


def measure(B, fast, full):
    import torch
    from fullsubnet_amd import _lib
    from fullsubnet_amd.streaming import StreamingEnhancer
    from fsn_synthetic import make_noisy
    L = _lib.lib()
    dev = torch.device("cuda")
    mag = torch.rand((B, 1, 257, 1), device=dev) + 0.1
    crm = torch.empty((B, 2, 257, 1), device=dev)

    def entry(step, bytes_of, ws_of, cfg, packed):
        state = torch.zeros(bytes_of(cfg, B), dtype=torch.uint8, device=dev)

        def call(steps_done):
            ws = _lib.workspace(ws_of(cfg, B, 1), dev)
            _lib.check(step(cfg, packed.data_ptr(), state.data_ptr(), state.numel(), steps_done, _lib.dev_ptr(mag), B, 1, _lib.dev_ptr(crm),
                            ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
        return call

    fcfg = fast.stream_cfg()
    fast_call = entry(L.fsn_fast_stream_step, L.fsn_fast_stream_state_bytes, L.fsn_fast_stream_workspace_bytes, ctypes.byref(fcfg),
                      fast.stream_packed_weights())
    full_call = entry(L.fsn_fullsubnet_stream_step, L.fsn_fullsubnet_stream_state_bytes, L.fsn_fullsubnet_stream_workspace_bytes,
                      ctypes.byref(full._cfg), full.packed_weights())
    res = {"streams": B,
           "fast_bn_ms": timed(lambda i: fast_call(2 * i)),        # t % 2 == 0: a low-rate frame completes
           "fast_held_ms": timed(lambda i: fast_call(2 * i + 1)),  # t % 2 == 1: n_low = 0
           "full_ms": timed(full_call)}
    total = WARMUP + TICKS * REPEATS + 2
    noisy = torch.from_numpy(make_noisy(B, HOP * total, seed=1)).cuda()
    for name, model in (("fast_tick_ms", fast), ("full_tick_ms", full)):
        enh = StreamingEnhancer(model, batch_size=B)
        enh.process(noisy[:, :HOP])  # the first hop alone completes no frame
        res[name] = timed(lambda i: enh.process(noisy[:, (i + 1) * HOP:(i + 2) * HOP]))
    return res


def table(rows, commit):
    out = ["# Fast FullSubNet as a stream: time per frame tick", "",
           f"{datetime.date.today().isoformat()}, commit {commit}, one MI355X; `tools/bench_fast_stream.py`: k = 1, B streams in lockstep, "
           f"shipped configuration (shrink 2, look-ahead 2, neighbours (5, 0), bottleneck 384 x 2), median of {REPEATS} blocks of {TICKS} "
           f"calls after {WARMUP} warm-up calls, device events around each block.", "",
           "| streams | fast step, a low-rate frame completes (ms) | fast step, held output (ms) | fast step, mean of the two phases (ms) | "
           "fsn_fullsubnet_stream_step (ms) | fast / FullSubNet | StreamingEnhancer.process tick, fast (ms) | ... FullSubNet (ms) | "
           "fast tick, share of the 16 ms hop |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        mean = 0.5 * (r["fast_bn_ms"] + r["fast_held_ms"])
        out.append(f"| {r['streams']} | {r['fast_bn_ms']:.3f} | {r['fast_held_ms']:.3f} | {mean:.3f} | {r['full_ms']:.3f} | {mean / r['full_ms']:.2f} | "
                   f"{r['fast_tick_ms']:.3f} | {r['full_tick_ms']:.3f} | {r['fast_tick_ms'] / HOP_MS * 100:.1f} % |")
    out.append("")
    one = next((r for r in rows if r["streams"] == 1), None)
    if one:
        worst = max(one["fast_tick_ms"], one["fast_bn_ms"])
        verdict = "stays under" if worst < HOP_MS else "DOES NOT stay under"
        out.append(f"One stream's tick {verdict} the 16 ms hop it serves: {one['fast_tick_ms']:.3f} ms per `process` call (the two phases of a "
                   f"block alternate in it), {one['fast_bn_ms']:.3f} ms for the step with the bottleneck alone: a margin of "
                   f"{HOP_MS / worst:.1f} x.")
    out.append("Columns: the two fast-step columns are the same entry at the two phases of a down-sampling block of 2 - at even steps the "
               "bottleneck's two layers run on B x 64 rows, at odd steps they are skipped.  The ticks add the STFT slab, the mask and the "
               "overlap-add of `StreamingEnhancer` around the step.  Every LSTM layer of the fast step is the per-step stateful layer entry "
               "(a projection GEMM, a step launch per frame and a state copy), so a k = 1 call enqueues 28 launches and copies with the "
               "bottleneck and 21 without it.")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32, 64])
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--write", action="store_true", help="write profiles/fast_stream.md")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fast_stream.md"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_fast_stream needs a ROCm device: nothing is measured without one", file=sys.stderr)
        return 1
    fast, full = models()
    rows = []
    for B in args.streams:
        rows.append(measure(B, fast, full))
        print(rows[-1], flush=True)
    text = table(rows, args.commit)
    print(text)
    if args.write:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
