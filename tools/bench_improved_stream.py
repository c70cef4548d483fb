"""Time per frame tick of Improved FullSubNet as a stream at 48 kHz, on one MI355X:

    python tools/bench_improved_stream.py [--streams 1 8 32] [--commit SHA] [--write]

For B streams in lockstep at the reference's 48 kHz configuration (improved_fullsubnet/model.py:603-620: 960 / 480, 481 bins,
sections of 20 / 25 / 6 / 4 units, 512 / 384 hidden units), k = 1:
  step, per section    fsn_improved_stream_step with the sections' blocks as a chain of stateful layer launches per section,
                       odd sections on the auxiliary stream (the library's default)
  step, multi-set      ... as one step launch per layer over all sections (fsn_debug_improved_stream_form(1))
  tick                 StreamingEnhancer(model, batch_size=B).process(one 480-sample hop): STFT slab, model step, mask,
                       overlap-add - beside the 10 ms the hop lasts
Each figure is the median over REPEATS blocks of TICKS calls, timed with device events around the block (one synchronise per
block) after WARMUP calls of the same shape.  --write puts the table into profiles/improved_stream.md."""
import argparse
import ctypes
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, TICKS, REPEATS, HOP = 20, 200, 7, 480
HOP_MS = 10.0
FORMS = {0: "chains", 1: "multi"}


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


def model():
    import torch
    from fullsubnet_amd.improved_fullsubnet import Model
    from fsn_synthetic import IMPROVED_48K, make_improved_params
    m = Model(**IMPROVED_48K, norm_type="cumulative_laplace_norm", sb_norm_type="cumulative_laplace_norm")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_improved_params(IMPROVED_48K, seed=3).items()}, strict=True)
    return m.cuda().eval()


def measure(B, m):
    import torch
    from fullsubnet_amd import _lib
    from fullsubnet_amd.streaming import StreamingEnhancer
    from fsn_synthetic import make_noisy
    L = _lib.lib()
    dev = torch.device("cuda")
    F = m.num_freqs
    mag = torch.rand((B, F, 1), device=dev) + 0.1
    mask = torch.empty((B, 2, F, 1), device=dev)
    cfg = m.stream_cfg()
    c = ctypes.byref(cfg)
    packed = m.stream_packed_weights()
    state = torch.zeros(L.fsn_improved_stream_state_bytes(c, B), dtype=torch.uint8, device=dev)

    def call(steps_done):
        ws = _lib.workspace(L.fsn_improved_stream_workspace_bytes(c, B, 1), dev)
        _lib.check(L.fsn_improved_stream_step(c, packed.data_ptr(), state.data_ptr(), state.numel(), steps_done, _lib.dev_ptr(mag), B, 1,
                                              _lib.dev_ptr(mask), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))

    default = L.fsn_debug_improved_stream_form(-1)
    res = {"streams": B, "default": FORMS[default]}
    for form, name in FORMS.items():
        assert L.fsn_debug_improved_stream_form(form) == form
        state.zero_()
        res[f"{name}_ms"] = timed(call)
    L.fsn_debug_improved_stream_form(default)
    total = WARMUP + TICKS * REPEATS + 2
    noisy = torch.from_numpy(make_noisy(B, HOP * total, seed=1)).cuda()
    enh = StreamingEnhancer(m, batch_size=B)
    enh.process(noisy[:, :HOP])  # the first hop alone completes no frame
    res["tick_ms"] = timed(lambda i: enh.process(noisy[:, (i + 1) * HOP:(i + 2) * HOP]))
    return res


def table(rows, commit):
    one = next((r for r in rows if r["streams"] == 1), None)
    head = "# Improved FullSubNet as a stream at 48 kHz: time per frame tick"
    if one:
        under = one["tick_ms"] < HOP_MS
        head += (f" - one stream's tick of {one['tick_ms']:.3f} ms " + ("stays under" if under else "DOES NOT stay under") +
                 " the 10 ms hop")
    out = [head, "",
           f"{datetime.date.today().isoformat()}, commit {commit}, one MI355X; `tools/bench_improved_stream.py`: k = 1, B streams in "
           f"lockstep, the 48 kHz configuration (960 / 480, 481 bins, 20 / 25 / 6 / 4 units, 512 / 384 hidden), median of {REPEATS} "
           f"blocks of {TICKS} calls after {WARMUP} warm-up calls, device events around each block.", "",
           "| streams | fsn_improved_stream_step, per-section chains on two streams (ms) | ... multi-set step launches (ms) | "
           "multi / chains | StreamingEnhancer.process tick (ms) | share of the 10 ms hop |",
           "|---|---|---|---|---|---|"]
    for r in rows:
        out.append(f"| {r['streams']} | {r['chains_ms']:.3f} | {r['multi_ms']:.3f} | {r['multi_ms'] / r['chains_ms']:.2f} | {r['tick_ms']:.3f} | "
                   f"{r['tick_ms'] / HOP_MS * 100:.1f} % |")
    out.append("")
    if rows:
        out.append(f"The tick runs the library's default form ({rows[0]['default']}).  A k = 1 call enqueues 26 launches and copies in the "
                   "multi-set form (10 around the sections, 3 x 4 + 4 for them) and 38 as chains (10 + 7 x 4); the tick adds the STFT "
                   "slab, the two mask products and the overlap-add of `StreamingEnhancer`.")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--write", action="store_true", help="write profiles/improved_stream.md")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "improved_stream.md"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("bench_improved_stream needs a ROCm device: nothing is measured without one", file=sys.stderr)
        return 1
    m = model()
    rows = []
    for B in args.streams:
        rows.append(measure(B, m))
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
