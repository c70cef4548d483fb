"""Build libfsn_hip.so (gfx950 only) in-tree with hipcc.  Used by __graft_entry__.build().

Every translation unit is compiled to its own object under csrc/_obj/ (only the stale ones, in parallel), then linked.
"""
import concurrent.futures
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libfsn_hip.so")
# every header a translation unit may include: a forgotten one means stale objects
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(HERE, "..", "include", "fsn_hip.h")]
EXPORTS = os.path.join(CSRC, "fsn_exports.map")  # the library exports the fsn_* entries of fsn_hip.h and nothing else
SOURCES = ["fft_kernels.hip", "dft_kernels.hip", "elementwise_kernels.hip", "gemm_kernels.hip",
           "gemm_f16x3_kernels.hip", "lstm_rec_kernels.hip", "lstm_rec_in_kernels.hip", "lstm_rec_x_kernels.hip",
           "lstm_step_kernels.hip", "lstm_group_kernels.hip",
           "lstm_group_bptt_kernels.hip", "lstm_group16_kernels.hip", "fb_chain_kernels.hip", "fb_chain_bptt_kernels.hip",
           "lstm_f16x3_kernels.hip", "bptt_step_kernels.hip", "gemm_tn_kernels.hip", "gemm_tn16_kernels.hip",
           "gru_kernels.hip", "birnn_step_kernels.hip", "optim_kernels.hip",
           "norm_kernels.hip", "section_kernels.hip", "train_glue_kernels.hip", "fast_glue_kernels.hip",
           "stream_pool_kernels.hip", "mix_kernels.hip", "stoi_kernels.hip", "resample_kernels.hip",
           "resample_stream_kernels.hip", "fast_stream_kernels.hip", "fast_stream_pool_kernels.hip",
           "fast_segment_kernels.hip",
           "improved_stream_kernels.hip", "improved_segment_kernels.hip", "improved_stream_pool_kernels.hip",
           "fsn_api.hip", "fsn_api_fast_stream.hip", "fsn_api_improved_stream.hip", "fsn_api_improved_segment.hip",
           "fsn_api_improved_stream_pool.hip", "fsn_api_mix.hip", "fsn_api_metrics.hip", "fsn_api_resample.hip", "fsn_api_fullsubnet.hip", "fsn_api_layers.hip", "fsn_api_gru.hip", "fsn_api_birnn.hip", "fsn_api_train.hip"]
# -ffp-contract=off: elementwise code follows the reference's mul/add rounding sequence; fused
# multiply-adds are written explicitly (fma / MFMA) where they are wanted.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-pass-failed",
         "-Wno-unused-value"]
LINK_FLAGS = ["--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + EXPORTS]


def _sources():
    return [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]


def _obj(src):
    return os.path.join(OBJ, os.path.splitext(src)[0] + ".o")


def _stale(src):
    o = _obj(src)
    if not os.path.exists(o):
        return True
    t = os.path.getmtime(o)
    return any(os.path.getmtime(d) > t for d in [os.path.join(CSRC, src)] + HEADERS)


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in _sources()] + HEADERS + [EXPORTS]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)
    todo = [s for s in _sources() if force or _stale(s)]

    def compile_one(src):
        cmd = [hipcc] + FLAGS + ["-c", os.path.join(CSRC, src), "-o", _obj(src)]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)

    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(len(todo), os.cpu_count() or 1, 16))) as pool:
        list(pool.map(compile_one, todo))
    cmd = [hipcc] + LINK_FLAGS + [_obj(s) for s in _sources()] + ["-o", LIB]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
