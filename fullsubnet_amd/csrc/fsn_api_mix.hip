// C ABI of the on-device mixing of training pairs: fsn_conv_rows, fsn_mix_pairs, fsn_rir_shorten, fsn_mix_pairs_target
// and their size queries
// (include/fsn_hip.h "training pairs mixed on the device"; kernels: mix_kernels.hip).
#include <stddef.h>

#include "fsn_api_internal.h"

namespace {

constexpr int kMinLogN = 2;   // the four-step split wants two factors
// (the longest: 2 FSN_MIX_MAX_L - 1 <= 2^18 = 512 x 512, two sub-transforms of the kernels' LDS size)

// log2 of the circular length that holds L samples convolved with h_len (> 0) taps, cut at L outputs
int conv_log_n(int L, int h_len) {
    const long need = (long)L + (h_len < L ? h_len : L) - 1;
    int k = kMinLogN;
    while ((1L << k) < need) ++k;
    return k;
}

size_t z_bytes(int B, int logN) { return (size_t)B * ((size_t)16 << logN); }

// What the transform part of a workspace pays for: the largest circular length up to the one of max_h_len = L whose B rows
// fit in `bytes` (*logN; 0 with *planned false: none - rows with a response come back as NaN).
void conv_plan(int B, int L, size_t bytes, int* logN, bool* planned) {
    *planned = false;
    *logN = conv_log_n(L, 1);  // indexes the row for the copies
    for (int k = conv_log_n(L, L); k >= conv_log_n(L, 1); --k)
        if (z_bytes(B, k) <= bytes) {
            *logN = k;
            *planned = true;
            return;
        }
}

bool shape_ok(const char* who, int B, int L, int max_h_len) {
    if (B < 1 || L < 1 || L > FSN_MIX_MAX_L || max_h_len < 0) {
        fsn_set_error("%s: B = %d, L = %d, longest response %d: B >= 1, 1 <= L <= %d and a length >= 0 are required", who, B, L,
                      max_h_len, FSN_MIX_MAX_L);
        return false;
    }
    return true;
}

// the transform part of a workspace: B ints (rows whose signal and response are not all zeros), then the transform's rows
size_t live_bytes(int B) { return fsn_round_up_sz((size_t)B * sizeof(int), 256); }
size_t conv_part_bytes(int B, int L, int max_h_len) {
    return live_bytes(B) + (max_h_len > 0 ? z_bytes(B, conv_log_n(L, max_h_len)) : 0);
}

size_t row_bytes(int B, int L) { return fsn_round_up_sz((size_t)B * L * sizeof(float), 256); }

// fsn_mix_pairs_target on top of fsn_mix_pairs: the second convolution's row, the shortened taps ([B][tap_ld(L)]: taps
// from L on reach no output, and the call - unlike the size query - is not told the longest response) and their Taps
int tap_ld(int L) { return (L + 3) & ~3; }  // rows of whole 16-byte words
size_t target_part_bytes(int B, int L) {
    return row_bytes(B, L) + row_bytes(B, tap_ld(L)) + fsn_round_up_sz((size_t)B * sizeof(long), 256) +
           fsn_round_up_sz((size_t)B * sizeof(int), 256);
}

int workspace_ok(const char* who, const void* workspace, size_t workspace_bytes, size_t least) {
    FSN_REQUIRE(workspace, "%s: NULL workspace", who);
    FSN_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
    if (workspace_bytes < least) {
        fsn_set_error("%s: workspace of %zu bytes, at least %zu are needed", who, workspace_bytes, least);
        return FSN_ERR_WORKSPACE;
    }
    return FSN_OK;
}

}  // namespace

extern "C" size_t fsn_conv_rows_workspace_bytes(int B, int L, int max_h_len) {
    if (!shape_ok("fsn_conv_rows_workspace_bytes", B, L, max_h_len)) return 0;
    return conv_part_bytes(B, L, max_h_len);
}

extern "C" int fsn_conv_rows(const float* x, int B, int L, const void* h_slab, int slab_format, const long* h_off,
                             const int* h_len, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    if (!shape_ok("fsn_conv_rows", B, L, 0)) return FSN_ERR_ARG;
    FSN_REQUIRE(slab_format == FSN_SLAB_F32 || slab_format == FSN_SLAB_I16, "fsn_conv_rows: slab_format %d", slab_format);
    FSN_REQUIRE(x && y && h_slab && h_off && h_len, "fsn_conv_rows: NULL pointer argument");
    FSN_REQUIRE(x != y, "fsn_conv_rows: y must not alias x");
    FSN_TRY(workspace_ok("fsn_conv_rows", workspace, workspace_bytes, conv_part_bytes(B, L, 0)));
    int logN;
    bool planned;
    conv_plan(B, L, workspace_bytes - live_bytes(B), &logN, &planned);
    FsnCallScope scope(stream);
    return fsn_launch_conv_rows(x, B, L, h_slab, slab_format, h_off, sizeof(long), h_len, sizeof(int), y,
                                planned ? static_cast<char*>(workspace) + live_bytes(B) : nullptr, static_cast<int*>(workspace),
                                logN, static_cast<hipStream_t>(stream));
}

extern "C" size_t fsn_mix_workspace_bytes(int B, int L, int max_rir_len) {
    if (!shape_ok("fsn_mix_workspace_bytes", B, L, max_rir_len)) return 0;
    return 3 * row_bytes(B, L) + conv_part_bytes(B, L, max_rir_len);
}

extern "C" int fsn_mix_pairs(const void* clean_slab, const void* noise_slab, const void* rir_slab, int slab_format,
                             const fsn_mix_item* items, const fsn_mix_seg* segs, int n_segs, int B, int L, float eps,
                             float* noisy, float* clean, void* workspace, size_t workspace_bytes, void* stream) {
    if (!shape_ok("fsn_mix_pairs", B, L, 0)) return FSN_ERR_ARG;
    FSN_REQUIRE(slab_format == FSN_SLAB_F32 || slab_format == FSN_SLAB_I16, "fsn_mix_pairs: slab_format %d", slab_format);
    FSN_REQUIRE(n_segs >= 0, "fsn_mix_pairs: n_segs = %d", n_segs);
    FSN_REQUIRE(eps >= 0.f, "fsn_mix_pairs: eps = %g", (double)eps);
    FSN_REQUIRE(clean_slab && noise_slab && items && noisy && clean && (segs || n_segs == 0),
                "fsn_mix_pairs: NULL pointer argument");
    FSN_REQUIRE(noisy != clean, "fsn_mix_pairs: noisy and clean must be two arrays");
    FSN_TRY(workspace_ok("fsn_mix_pairs", workspace, workspace_bytes, 3 * row_bytes(B, L) + conv_part_bytes(B, L, 0)));
    Carver ws(workspace);
    float* c0 = ws.take<float>((size_t)B * L);
    float* c1 = ws.take<float>((size_t)B * L);
    float* nz = ws.take<float>((size_t)B * L);
    int* live = ws.take<int>(B);
    char* Z = ws.take<char>(0);
    int logN;
    bool planned;
    conv_plan(B, L, workspace_bytes - ws.off, &logN, &planned);
    FSN_REQUIRE(rir_slab || !planned, "fsn_mix_pairs: NULL response slab with a workspace sized for responses");
    FsnCallScope scope(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FSN_TRY(fsn_launch_mix_gather(clean_slab, noise_slab, slab_format, items, segs, n_segs, B, L, c0, nz, s));
    FSN_TRY(fsn_launch_conv_rows(c0, B, L, rir_slab, slab_format, &items->rir_off, sizeof(fsn_mix_item), &items->rir_len,
                                 sizeof(fsn_mix_item), c1, planned ? Z : nullptr, live, logN, s));
    return fsn_launch_mix_level(c1, nz, items, B, L, eps, noisy, clean, s);
}

extern "C" int fsn_rir_shorten(const void* h_slab, int slab_format, const long* h_off, const int* h_len, int B, int max_h_len,
                               const fsn_mix_target* targets, float* out, int ld, float* win, int* idx, void* stream) {
    FSN_REQUIRE(B >= 1 && max_h_len >= 0, "fsn_rir_shorten: B = %d, longest response %d: B >= 1 and a length >= 0 are required",
                B, max_h_len);
    FSN_REQUIRE(slab_format == FSN_SLAB_F32 || slab_format == FSN_SLAB_I16, "fsn_rir_shorten: slab_format %d", slab_format);
    FSN_REQUIRE(h_slab && h_off && h_len && targets && out, "fsn_rir_shorten: NULL pointer argument");
    FSN_REQUIRE(ld >= max_h_len && ld >= 1, "fsn_rir_shorten: ld = %d is too small for the longest response of %d taps", ld,
                max_h_len);
    FSN_REQUIRE(out != win, "fsn_rir_shorten: out and win must be two arrays");
    FsnCallScope scope(stream);
    return fsn_launch_rir_shorten(h_slab, slab_format, h_off, sizeof(long), h_len, sizeof(int), B, targets, out, ld, win, idx,
                                  nullptr, nullptr, static_cast<hipStream_t>(stream));
}

extern "C" size_t fsn_mix_target_workspace_bytes(int B, int L, int max_rir_len) {
    if (!shape_ok("fsn_mix_target_workspace_bytes", B, L, max_rir_len)) return 0;
    return 3 * row_bytes(B, L) + target_part_bytes(B, L) + conv_part_bytes(B, L, max_rir_len);
}

extern "C" int fsn_mix_pairs_target(const void* clean_slab, const void* noise_slab, const void* rir_slab, int slab_format,
                                    const fsn_mix_item* items, const fsn_mix_seg* segs, int n_segs, int B, int L, float eps,
                                    const fsn_mix_target* targets, float* noisy, float* clean, float* target, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (!shape_ok("fsn_mix_pairs_target", B, L, 0)) return FSN_ERR_ARG;
    FSN_REQUIRE(slab_format == FSN_SLAB_F32 || slab_format == FSN_SLAB_I16, "fsn_mix_pairs_target: slab_format %d", slab_format);
    FSN_REQUIRE(n_segs >= 0, "fsn_mix_pairs_target: n_segs = %d", n_segs);
    FSN_REQUIRE(eps >= 0.f, "fsn_mix_pairs_target: eps = %g", (double)eps);
    FSN_REQUIRE(clean_slab && noise_slab && items && targets && noisy && target && (segs || n_segs == 0),
                "fsn_mix_pairs_target: NULL pointer argument");
    FSN_REQUIRE(noisy != clean && noisy != target && clean != target,
                "fsn_mix_pairs_target: noisy, clean and target must be three arrays");
    FSN_TRY(workspace_ok("fsn_mix_pairs_target", workspace, workspace_bytes,
                         3 * row_bytes(B, L) + target_part_bytes(B, L) + conv_part_bytes(B, L, 0)));
    Carver ws(workspace);
    float* c0 = ws.take<float>((size_t)B * L);
    float* c1 = ws.take<float>((size_t)B * L);
    float* nz = ws.take<float>((size_t)B * L);
    float* c2 = ws.take<float>((size_t)B * L);
    float* hs = ws.take<float>((size_t)B * tap_ld(L));
    long* t_off = ws.take<long>(B);
    int* t_len = ws.take<int>(B);
    int* live = ws.take<int>(B);
    char* Z = ws.take<char>(0);
    int logN;
    bool planned;
    conv_plan(B, L, workspace_bytes - ws.off, &logN, &planned);
    FSN_REQUIRE(rir_slab || !planned, "fsn_mix_pairs_target: NULL response slab with a workspace sized for responses");
    FsnCallScope scope(stream);
    hipStream_t s = static_cast<hipStream_t>(stream);
    FSN_TRY(fsn_launch_mix_gather(clean_slab, noise_slab, slab_format, items, segs, n_segs, B, L, c0, nz, s));
    FSN_TRY(fsn_launch_conv_rows(c0, B, L, rir_slab, slab_format, &items->rir_off, sizeof(fsn_mix_item), &items->rir_len,
                                 sizeof(fsn_mix_item), c1, planned ? Z : nullptr, live, logN, s));
    // the same plan a second time, on the shortened taps (the transform and its flags are free again: same stream)
    FSN_TRY(fsn_launch_rir_shorten(planned ? rir_slab : nullptr, slab_format, &items->rir_off, sizeof(fsn_mix_item), &items->rir_len,
                                   sizeof(fsn_mix_item), B, targets, hs, tap_ld(L), nullptr, nullptr, t_off, t_len, s));
    FSN_TRY(fsn_launch_conv_rows(c0, B, L, hs, FSN_SLAB_F32, t_off, sizeof(long), t_len, sizeof(int), c2,
                                 planned ? Z : nullptr, live, logN, s));
    return fsn_launch_mix_level_target(c1, nz, c2, t_len, items, B, L, eps, noisy, clean, target, s);
}
