// Launchers of birnn_step_kernels.hip, called from fsn_api_birnn.hip: a bidirectional nn.LSTM / nn.GRU layer, both
// directions of a time step in ONE launch.  Step s of a layer over T frames advances the forward direction at frame s and
// the reverse direction at frame T - 1 - s; BPTT step s takes the forward direction at frame T - 1 - s and the reverse one
// at frame s.  Direction 0 is forward, direction 1 is torch's `*_reverse`.
#pragma once
#include "fsn_common.h"

// Forward.  gx: fragment-ordered input projection of BOTH directions, tile (frame t, row tile i, column tile c) at
// (t * N / 16 + i) * 2 g H / 16 + c with direction d's gate k of unit group u at c = d g H / 16 + k H / 16 + u (g = 4 / 3).
// hseq [T][N][ldh]: direction d's hidden state in columns [d H, (d + 1) H).  save[d] (training, else NULL): the activated
// gates [T][N][4H] (LSTM i | f | g | o, GRU r | z | n | hn) and, LSTM only, the cell sequence [T][N][H] behind them.
// c[d] [N][H]: the LSTM's cell state of direction d in inference (save == NULL), updated in place.
struct FsnBiLayer {
    const float* gx;
    const float* whh_p[2];  // packed W_hh of each direction
    const float* b_hn[2];   // GRU: b_hh's n block of each direction
    float* hseq;
    long ldh;
    float* c[2];
    float* save[2];
    int T, N, H;
};
int fsn_launch_bilstm_step(const FsnBiLayer& L, int s, hipStream_t stream);
int fsn_launch_bigru_step(const FsnBiLayer& L, int s, hipStream_t stream);

// BPTT.  dh [T][N][lddh] with direction d's gradient in columns [d H, (d + 1) H); dg [T][N][2 g H]: the gate gradients of
// both directions side by side; GRU: dghn[d] [T][N][H]; carry[d] [N][H]: dc (LSTM) / the
// z-path carry (GRU), first written at s == 0.
struct FsnBiBptt {
    const float* dh;
    long lddh;
    const float* whhT_p[2];  // packed W_hh^T of each direction
    const float* save[2];
    const float* hseq;
    long ldh;
    float* dg;
    float* dghn[2];
    float* carry[2];
    int T, N, H;
};
int fsn_launch_bilstm_bptt_step(const FsnBiBptt& B, int s, hipStream_t stream);
int fsn_launch_bigru_bptt_step(const FsnBiBptt& B, int s, hipStream_t stream);

// out [rows][ldo], columns [0, cols) = a + b, both [rows][ld]: the two directions' shares of dX
int fsn_launch_add_rows(const float* a, const float* b, long ld, float* out, long ldo, long rows, int cols, hipStream_t stream);

// dst [T][N][ldd], columns [0, K) = the same columns of src [T][N][lds] at frame T - 1 - t: a direction's operands in the
// order ITS recurrence visits them, so that the weight-gradient sums of the reverse direction run in step order
int fsn_launch_time_flip(const float* src, long lds, float* dst, long ldd, int T, int N, int K, hipStream_t stream);
