// rescore.hip -- K10i: two-pass decoding: the attention decoder's log-likelihood of given token strings, read off the
// teacher-forced Speller's logits, and the re-ranking of a first pass' N-best list with it.
//
// las_rescore_score   one workgroup of 256 lanes per (row, step) over logits [R, U, V] taken in place through strides (as las_ce_loss):
//                     row maximum, sum of exp, lse = m + logf(s), term = z[y] - lse.  The first 20 classes of a lane (5120 of the row)
//                     stay in registers between the maximum and the sum: such a row is read once; classes from 5120 on are read twice.
//                     Lane i reads classes i, i + 256, ...: one dword per lane, so a wave reads 256 consecutive bytes whatever the
//                     alignment of the row base (rows are V floats apart: with odd V only every fourth base is 16-byte aligned, and
//                     nothing here needs it to be).  Measured against it: one 16-byte load per four classes where the base is aligned, four
//                     bounds-checked dwords where it is not -- 23.4 against 19.4 us on 64 x 77 x 5000 logits: the dword form
//                     already reads faster than a device copy moves.  Steps t >= len[r] are neither read nor written.  A second launch,
//                     one wave per row, adds a row's terms in step order in float64.
// las_rescore_rank    one workgroup of 64 lanes per utterance: total = (float)((1 - w) att + w first), each product and the sum rounded
//                     on its own (nothing contracted); a slot's rank is the count of the slots that come before it.
// No atomics: two runs give the same bits.
#include "las_common.h"
#include <math.h>

namespace {

constexpr int SCORE_NT = 256;
constexpr int SCORE_REGS = 20;                        // classes a lane keeps in registers: 5120 in all (as las_ctc_frame_topk)
constexpr int RANK_MAX_K = 64;
constexpr int SUM_NT = 64;

__global__ __launch_bounds__(SCORE_NT) void rescore_score_kernel(const float* __restrict__ logits, long long sb, long long st,
                                                                 const int* __restrict__ y, int ldy, const int* __restrict__ len, int U,
                                                                 int V, float* __restrict__ terms, int ldt) {
    __shared__ float red[SCORE_NT / 64];
    const int r = blockIdx.x / U, t = blockIdx.x - r * U, tid = threadIdx.x;
    const int L = clampi(len[r], 0, U);
    if (t >= L) return;
    const float* z = logits + (long long)r * sb + (long long)t * st;

    float reg[SCORE_REGS];
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < SCORE_REGS; ++j) {
        const int v = tid + SCORE_NT * j;
        reg[j] = v < V ? z[v] : -INFINITY;                             // (a class past V: no maximum, and expf(-inf - m) adds +0)
        m = fmaxf(m, reg[j]);
    }
    for (int v = tid + SCORE_NT * SCORE_REGS; v < V; v += SCORE_NT) m = fmaxf(m, z[v]);
    m = block_max<SCORE_NT>(m, red);
    float term = -INFINITY;                                            // (m = -inf: no class has mass; z - m would be NaN)
    const int c = y[(size_t)r * ldy + t];
    if (m > -INFINITY) {                                               // (uniform: m is the workgroup's)
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < SCORE_REGS; ++j) s += expf(reg[j] - m);
        for (int v = tid + SCORE_NT * SCORE_REGS; v < V; v += SCORE_NT) s += expf(z[v] - m);
        s = block_sum<SCORE_NT>(s, red);
        if (tid == 0 && c >= 0 && c < V) term = z[c] - (m + logf(s));
    }
    if (tid == 0) terms[(size_t)r * ldt + t] = term;                   // (a label outside [0, V): -inf, nothing read for it)
}

// one wave per row: its terms in step order in float64
__global__ __launch_bounds__(SUM_NT) void rescore_sum_kernel(const float* __restrict__ terms, int ldt, const int* __restrict__ len, int U,
                                                             double* __restrict__ att) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const double s = wave_terms_sum_f64(terms + (size_t)r * ldt, clampi(len[r], 0, U), lane);
    if (lane == 0) att[r] = s;
}

__global__ __launch_bounds__(RANK_MAX_K) void rescore_rank_kernel(const float* __restrict__ first, const double* __restrict__ att,
                                                                  const int* __restrict__ nhyp, int K, double w,
                                                                  float* __restrict__ total, int* __restrict__ order) {
    __shared__ float tot[RANK_MAX_K];
    const int u = blockIdx.x, k = threadIdx.x;
    const int nh = clampi(nhyp[u], 0, K);
    const size_t base = (size_t)u * K;
    float mine = 0.f;
    if (k < nh) {
        mine = (float)__dadd_rn(__dmul_rn(1.0 - w, att[base + k]), __dmul_rn(w, (double)first[base + k]));
        tot[k] = mine;
        total[base + k] = mine;
    }
    __syncthreads();
    if (k >= nh) return;
    // slots that come before k: a larger total, or the same total in a lower slot; NaN behind every number, among themselves in slot order
    const bool nan_k = mine != mine;
    int rank = 0;
    for (int j = 0; j < nh; ++j) {
        const float tj = tot[j];
        const bool nan_j = tj != tj;
        const bool before = nan_k ? (!nan_j || j < k) : (!nan_j && (tj > mine || (tj == mine && j < k)));
        rank += before ? 1 : 0;
    }
    order[base + rank] = k;                                            // (the ranks of nh slots are a permutation of 0 .. nh - 1)
}

}  // namespace

extern "C" size_t las_rescore_workspace_bytes(int R, int U) {
    if (R <= 0 || U <= 0) return 0;
    return (size_t)R * (size_t)U * sizeof(float);
}

extern "C" int las_rescore_score(const float* logits, long long sb, long long st, const int* y, int ldy, const int* len, int R, int U,
                                 int V, double* att, float* step_lp, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(logits && y && len && att, "las_rescore_score: null pointer");
    LAS_ARG(R > 0 && U > 0 && V >= 1 && V <= (1 << 30) && (long long)R * U <= 0x7fffffffLL, "las_rescore_score: bad dims (R = %d, U = %d, V = %d)", R, U, V);
    LAS_ARG(ldy >= U, "las_rescore_score: ldy = %d < U = %d", ldy, U);
    LAS_ARG(sb >= 0 && st >= 0, "las_rescore_score: negative stride");
    float* terms = step_lp;
    int ldt = ldy;
    if (!terms) {
        const size_t need = las_rescore_workspace_bytes(R, U);
        LAS_ARG(ws && ws_bytes >= need, "las_rescore_score: without step_lp a workspace of %zu bytes is needed (got %zu)", need, ws ? ws_bytes : (size_t)0);
        terms = (float*)ws;
        ldt = U;
    }
    hipLaunchKernelGGL(rescore_score_kernel, dim3(R * U), dim3(SCORE_NT), 0, (hipStream_t)stream, logits, sb, st, y, ldy, len, U, V, terms, ldt);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(rescore_sum_kernel, dim3(R), dim3(SUM_NT), 0, (hipStream_t)stream, terms, ldt, len, U, att);
    LAS_LAUNCHED();
    return 0;
}

extern "C" int las_rescore_rank(const float* first, const double* att, const int* nhyp, int n, int K, double w, float* total, int* order,
                                void* stream) {
    LAS_ARG(first && att && nhyp && total && order, "las_rescore_rank: null pointer");
    LAS_ARG(n > 0, "las_rescore_rank: bad dims (n = %d)", n);
    LAS_ARG(K >= 1 && K <= RANK_MAX_K, "las_rescore_rank: 1 <= K <= %d (got %d)", RANK_MAX_K, K);
    LAS_ARG(w >= 0.0 && w <= 1.0, "las_rescore_rank: the weight is inside [0, 1] (got %g)", w);       // (NaN fails both comparisons)
    hipLaunchKernelGGL(rescore_rank_kernel, dim3(n), dim3(RANK_MAX_K), 0, (hipStream_t)stream, first, att, nhyp, K, w, total, order);
    LAS_LAUNCHED();
    return 0;
}
