// nbest.hip -- consensus over the N-best list a search ends with: the unit-cost Levenshtein distances among the hypotheses of
// an utterance, the expected distance (risk) of each under the posteriors and the hypothesis of least risk (las_nbest_risk); the alignment
// of every hypothesis to a pivot and the posterior mass that agrees with each pivot token (las_nbest_confidence).  The reference has
// nothing of this kind; the yardstick is the numpy restatement tests/nbest_ref.py.
//
// One wavefront per dynamic programme, no atomics, nothing depends on the launch geometry:
//   nb_edit_dp            rows i = tokens of a, columns j = tokens of b, 64 columns (one per lane) at a time, all rows of a column chunk
//                         before the next chunk.  With t[j] = min(D[i-1][j] + 1, D[i-1][j-1] + cost) the in-row dependency resolves to
//                         D[i][j] = j + min(D[i][j0-1] - (j0-1), prefixmin_{j0 <= k <= j} (t[k] - k)): one inclusive wave scan (six DPP steps) per
//                         row, the chunk's left boundary column D[., j0-1] travels through LDS (one word per row, written by lane 63 of the
//                         chunk before).  The row above lives in a register per lane, the diagonal comes from the lane below (wave_shr:1):
//                         per row one LDS broadcast read (the a token), one LDS read and one LDS write.
//                         Back-trace directions (2 bits per cell, the header's rule evaluated where the cell is computed) are packed by every
//                         lane over 16 consecutive rows of its column and stored coalesced: [ceil(U/16), pitch] words per hypothesis.
//   nbest_pairs_kernel    one wave per unordered pair (i < j) of live slots, four pairs per workgroup: 64 x 16 hypotheses are 7,680 waves
//   nbest_risk_kernel     one workgroup per utterance: lane i adds w[k] * dist[i][k] over k in order (product and sum separate), lane 0 picks
//   nbest_align_kernel    one wave per live hypothesis: the DP against the pivot with directions into the workspace
//   nbest_trace_kernel    one workgroup per utterance, a wave per hypothesis in turn: the direction words are staged into LDS in whole
//                         16-row blocks (as many as fit 8 KB), lane 0 walks them, the match row is collected in LDS and stored coalesced;
//                         then conf is summed over the match rows in slot order
// The directions have ONE home, the workspace: at U = 1024 a hypothesis' table is 256 KB and cannot live in LDS, and the staged walk reads
// LDS at every size (the argument of ctc_align.hip).
// Bounds: U <= NB_MAX_U because a wave keeps the a tokens and the boundary column (2 x 4 KB) in static LDS, four waves to a workgroup.
#include "las_common.h"

// risk and conf are one fp32 product and one fp32 sum per slot: the compiler must not fuse them (hipcc contracts by default; the
// pragma covers the operators written in this file, which is why the sums below use * and + and not __fmul_rn / __fadd_rn, whose
// bodies live in a header compiled with contraction on)
#pragma clang fp contract(off)

namespace {

constexpr int NB_MAX_U = 1024;           // tokens per hypothesis
constexpr int NB_MAX_K = 64;             // hypothesis slots per utterance (one lane each in nbest_risk_kernel)
constexpr int NB_WAVES = 4;              // dynamic programmes per workgroup
constexpr int NB_BIG = 1 << 24;          // "no candidate" in the prefix minimum (distances are <= 1024)
constexpr int NB_STAGE = 2048;           // direction words a wave stages at a time (8 KB): >= 2 row blocks of <= 1024 columns

__host__ __device__ inline int nb_pitch(int U) { return (U + 63) / 64 * 64; }
__host__ __device__ inline int nb_rows(int U) { return (U + 15) / 16; }
__host__ __device__ inline size_t nb_dir_words(int U) { return (size_t)nb_rows(U) * nb_pitch(U); }

__device__ __forceinline__ int nb_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// orders one wave's own LDS traffic (a wave's lanes exchange data through LDS without a workgroup barrier)
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// lane l reads lane l - CTRL's source; a lane without a source (or in a row ROWS masks out) keeps its own value.  EVERY lane must be active.
template <int CTRL, int ROWS> __device__ __forceinline__ int dpp_keep(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, ROWS, 0xf, false); }

// inclusive prefix minimum over the 64 lanes: row_shr:1, 2, 4, 8 inside the 16-lane rows, then row_bcast:15 into rows 1 and 3 and
// row_bcast:31 into rows 2 and 3
__device__ __forceinline__ int wave_prefix_min(int v) {
    v = min(v, dpp_keep<0x111, 0xf>(v));
    v = min(v, dpp_keep<0x112, 0xf>(v));
    v = min(v, dpp_keep<0x114, 0xf>(v));
    v = min(v, dpp_keep<0x118, 0xf>(v));
    v = min(v, dpp_keep<0x142, 0xa>(v));
    v = min(v, dpp_keep<0x143, 0xc>(v));
    return v;
}

// Levenshtein distance of a[0:La] and b[0:Lb] by one FULL wave (wave-uniform arguments); sa [>= La] and col [>= La + 1] are the wave's LDS.
// DIRS: the direction of every cell (i, j >= 1) goes to dirs[((i-1) / 16) * pitch + (j-1)], bits 2 ((i-1) % 16): 0 match, 1 substitution,
// 2 up (the a token stays unmatched), 3 left -- the header's rule in its order.
template <bool DIRS>
__device__ __forceinline__ int nb_edit_dp(const int* __restrict__ a, int La, const int* __restrict__ b, int Lb, int* sa, int* col,
                                          unsigned* __restrict__ dirs, int pitch) {
    const int lane = threadIdx.x & 63;
    La = __builtin_amdgcn_readfirstlane(La);                                   // (wave-uniform already: scalar loop counters)
    Lb = __builtin_amdgcn_readfirstlane(Lb);
    if (Lb == 0) return La;
    for (int i = lane; i < La; i += 64) sa[i] = a[i];
    for (int i = lane; i <= La; i += 64) col[i] = i;                           // D[i][0]
    wave_lds_sync();
    int up = 0;
    for (int j0 = 1; j0 <= Lb; j0 += 64) {
        const int j = j0 + lane;
        const bool act = j <= Lb;
        const int bj = act ? b[j - 1] : 0;
        int dprev = j0 - 1;                                                    // D[i-1][j0-1]
        unsigned bits = 0;
        up = j;                                                                // D[0][j]
        for (int i = 1; i <= La; ++i) {
            const int ai = sa[i - 1], cin = col[i];                            // (uniform addresses: broadcasts)
            int diag = __builtin_amdgcn_update_dpp(up, up, 0x138, 0xf, 0xf, false);    // wave_shr:1
            if (lane == 0) diag = dprev;
            const bool eq = ai == bj;
            const int t = min(up + 1, diag + (eq ? 0 : 1));
            const int x = wave_prefix_min(act ? t - j : NB_BIG);
            const int d = j + min(cin - (j0 - 1), x);
            if (DIRS) {
                const unsigned k = (eq && d == diag) ? 0u : (d == diag + 1 ? 1u : (d == up + 1 ? 2u : 3u));
                bits |= k << (2 * ((i - 1) & 15));
                if (((i - 1) & 15) == 15 || i == La) {
                    if (act) dirs[(size_t)((i - 1) >> 4) * pitch + (j - 1)] = bits;
                    bits = 0;
                }
            }
            dprev = cin;
            up = d;
            if (lane == 63) col[i] = d;                                        // D[i][j0+63]: the next chunk's boundary column
        }
        wave_lds_sync();
    }
    return __shfl(up, (Lb - 1) & 63);                                          // D[La][Lb] sits in the last chunk
}

// grid (ceil(K (K-1) / 2 / NB_WAVES), n), 64 NB_WAVES threads
__global__ __launch_bounds__(64 * NB_WAVES) void nbest_pairs_kernel(const int* __restrict__ tok, const int* __restrict__ len,
                                                                    const int* __restrict__ nhyp, int K, int U, int* __restrict__ dist) {
    __shared__ int sa[NB_WAVES][NB_MAX_U];
    __shared__ int col[NB_WAVES][NB_MAX_U + 1];
    const int u = blockIdx.y, wv = threadIdx.x >> 6;
    int p = blockIdx.x * NB_WAVES + wv;
    if (p >= K * (K - 1) / 2) return;
    int i = 0;
    while (p >= K - 1 - i) { p -= K - 1 - i; ++i; }                            // pair p of the upper triangle, row by row
    const int j = i + 1 + p;
    if (j >= nb_clamp(nhyp[u], K)) return;
    const size_t r = (size_t)u * K;
    const int d = nb_edit_dp<false>(tok + (r + i) * U, nb_clamp(len[r + i], U), tok + (r + j) * U, nb_clamp(len[r + j], U), sa[wv], col[wv],
                                    nullptr, 0);
    if ((threadIdx.x & 63) == 0) {
        dist[(r + i) * K + j] = d;
        dist[(r + j) * K + i] = d;
    }
}

// grid n, 64 threads: lane i = slot i
__global__ __launch_bounds__(64) void nbest_risk_kernel(const int* __restrict__ nhyp, const float* __restrict__ w, int K, int* __restrict__ dist,
                                                        float* __restrict__ risk, int* __restrict__ pick) {
    __shared__ float sr[NB_MAX_K], sw[NB_MAX_K];
    const int u = blockIdx.x, i = threadIdx.x;
    const int nh = nb_clamp(nhyp[u], K);
    const size_t r = (size_t)u * K;
    if (i < nh) {
        dist[(r + i) * K + i] = 0;
        float acc = 0.f;
        for (int k = 0; k < nh; ++k) {
            const int d = k == i ? 0 : dist[(r + i) * K + k];
            const float prod = w[r + k] * (float)d;                            // product and sum apart: numpy float32's bits
            acc = acc + prod;
        }
        risk[r + i] = acc;
        sr[i] = acc;
        sw[i] = w[r + i];
    }
    __syncthreads();
    if (i == 0) {
        int best = nh > 0 ? 0 : -1;
        for (int k = 1; k < nh; ++k)
            if (sr[k] < sr[best] || (sr[k] == sr[best] && sw[k] > sw[best])) best = k;     // ties: the larger w, then the lower index
        pick[u] = best;
    }
}

__device__ __forceinline__ int nb_pivot(const int* pivot, int u, int nh) {      // -1: nothing is written for the utterance
    const int pv = pivot[u];
    return (pv >= 0 && pv < nh) ? pv : -1;
}

// grid (ceil(K / NB_WAVES), n), 64 NB_WAVES threads: wave = slot k
__global__ __launch_bounds__(64 * NB_WAVES) void nbest_align_kernel(const int* __restrict__ tok, const int* __restrict__ len,
                                                                    const int* __restrict__ nhyp, const int* __restrict__ pivot, int K, int U,
                                                                    unsigned* __restrict__ dirs) {
    __shared__ int sa[NB_WAVES][NB_MAX_U];
    __shared__ int col[NB_WAVES][NB_MAX_U + 1];
    const int u = blockIdx.y, wv = threadIdx.x >> 6, k = blockIdx.x * NB_WAVES + wv;
    const int nh = nb_clamp(nhyp[u], K);
    if (k >= nh) return;
    const int pv = nb_pivot(pivot, u, nh);
    if (pv < 0) return;
    const size_t r = (size_t)u * K;
    nb_edit_dp<true>(tok + (r + pv) * U, nb_clamp(len[r + pv], U), tok + (r + k) * U, nb_clamp(len[r + k], U), sa[wv], col[wv],
                     dirs + (r + k) * nb_dir_words(U), nb_pitch(U));
}

// grid n, 64 NB_WAVES threads
__global__ __launch_bounds__(64 * NB_WAVES) void nbest_trace_kernel(const int* __restrict__ len, const int* __restrict__ nhyp,
                                                                    const float* __restrict__ w, const int* __restrict__ pivot, int K, int U,
                                                                    const unsigned* __restrict__ dirs, signed char* __restrict__ match,
                                                                    float* __restrict__ conf) {
    __shared__ unsigned stage[NB_WAVES][NB_STAGE];
    __shared__ signed char hit[NB_WAVES][NB_MAX_U];
    const int u = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nh = nb_clamp(nhyp[u], K);
    const int pv = nb_pivot(pivot, u, nh);
    if (pv < 0) return;                                                        // (the whole workgroup)
    const size_t r = (size_t)u * K;
    const int La = nb_clamp(len[r + pv], U), pitch = nb_pitch(U);
    unsigned* st = stage[wv];
    signed char* m = hit[wv];
    for (int k = wv; k < nh; k += NB_WAVES) {
        const unsigned* dw = dirs + (r + k) * nb_dir_words(U);
        for (int i = lane; i < La; i += 64) m[i] = 0;
        int i = La, j = nb_clamp(len[r + k], U);
        while (i > 0 && j > 0) {                                               // (wave-uniform)
            // columns [0, j) of the row blocks lo .. hi: what the walk can still visit, as many blocks as fit
            const int hi = (i - 1) >> 4, jw = j;
            const int fit = NB_STAGE / jw;                                     // >= 2
            const int lo = hi + 1 - fit > 0 ? hi + 1 - fit : 0;
            for (int rb = lo; rb <= hi; ++rb)
                for (int c = lane; c < jw; c += 64) st[(rb - lo) * jw + c] = dw[(size_t)rb * pitch + c];
            wave_lds_sync();
            if (lane == 0) {
                while (i > 0 && j > 0 && ((i - 1) >> 4) >= lo) {
                    const unsigned d = (st[(((i - 1) >> 4) - lo) * jw + (j - 1)] >> (2 * ((i - 1) & 15))) & 3u;
                    if (d == 0) m[i - 1] = 1;
                    if (d <= 2) --i;
                    if (d != 2) --j;
                }
            }
            i = __builtin_amdgcn_readfirstlane(i);
            j = __builtin_amdgcn_readfirstlane(j);
            wave_lds_sync();
        }
        wave_lds_sync();
        for (int q = lane; q < La; q += 64) match[(r + k) * U + q] = m[q];
        wave_lds_sync();
    }
    __syncthreads();                                                           // the match rows of all waves, read back below
    for (int q = threadIdx.x; q < La; q += 64 * NB_WAVES) {
        float acc = 0.f;
        for (int k = 0; k < nh; ++k) {
            const float prod = w[r + k] * (float)match[(r + k) * U + q];
            acc = acc + prod;
        }
        conf[(size_t)u * U + q] = acc;
    }
}

int nb_check_sizes(const char* who, int n, int K, int U) {
    LAS_ARG(n > 0 && n <= 65535, "%s: 1 <= n <= 65535 (got %d)", who, n);
    LAS_ARG(K >= 1 && K <= NB_MAX_K, "%s: 1 <= K <= %d hypothesis slots (got %d)", who, NB_MAX_K, K);
    LAS_ARG(U >= 1 && U <= NB_MAX_U, "%s: U=%d tokens per hypothesis, 1 <= U <= %d", who, U, NB_MAX_U);
    return 0;
}

}  // namespace

extern "C" size_t las_nbest_workspace_bytes(int n, int K, int U) {
    if (n <= 0 || K <= 0 || U <= 0) return 0;
    return (size_t)n * K * nb_dir_words(U) * sizeof(unsigned);
}

extern "C" int las_nbest_risk(const int* tok, const int* len, const int* nhyp, const float* w, int n, int K, int U, int* dist, float* risk,
                              int* pick, void* stream) {
    LAS_ARG(tok && len && nhyp && w && dist && risk && pick, "las_nbest_risk: tok, len, nhyp, w, dist, risk and pick must be given");
    if (nb_check_sizes("las_nbest_risk", n, K, U)) return -1;
    hipStream_t s = (hipStream_t)stream;
    if (K > 1) {
        hipLaunchKernelGGL(nbest_pairs_kernel, dim3(cdiv(K * (K - 1) / 2, NB_WAVES), n), dim3(64 * NB_WAVES), 0, s, tok, len, nhyp, K, U, dist);
        LAS_LAUNCHED();
    }
    hipLaunchKernelGGL(nbest_risk_kernel, dim3(n), dim3(64), 0, s, nhyp, w, K, dist, risk, pick);
    LAS_LAUNCHED();
    return 0;
}

extern "C" int las_nbest_confidence(const int* tok, const int* len, const int* nhyp, const float* w, const int* pivot, int n, int K, int U,
                                    signed char* match, float* conf, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(tok && len && nhyp && w && pivot && match && conf,
            "las_nbest_confidence: tok, len, nhyp, w, pivot, match and conf must be given");
    if (nb_check_sizes("las_nbest_confidence", n, K, U)) return -1;
    LAS_ARG(ws && ws_bytes >= las_nbest_workspace_bytes(n, K, U), "las_nbest_confidence: workspace too small (%zu < %zu)", ws_bytes,
            las_nbest_workspace_bytes(n, K, U));
    LAS_ARG(((uintptr_t)ws & 3) == 0, "las_nbest_confidence: the workspace must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nbest_align_kernel, dim3(cdiv(K, NB_WAVES), n), dim3(64 * NB_WAVES), 0, s, tok, len, nhyp, pivot, K, U, (unsigned*)ws);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(nbest_trace_kernel, dim3(n), dim3(64 * NB_WAVES), 0, s, len, nhyp, w, pivot, K, U, (const unsigned*)ws, match, conf);
    LAS_LAUNCHED();
    return 0;
}
