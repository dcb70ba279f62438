// nbest.hip -- consensus over the N-best list a search ends with: the unit-cost Levenshtein distances among the hypotheses of
// an utterance, the expected distance (risk) of each under the posteriors and the hypothesis of least risk (las_nbest_risk); the alignment
// of every hypothesis to a pivot and the posterior mass that agrees with each pivot token (las_nbest_confidence).  The reference has
// nothing of this kind; the yardstick is the numpy restatement tests/nbest_ref.py.  At the end of the file: the list's confusion
// network (las_nbest_network; yardstick tests/confnet_ref.py), which shares the scan and the direction packing below.
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
            int diag = wave_shr1_keep(up);                                     // D[i-1][j-1] of the lane before
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
    if (j >= clampi(nhyp[u], 0, K)) return;
    const size_t r = (size_t)u * K;
    const int d = nb_edit_dp<false>(tok + (r + i) * U, clampi(len[r + i], 0, U), tok + (r + j) * U, clampi(len[r + j], 0, U), sa[wv], col[wv],
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
    const int nh = clampi(nhyp[u], 0, K);
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
    const int nh = clampi(nhyp[u], 0, K);
    if (k >= nh) return;
    const int pv = nb_pivot(pivot, u, nh);
    if (pv < 0) return;
    const size_t r = (size_t)u * K;
    nb_edit_dp<true>(tok + (r + pv) * U, clampi(len[r + pv], 0, U), tok + (r + k) * U, clampi(len[r + k], 0, U), sa[wv], col[wv],
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
    const int nh = clampi(nhyp[u], 0, K);
    const int pv = nb_pivot(pivot, u, nh);
    if (pv < 0) return;                                                        // (the whole workgroup)
    const size_t r = (size_t)u * K;
    const int La = clampi(len[r + pv], 0, U), pitch = nb_pitch(U);
    unsigned* st = stage[wv];
    signed char* m = hit[wv];
    for (int k = wv; k < nh; k += NB_WAVES) {
        const unsigned* dw = dirs + (r + k) * nb_dir_words(U);
        for (int i = lane; i < La; i += 64) m[i] = 0;
        int i = La, j = clampi(len[r + k], 0, U);
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

// ---- las_nbest_network (include/las_hip.h K10h) ------------------------------------------------------------------------------
// One workgroup of ONE wave per utterance: the merges of an utterance are sequential, the utterances run side by side.  A bin is a ROW of
// the workspace that never moves -- [slot symbols | distinct symbols in order of their first contributing slot], 4 ceil(K/4) words each --
// and the network is the order of the rows: ord (LDS) maps a bin's place to its row, cnt (LDS, per row) holds the length of the
// distinct-symbol list and whether EPS is in it.  Per merge of hypothesis b into the B bins so far:
//   pre-pass   lane = bin: cup(i) and the first column D[i][0] (a wave prefix sum, carried over the 64-bin blocks) into LDS
//   per chunk of 64 columns
//     masks    lane = bin: has(i, b_j) for the chunk's 64 columns as one 64-bit word per bin, from the bin's distinct symbols (a few
//              entries, four to a load, the next load in flight under the compares; scanning the slots merged so far would be up to 63).
//              The loads of 64 bins are in flight together and nothing of this sits on the row-to-row chain
//     rows     nb_edit_dp's row step: lane = column, the up move costs the row-uniform cup(i), the diagonal asks bit `lane` of the bin's mask
//   walk       lane 0 over the staged direction words (nbest_trace_kernel's staging); step t describes the new network's bin B + ins - 1 - t:
//              the place it had (or, for a new bin, the row it gets), b's token or EPS, and whether that symbol is new to the bin -- which
//              the rule that fired already says (a match: no; a cost-1 diagonal: yes; EPS: cup(i); a new bin: yes).  The tails along
//              i = 0 / j = 0 need no table and are written by all lanes
//   rebuild    lane = step, all steps independent: the bin's row gets b's symbol in slot k (a new row EPS in the slots before) and, where it
//              is new, one more distinct symbol; the new order goes into the other half of ord.  Stores only: no row is read or moved
// At the end cols is the rows' slot symbols gathered in bin order, and one lane per bin adds the masses in slot order.
namespace {

constexpr int CN_MAX_BINS = 2048;
constexpr int CN_EPS = -1;
constexpr int CN_NEW = 0x4000;                                                 // in a step's token word: the symbol is new to its bin

__host__ __device__ inline int cn_kp(int K) { return (K + 3) & ~3; }           // a row's two halves start 16-byte aligned
__host__ __device__ inline size_t cn_dir_words(int U, int max_bins) { return (size_t)nb_rows(max_bins) * nb_pitch(U); }
__host__ __device__ inline size_t cn_utt_words(int K, int U, int max_bins) { return cn_dir_words(U, max_bins) + (size_t)max_bins * 2 * cn_kp(K); }

// grid n, 64 threads
__global__ __launch_bounds__(64) void nbest_network_kernel(const int* __restrict__ sym, const int* __restrict__ len, const int* __restrict__ nhyp,
                                                           const float* __restrict__ w, int K, int U, int max_bins, unsigned* ws, int* cols,
                                                           int* nbins, signed char* merged, int* best, float* post) {
    __shared__ unsigned long long smask[CN_MAX_BINS];                          // has(i, b_j) of the chunk in flight, bit = lane
    __shared__ int col[CN_MAX_BINS + 1];                                       // the boundary column D[., j0-1]
    __shared__ __attribute__((aligned(16))) int sb[NB_MAX_U];                  // b, negatives read as 0 (read four tokens at a time)
    __shared__ unsigned stage[NB_STAGE];
    __shared__ short psrc[CN_MAX_BINS], ptok[CN_MAX_BINS];                     // the walk's steps, back to front
    __shared__ short ord[2][CN_MAX_BINS];                                      // place -> row, the current and the next network
    __shared__ unsigned char cnt[CN_MAX_BINS], scup[CN_MAX_BINS];              // per row: distinct symbols, bit 7 = EPS among them; per place: cup
    __shared__ float sw[NB_MAX_K];
    const int u = blockIdx.x, lane = threadIdx.x;
    const int nh = __builtin_amdgcn_readfirstlane(clampi(nhyp[u], 0, K));
    const size_t r = (size_t)u * K;
    const int Kp = cn_kp(K);
    unsigned* dirs = ws + (size_t)u * cn_utt_words(K, U, max_bins);
    int* rows = (int*)(dirs + cn_dir_words(U, max_bins));                      // row p: slot symbols at rows[p 2 Kp], distinct symbols Kp behind
    const int pitch = nb_pitch(U);
    int B = 0, nmerged = 0, cur = 0;
    unsigned long long mmask = 0;                                              // bit k: slot k was merged
    if (lane < nh) sw[lane] = w[r + lane];
    for (int k = 0; k < nh; ++k) {
        const int L = __builtin_amdgcn_readfirstlane(clampi(len[r + k], 0, U));
        const int* b = sym + (r + k) * U;
        __syncthreads();                                                       // the merge before is done with the LDS, and its stores are visible
        for (int j = lane; j < L; j += 64) sb[j] = max(b[j], 0);
        int carry = 0;
        for (int i0 = 0; i0 < B; i0 += 64) {
            const int i = i0 + lane;
            const int cu = (i < B && !(cnt[ord[cur][i]] & 0x80)) ? 1 : 0;
            int sc = cu;
            for (int o = 1; o < 64; o <<= 1) {
                const int v = __shfl_up(sc, o);
                if (lane >= o) sc += v;
            }
            if (i < B) {
                scup[i] = (unsigned char)cu;
                col[i + 1] = carry + sc;
            }
            carry += __shfl(sc, 63);
        }
        if (lane == 0) col[0] = 0;
        __syncthreads();
        if (B > 0 && L > 0) {
            for (int j0 = 1; j0 <= L; j0 += 64) {
                // all 64 columns of the chunk, four tokens to an LDS read, a fixed trip count so that the reads run ahead of the compares;
                // columns beyond L hold whatever sb held before (written or not): their bits are computed and never used
                const int4* tb = (const int4*)(sb + j0 - 1);
                for (int i = lane; i < B; i += 64) {
                    const int row = ord[cur][i], n = cnt[row] & 0x7f;
                    const int4* ds = (const int4*)(rows + ((size_t)row * 2 + 1) * Kp);
                    unsigned long long m = 0;
                    int4 v = ds[0];
                    for (int c = 0; c < n; c += 4) {
                        int4 nx = v;
                        if (c + 4 < n) nx = ds[(c >> 2) + 1];
                        const int e0 = v.x, e1 = c + 1 < n ? v.y : -2, e2 = c + 2 < n ? v.z : -2, e3 = c + 3 < n ? v.w : -2;    // (-2: no symbol)
#pragma unroll 4
                        for (int g = 0; g < 16; ++g) {
                            const int4 t = tb[g];
                            const unsigned h = (unsigned)((t.x == e0) | (t.x == e1) | (t.x == e2) | (t.x == e3)) |
                                               (unsigned)((t.y == e0) | (t.y == e1) | (t.y == e2) | (t.y == e3)) << 1 |
                                               (unsigned)((t.z == e0) | (t.z == e1) | (t.z == e2) | (t.z == e3)) << 2 |
                                               (unsigned)((t.w == e0) | (t.w == e1) | (t.w == e2) | (t.w == e3)) << 3;
                            m |= (unsigned long long)h << (4 * g);
                        }
                        v = nx;
                    }
                    smask[i] = m;
                }
                __syncthreads();
                const int j = j0 + lane;
                const bool act = j <= L;
                int dprev = j0 - 1;
                unsigned bits = 0;
                int up = j;
                for (int i = 1; i <= B; ++i) {
                    const unsigned long long m = smask[i - 1];                 // (uniform addresses: broadcasts)
                    const int cu = scup[i - 1], cin = col[i];
                    int diag = wave_shr1_keep(up);                                     // D[i-1][j-1] of the lane before
                    if (lane == 0) diag = dprev;
                    const bool eq = (m >> lane) & 1ull;
                    const int t = min(up + cu, diag + (eq ? 0 : 1));
                    const int x = wave_prefix_min(act ? t - j : NB_BIG);
                    const int d = j + min(cin - (j0 - 1), x);
                    const unsigned dk = (eq && d == diag) ? 0u : (d == diag + 1 ? 1u : (d == up + cu ? 2u : 3u));
                    bits |= dk << (2 * ((i - 1) & 15));
                    if (((i - 1) & 15) == 15 || i == B) {
                        if (act) dirs[(size_t)((i - 1) >> 4) * pitch + (j - 1)] = bits;
                        bits = 0;
                    }
                    dprev = cin;
                    up = d;
                    if (lane == 63) col[i] = d;
                }
                __syncthreads();
            }
        }
        // the walk from (B, L): step t describes the new network's bin B + ins - 1 - t
        int i = B, j = L, t = 0, ins = 0;
        while (i > 0 && j > 0) {                                               // (wave-uniform)
            const int hi = (i - 1) >> 4, jw = j;
            const int fit = NB_STAGE / jw;                                     // >= 2
            const int lo = hi + 1 - fit > 0 ? hi + 1 - fit : 0;
            for (int rb = lo; rb <= hi; ++rb)
                for (int c = lane; c < jw; c += 64) stage[(rb - lo) * jw + c] = dirs[(size_t)rb * pitch + c];
            __syncthreads();
            if (lane == 0) {
                while (i > 0 && j > 0 && ((i - 1) >> 4) >= lo) {
                    const unsigned d = (stage[(((i - 1) >> 4) - lo) * jw + (j - 1)] >> (2 * ((i - 1) & 15))) & 3u;
                    if (t < CN_MAX_BINS) {
                        psrc[t] = (short)(d == 3 ? -1 - ins : i - 1);
                        ptok[t] = (short)(d == 2 ? -1 : (d == 0 ? j : j | CN_NEW));
                    }
                    ++t;
                    if (d == 3) ++ins;
                    if (d <= 2) --i;
                    if (d != 2) --j;
                }
            }
            i = __builtin_amdgcn_readfirstlane(i);
            j = __builtin_amdgcn_readfirstlane(j);
            t = __builtin_amdgcn_readfirstlane(t);
            ins = __builtin_amdgcn_readfirstlane(ins);
            __syncthreads();
        }
        for (int q = lane; q < i; q += 64)                                     // column 0: the remaining bins get EPS
            if (t + q < CN_MAX_BINS) {
                psrc[t + q] = (short)(i - 1 - q);
                ptok[t + q] = -1;
            }
        for (int q = lane; q < j; q += 64)                                     // row 0: the remaining tokens become new bins at the front
            if (t + q < CN_MAX_BINS) {
                psrc[t + q] = (short)(-1 - ins - q);
                ptok[t + q] = (short)((j - q) | CN_NEW);
            }
        ins += j;
        __syncthreads();
        const int Bn = B + ins;
        if (Bn > max_bins) continue;                                           // the overflow rule: the network stays as it is
        for (int q = lane; q < Bn; q += 64) {
            const int src = psrc[q], tk = ptok[q];
            const int s = tk < 0 ? CN_EPS : sb[(tk & (CN_NEW - 1)) - 1];
            int row;
            if (src >= 0) {
                row = ord[cur][src];
                int* rp = rows + (size_t)row * 2 * Kp;
                rp[k] = s;
                if (tk < 0 ? scup[src] != 0 : (tk & CN_NEW) != 0) {            // one more distinct symbol
                    const int c = cnt[row], n = c & 0x7f;
                    if (n < K) rp[Kp + n] = s;
                    cnt[row] = (unsigned char)((c & 0x80) | (n < K ? n + 1 : n) | (tk < 0 ? 0x80 : 0));
                }
            } else {                                                           // a new bin in the row B + (its number among the new ones)
                row = B - 1 - src;
                int* rp = rows + (size_t)row * 2 * Kp;
                for (int l = 0; l < k; ++l) rp[l] = CN_EPS;
                rp[k] = s;
                if (nmerged > 0) rp[Kp] = CN_EPS;                              // EPS for every slot merged before
                rp[Kp + (nmerged > 0 ? 1 : 0)] = s;
                cnt[row] = (unsigned char)(nmerged > 0 ? 0x82 : 1);
            }
            ord[cur ^ 1][Bn - 1 - q] = (short)row;
        }
        cur ^= 1;
        B = Bn;
        ++nmerged;
        mmask |= 1ull << k;
    }
    __syncthreads();
    if (lane == 0) nbins[u] = B;
    if (lane < nh) merged[r + lane] = (signed char)((mmask >> lane) & 1ull);
    for (int k = 0; k < nh; ++k) {
        if (!((mmask >> k) & 1ull)) continue;
        for (int i = lane; i < B; i += 64) cols[(r + k) * max_bins + i] = rows[(size_t)ord[cur][i] * 2 * Kp + k];
    }
    for (int i = lane; i < B; i += 64) {
        const int row = ord[cur][i], n = cnt[row] & 0x7f;
        const int* rp = rows + (size_t)row * 2 * Kp;
        int bs = CN_EPS;
        float bm = 0.f;
        for (int c = 0; c < n; ++c) {                                          // the list is in order of the first contributing slot
            const int s = rp[Kp + c];
            float acc = 0.f;
            for (int k = 0; k < nh; ++k)
                if (((mmask >> k) & 1ull) && rp[k] == s) acc = acc + sw[k];
            if (c == 0 || acc > bm) {
                bs = s;
                bm = acc;
            }
        }
        best[(size_t)u * max_bins + i] = bs;
        post[(size_t)u * max_bins + i] = bm;
    }
}

}  // namespace

extern "C" size_t las_nbest_network_workspace_bytes(int n, int K, int U, int max_bins) {
    if (n <= 0 || K <= 0 || U <= 0 || max_bins <= 0) return 0;
    return (size_t)n * cn_utt_words(K, U, max_bins) * sizeof(unsigned);
}

extern "C" int las_nbest_network(const int* sym, const int* len, const int* nhyp, const float* w, int n, int K, int U, int max_bins, int* cols,
                                 int* nbins, signed char* merged, int* best, float* post, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(sym && len && nhyp && w && cols && nbins && merged && best && post,
            "las_nbest_network: sym, len, nhyp, w, cols, nbins, merged, best and post must be given");
    if (nb_check_sizes("las_nbest_network", n, K, U)) return -1;
    LAS_ARG(max_bins >= 1 && max_bins <= CN_MAX_BINS, "las_nbest_network: max_bins=%d, 1 <= max_bins <= %d", max_bins, CN_MAX_BINS);
    LAS_ARG(ws && ws_bytes >= las_nbest_network_workspace_bytes(n, K, U, max_bins), "las_nbest_network: workspace too small (%zu < %zu)",
            ws_bytes, las_nbest_network_workspace_bytes(n, K, U, max_bins));
    LAS_ARG(((uintptr_t)ws & 15) == 0, "las_nbest_network: the workspace must be 16-byte aligned");
    hipLaunchKernelGGL(nbest_network_kernel, dim3(n), dim3(64), 0, (hipStream_t)stream, sym, len, nhyp, w, K, U, max_bins, (unsigned*)ws, cols,
                       nbins, merged, best, post);
    LAS_LAUNCHED();
    return 0;
}
