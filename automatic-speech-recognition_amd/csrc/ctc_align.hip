// ctc_align.hip -- CTC Viterbi (forced) alignment of a token sequence to the encoder frames: the max-plus form of the
// extended-label recursion of ctc.hip with a back-trace.  Input: las_ctc_log_softmax's class-major log-probabilities [n, Vc, T'],
// blank = class Vc - 1.  The reference has nothing of this kind; the yardstick is the float64 restatement tests/ctc_align_ref.py.
//
// Three launches, stream-ordered on the caller's stream, no atomics:
//   ctc_align_gather_kernel   one workgroup per (utterance, 64 frames, 64 columns): the rows lp[u, blank, :] and lp[u, y_j, :] (contiguous
//                             over t) are read coalesced, transposed through LDS and written frame-major [n, T', U+1] (column 0 blank,
//                             column j+1 label j): what the recursion's lanes read at one frame is contiguous
//   ctc_align_viterbi_kernel  one workgroup per utterance, one extended-label state per lane (S = 2L+1 <= 1023), best-path scores in fp64 in
//                             two LDS buffers, ONE barrier per frame.  best(t, s) = lp + max(prev(s), prev(s-1), prev(s-2) if allowed);
//                             on equal values the smaller step wins.  The chain has T' dependent steps (latency-bound): the emissions are
//                             loaded CA_PF frames ahead into a register ring and the barrier orders LDS traffic only, so those loads (and
//                             the back-pointer stores) stay in flight across it.  Every lane packs its 2-bit step choices of 16 consecutive
//                             frames into one word and stores it to the workspace: [n, ceil(T'/16), SP] words, coalesced, off the chain.
//   ctc_align_trace_kernel    one workgroup per utterance: the back-pointer words are staged into LDS in blocks of whole 16-frame rows (as
//                             many as fit: all of them at the recipe's T' = 319, S = 383; 128 frames at a time at S = 1023), one lane walks
//                             the T' dependent steps there, then frame_state / first / last are filled in parallel from the per-frame states.
// The back-pointers have ONE home, the workspace: at T' = 2048, S = 1023 the packed table is 512 KB and cannot live in LDS, and the
// staged walk reads LDS at every size, so a second, LDS-only path would save one coalesced store and load of the table (30 KB at the
// recipe's sizes) and nothing on the dependent chains.
//
// A row that cannot be aligned (y_len outside [0, U], a label outside [0, Vc-2], or no path: L + repeats > enc_len) gets score = -inf,
// first / last = -1 for its labels and frame_state = -1; the other rows of the launch are unaffected.
#include "las_common.h"
#include <math.h>

namespace {

constexpr int CA_MAX_STATES = 1023;      // one state per lane of a 1024-thread workgroup: U <= 511 (ctc.hip's limit)
constexpr int CA_MAX_TP = 2048;          // ctc_prefix.hip's limit
constexpr int CA_PF = 8;                 // frames the emission loads run ahead of the recursion
constexpr int CA_TILE = 64;
constexpr int CA_STAGE_WORDS = 8192;     // back-pointer words staged in LDS at a time (32 KB): >= 8 rows of SP <= 1024 words

struct AlignWs {
    float* glp;          // [n, T', U+1]          log-probabilities, column 0 blank, column j+1 label j
    unsigned* bp;        // [n, ceil(T'/16), SP]  word (r, s): the 2-bit steps into state s at frames 16 r .. 16 r + 15
    int* fs;             // [n, T']               per-frame states when the caller wants no frame_state
    int* fin;            // [n]                   final state of the best path; -1: the row cannot be aligned
};

__host__ __device__ inline int ca_sp(int U) { return (2 * U + 1 + 63) / 64 * 64; }
__host__ __device__ inline int ca_rows(int Tp) { return (Tp + 15) / 16; }

__host__ __device__ inline size_t align_ws_layout(int n, int Tp, int U, char* base, AlignWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    char* glp = take((size_t)n * Tp * (U + 1) * 4);
    char* bp = take((size_t)n * ca_rows(Tp) * ca_sp(U) * 4);
    char* fs = take((size_t)n * Tp * 4);
    char* fin = take((size_t)n * 4);
    if (w) { w->glp = (float*)glp; w->bp = (unsigned*)bp; w->fs = (int*)fs; w->fin = (int*)fin; }
    return o;
}

// grid (ceil(T'/64), ceil((U+1)/64), n), 256 threads
__global__ __launch_bounds__(256) void ctc_align_gather_kernel(const float* __restrict__ lp, int Vc, int Tp, const int* __restrict__ enc_len,
                                                               const int* __restrict__ y, int ldy, const int* __restrict__ y_len, int U,
                                                               AlignWs w) {
    __shared__ float tile[CA_TILE][CA_TILE + 1];
    const int u = blockIdx.z, t0 = blockIdx.x * CA_TILE, j0 = blockIdx.y * CA_TILE;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int T = clampi(enc_len[u], 1, Tp), L = clampi(y_len[u], 0, U);
    if (t0 >= T || j0 > L) return;
    const float* row = lp + (size_t)u * Vc * Tp;
    for (int k = wv * 16; k < wv * 16 + 16; ++k) {
        const int j = j0 + k, t = t0 + lane;
        int c = -1;
        if (j == 0) c = Vc - 1;
        else if (j <= L) c = y[(size_t)u * ldy + j - 1];
        tile[k][lane] = (c >= 0 && c < Vc && t < T) ? row[(size_t)c * Tp + t] : 0.f;      // (a label outside the classes is never read)
    }
    __syncthreads();
    float* g = w.glp + (size_t)u * Tp * (U + 1);
    for (int f = wv * 16; f < wv * 16 + 16; ++f) {
        const int t = t0 + f, j = j0 + lane;
        if (t < T && j <= L) g[(size_t)t * (U + 1) + j] = tile[lane][f];
    }
}

// grid n, SP = 64 ceil((2U+1)/64) threads, state s = threadIdx.x
__global__ __launch_bounds__(1024) void ctc_align_viterbi_kernel(int Vc, int Tp, const int* __restrict__ enc_len, const int* __restrict__ y,
                                                                 int ldy, const int* __restrict__ y_len, int U, double* __restrict__ score,
                                                                 AlignWs w) {
    __shared__ double buf[2][CA_MAX_STATES + 1];
    const int u = blockIdx.x, s = threadIdx.x, SP = blockDim.x;
    const int T = clampi(enc_len[u], 1, Tp);
    const int Lraw = y_len[u];
    const int L = clampi(y_len[u], 0, U), S = 2 * L + 1;
    const bool act = s < S, odd = s & 1;
    const int* lab = y + (size_t)u * ldy;
    const int c = (act && odd) ? lab[s >> 1] : 0;
    const int bad = __syncthreads_or((Lraw < 0 || Lraw > U || c < 0 || c > Vc - 2) ? 1 : 0);
    if (bad) {
        if (s == 0) { score[u] = -INFINITY; w.fin[u] = -1; }
        return;
    }
    const bool skip_in = act && odd && s >= 3 && c != lab[(s >> 1) - 1];      // s - 2 -> s: between two labels of different classes
    const int col = odd ? (s >> 1) + 1 : 0;
    const int W = U + 1;
    const float* glp = w.glp + (size_t)u * Tp * W;
    unsigned* bp = w.bp + (size_t)u * ca_rows(Tp) * SP;

    double a = (act && s <= 1) ? (double)glp[col] : -INFINITY;
    buf[0][s] = a;
    float e[CA_PF];
#pragma unroll
    for (int i = 0; i < CA_PF; ++i) e[i] = (act && 1 + i < T) ? glp[(size_t)(1 + i) * W + col] : 0.f;
    unsigned bits = 0;
    if (T == 1) bp[s] = 0;
    lds_barrier();
    int cur = 0;
    for (int t0 = 1; t0 < T; t0 += CA_PF) {
#pragma unroll
        for (int i = 0; i < CA_PF; ++i) {
            const int t = t0 + i;
            if (t >= T) continue;                                              // (uniform)
            const float ev = e[i];
            if (act && t + CA_PF < T) e[i] = glp[(size_t)(t + CA_PF) * W + col];   // in flight across CA_PF steps
            if (act) {
                const double* p = buf[cur];
                double m = p[s];
                unsigned k = 0;
                const double a1 = s >= 1 ? p[s - 1] : -INFINITY;
                const double a2 = skip_in ? p[s - 2] : -INFINITY;
                if (a1 > m) { m = a1; k = 1; }                                 // equal values: the smaller step stays
                if (a2 > m) { m = a2; k = 2; }
                a = m + (double)ev;
                bits |= k << (2 * (t & 15));
            }
            buf[cur ^ 1][s] = a;
            if ((t & 15) == 15 || t == T - 1) { bp[(size_t)(t >> 4) * SP + s] = bits; bits = 0; }
            cur ^= 1;
            lds_barrier();
        }
    }
    if (s == 0) {
        const double* p = buf[cur];
        int fin = S - 1;                                                       // 2L, unless 2L - 1 is strictly better
        if (S >= 2 && p[S - 2] > p[S - 1]) fin = S - 2;
        const double best = p[fin];
        score[u] = best;
        w.fin[u] = best == -INFINITY ? -1 : fin;                               // no path: L + repeats > T
    }
}

// grid n, 256 threads
__global__ __launch_bounds__(256) void ctc_align_trace_kernel(int Tp, const int* __restrict__ enc_len, const int* __restrict__ y_len, int U,
                                                              int* __restrict__ first, int* __restrict__ last, int* __restrict__ frame_state,
                                                              AlignWs w) {
    __shared__ __attribute__((aligned(16))) unsigned words[CA_STAGE_WORDS];
    __shared__ int st[CA_MAX_TP];
    const int u = blockIdx.x, tid = threadIdx.x;
    const int T = clampi(enc_len[u], 1, Tp), L = clampi(y_len[u], 0, U);
    const int fin = w.fin[u];
    int* fst = frame_state ? frame_state + (size_t)u * Tp : w.fs + (size_t)u * Tp;
    if (fin < 0) {
        for (int j = tid; j < L; j += 256) { first[(size_t)u * U + j] = -1; last[(size_t)u * U + j] = -1; }
        for (int t = tid; t < Tp; t += 256) fst[t] = -1;
        return;
    }
    const int SP = ca_sp(U);
    const unsigned* bp = w.bp + (size_t)u * ca_rows(Tp) * SP;
    const int R = CA_STAGE_WORDS / SP;                                         // rows of 16 frames staged at a time (>= 8)
    int s = fin;
    for (int r1 = ca_rows(T); r1 > 0;) {
        const int r0 = r1 > R ? r1 - R : 0;
        const uint4* src = (const uint4*)(bp + (size_t)r0 * SP);               // (SP is a multiple of 64 words, the table 256-byte aligned)
        for (int i = tid; i < (r1 - r0) * SP / 4; i += 256) ((uint4*)words)[i] = src[i];
        __syncthreads();
        if (tid == 0) {
            const int hi = r1 * 16 < T ? r1 * 16 : T;
            for (int t = hi - 1; t >= r0 * 16; --t) {
                st[t] = s;
                const int k = t > 0 ? (int)((words[((t >> 4) - r0) * SP + s] >> (2 * (t & 15))) & 3u) : 0;
                s = s - k < 0 ? 0 : s - k;
            }
        }
        __syncthreads();
        r1 = r0;
    }
    for (int t = tid; t < Tp; t += 256) fst[t] = t < T ? st[t] : -1;
    // the path visits every label's state exactly once, over consecutive frames: one writer per entry
    for (int t = tid; t < T; t += 256) {
        const int q = st[t];
        if (!(q & 1)) continue;
        const int j = q >> 1;
        if (j >= L) continue;
        if (t == 0 || st[t - 1] != q) first[(size_t)u * U + j] = t;
        if (t == T - 1 || st[t + 1] != q) last[(size_t)u * U + j] = t;
    }
}

}  // namespace

extern "C" size_t las_ctc_align_workspace_bytes(int n, int Tp, int U) {
    if (n <= 0 || Tp <= 0 || U < 0) return 0;
    return align_ws_layout(n, Tp, U, nullptr, nullptr);
}

extern "C" int las_ctc_align(const float* lp, int Vc, int Tp, const int* enc_len, int n, const int* y, int ldy, const int* y_len, int U,
                             int* first, int* last, int* frame_state, double* score, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(lp && enc_len && y_len && score, "las_ctc_align: lp, enc_len, y_len and score must be given");
    LAS_ARG(U == 0 || (y && first && last), "las_ctc_align: y, first and last must be given when U > 0");
    LAS_ARG(n > 0 && n <= 65535 && Vc >= 2 && U >= 0 && ldy >= U, "las_ctc_align: bad sizes (n=%d Vc=%d U=%d ldy=%d)", n, Vc, U, ldy);
    LAS_ARG(2 * U + 1 <= CA_MAX_STATES, "las_ctc_align: U=%d labels per utterance, at most %d", U, (CA_MAX_STATES - 1) / 2);
    LAS_ARG(Tp > 0 && Tp <= CA_MAX_TP, "las_ctc_align: 1 <= T' <= %d (got %d)", CA_MAX_TP, Tp);
    LAS_ARG(ws && ws_bytes >= las_ctc_align_workspace_bytes(n, Tp, U), "las_ctc_align: workspace too small (%zu < %zu)", ws_bytes,
            las_ctc_align_workspace_bytes(n, Tp, U));
    hipStream_t s = (hipStream_t)stream;
    AlignWs w;
    align_ws_layout(n, Tp, U, (char*)ws, &w);
    hipLaunchKernelGGL(ctc_align_gather_kernel, dim3(cdiv(Tp, CA_TILE), cdiv(U + 1, CA_TILE), n), dim3(256), 0, s, lp, Vc, Tp, enc_len, y, ldy,
                       y_len, U, w);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(ctc_align_viterbi_kernel, dim3(n), dim3(ca_sp(U)), 0, s, Vc, Tp, enc_len, y, ldy, y_len, U, score, w);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(ctc_align_trace_kernel, dim3(n), dim3(256), 0, s, Tp, enc_len, y_len, U, first, last, frame_state, w);
    LAS_LAUNCHED();
    return 0;
}
