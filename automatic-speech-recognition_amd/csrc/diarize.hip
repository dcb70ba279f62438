// diarize.hip -- speaker diarization of long recordings without a trained model (las_hip.h K17): the Bayesian information
// criterion between full-covariance Gaussians over the static MFCCs (Chen & Gopalakrishnan 1998) finds the speaker changes inside a run
// of speech (las_bic_change) and drives the agglomerative clustering of the pieces (las_bic_cluster).
//
// The statistics of a set of frames are ONE packed lower triangle: that of sum [x; 1] [x; 1]^T over the set's masked frames, a
// (D + 1) x (D + 1) matrix whose last row holds S1 and n and whose leading D x D block is S2 -- NS = (D + 1)(D + 2) / 2 doubles, entry
// tri(i, j).  Every fp32 feature is widened first, so a product is exact and an entry is one sequential chain of roundings in frame
// order.  Statistics add: a union's are the sum of its parts'.
//
//   bic_change_kernel   one candidate per workgroup of four waves.  Thread e owns entry e of the triangle; the window's frames are
//                       staged 64 at a time into LDS (the D used columns of the listed rows only, a column of ones behind them) and
//                       every thread walks them in order, once for the left window and once for the right one.  Three waves then
//                       factor the three covariances (left, right, both) side by side, each in its own LDS triangle, and one thread
//                       writes v.  The window is summed directly whatever hop is: no second path for a hop that does not divide w.
//   bic_peak_kernel     one candidate per thread: the +-R neighbours of its own sequence.
//   bic_unit_kernel     one unit per workgroup: its statistics as above, and its own log-determinant behind them.
//   bic_pair_kernel     one pair (i, j) per WAVE, four per workgroup, no workgroup barrier: the union's covariance straight from the
//                       two records, one factorisation, d(i, j).
//   bic_loop_kernel     one workgroup of 1024 threads per recording, the whole agglomerative loop: a block arg-min over per-row minima
//                       (ties: the smallest i, then the smallest j), the merge, row i recomputed by the sixteen waves (a unit each at
//                       a time), the row minima repaired (a row is scanned again only when its minimum sat in column i or j).
// The factorisation (wave_chol_logdet) is a right-looking Cholesky on a packed triangle in LDS by one wave: the lanes exchange through
// LDS with wave-local ordering only.  No atomics, no cross-workgroup synchronisation; a value depends on its own frames and the scalar
// arguments alone, so a recording gives the bits it gives alone and two calls give the same bits.
#include "las_common.h"
#include <math.h>
#include <limits.h>

namespace {

constexpr int MAXD = LAS_BIC_MAX_DIM;
constexpr int MAXP = MAXD * (MAXD + 1) / 2;           // packed D x D triangle
constexpr int MAXNS = (MAXD + 1) * (MAXD + 2) / 2;    // packed (D + 1) x (D + 1) triangle: the statistics
constexpr int NT = 256;                               // threads of the statistics kernels (>= MAXNS: an entry each)
constexpr int CH = 64;                                // frames staged at a time
constexpr int PITCH = MAXD + 1;                       // floats per staged frame: D features and the one (odd: no bank pattern)
constexpr int NT_LOOP = 1024;                         // threads of the loop kernel = LAS_BIC_MAX_UNITS
constexpr int NW_LOOP = NT_LOOP / 64;
static_assert(NT >= MAXNS && NT_LOOP == LAS_BIC_MAX_UNITS, "an entry per thread; a unit per thread");

__host__ __device__ inline int tri(int i, int j) { return i * (i + 1) / 2 + j; }      // (j <= i)
__host__ __device__ inline int stat_count(int D) { return (D + 1) * (D + 2) / 2; }
__host__ __device__ inline int rec_words(int D) { return stat_count(D) + 1; }         // the statistics and the log-determinant

// the largest s in [0, n) with off[s] <= g (off ascending, off[0] <= g < off[n])
__device__ __forceinline__ int owner_of(const int* __restrict__ off, int n, int g) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// the masked frames [row0, row0 + nrows) added to acc in frame order: this thread's entry is the product of the staged columns ci and
// cj (column D is the one).  Every thread of the NT calls it; xs [CH, PITCH] and ms [CH] are the workgroup's staging buffers.
__device__ __forceinline__ void accumulate(const float* __restrict__ feat, long long ld, int D, const unsigned char* __restrict__ mask,
                                           long long row0, int nrows, int ci, int cj, bool has, double& acc, float* xs, unsigned char* ms) {
    for (int f0 = 0; f0 < nrows; f0 += CH) {          // (uniform)
        const int nf = min(CH, nrows - f0);
        __syncthreads();                              // the previous chunk has been read
        for (int g = threadIdx.x; g < nf * D; g += NT) {
            const int r = g / D, c = g - r * D;
            xs[r * PITCH + c] = feat[(row0 + f0 + r) * ld + c];
        }
        for (int g = threadIdx.x; g < nf; g += NT) ms[g] = mask ? mask[row0 + f0 + g] : (unsigned char)1;
        __syncthreads();
        if (has)
            for (int r = 0; r < nf; ++r)
                if (ms[r]) acc = fma((double)xs[r * PITCH + ci], (double)xs[r * PITCH + cj], acc);
    }
}

// entry e of the statistics triangle -> its two columns
__device__ __forceinline__ void entry_columns(int e, int& ci, int& cj) {
    int i = 0;
    while (tri(i + 1, 0) <= e) ++i;
    ci = i;
    cj = e - tri(i, 0);
}

// A = (S2 - S1 S1^T / n) / n + floor I as a packed triangle in LDS, by one wave; get(q) is entry q of the statistics.  -> n
template <class F>
__device__ __forceinline__ double wave_covariance(double* A, int D, F get, double floor_, int lane) {
    const double n = get(tri(D, D));
    const int li = lane >> 3, lj = lane & 7;
    for (int i = li; i < D; i += 8)
        for (int j = lj; j <= i; j += 8)
            A[tri(i, j)] = (get(tri(i, j)) - get(tri(D, i)) * get(tri(D, j)) / n) / n + (i == j ? floor_ : 0.0);
    return n;
}

// log det of the symmetric matrix whose packed lower triangle A (LDS, this wave's own) holds, by a right-looking Cholesky; A is
// destroyed.  All 64 lanes call it and all get the result; a pivot that is not positive gives NaN or -inf, never a fault.
__device__ __forceinline__ double wave_chol_logdet(double* A, int D, int lane) {
    const int li = lane >> 3, lj = lane & 7;
    double ld = 0.0;
    for (int k = 0; k < D; ++k) {
        wave_lds_sync();
        const double p = A[tri(k, k)];
        ld += log(p);
        const double s = sqrt(p);
        for (int i = k + 1 + lane; i < D; i += 64) A[tri(i, k)] /= s;
        wave_lds_sync();
        for (int i = k + 1 + li; i < D; i += 8)
            for (int j = k + 1 + lj; j <= i; j += 8) A[tri(i, j)] -= A[tri(i, k)] * A[tri(j, k)];
    }
    wave_lds_sync();
    return ld;
}

__device__ __forceinline__ double delta_bic(double n1, double L1, double n2, double L2, double LU, int D, double lambda) {
    const double n = n1 + n2;
    return 0.5 * (n * LU - n1 * L1 - n2 * L2) - lambda * 0.5 * (double)(D + D * (D + 1) / 2) * log(n);
}

__global__ __launch_bounds__(NT) void bic_change_kernel(const float* __restrict__ feat, long long ld, int D, const unsigned char* __restrict__ mask,
                                                        const int* __restrict__ seq_off, const int* __restrict__ cand_off, int S, int w, int hop,
                                                        int nmin, double lambda, double floor_, double* __restrict__ v) {
    __shared__ float xs[CH * PITCH];
    __shared__ unsigned char ms[CH];
    __shared__ double st[3][MAXNS];                   // left, right, both
    __shared__ double A[3][MAXP];
    __shared__ double L[3];
    const int tid = threadIdx.x, g = blockIdx.x;      // (g < cand_off[S]: the grid)
    const int s = owner_of(cand_off, S, g);
    const long long row0 = (long long)seq_off[s] + (long long)(g - cand_off[s]) * hop;   // the left window's first row: t - w
    const int NS = stat_count(D);
    const bool has = tid < NS;
    int ci = 0, cj = 0;
    if (has) entry_columns(tid, ci, cj);
    for (int r = tid; r < CH; r += NT) xs[r * PITCH + D] = 1.0f;
    double left = 0.0, right = 0.0;
    accumulate(feat, ld, D, mask, row0, w, ci, cj, has, left, xs, ms);
    accumulate(feat, ld, D, mask, row0 + w, w, ci, cj, has, right, xs, ms);
    if (has) { st[0][tid] = left; st[1][tid] = right; st[2][tid] = left + right; }
    __syncthreads();
    const int wv = tid >> 6, lane = tid & 63;
    if (wv < 3) {                                     // (wave-uniform; no workgroup barrier inside)
        const double* q = st[wv];
        wave_covariance(A[wv], D, [q](int e) { return q[e]; }, floor_, lane);
        const double l = wave_chol_logdet(A[wv], D, lane);
        if (lane == 0) L[wv] = l;
    }
    __syncthreads();
    if (tid == 0) {
        const double n1 = st[0][tri(D, D)], n2 = st[1][tri(D, D)];
        v[g] = (n1 < (double)nmin || n2 < (double)nmin) ? -INFINITY : delta_bic(n1, L[0], n2, L[1], L[2], D, lambda);
    }
}

__global__ __launch_bounds__(NT) void bic_peak_kernel(const double* __restrict__ v, const int* __restrict__ cand_off, int S, int total, int R,
                                                      unsigned char* __restrict__ peak) {
    const long long gl = (long long)blockIdx.x * NT + threadIdx.x;
    if (gl >= total) return;
    const int g = (int)gl;
    const int s = owner_of(cand_off, S, g);
    const int lo = cand_off[s], hi = cand_off[s + 1];
    const double x = v[g];
    bool is_peak = x > 0.0;
    for (int c = max(lo, g - R); is_peak && c < g; ++c) is_peak = x > v[c];
    for (int c = g + 1; is_peak && c < hi && c <= g + R; ++c) is_peak = x >= v[c];
    peak[g] = is_peak ? 1 : 0;
}

__global__ __launch_bounds__(NT) void bic_unit_kernel(const float* __restrict__ feat, long long ld, int D, const unsigned char* __restrict__ mask,
                                                      const int* __restrict__ seq_off, const int* __restrict__ seq_len, double floor_,
                                                      double* __restrict__ stats) {
    __shared__ float xs[CH * PITCH];
    __shared__ unsigned char ms[CH];
    __shared__ double st[MAXNS];
    __shared__ double A[MAXP];
    const int tid = threadIdx.x, s = blockIdx.x;
    const int NS = stat_count(D);
    const bool has = tid < NS;
    int ci = 0, cj = 0;
    if (has) entry_columns(tid, ci, cj);
    for (int r = tid; r < CH; r += NT) xs[r * PITCH + D] = 1.0f;
    double acc = 0.0;
    accumulate(feat, ld, D, mask, seq_off[s], seq_len[s], ci, cj, has, acc, xs, ms);
    double* rec = stats + (long long)s * rec_words(D);
    if (has) { st[tid] = acc; rec[tid] = acc; }
    __syncthreads();
    if (tid < 64) {
        wave_covariance(A, D, [&](int e) { return st[e]; }, floor_, tid);
        const double l = wave_chol_logdet(A, D, tid);
        if (tid == 0) rec[NS] = l;
    }
}

// W [S, ldw]: row = the unit's index in the call, column = a unit's index inside its recording; (i, j) with i < j is written
__global__ __launch_bounds__(NT) void bic_pair_kernel(const double* __restrict__ stats, int D, const int* __restrict__ rec_off, int n_rec,
                                                      double lambda, double floor_, double* __restrict__ W, double* __restrict__ dist, int ldw) {
    __shared__ double A[NT / 64][MAXP];
    const int gi = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = owner_of(rec_off, n_rec, gi);
    const int base = rec_off[r], Sr = rec_off[r + 1] - base;
    const int i = gi - base, j = blockIdx.y * (NT / 64) + wv;
    if (j <= i || j >= Sr) return;                    // (wave-uniform)
    const int NS = stat_count(D), RW = rec_words(D);
    const double* a = stats + (long long)gi * RW;
    const double* b = stats + (long long)(base + j) * RW;
    wave_covariance(A[wv], D, [a, b](int e) { return a[e] + b[e]; }, floor_, lane);
    const double LU = wave_chol_logdet(A[wv], D, lane);
    if (lane == 0) {
        const double d = delta_bic(a[tri(D, D)], a[NS], b[tri(D, D)], b[NS], LU, D, lambda);
        W[(long long)gi * ldw + j] = d;
        if (dist) dist[(long long)gi * ldw + j] = d;
    }
}

struct Best { double v; int i; };
// the least v over the workgroup, the smallest i among equals; every thread calls it and gets it
__device__ __forceinline__ Best block_argmin(Best b, double* redv, int* redi) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(b.v, o);
        const int oi = __shfl_xor(b.i, o);
        if (ov < b.v || (ov == b.v && oi < b.i)) { b.v = ov; b.i = oi; }
    }
    __syncthreads();                                  // (the previous call's readers are through)
    if (lane == 0) { redv[wv] = b.v; redi[wv] = b.i; }
    __syncthreads();
    b.v = redv[0];
    b.i = redi[0];
    for (int k = 1; k < NW_LOOP; ++k)
        if (redv[k] < b.v || (redv[k] == b.v && redi[k] < b.i)) { b.v = redv[k]; b.i = redi[k]; }
    return b;
}

__global__ __launch_bounds__(NT_LOOP) void bic_loop_kernel(double* __restrict__ stats, int D, const int* __restrict__ rec_off, int K, double lambda,
                                                           double floor_, double* __restrict__ W, int ldw, int* __restrict__ label,
                                                           int* __restrict__ n_clusters, int* __restrict__ merges,
                                                           double* __restrict__ merge_val, int* __restrict__ n_merges) {
    __shared__ double rowv[NT_LOOP];                  // the least d(r, k) over the live k > r ...
    __shared__ int rowj[NT_LOOP];                     // ... and the smallest k that has it (-1: no live k behind r)
    __shared__ double newd[NT_LOOP];                  // d(i, k) of the row just recomputed
    __shared__ int rep[NT_LOOP];                      // the cluster a unit is in = its earliest unit
    __shared__ unsigned char live[NT_LOOP];
    __shared__ double A[NW_LOOP][MAXP];
    __shared__ double sti[MAXNS + 1];                 // the merged cluster's record
    __shared__ double redv[NW_LOOP];
    __shared__ int redi[NW_LOOP];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, rc = blockIdx.x;
    const int base = rec_off[rc], Sr = rec_off[rc + 1] - base;       // (1 <= Sr <= NT_LOOP: the entry)
    const int NS = stat_count(D), RW = rec_words(D);
    stats += (long long)base * RW;
    W += (long long)base * ldw;

    auto scan_row = [&](int r) {                      // row r of W over the live k behind r: the first of equal minima
        double bv = INFINITY;
        int bj = -1;
        for (int k = r + 1; k < Sr; ++k)
            if (live[k]) {
                const double d = W[(long long)r * ldw + k];
                if (bj < 0 || d < bv) { bv = d; bj = k; }
            }
        rowv[r] = bv;
        rowj[r] = bj;
    };

    live[tid] = tid < Sr;
    rep[tid] = tid;
    __syncthreads();
    if (tid < Sr) scan_row(tid);
    int nlive = Sr, nm = 0;
    for (;;) {                                        // (uniform: every thread sees the same arg-min and counts)
        __syncthreads();
        Best b = {INFINITY, INT_MAX};
        if (tid < Sr && live[tid] && rowj[tid] >= 0) { b.v = rowv[tid]; b.i = tid; }
        b = block_argmin(b, redv, redi);
        if (nlive <= 1 || b.i == INT_MAX) break;
        if (K > 0 ? nlive <= K : !(b.v < 0.0)) break;
        const int bi = b.i, bj = rowj[bi];
        __syncthreads();                              // (rowj[bi] has been read by everybody)
        if (tid == 0 && merges) {
            merges[2 * (base - rc + nm)] = bi;        // (recording rc owns rows [base - rc, base - rc + Sr - 1) of merges)
            merges[2 * (base - rc + nm) + 1] = bj;
            merge_val[base - rc + nm] = b.v;
        }
        ++nm;
        --nlive;
        if (tid < NS) {
            const double x = stats[(long long)bi * RW + tid] + stats[(long long)bj * RW + tid];
            stats[(long long)bi * RW + tid] = x;
            sti[tid] = x;
        }
        if (tid == bj) live[tid] = 0;
        if (rep[tid] == bj) rep[tid] = bi;
        __syncthreads();
        if (wv == 0) {
            wave_covariance(A[0], D, [&](int e) { return sti[e]; }, floor_, lane);
            const double l = wave_chol_logdet(A[0], D, lane);
            if (lane == 0) { sti[NS] = l; stats[(long long)bi * RW + NS] = l; }
        }
        __syncthreads();
        for (int k = wv; k < Sr; k += NW_LOOP) {      // (wave-uniform; no workgroup barrier inside)
            if (!live[k] || k == bi) continue;
            const double* q = stats + (long long)k * RW;
            wave_covariance(A[wv], D, [&](int e) { return sti[e] + q[e]; }, floor_, lane);
            const double LU = wave_chol_logdet(A[wv], D, lane);
            if (lane == 0) {
                const double d = delta_bic(sti[tri(D, D)], sti[NS], q[tri(D, D)], q[NS], LU, D, lambda);
                newd[k] = d;
                W[(long long)min(k, bi) * ldw + max(k, bi)] = d;
            }
        }
        __syncthreads();
        if (tid < Sr && live[tid]) {
            const int r = tid;
            if (r == bi || rowj[r] == bi || rowj[r] == bj) scan_row(r);
            else if (r < bi) {
                const double d = newd[r];
                if (d < rowv[r] || (d == rowv[r] && bi < rowj[r])) { rowv[r] = d; rowj[r] = bi; }
            }
        }
    }
    if (tid < Sr) {
        int below = 0;
        for (int k = 0; k < rep[tid]; ++k) below += live[k];
        label[base + tid] = below;                    // clusters in the order of their earliest unit
    }
    if (tid == 0) {
        n_clusters[rc] = nlive;
        if (n_merges) n_merges[rc] = nm;
    }
}

int check_common(const char* who, const float* feat, long long N, long long ld, int D, const int* seq_off, const int* seq_off_host,
                 const int* seq_len_host, int S, int min_len, double lambda, double floor_) {
    LAS_ARG(feat && seq_off && seq_off_host && seq_len_host, "%s: null pointer (feat, seq_off, seq_off_host, seq_len_host)", who);
    LAS_ARG(D >= 1 && D <= MAXD, "%s: D=%d (1..%d)", who, D, MAXD);
    LAS_ARG(N >= 1 && N <= INT32_MAX && ld >= D && ld <= INT32_MAX, "%s: feat is [N=%lld, ld=%lld] (1 <= N, D <= ld, both <= INT32_MAX)", who, N, ld);
    LAS_ARG(S >= 1, "%s: S=%d sequences (>= 1)", who, S);
    LAS_ARG(isfinite(lambda) && isfinite(floor_) && floor_ >= 0.0, "%s: lambda=%g, floor=%g (finite; floor >= 0)", who, lambda, floor_);
    for (int s = 0; s < S; ++s) {
        const long long o = seq_off_host[s], l = seq_len_host[s];
        LAS_ARG(o >= 0 && l >= min_len && o + l <= N, "%s: sequence %d is rows [%lld, %lld) of %lld (length >= %d)", who, s, o, o + l, N, min_len);
    }
    return 0;
}

struct ClusterLayout { size_t stats, W, total; };
ClusterLayout cluster_layout(int S, int Smax, int D) {
    ClusterLayout L;
    size_t o = 0;
    L.stats = o; o += align256((size_t)S * rec_words(D) * sizeof(double));
    L.W = o;     o += align256((size_t)S * Smax * sizeof(double));
    L.total = o;
    return L;
}

}  // namespace

extern "C" long long las_bic_candidates(long long len, int w, int hop) {
    if (len < 0 || w < 1 || hop < 1) return -1;
    return len < 2ll * w ? 0 : (len - 2ll * w) / hop + 1;
}

extern "C" int las_bic_change(const float* feat, long long N, long long ld, int D, const unsigned char* mask, const int* seq_off,
                              const int* cand_off, const int* seq_off_host, const int* seq_len_host, int S, int w, int hop, int nmin, double lambda,
                              double floor, double* v, unsigned char* peak, void* stream) {
    if (check_common("las_bic_change", feat, N, ld, D, seq_off, seq_off_host, seq_len_host, S, 0, lambda, floor)) return -1;
    LAS_ARG(cand_off && v && peak, "las_bic_change: null pointer (cand_off, v, peak)");
    LAS_ARG(w >= 2 && hop >= 1 && nmin >= 1, "las_bic_change: w=%d (>= 2), hop=%d (>= 1), nmin=%d (>= 1)", w, hop, nmin);
    long long total = 0;
    for (int s = 0; s < S; ++s) total += las_bic_candidates(seq_len_host[s], w, hop);
    LAS_ARG(total <= INT32_MAX, "las_bic_change: %lld candidates", total);
    if (total == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bic_change_kernel, dim3((unsigned)total), dim3(NT), 0, st, feat, ld, D, mask, seq_off, cand_off, S, w, hop, nmin, lambda, floor, v);
    LAS_LAUNCHED();
    const int R = (w + hop - 1) / hop;
    hipLaunchKernelGGL(bic_peak_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, v, cand_off, S, (int)total, R, peak);
    LAS_LAUNCHED();
    return 0;
}

extern "C" size_t las_bic_cluster_workspace_bytes(int S, int Smax, int D) {
    if (S < 1 || Smax < 1 || Smax > S || Smax > LAS_BIC_MAX_UNITS || D < 1 || D > MAXD) return 0;
    return cluster_layout(S, Smax, D).total;
}

extern "C" int las_bic_cluster(const float* feat, long long N, long long ld, int D, const unsigned char* mask, const int* seq_off, const int* seq_len,
                               const int* rec_off, const int* seq_off_host, const int* seq_len_host, const int* n_masked_host, int S,
                               const int* rec_off_host, int n_rec, int K, double lambda, double floor, int* label, int* n_clusters, double* dist,
                               int* merges, double* merge_val, int* n_merges, void* ws, size_t ws_bytes, void* stream) {
    if (check_common("las_bic_cluster", feat, N, ld, D, seq_off, seq_off_host, seq_len_host, S, 1, lambda, floor)) return -1;
    LAS_ARG(seq_len && rec_off && rec_off_host && label && n_clusters && ws, "las_bic_cluster: null pointer (seq_len, rec_off, rec_off_host, label, n_clusters, ws)");
    LAS_ARG(!mask || n_masked_host, "las_bic_cluster: a mask needs n_masked_host, the units' masked frame counts");
    LAS_ARG((merges != nullptr) == (merge_val != nullptr), "las_bic_cluster: merges and merge_val go together");
    LAS_ARG(n_rec >= 1 && n_rec <= S && K >= 0, "las_bic_cluster: n_rec=%d (1..S=%d), K=%d (>= 0)", n_rec, S, K);
    LAS_ARG(rec_off_host[0] == 0 && rec_off_host[n_rec] == S, "las_bic_cluster: rec_off_host runs from %d to %d (0 to S=%d)", rec_off_host[0],
            rec_off_host[n_rec], S);
    int Smax = 0;
    for (int r = 0; r < n_rec; ++r) {
        const long long Sr = (long long)rec_off_host[r + 1] - rec_off_host[r];
        LAS_ARG(Sr >= 1 && Sr <= LAS_BIC_MAX_UNITS, "las_bic_cluster: recording %d has %lld units (1..%d)", r, Sr, LAS_BIC_MAX_UNITS);
        Smax = Sr > Smax ? (int)Sr : Smax;
    }
    for (int s = 0; s < S; ++s) {
        const int n = mask ? n_masked_host[s] : seq_len_host[s];
        LAS_ARG(n >= 1 && n <= seq_len_host[s], "las_bic_cluster: unit %d has %d masked frames of %d (>= 1)", s, n, seq_len_host[s]);
    }
    const size_t need = las_bic_cluster_workspace_bytes(S, Smax, D);
    LAS_ARG(ws_bytes >= need, "las_bic_cluster: workspace of %zu bytes, %zu needed", ws_bytes, need);
    LAS_ARG(((uintptr_t)ws & 7) == 0, "las_bic_cluster: ws is 8-byte aligned");
    const ClusterLayout L = cluster_layout(S, Smax, D);
    double* stats = (double*)((char*)ws + L.stats);
    double* W = (double*)((char*)ws + L.W);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bic_unit_kernel, dim3(S), dim3(NT), 0, st, feat, ld, D, mask, seq_off, seq_len, floor, stats);
    LAS_LAUNCHED();
    if (Smax > 1) {
        hipLaunchKernelGGL(bic_pair_kernel, dim3(S, (Smax + NT / 64 - 1) / (NT / 64)), dim3(NT), 0, st, stats, D, rec_off, n_rec, lambda, floor, W, dist, Smax);
        LAS_LAUNCHED();
    }
    hipLaunchKernelGGL(bic_loop_kernel, dim3(n_rec), dim3(NT_LOOP), 0, st, stats, D, rec_off, K, lambda, floor, W, Smax, label, n_clusters, merges,
                       merge_val, n_merges);
    LAS_LAUNCHED();
    return 0;
}
