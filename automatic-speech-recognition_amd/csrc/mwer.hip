// mwer.hip -- K10j: minimum word error rate training: the expected number of word errors over the hypotheses of every
// utterance, read off the Speller's logits of those hypotheses, and its gradient with respect to the logits.
//
// las_mwer_loss   three launches over logits [n K, U, V] taken in place through strides (as las_ce_loss / las_rescore_score):
//   1  one wave per (row, step), four to a workgroup (ce_rows_kernel's shape): row maximum, sum of exp, lse = m + logf(s) and the
//      label's term z[y] - lse, both kept in the workspace.  Up to 8192 classes a lane keeps its values in registers between the
//      maximum and the sum (as ce_rows_reg_kernel): the row is read once; larger rows are read twice.  Steps t >= len[r] and the rows of
//      absent slots are skipped.
//   2  one workgroup per utterance: a row's terms added in step order in float64 (a wave per row: wave_terms_sum_f64), then
//      posterior, expected errors and the rows' coefficients in float64, every sum in slot order.
//   3  one wave per (row, step) again: dlogits = coef (onehot - expf(z - lse)), exact zeros wherever the contract asks for them -- those
//      rows are stored without a look at the logits.  One more workgroup behind the grid adds the utterances' risks in a fixed order
//      (with dlogits = NULL that workgroup is the whole launch).
// The logits are read twice and written once; every load and store is one dword per lane (rows are V floats apart: nothing here needs
// an aligned base).  No atomics: two runs give the same bits.
#include "las_common.h"
#include <math.h>

namespace {

constexpr int MWER_MAX_K = 64;
constexpr int MWER_MAX_U = 1024;
constexpr int UTT_NT = 256;

// the workspace: [risk fp64 n | lse fp32 n K U | term fp32 n K U | coef fp32 n K]
struct MwerWs {
    double* risk;
    float *lse, *term, *coef;
};
__host__ __device__ inline MwerWs carve_ws(void* ws, const int n, const int K, const int U) {
    MwerWs w;
    w.risk = (double*)ws;
    w.lse = (float*)(w.risk + n);
    w.term = w.lse + (size_t)n * K * U;
    w.coef = w.term + (size_t)n * K * U;
    return w;
}

// NV > 0: a lane's NV classes (lane, lane + 64, ...) stay in registers, V <= 64 NV; NV = 0: any V, the row is read twice.  The same
// arithmetic in the same order either way: lane i takes the maximum and adds expf(z - m) over classes i, i + 64, ... in ascending order
// from 0.f, then the wave's butterfly (wave_max / wave_sum).
template <int NV>
__global__ __launch_bounds__(256) void mwer_lse_kernel(const float* __restrict__ logits, long long sb, long long st, int V,
                                                       const int* __restrict__ y, int ldy, const int* __restrict__ len,
                                                       const int* __restrict__ nhyp, int n, int K, int U, float* __restrict__ lse,
                                                       float* __restrict__ term) {
    const int lane = threadIdx.x & 63;
    const long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= (long long)n * K * U) return;                           // (a wave's own index: the whole wave leaves)
    const int r = (int)(idx / U), t = (int)(idx - (long long)r * U);
    const int u = r / K, k = r - u * K;
    if (k >= clampi(nhyp[u], 0, K)) return;                               // an absent slot: nothing of it is read
    if (t >= clampi(len[r], 0, U)) return;
    const float* z = logits + (long long)r * sb + (long long)t * st;
    float m = -INFINITY, s = 0.f;
    if (NV > 0) {
        // the instantiation is the register budget, nv = ceil(V / 64) the values a lane really holds: V = 1025 does 17 rounds in the
        // 80-value kernel, not 80 (nv is uniform: a scalar branch per unrolled round; a skipped round would have added +0)
        const int nv = (V + 63) >> 6;
        float v[NV > 0 ? NV : 1];
#pragma unroll
        for (int i = 0; i < NV; ++i) if (i < nv) { const int c = lane + 64 * i; v[i] = c < V ? z[c] : -INFINITY; }
#pragma unroll
        for (int i = 0; i < NV; ++i) if (i < nv) m = fmaxf(m, v[i]);
        m = wave_max(m);
        if (m > -INFINITY) {                                           // (uniform: m is the wave's)
#pragma unroll
            for (int i = 0; i < NV; ++i) if (i < nv) s += expf(v[i] - m);   // (a class past V in the last round: expf(-inf) adds +0)
            s = wave_sum(s);
        }
    } else {
        for (int c = lane; c < V; c += 64) m = fmaxf(m, z[c]);
        m = wave_max(m);
        if (m > -INFINITY) {
            for (int c = lane; c < V; c += 64) s += expf(z[c] - m);
            s = wave_sum(s);
        }
    }
    if (lane == 0) {
        float l = -INFINITY, tm = -INFINITY;                           // (m = -inf: no class has mass; z - m would be NaN)
        if (m > -INFINITY) {
            l = m + logf(s);
            const int c = y[(size_t)r * ldy + t];
            if (c >= 0 && c < V) tm = z[c] - l;                        // (a label outside [0, V): -inf, nothing read for it)
        }
        lse[idx] = l;
        term[idx] = tm;
    }
}

// one workgroup per utterance.  Waves 0 .. 3 add the terms of slots w, w + 4, ... in step order; then thread k < nhyp is slot k, and
// every sum over the slots runs in slot order in every thread (<= 64 LDS broadcasts).
__global__ __launch_bounds__(UTT_NT) void mwer_utt_kernel(const int* __restrict__ len, const int* __restrict__ nhyp,
                                                          const float* __restrict__ err, int n, int K, int U, int mode,
                                                          const float* __restrict__ scale_ptr, double* __restrict__ seq_lp,
                                                          float* __restrict__ post, float* __restrict__ coef, float* __restrict__ risk,
                                                          MwerWs w) {
    __shared__ double lp[MWER_MAX_K], ex[MWER_MAX_K], pp[MWER_MAX_K], ee[MWER_MAX_K];
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int nh = clampi(nhyp[u], 0, K);
    const size_t base = (size_t)u * K;
    for (int k = tid >> 6; k < nh; k += UTT_NT / 64) {                 // (k is the wave's: uniform control flow around the shuffles)
        const size_t r = base + k;
        const double s = wave_terms_sum_f64(w.term + r * U, clampi(len[r], 0, U), lane);
        if (lane == 0) {
            lp[k] = s;
            if (seq_lp) seq_lp[r] = s;
        }
    }
    __syncthreads();
    const bool live = tid < nh;
    const double sc = (double)scale_ptr[0];
    double mine = 0.0;
    if (live) {
        ee[tid] = (double)err[base + tid];
        if (mode == 0) {
            double m = lp[0];
            for (int j = 1; j < nh; ++j) m = fmax(m, lp[j]);
            mine = m > -INFINITY ? exp(lp[tid] - m) : 0.0;             // (every hypothesis -inf: no posterior, no gradient)
            ex[tid] = mine;
        }
    }
    __syncthreads();
    if (live) {
        if (mode == 0) {
            double s = 0.0;
            for (int j = 0; j < nh; ++j) s += ex[j];
            mine = s > 0.0 ? mine / s : 0.0;
        } else {
            mine = 1.0 / (double)nh;
        }
        pp[tid] = mine;
    }
    __syncthreads();
    if (tid < K) {
        float c32 = 0.f;                                               // (an absent slot: its gradient rows are zeros)
        if (live) {
            double rk = 0.0, c;
            if (mode == 0) {
                // err - Wbar as sum_j post_j (err - err_j): every term is exactly 0 when the errors are all equal
                double d = 0.0;
                for (int j = 0; j < nh; ++j) { rk += pp[j] * ee[j]; d += pp[j] * (ee[tid] - ee[j]); }
                c = sc * mine * d;
            } else {
                for (int j = 0; j < nh; ++j) rk += ee[j];
                rk = rk / (double)nh;
                c = sc * (ee[tid] - rk) / (double)nh;
            }
            const float p32 = (float)mine;
            c32 = (float)c;
            if (post) post[base + tid] = p32;
            if (coef) coef[base + tid] = c32;
            if (p32 == 0.f) c32 = 0.f;
            if (tid == 0) {
                w.risk[u] = rk;
                if (risk) risk[u] = (float)rk;
            }
        }
        w.coef[base + tid] = c32;
    }
    if (nh == 0 && tid == 0) {
        w.risk[u] = 0.0;
        if (risk) risk[u] = 0.f;
    }
}

// loss[0] = (float)(scale * sum_u risk[u]): lane i of one wave adds utterances i, i + 64, ... in ascending order from 0.0, lane 0 the
// 64 partial sums in lane order
__device__ __forceinline__ void mwer_loss_sum(const double* __restrict__ risk, const int n, const float* __restrict__ scale_ptr,
                                              float* __restrict__ loss, double* part) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        double s = 0.0;
        for (int u = tid; u < n; u += 64) s += risk[u];
        part[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < 64; ++i) s += part[i];
        loss[0] = (float)((double)scale_ptr[0] * s);
    }
}

__global__ __launch_bounds__(256) void mwer_loss_kernel(const double* __restrict__ risk, int n, const float* __restrict__ scale_ptr,
                                                        float* __restrict__ loss) {
    __shared__ double part[64];
    mwer_loss_sum(risk, n, scale_ptr, loss, part);
}

// one wave per (row, step) over ALL n K rows and U steps, four to a workgroup; workgroup gridDim.x - 1 adds up the loss instead
__global__ __launch_bounds__(256) void mwer_grad_kernel(const float* __restrict__ logits, long long sb, long long st, int V,
                                                        const int* __restrict__ y, int ldy, const int* __restrict__ len, int n, int K,
                                                        int U, const float* __restrict__ scale_ptr, float* __restrict__ loss,
                                                        float* __restrict__ dlogits, MwerWs w) {
    __shared__ double part[64];
    if (blockIdx.x == gridDim.x - 1) {                                 // (uniform: the whole workgroup)
        mwer_loss_sum(w.risk, n, scale_ptr, loss, part);
        return;
    }
    const int lane = threadIdx.x & 63;
    const long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= (long long)n * K * U) return;
    const int r = (int)(idx / U), t = (int)(idx - (long long)r * U);
    const long long off = (long long)r * sb + (long long)t * st;
    float* d = dlogits + off;
    const float c = w.coef[r];                                         // 0: an absent slot, no posterior, or no share in the gradient
    float l = -INFINITY;
    if (c != 0.f && t < clampi(len[r], 0, U)) l = w.lse[idx];
    if (!(l > -INFINITY)) {                                            // (also a step without mass: expf(-inf + inf) would be NaN)
        for (int v = lane; v < V; v += 64) d[v] = 0.f;
        return;
    }
    const float* z = logits + off;
    const int label = y[(size_t)r * ldy + t];
#pragma unroll 4
    for (int v = lane; v < V; v += 64) d[v] = c * ((v == label ? 1.f : 0.f) - expf(z[v] - l));
}

}  // namespace

extern "C" size_t las_mwer_workspace_bytes(int n, int K, int U) {
    if (n <= 0 || K <= 0 || U <= 0) return 0;
    const size_t rows = (size_t)n * (size_t)K;
    return (size_t)n * sizeof(double) + (2 * rows * (size_t)U + rows) * sizeof(float);
}

extern "C" int las_mwer_loss(const float* logits, long long sb, long long st, int V, const int* y, int ldy, const int* len,
                             const int* nhyp, const float* err, int n, int K, int U, int mode, const float* scale_ptr, double* seq_lp,
                             float* post, float* coef, float* risk, float* loss, float* dlogits, void* ws, size_t ws_bytes,
                             void* stream) {
    LAS_ARG(logits && y && len && nhyp && err && scale_ptr && loss, "las_mwer_loss: null pointer");
    LAS_ARG(n >= 1 && V >= 1, "las_mwer_loss: bad dims (n = %d, V = %d)", n, V);
    LAS_ARG(K >= 1 && K <= MWER_MAX_K, "las_mwer_loss: 1 <= K <= %d (got %d)", MWER_MAX_K, K);
    LAS_ARG(U >= 1 && U <= MWER_MAX_U, "las_mwer_loss: 1 <= U <= %d (got %d)", MWER_MAX_U, U);
    LAS_ARG((long long)n * K * U < 0x80000000LL, "las_mwer_loss: n K U = %lld, at most 2^31 - 1", (long long)n * K * U);
    LAS_ARG(ldy >= U, "las_mwer_loss: ldy = %d < U = %d", ldy, U);
    LAS_ARG(sb >= 0 && st >= 0, "las_mwer_loss: negative stride");
    LAS_ARG(mode == 0 || mode == 1, "las_mwer_loss: mode is 0 (N-best renormalisation) or 1 (sampling estimate), got %d", mode);
    const size_t need = las_mwer_workspace_bytes(n, K, U);
    LAS_ARG(ws && ws_bytes >= need, "las_mwer_loss: a workspace of %zu bytes is needed (got %zu)", need, ws ? ws_bytes : (size_t)0);
    LAS_ARG((((uintptr_t)ws) & 7) == 0, "las_mwer_loss: the workspace must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const MwerWs w = carve_ws(ws, n, K, U);
    const long long waves = (long long)n * K * U;
    const dim3 grid(cdiv(waves, 4));
#define MWER_LSE(NV) hipLaunchKernelGGL(mwer_lse_kernel<NV>, grid, dim3(256), 0, s, logits, sb, st, V, y, ldy, len, nhyp, n, K, U, w.lse, w.term)
    if (V <= 64) MWER_LSE(1);
    else if (V <= 64 * 16) MWER_LSE(16);
    else if (V <= 64 * 80) MWER_LSE(80);
    else if (V <= 64 * 128) MWER_LSE(128);
    else MWER_LSE(0);
#undef MWER_LSE
    LAS_LAUNCHED();
    hipLaunchKernelGGL(mwer_utt_kernel, dim3(n), dim3(UTT_NT), 0, s, len, nhyp, err, n, K, U, mode, scale_ptr, seq_lp, post, coef, risk, w);
    LAS_LAUNCHED();
    if (dlogits)
        hipLaunchKernelGGL(mwer_grad_kernel, dim3(grid.x + 1), dim3(256), 0, s, logits, sb, st, V, y, ldy, len, n, K, U, scale_ptr, loss,
                           dlogits, w);
    else
        hipLaunchKernelGGL(mwer_loss_kernel, dim3(1), dim3(256), 0, s, (const double*)w.risk, n, scale_ptr, loss);
    LAS_LAUNCHED();
    return 0;
}
