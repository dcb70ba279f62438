// ctc.hip -- the CTC term of joint CTC-attention training (reference las/las.py:75-77, 259-261, 335-349; TF 1.13 tf.nn.ctc_loss with
// ctc_merge_repeated = True, preprocess_collapse_repeated = False: standard CTC, blank = the last class Vc - 1, softmax inside the loss).
//
// Four launches, all stream-ordered on the caller's stream, no atomics (every sum has a fixed order: bit-reproducible):
//   ctc_labels_kernel   one workgroup per utterance: the row's labels (the nonzero entries of y, in order; the last of them dropped on
//                       `drop_last_row`), their count, and for every label the next position of the same class (the chain the
//                       posterior sums walk) and whether it is the class's first occurrence
//   ctc_gather_kernel   one wave per (b, t) row: max / log-sum-exp over the Vc logits (read once), the log-probabilities of the blank and
//                       of the row's labels in compact form [B, T', U+1] (column 0 blank, column j+1 label j).  No [B, T', Vc] log-softmax.
//   ctc_alpha_beta_kernel
//                       one workgroup per utterance, one extended-label state per lane (S = 2L+1 <= 1023).  Log-space alpha (fp64) over
//                       t < enc_len (two LDS buffers, one barrier per step; two per beta step), stored to the workspace; then beta backwards, and at every t
//                       the posteriors gamma_t(k) = sum_{s: l'_s = k} alpha_t(s) beta_t(s) / p of the blank and of every DISTINCT class of
//                       the row (the repeats of a class summed along the chain, in label order); writes nll_b = -log p.
//   ctc_grad_kernel     one wave per (b, t) row: grad = scale * (softmax - gamma), dense softmax first, then the corrections at the row's
//                       distinct classes (distinct: no two lanes write one element).  fp32 or bf16.  t >= enc_len[b]: zeros.
// plus a single-wave fixed-order sum: loss = scale * sum_b nll_b.
//
// A row that cannot be aligned (L + repeats > enc_len, or a label outside [0, Vc-2]) gets nll = +inf and a zero gradient row; TF raises
// "Not enough time for target transition sequence" there instead (LAS.train refuses L > enc_len on the host before it launches).
#include "las_common.h"
#include <math.h>

namespace {

constexpr int CTC_MAX_STATES = 1023;     // one state per lane of a 1024-thread workgroup: U <= 511 labels per utterance

// The recursions carry log alpha / log beta in fp64 and take exp / log of the (small) differences in fp32: the values reach -100s after a
// few dozen frames, where an fp32 ulp (8e-6) per step would show up in the posteriors; fp32 transcendentals on O(1) arguments do not.
__device__ __forceinline__ double lse2(double a, double b) {
    const double m = fmax(a, b);
    return m == -INFINITY ? -INFINITY : m + (double)logf(expf((float)(a - m)) + expf((float)(b - m)));
}
__device__ __forceinline__ double lse3(double a, double b, double c) {
    const double m = fmax(fmax(a, b), c);
    return m == -INFINITY ? -INFINITY : m + (double)logf(expf((float)(a - m)) + expf((float)(b - m)) + expf((float)(c - m)));
}

struct CtcWs {
    int* lab;        // [B, U]   labels
    int* nxt;        // [B, U]   next position of the same class (-1: none)
    int* first;      // [B, U]   1: first occurrence of its class in the row
    int* len;        // [B]      label count L_b after the drop; -1: a label is outside [0, Vc-2]
    float* lse;      // [B, T']  log-sum-exp of the row's logits
    float* glp;      // [B, T', U+1]  log-probabilities: column 0 blank, column j+1 label j
    double* alpha;   // [B, T', 2U+1] log alpha
    float* gam;      // [B, T', U+1]  posteriors: column 0 blank, column j+1 the class of label j (first occurrences only)
};

__host__ __device__ inline size_t ctc_ws_layout(int B, int Tp, int U, char* base, CtcWs* w) {
    size_t o = 0;
    auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += align256(bytes); return p; };
    char* lab = take((size_t)B * U * 4);
    char* nxt = take((size_t)B * U * 4);
    char* first = take((size_t)B * U * 4);
    char* len = take((size_t)B * 4);
    char* lse = take((size_t)B * Tp * 4);
    char* glp = take((size_t)B * Tp * (U + 1) * 4);
    char* alpha = take((size_t)B * Tp * (2 * U + 1) * 8);
    char* gam = take((size_t)B * Tp * (U + 1) * 4);
    if (w) {
        w->lab = (int*)lab; w->nxt = (int*)nxt; w->first = (int*)first; w->len = (int*)len;
        w->lse = (float*)lse; w->glp = (float*)glp; w->alpha = (double*)alpha; w->gam = (float*)gam;
    }
    return o;
}

// one workgroup of 512 threads per utterance, thread u = column u of y (U <= 511): ballot compaction of the nonzero entries in LDS, then
// thread j finds the previous / next label of its class (O(L) LDS reads per thread)
__global__ __launch_bounds__(512) void ctc_labels_kernel(const int* __restrict__ y, int ldy, int U, int Vc, int drop_last_row, CtcWs w) {
    __shared__ int lab_sh[512];
    __shared__ int cnt[8];
    const int b = blockIdx.x;
    const int u = threadIdx.x, lane = u & 63, wv = u >> 6;
    const int v = u < U ? y[(long long)b * ldy + u] : 0;
    const unsigned long long m = __ballot(v != 0);
    const int pre = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) cnt[wv] = __popcll(m);
    __syncthreads();
    int off = 0, L = 0;
    for (int i = 0; i < 8; ++i) { off += i < wv ? cnt[i] : 0; L += cnt[i]; }
    if (v != 0) lab_sh[off + pre] = v;
    __syncthreads();
    if (b == drop_last_row && L > 0) --L;               // las/las.py:338 `[:-1]`: the batch's last nonzero entry
    int bad = 0;
    if (u < L) {
        const int c = lab_sh[u];
        bad = c < 0 || c > Vc - 2;
        int f = 1, n = -1;
        for (int k = 0; k < u && f; ++k) f = lab_sh[k] != c;
        for (int k = u + 1; k < L; ++k) if (lab_sh[k] == c) { n = k; break; }
        w.lab[(long long)b * U + u] = c;
        w.nxt[(long long)b * U + u] = n;
        w.first[(long long)b * U + u] = f;
    }
    bad = __syncthreads_or(bad);
    if (u == 0) w.len[b] = bad ? -1 : L;
}

// one wave per (b, t) row
__global__ __launch_bounds__(256) void ctc_gather_kernel(const float* __restrict__ logits, long long sb, long long st, int Vc,
                                                         const int* __restrict__ enc_len, int B, int Tp, int U, CtcWs w) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)B * Tp) return;
    const int b = (int)(row / Tp), t = (int)(row % Tp);
    const int L = w.len[b];
    if (t >= enc_len[b] || L < 0) return;
    const float* lp = logits + b * sb + t * st;
    float m = -INFINITY;
    for (int k = lane; k < Vc; k += 64) m = fmaxf(m, lp[k]);
    m = wave_max(m);
    float se = 0.f;
    for (int k = lane; k < Vc; k += 64) se += expf(lp[k] - m);
    se = wave_sum(se);
    const float lse = m + logf(se);
    if (lane == 0) w.lse[row] = lse;
    float* g = w.glp + row * (U + 1);
    const int* lab = w.lab + (long long)b * U;
    for (int j = lane; j <= L; j += 64) g[j] = lp[j == 0 ? Vc - 1 : lab[j - 1]] - lse;
}

// one workgroup per utterance, blockDim = 64 * ceil((2U+1) / 64) threads, state s = threadIdx.x
__global__ __launch_bounds__(1024) void ctc_alpha_beta_kernel(const int* __restrict__ enc_len, int Tp, int U, float* __restrict__ nll,
                                                              CtcWs w) {
    __shared__ double buf[2][CTC_MAX_STATES + 1];
    __shared__ int nxt_sh[512];
    __shared__ float red[16];
    __shared__ double logp_sh;
    const int b = blockIdx.x;
    const int s = threadIdx.x;
    const int L = w.len[b];
    const int T = min(enc_len[b], Tp);
    if (L < 0 || T <= 0) {                                // a bad label, or no frames: only L = 0 aligns with nothing
        if (s == 0) {
            nll[b] = L == 0 ? 0.f : INFINITY;
            if (L != 0) w.len[b] = -1;                     // zero gradient row (every thread has read len above: no thread waits)
        }
        return;
    }
    const int S = 2 * L + 1;
    const int SW = 2 * U + 1;
    const int* lab = w.lab + (long long)b * U;
    const bool act = s < S;
    const int col = (s & 1) ? (s >> 1) + 1 : 0;
    // s - 2 -> s and s -> s + 2 are allowed between two labels of different classes
    const bool skip_in = act && (s & 1) && s >= 3 && lab[s >> 1] != lab[(s >> 1) - 1];
    const bool skip_out = act && (s & 1) && s + 2 < S && lab[(s >> 1) + 1] != lab[s >> 1];
    const bool chain = s < L && w.first[(long long)b * U + s];
    if (s < L) nxt_sh[s] = w.nxt[(long long)b * U + s];
    const float* glp = w.glp + (long long)b * Tp * (U + 1);
    double* alpha = w.alpha + (long long)b * Tp * SW;

    // ---- alpha (log space) ----
    double a = (act && s <= 1) ? (double)glp[col] : -INFINITY;
    if (act) alpha[s] = a;
    buf[0][s] = a;
    float e_next = (act && T > 1) ? glp[(long long)(U + 1) + col] : -INFINITY;
    __syncthreads();
    int cur = 0;
    for (int t = 1; t < T; ++t) {
        const float e = e_next;
        if (act && t + 1 < T) e_next = glp[(long long)(t + 1) * (U + 1) + col];      // (in flight across the step)
        if (act) {
            const double* p = buf[cur];
            const double a1 = s >= 1 ? p[s - 1] : -INFINITY;
            const double a2 = skip_in ? p[s - 2] : -INFINITY;
            a = lse3(p[s], a1, a2) + e;
            alpha[(long long)t * SW + s] = a;
        }
        buf[cur ^ 1][s] = a;
        cur ^= 1;
        __syncthreads();
    }
    if (s == 0) {
        const double* p = buf[cur];
        const double lp = S >= 2 ? lse2(p[S - 1], p[S - 2]) : p[S - 1];
        logp_sh = lp;
        nll[b] = lp == -INFINITY ? INFINITY : (float)-lp;
        if (lp == -INFINITY) w.len[b] = -1;               // not alignable (repeats): zero gradient row
    }
    __syncthreads();
    const double logp = logp_sh;
    if (logp == -INFINITY) return;

    // ---- beta (emission at t excluded) and the posteriors gamma_t ----
    double bt = (act && s >= S - 2) ? 0.0 : -INFINITY;
    float* gam = w.gam + (long long)b * Tp * (U + 1);
    const int nw = blockDim.x >> 6;
    double al = act ? alpha[(long long)(T - 1) * SW + s] : -INFINITY;
    float e = act ? glp[(long long)(T - 1) * (U + 1) + col] : -INFINITY;
    for (int t = T - 1; t >= 0; --t) {
        double al_next = -INFINITY;
        float e_nx = -INFINITY;
        if (act && t > 0) {                               // (next step's loads in flight across this one)
            al_next = alpha[(long long)(t - 1) * SW + s];
            e_nx = glp[(long long)(t - 1) * (U + 1) + col];
        }
        const float pr = act ? expf((float)(al + bt - logp)) : 0.f;
        buf[0][s] = pr;
        const double q = e + bt;                           // lp_t(s) + beta_t(s): what beta_{t-1} sums over
        buf[1][s] = q;
        const float v = wave_sum((act && !(s & 1)) ? pr : 0.f);
        if ((s & 63) == 0) red[s >> 6] = v;
        __syncthreads();
        float* g = gam + (long long)t * (U + 1);
        if (s == 0) {                                     // blank: fixed-order sum of the even states
            float tot = 0.f;
            for (int i = 0; i < nw; ++i) tot += red[i];
            g[0] = tot;
        }
        if (chain) {                                      // one lane per distinct class: its repeats, in label order
            float tot = 0.f;
            for (int j = s; j >= 0; j = nxt_sh[j]) tot += (float)buf[0][2 * j + 1];
            g[s + 1] = tot;
        }
        if (act) {
            const double q1 = s + 1 < S ? buf[1][s + 1] : -INFINITY;
            const double q2 = skip_out ? buf[1][s + 2] : -INFINITY;
            bt = lse3(q, q1, q2);
        }
        al = al_next;
        e = e_nx;
        __syncthreads();
    }
}

// one wave per (b, t) row
template <typename OutT>
__device__ __forceinline__ void put(OutT* p, float v);
template <> __device__ __forceinline__ void put<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void put<unsigned short>(unsigned short* p, float v) { *p = f2bf(v); }

template <typename OutT>
__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ logits, long long sb, long long st, int Vc,
                                                       const int* __restrict__ enc_len, int B, int Tp, int U,
                                                       const float* __restrict__ scale_ptr, OutT* __restrict__ grad, long long gsb,
                                                       long long gst, CtcWs w) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long long)B * Tp) return;
    const int b = (int)(row / Tp), t = (int)(row % Tp);
    OutT* gp = grad + b * gsb + t * gst;
    const int L = w.len[b];
    if (t >= enc_len[b] || L < 0) {
        for (int k = lane; k < Vc; k += 64) put<OutT>(gp + k, 0.f);
        return;
    }
    const float* lp = logits + b * sb + t * st;
    const float lse = w.lse[row];
    const float sc = scale_ptr[0];
    for (int k = lane; k < Vc; k += 64) put<OutT>(gp + k, sc * expf(lp[k] - lse));
    // the corrections overwrite some of those elements: the dense stores of this wave complete first
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0);
    const float* g = w.gam + row * (U + 1);
    const int* lab = w.lab + (long long)b * U;
    const int* first = w.first + (long long)b * U;
    for (int j = lane; j <= L; j += 64) {
        if (j > 0 && !first[j - 1]) continue;
        const int k = j == 0 ? Vc - 1 : lab[j - 1];
        put<OutT>(gp + k, sc * (expf(lp[k] - lse) - g[j]));
    }
}

// loss[0] = scale * sum_b nll_b, fixed order (one wave)
__global__ __launch_bounds__(64) void ctc_sum_kernel(const float* __restrict__ nll, int B, const float* __restrict__ scale_ptr,
                                                     float* __restrict__ loss) {
    float v = 0.f;
    for (int i = threadIdx.x; i < B; i += 64) v += nll[i];
    v = wave_sum(v);
    if (threadIdx.x == 0) loss[0] = v * scale_ptr[0];
}

}  // namespace

extern "C" size_t las_ctc_workspace_bytes(int B, int Tp, int U) {
    if (B <= 0 || Tp <= 0 || U < 0) return 0;
    return ctc_ws_layout(B, Tp, U, nullptr, nullptr);
}

extern "C" int las_ctc_loss(const float* logits, long long sb, long long st, int Vc, const int* y, int ldy, int U, const int* enc_len,
                            int B, int Tp, int drop_last_row, float* nll, float* loss, const float* scale_ptr, void* grad, int grad_dtype,
                            long long gsb, long long gst, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(logits && y && enc_len && nll, "las_ctc_loss: logits, y, enc_len and nll must be given");
    LAS_ARG(B > 0 && Tp > 0 && Vc >= 2 && U >= 0 && ldy >= U, "las_ctc_loss: bad sizes (B=%d T'=%d Vc=%d U=%d ldy=%d)", B, Tp, Vc, U, ldy);
    LAS_ARG(2 * U + 1 <= CTC_MAX_STATES, "las_ctc_loss: U=%d labels per utterance, at most %d", U, (CTC_MAX_STATES - 1) / 2);
    LAS_ARG(st >= Vc && sb >= (long long)Tp * st, "las_ctc_loss: logits strides (%lld, %lld) overlap rows of %d", sb, st, Vc);
    LAS_ARG(drop_last_row >= -1 && drop_last_row < B, "las_ctc_loss: drop_last_row=%d outside [-1, %d)", drop_last_row, B);
    LAS_ARG(!(loss || grad) || scale_ptr, "las_ctc_loss: loss / grad need scale_ptr");
    LAS_ARG(!grad || grad_dtype == LAS_DT_F32 || grad_dtype == LAS_DT_BF16, "las_ctc_loss: grad_dtype %d", grad_dtype);
    LAS_ARG(!grad || (gst >= Vc && gsb >= (long long)Tp * gst), "las_ctc_loss: grad strides (%lld, %lld) overlap rows of %d", gsb, gst, Vc);
    LAS_ARG(ws && ws_bytes >= las_ctc_workspace_bytes(B, Tp, U), "las_ctc_loss: workspace too small (%zu < %zu)", ws_bytes,
            las_ctc_workspace_bytes(B, Tp, U));
    hipStream_t s = (hipStream_t)stream;
    CtcWs w;
    ctc_ws_layout(B, Tp, U, (char*)ws, &w);
    hipLaunchKernelGGL(ctc_labels_kernel, dim3(B), dim3(512), 0, s, y, ldy, U, Vc, drop_last_row, w);
    LAS_LAUNCHED();
    const dim3 rows(cdiv((long long)B * Tp, 4));
    hipLaunchKernelGGL(ctc_gather_kernel, rows, dim3(256), 0, s, logits, sb, st, Vc, enc_len, B, Tp, U, w);
    LAS_LAUNCHED();
    const int nt = (2 * U + 1 + 63) / 64 * 64;
    hipLaunchKernelGGL(ctc_alpha_beta_kernel, dim3(B), dim3(nt), 0, s, enc_len, Tp, U, nll, w);
    LAS_LAUNCHED();
    if (grad) {
        if (grad_dtype == LAS_DT_BF16)
            hipLaunchKernelGGL(ctc_grad_kernel<unsigned short>, rows, dim3(256), 0, s, logits, sb, st, Vc, enc_len, B, Tp, U, scale_ptr,
                               (unsigned short*)grad, gsb, gst, w);
        else
            hipLaunchKernelGGL(ctc_grad_kernel<float>, rows, dim3(256), 0, s, logits, sb, st, Vc, enc_len, B, Tp, U, scale_ptr,
                               (float*)grad, gsb, gst, w);
        LAS_LAUNCHED();
    }
    if (loss) {
        hipLaunchKernelGGL(ctc_sum_kernel, dim3(1), dim3(64), 0, s, (const float*)nll, B, scale_ptr, loss);
        LAS_LAUNCHED();
    }
    return 0;
}
