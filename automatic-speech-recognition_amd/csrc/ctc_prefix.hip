// ctc_prefix.hip -- CTC prefix scores for joint CTC-attention beam search (Watanabe et al. 2017, Algorithm 2; the
// equations of ESPnet's CTCPrefixScore, with EOS scored as an ordinary final label).
//
// Two entry points (include/las_hip.h):
//   las_ctc_log_softmax   once per batch: the CTC head's logits [n, T', V+1] -> class-major log-probabilities [n, V+1, T'] (a candidate's
//                         column is contiguous over t).  One workgroup per (utterance, 64 frames): log-sum-exp of each frame, then the
//                         tile is transposed through LDS 64 classes at a time.
//   las_ctc_prefix_step   once per search step, between the step's logits and las_beam_loop_step.  One workgroup per hypothesis row:
//                           1. the row's state r^n, r^b of its parent g is advanced by the token c that entered the step (at step 0: the
//                              empty prefix's state), and psi(h = g.c) is recomputed by the SAME device function that scored c as a
//                              candidate of g one step earlier (identical inputs: the gathered state is a bit copy), so a hypothesis'
//                              prefix-score deltas telescope exactly;
//                           2. the row's candidate bank (the top-64 of its logits by (logit, token id); every token when V <= 64) is scored:
//                              psi(h.v) = logsumexp(start(v), logsumexp_{t >= 1} (phi_{t-1}(h, v) + y_t[v])), one wave per candidate, lanes
//                              over t; the EOS candidate is the full-sequence probability of h.EOS, a chain that runs in lock step with the
//                              advance of step 1;
//                           3. joint[row][v] = logit[v] + lam * (psi(h.v) - psi(h)) for the candidates, -inf for every other token.
//                         Live rows only, by the rule every scorer shares (search_rows.h): the launch is the same every step and is
//                         captured into the search's HIP graph.  No atomics; fixed reduction orders: same bits every run.
//
// State row (state_width >= 2 T' + 2 floats): [0, T') r^n_t(h), [T', 2 T') r^b_t(h), [2 T'] psi(h), [2 T' + 1] last label of h (-1: empty).
// All values are log-probabilities in fp32; LOGZERO = -1e10 (ESPnet's constant) instead of -inf keeps impossible prefixes finite.
#include "las_common.h"
#include "search_rows.h"
#include <math.h>

namespace {

constexpr float CP_LOGZERO = -1e10f;
constexpr int CP_TOPN = 64;                  // the reference's candidate bank (las/beam_search.py:123)
constexpr int CP_MAX_SLOTS = 64;             // candidate selection: V <= 64 x 256 tokens held in registers
constexpr int CP_MAX_TP = 2048;              // six [T'] fp32 arrays in LDS (48 KB)

__device__ __forceinline__ float lae(float a, float b) {                    // log(exp(a) + exp(b)), both finite
    const float m = fmaxf(a, b);
    return m + __logf(1.f + __expf(-fabsf(a - b)));
}
// psi(h.v) by one wave: logsumexp of `start` and of phi[t-1] + y[t] for 1 <= t < T.  phi: LDS, y: the candidate's column (LDS or global),
// read once: every lane keeps a running (max, sum of exp) pair, and the pairs meet in an xor butterfly (the combination is symmetric in
// its two operands, so every lane ends with the same bits).  Called with the same arguments for (h, v) as a candidate and for h.v's own
// psi one step later: the same bits.
__device__ __forceinline__ float wave_psi(const float* phi, const float* y, int T, float start, int lane) {
    constexpr float NONE = -3.0e38f;                    // (finite: two empty lanes combine to an empty pair, not NaN)
    float m = lane == 0 ? start : NONE, s = lane == 0 ? 1.f : 0.f;
    for (int t = 1 + lane; t < T; t += 64) {
        const float x = phi[t - 1] + y[t];
        if (x > m) { s = s * __expf(m - x) + 1.f; m = x; }
        else s += __expf(x - m);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float m2 = __shfl_xor(m, off, 64), s2 = __shfl_xor(s, off, 64);
        const float mm = fmaxf(m, m2);
        s = s * __expf(m - mm) + s2 * __expf(m2 - mm);
        m = mm;
    }
    return m + __logf(s);
}

struct CtcPrefixDev : SearchRows {                                     // (the rows and search_row_live: search_rows.h)
    const float* lp; const int* enc_len; const float* logits; float* joint;
    int V, Tp, end_id; float lam;
};

// BANK: V > 64, the top-64 cut binds and is selected here (a V <= 64 vocabulary takes every token and needs none of its registers)
template <bool BANK>
__global__ __launch_bounds__(256) void ctc_prefix_step_kernel(CtcPrefixDev a) {
    extern __shared__ float cp_lds[];
    __shared__ int cand[CP_TOPN];
    __shared__ int wcnt[2][4];
    __shared__ float psi_s[2];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int t_step, u;
    if (!search_row_live(a, row, t_step, u)) return;                   // (a row that is not live: its joint row is never ranked)
    const int Tp = a.Tp, V = a.V, Vc = V + 1, W = a.width;
    const int T = clampi(a.enc_len[u], 1, Tp);
    float* RN = cp_lds;                 // r^n of the parent, then of h
    float* RB = RN + Tp;                // r^b ...
    float* P = RB + Tp;                 // phi of the parent for c (t-1 -> index t-1), then phi_o of h
    float* YC = P + Tp;                 // y_t[c], y_t[blank], y_t[EOS]
    float* YB = YC + Tp;
    float* YE = YB + Tp;
    const float* col = a.lp + (size_t)u * Vc * Tp;
    const int c = clampi(a.token[row], 0, V - 1);                      // (always a token id; clamped: no read outside lp)
    const bool first = t_step == 0;     // h = [SOS]: the empty prefix (no advance)
    const float* sp = a.st_in + (size_t)row * W;
    for (int i = tid; i < T; i += 256) {
        YC[i] = col[(size_t)c * Tp + i]; YB[i] = col[(size_t)V * Tp + i]; YE[i] = col[(size_t)a.end_id * Tp + i];
        if (!first) { RN[i] = sp[i]; RB[i] = sp[Tp + i]; }
    }
    const int last_g = first ? -1 : (int)sp[2 * Tp + 1];
    const int last_h = first ? -1 : c;
    const float* lg = a.logits + (size_t)row * V;
    float* jo = a.joint + (size_t)row * V;

    // ---- the candidate bank (V > 64: top-64 by (logit, token id), the order of las_beam_step's keys)
    int ncand;
    if constexpr (!BANK) {
        if (tid < V) cand[tid] = tid;
        ncand = V;
    } else {
        const int NS = (V + 255) >> 8;
        unsigned KA[CP_MAX_SLOTS];
#pragma unroll
        for (int s = 0; s < CP_MAX_SLOTS; ++s) {
            const int v = s * 256 + tid;
            KA[s] = (s < NS && v < V) ? order_key(lg[v] + 0.f) : 0u;
        }
        // largest TA with count(key >= TA) >= 64 (counts: per-slot ballots, the four waves' sums through LDS, one barrier per probe)
        auto count_ge = [&](auto pred, int parity) {
            int cnt = 0;
#pragma unroll
            for (int s = 0; s < CP_MAX_SLOTS; ++s) {
                if (s >= NS) continue;
                const int v = s * 256 + tid;
                cnt += __builtin_popcountll(__builtin_amdgcn_ballot_w64(v < V && pred(KA[s], v)));
            }
            if (lane == 0) wcnt[parity][w] = cnt;
            __syncthreads();
            return wcnt[parity][0] + wcnt[parity][1] + wcnt[parity][2] + wcnt[parity][3];
        };
        unsigned TA = 0;
        int par = 0;
        for (int b = 31; b >= 0; --b) {
            const unsigned probe = TA | (1u << b);
            if (count_ge([&](unsigned k, int) { return k >= probe; }, par) >= CP_TOPN) TA = probe;
            par ^= 1;
        }
        const int gt = count_ge([&](unsigned k, int) { return k > TA; }, par);
        par ^= 1;
        const int eq = count_ge([&](unsigned k, int) { return k == TA; }, par);
        par ^= 1;
        int TV = 0;
        if (eq > CP_TOPN - gt) {                        // equal logits at the cut: the larger token ids
            for (int b = 13; b >= 0; --b) {
                const int probe = TV | (1 << b);
                if (count_ge([&](unsigned k, int v) { return k == TA && v >= probe; }, par) >= CP_TOPN - gt) TV = probe;
                par ^= 1;
            }
        }
        // compaction in (wave, slot, lane) order; every other token gets -inf
        int mine = 0;
#pragma unroll
        for (int s = 0; s < CP_MAX_SLOTS; ++s) {
            if (s >= NS) continue;
            const int v = s * 256 + tid;
            mine += __builtin_popcountll(__builtin_amdgcn_ballot_w64(v < V && (KA[s] > TA || (KA[s] == TA && v >= TV))));
        }
        if (lane == 0) wcnt[par][w] = mine;
        __syncthreads();
        int base = 0;
        for (int ww = 0; ww < w; ++ww) base += wcnt[par][ww];
        const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
        for (int s = 0; s < CP_MAX_SLOTS; ++s) {
            if (s >= NS) continue;
            const int v = s * 256 + tid;
            const bool sel = v < V && (KA[s] > TA || (KA[s] == TA && v >= TV));
            const unsigned long long m = __builtin_amdgcn_ballot_w64(sel);
            if (sel) { const int pos = base + __popcll(m & lt); if (pos < CP_TOPN) cand[pos] = v; }
            else if (v < V) jo[v] = -INFINITY;
            base += __popcll(m);
        }
        ncand = CP_TOPN;
    }
    __syncthreads();                                    // YC / YB / YE, the parent's state, cand[]

    // ---- 1. advance: phi of the parent for c, psi(h) (wave 0), the chains of h and of h.EOS (wave 1, lane 0)
    if (!first)
        for (int i = tid; i < T - 1; i += 256) P[i] = (c == last_g) ? RB[i] : lae(RB[i], RN[i]);
    __syncthreads();
    if (w == 0) {
        const float psi_h = first ? 0.f : wave_psi(P, YC, T, last_g < 0 ? YC[0] : CP_LOGZERO, lane);
        if (lane == 0) psi_s[0] = psi_h;
    } else if (w == 1 && lane == 0) {
        float hn, hb;
        if (first) { hn = CP_LOGZERO; hb = YB[0]; }
        else { hn = last_g < 0 ? YC[0] : CP_LOGZERO; hb = CP_LOGZERO; }
        float en = first ? YE[0] : CP_LOGZERO, eb = CP_LOGZERO;
        RN[0] = hn; RB[0] = hb;
        for (int i = 1; i < T; ++i) {
            const float ph = (a.end_id == last_h) ? hb : lae(hb, hn);          // phi_{i-1}(h, EOS)
            const float en2 = lae(en, ph) + YE[i], eb2 = lae(eb, en) + YB[i];
            float hn2, hb2;
            if (first) { hn2 = CP_LOGZERO; hb2 = hb + YB[i]; }
            else { hn2 = lae(hn, P[i - 1]) + YC[i]; hb2 = lae(hb, hn) + YB[i]; }
            hn = hn2; hb = hb2; en = en2; eb = eb2;
            RN[i] = hn; RB[i] = hb;
        }
        psi_s[1] = lae(en, eb);
    }
    __syncthreads();
    const float psi_h = psi_s[0], psi_e = psi_s[1];
    float* so = a.st_out + (size_t)row * W;
    for (int i = tid; i < T; i += 256) { so[i] = RN[i]; so[Tp + i] = RB[i]; }
    if (tid == 0) { so[2 * Tp] = psi_h; so[2 * Tp + 1] = (float)last_h; }
    for (int i = tid; i < T - 1; i += 256) P[i] = lae(RB[i], RN[i]);         // phi_o of h (the same expression as P of the next step)
    __syncthreads();

    // ---- 2./3. the candidates, one wave each
    for (int k = w; k < ncand; k += 4) {
        const int v = cand[k];
        float psi;
        if (v == a.end_id) psi = psi_e;
        else {
            const float* yv = col + (size_t)v * Tp;
            psi = wave_psi(v == last_h ? RB : P, yv, T, first ? yv[0] : CP_LOGZERO, lane);
        }
        if (lane == 0) jo[v] = __fadd_rn(lg[v], __fmul_rn(a.lam, __fsub_rn(psi, psi_h)));
    }
}

// ---- class-major log-softmax of the head's logits
constexpr int LS_TILE = 64;
__global__ __launch_bounds__(256) void ctc_log_softmax_kernel(const float* __restrict__ x, int Tp, int Vc, float* __restrict__ out) {
    __shared__ float lse[LS_TILE];
    __shared__ float tile[LS_TILE][LS_TILE + 1];
    const int u = blockIdx.y, t0 = blockIdx.x * LS_TILE, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* xu = x + ((size_t)u * Tp) * Vc;
    for (int f = w * 16; f < w * 16 + 16; ++f) {
        const int t = t0 + f;
        float m = -INFINITY, s = 0.f;
        if (t < Tp) {
            const float* r = xu + (size_t)t * Vc;
            for (int v = lane; v < Vc; v += 64) m = fmaxf(m, r[v]);
            m = wave_max(m);                                            // (every lane is here: t < Tp is the wave's, t = t0 + f and
            for (int v = lane; v < Vc; v += 64) s += expf(r[v] - m);   //  f runs over [16 w, 16 w + 16) in every lane of wave w)
            s = wave_sum(s);
        }
        if (lane == 0) lse[f] = t < Tp ? m + logf(s) : 0.f;
    }
    __syncthreads();
    float* ou = out + (size_t)u * Vc * Tp;
    for (int c0 = 0; c0 < Vc; c0 += LS_TILE) {
        for (int f = w * 16; f < w * 16 + 16; ++f) {
            const int t = t0 + f, cc = c0 + lane;
            tile[f][lane] = (t < Tp && cc < Vc) ? xu[(size_t)t * Vc + cc] - lse[f] : 0.f;
        }
        __syncthreads();
        for (int k = w * 16; k < w * 16 + 16; ++k) {
            const int cc = c0 + k, t = t0 + lane;
            if (cc < Vc && t < Tp) ou[(size_t)cc * Tp + t] = tile[lane][k];
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int las_ctc_log_softmax(const float* logits, int n, int Tp, int Vc, float* out, void* stream) {
    LAS_ARG(logits && out, "las_ctc_log_softmax: null pointer");
    LAS_ARG(n > 0 && Tp > 0 && Vc > 1, "las_ctc_log_softmax: bad dims (n %d, Tp %d, Vc %d)", n, Tp, Vc);
    hipLaunchKernelGGL(ctc_log_softmax_kernel, dim3(cdiv(Tp, LS_TILE), n), dim3(256), 0, (hipStream_t)stream, logits, Tp, Vc, out);
    LAS_LAUNCHED();
    return 0;
}

extern "C" int las_ctc_prefix_step(const float* lp, const int* enc_len, int nutt, int beam, int Tp, int V, int end_id,
                                   const float* logits, float* joint, float lam, const float* state_in, float* state_out,
                                   int state_width, const int* token, const int* step, const int* nlive, const int* done,
                                   const int* dec_step, int Umax, void* stream) {
    LAS_ARG(Tp > 0 && Tp <= CP_MAX_TP, "las_ctc_prefix_step: 1 <= T' <= %d (got %d)", CP_MAX_TP, Tp);
    CtcPrefixDev a;
    if (search_rows_args(a, "las_ctc_prefix_step", 2 * Tp + 2, nutt, beam, state_in, state_out, state_width,
                         token, step, nlive, done, dec_step, Umax)) return -1;
    LAS_ARG(lp && enc_len && logits && joint && token, "las_ctc_prefix_step: null pointer");
    LAS_ARG(V > 1 && end_id >= 0 && end_id < V, "las_ctc_prefix_step: bad dims");
    LAS_ARG(V <= CP_MAX_SLOTS * 256, "las_ctc_prefix_step: V <= %d (got %d)", CP_MAX_SLOTS * 256, V);
    a.lp = lp; a.enc_len = enc_len; a.logits = logits; a.joint = joint; a.V = V; a.Tp = Tp; a.end_id = end_id; a.lam = lam;
    const size_t lds = (size_t)6 * Tp * sizeof(float);
    if (V > CP_TOPN) hipLaunchKernelGGL(ctc_prefix_step_kernel<true>, dim3(nutt * beam), dim3(256), lds, (hipStream_t)stream, a);
    else             hipLaunchKernelGGL(ctc_prefix_step_kernel<false>, dim3(nutt * beam), dim3(256), lds, (hipStream_t)stream, a);
    LAS_LAUNCHED();
    return 0;
}
