// kws.hip -- keyword search (spoken-term detection) on the CTC head: where in a recording is a listed phrase said, and how
// sure is the model?  Input: las_ctc_log_softmax's class-major log-probabilities [n, Vc, T'], blank = class Vc - 1.  The reference has
// nothing of this kind; the yardstick is the float64 restatement tests/kws_ref.py.
//
// The score (part of the contract, include/las_hip.h K10j).  m[u, t] = max_c lp[u, c, t] (an fp32 maximum: exact in any order);
// e(c, t) = (double)lp[u, c, t] - (double)m[u, t] <= 0, exactly 0.0 where c is the frame's arg-max.  A path's score is its
// log-likelihood ratio against the frame-wise best path over the same window: <= 0, exactly 0.0 when the phrase IS the greedy path.
// States s = 0 .. 2L - 2: even s = 2j is label j, odd s the blank between labels j and j + 1; no leading or trailing blank, the window
// starts on the first label and ends on the last: S = 2L - 1 <= 63.  Every state carries (best, start): no back-pointers, no back-trace.
// For t < T_u the candidates in this order, a later one replacing an earlier one only if STRICTLY greater:
//   1. stay (best(t-1, s), start(t-1, s));  2. s - 1 for s >= 1;  3. s - 2 for even s >= 2 whose label differs from the label before
//   it;  4. the fresh start (0.0, t) for s = 0 only;   then best(t, s) = chosen + e(label_s, t), the start carried.
// In front of t = 0 every state is (-inf, -1).  One fp64 subtraction and one fp64 addition per state and frame, in frame order, no
// products: a float64 restatement that does the same gives the same bits.  end_score[u, p, t] = best(t, 2L - 2), end_start its start;
// -inf / -1 for t >= T_u.  Hits and `best` are derived from the end series while it is produced (K10j states the rule).
//
// Two launches, stream-ordered on the caller's stream, no atomics:
//   kws_frame_max_kernel  one workgroup per (utterance, 64 frames): lanes along t (coalesced in the class-major layout), the Vc classes
//                         split over the workgroup's second dimension (16) and combined through LDS.  Reads lp once.
//   kws_search_kernel     one wavefront per (utterance, phrase), one state per lane; a 256-thread workgroup is four phrases of one
//                         utterance (they share that utterance's m and blank rows in cache).  No LDS, no barrier: the two predecessor
//                         reads are cross-lane moves of (double, int) inside the wave (DPP wave_shr:1, applied once and twice).  Lane s's emission row lp[u, c_s, :] is contiguous
//                         over t and loaded 16 frames ahead, four frames a load, in a register ring (ctc_align_viterbi_kernel's idea), so the loads stay
//                         off the T'-step dependent chain.  The end state's pair is broadcast every frame (v_readlane) and parked in lane
//                         t & 63; once per 64 frames the block's series is stored (when asked for), `best` takes the block's maximum
//                         and the candidate frames alone -- one ballot -- go through the hit rule as wave-uniform scalar work.  The
//                         kept list lives in the registers of lanes 0 .. H-1 (lane k = kept hit k): no indexed array, no scratch.
#include "las_common.h"
#include <math.h>

namespace {

constexpr int KW_MAX_L = 32;             // labels per phrase: S = 2L - 1 <= 63 states, one per lane of a wave
constexpr int KW_MAX_TP = 2048;          // las_ctc_align's limit
constexpr int KW_MAX_H = 8;              // kept hits per (utterance, phrase)
constexpr int KW_PF = 16;                // frames the emission loads run ahead of the recursion: a ring of four 4-frame groups
constexpr int KW_FM_Y = 16;              // class slices of kws_frame_max_kernel
constexpr int KW_WAVES = 4;              // phrases per workgroup of kws_search_kernel

typedef float kw_f4u __attribute__((ext_vector_type(4), aligned(4)));      // four floats at any float's address

// a lane's double in every lane (wave-uniform lane index): two v_readlane_b32
__device__ __forceinline__ double kw_readlane(double v, int lane) {
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane), lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    return __hiloint2double(hi, lo);
}

// grid (ceil(T'/64), n), block (64, KW_FM_Y)
__global__ __launch_bounds__(64 * KW_FM_Y) void kws_frame_max_kernel(const float* __restrict__ lp, int Vc, int Tp,
                                                                      const int* __restrict__ enc_len, float* __restrict__ m) {
    __shared__ float part[KW_FM_Y][64];
    const int u = blockIdx.y, t = blockIdx.x * 64 + threadIdx.x;
    const int T = clampi(enc_len[u], 1, Tp);
    if ((int)blockIdx.x * 64 >= T) return;                                     // (uniform: frames t >= T_u are never read)
    float v = -INFINITY;
    if (t < T) {
        const float* col = lp + (size_t)u * Vc * Tp + t;
#pragma unroll 4
        for (int c = threadIdx.y; c < Vc; c += KW_FM_Y) v = fmaxf(v, col[(size_t)c * Tp]);
    }
    part[threadIdx.y][threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.y == 0 && t < T) {
#pragma unroll
        for (int i = 1; i < KW_FM_Y; ++i) v = fmaxf(v, part[i][threadIdx.x]);
        m[(size_t)u * Tp + t] = v;
    }
}

// grid (ceil(P/4), n), 256 threads: wave w of workgroup (g, u) searches phrase 4 g + w in utterance u; state s = lane
__global__ __launch_bounds__(64 * KW_WAVES) void kws_search_kernel(const float* __restrict__ lp, const float* __restrict__ m, int Vc, int Tp,
                                                                    const int* __restrict__ enc_len, const int* __restrict__ y, int ldy,
                                                                    const int* __restrict__ y_len, const float* __restrict__ thr, int P,
                                                                    int U, int H, int* __restrict__ hit_start, int* __restrict__ hit_end,
                                                                    double* __restrict__ hit_score, int* __restrict__ count,
                                                                    double* __restrict__ best_score, int* __restrict__ best_span,
                                                                    double* __restrict__ end_score, int* __restrict__ end_start) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.y, p = blockIdx.x * KW_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (p >= P) return;                                                        // (wave-uniform; there is no barrier to miss)
    const int T = clampi(enc_len[u], 1, Tp);
    const size_t up = (size_t)u * P + p;
    const int Lraw = y_len[p], Lmax = U < KW_MAX_L ? U : KW_MAX_L;
    bool ok = Lraw >= 1 && Lraw <= Lmax;
    const int L = ok ? Lraw : 1, S = 2 * L - 1;
    const bool act = lane < S, even = !(lane & 1);
    int c = Vc - 1;                                                            // odd states: the blank
    if (ok && act && even) c = y[(size_t)p * ldy + (lane >> 1)];
    if (__any(c < 0 || c > Vc - 1 || (even && act && c == Vc - 1))) ok = false;    // a label outside [0, Vc - 2]: nothing is read for it
    double* es = end_score ? end_score + up * Tp : nullptr;
    int* et = end_score ? end_start + up * Tp : nullptr;
    if (!ok) {                                                                 // a phrase that cannot be searched
        if (lane == 0) {
            count[up * 2] = 0; count[up * 2 + 1] = 0;
            best_score[up] = -INFINITY; best_span[up * 2] = -1; best_span[up * 2 + 1] = -1;
        }
        if (es) for (int t = lane; t < Tp; t += 64) { es[t] = -INFINITY; et[t] = -1; }
        return;
    }
    const int cprev = __shfl_up(c, 2);                                          // the label before this state's (even lanes >= 2)
    const bool skip = act && even && lane >= 2 && c != cprev;
    const float* row = lp + ((size_t)u * Vc + c) * Tp;
    const float* mu = m + (size_t)u * Tp;
    const double thr_d = (double)thr[p];

    double b = -INFINITY;                                                      // best(t - 1, s), start(t - 1, s)
    int st = -1;
    // Four frames of a row per load: every lane reads another row, so a load instruction touches up to 63 cache lines whatever its width,
    // and the address path, not the data, is what the loads cost.  The rows start at any multiple of four bytes (T' % 4 is anything):
    // the 16-byte load is an unaligned one, and the last group of a row is read float by float so that nothing is read behind lp.
    auto load4 = [&](const float* base, int t, bool on) {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on && t < T) {
            if (t + 4 <= Tp) {
                const kw_f4u q = *(const kw_f4u*)(base + t);                    // one global_load_dwordx4, four-byte aligned
                r = make_float4(q.x, q.y, q.z, q.w);
            } else {
                r.x = base[t];
                if (t + 1 < Tp) r.y = base[t + 1];
                if (t + 2 < Tp) r.z = base[t + 2];
            }
        }
        return r;
    };
    float4 er[KW_PF / 4], mr[KW_PF / 4];
#pragma unroll
    for (int g = 0; g < KW_PF / 4; ++g) {
        er[g] = load4(row, 4 * g, act);
        mr[g] = load4(mu, 4 * g, true);
    }
    // wave-uniform bookkeeping of the end series
    // (best_sc starts at 0.0 beside a flag, not at -inf: the compiler here encodes a wave-uniform fp64 -inf as s_mov_b64 with a 64-bit
    //  literal, of which the instruction holds the low 32 bits only -- the register would start at 0.0)
    bool open = false, reached = false;
    double o_sc = 0.0, best_sc = 0.0;
    int o_st = 0, o_en = 0, best_st = -1, best_en = -1, kept = 0, total = 0;
    double k_sc = 0.0, ser_sc = -INFINITY;                                     // lane k: kept hit k;  lane t & 63: frame t of the series
    int k_st = 0, k_en = 0, ser_st = -1;

    auto close_hit = [&](double sc, int s0, int s1) {
        ++total;
        if (kept < H) {
            if (lane == kept) { k_sc = sc; k_st = s0; k_en = s1; }
            ++kept;
            return;
        }
        double wsc = kw_readlane(k_sc, 0);                                     // the weakest kept hit: the smallest score, the earliest among equals
        int wi = 0;
#pragma unroll
        for (int k = 1; k < KW_MAX_H; ++k) {
            const double v = kw_readlane(k_sc, k);
            if (k < H && v < wsc) { wsc = v; wi = k; }
        }
        if (sc > wsc) {                                                        // (uniform) the survivors shift down, the new hit is appended
            const double n_sc = __shfl_down(k_sc, 1);
            const int n_st = __shfl_down(k_st, 1), n_en = __shfl_down(k_en, 1);
            if (lane >= wi && lane < H - 1) { k_sc = n_sc; k_st = n_st; k_en = n_en; }
            if (lane == H - 1) { k_sc = sc; k_st = s0; k_en = s1; }
        }
    };

    // The end state's pair of frame t is parked in lane t & 63; every 64 frames (and at T_u) the block is looked at as a whole: the series
    // is stored coalesced, `best` takes the block's maximum, and only the candidate frames -- one ballot -- go through the scalar hit
    // rule, in frame order.  So the per-frame dependent chain carries the recursion and one broadcast, and none of the bookkeeping.
    for (int tb = 0; tb < T; tb += 64) {
        const int tend = tb + 64 < T ? tb + 64 : T;
        for (int t0 = tb; t0 < tend; t0 += KW_PF) {
#pragma unroll
            for (int g = 0; g < KW_PF / 4; ++g) {
                const int tg = t0 + 4 * g;
                if (tg >= tend) continue;                                      // (uniform)
                const float4 e4 = er[g], m4 = mr[g];
                if (tg + KW_PF < T) {                                          // in flight across KW_PF steps
                    er[g] = load4(row, tg + KW_PF, act);
                    mr[g] = load4(mu, tg + KW_PF, true);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int t = tg + j;
                    if (t >= tend) continue;                                   // (uniform)
                    const float ev = j == 0 ? e4.x : j == 1 ? e4.y : j == 2 ? e4.z : e4.w;
                    const float mv = j == 0 ? m4.x : j == 1 ? m4.y : j == 2 ? m4.z : m4.w;
                    const double b1 = wave_shr1(b), b2 = wave_shr1(b1);        // lanes 0 (and 1 for the second) read nothing they use
                    const int s1 = wave_shr1(st), s2 = wave_shr1(s1);
                    double cb = b;
                    int cs = st;
                    if (lane >= 1 && b1 > cb) { cb = b1; cs = s1; }            // equal values: the earlier candidate stays
                    if (skip && b2 > cb) { cb = b2; cs = s2; }
                    if (lane == 0 && 0.0 > cb) { cb = 0.0; cs = t; }
                    const double e = (double)ev - (double)mv;
                    b = act ? cb + e : -INFINITY;
                    st = act ? cs : -1;
                    const double esc = kw_readlane(b, S - 1);
                    const int est = __builtin_amdgcn_readlane(st, S - 1);
                    if (lane == t - tb) { ser_sc = esc; ser_st = est; }
                }
            }
        }
        const int tt = tb + lane;
        const bool valid = tt < tend;
        if (es && valid) { es[tt] = ser_sc; et[tt] = ser_st; }
        const double v = valid ? ser_sc : -INFINITY;
        double mx = v;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d));
        mx = kw_readlane(mx, 0);
        if (mx > -INFINITY) {                                                  // (uniform) the end state was reached in this block
            if (!reached || mx >= best_sc) {                                   // equal values: the later end, in the block and across blocks
                const int k = 63 - __builtin_clzll(__ballot(valid && v == mx));
                reached = true; best_sc = mx; best_st = __builtin_amdgcn_readlane(ser_st, k); best_en = tb + k;
            }
            unsigned long long cand = __ballot(valid && v > -INFINITY && v >= thr_d);
            while (cand) {                                                     // the candidates, in frame order
                const int k = __builtin_ctzll(cand);
                cand &= cand - 1;
                const double sc = kw_readlane(ser_sc, k);
                const int s0 = __builtin_amdgcn_readlane(ser_st, k);
                if (open && s0 <= o_en) {
                    if (sc >= o_sc) { o_sc = sc; o_st = s0; o_en = tb + k; }
                } else {
                    if (open) close_hit(o_sc, o_st, o_en);
                    open = true; o_sc = sc; o_st = s0; o_en = tb + k;
                }
            }
        }
    }
    if (open) close_hit(o_sc, o_st, o_en);
    if (lane < kept) {
        hit_start[up * H + lane] = k_st;
        hit_end[up * H + lane] = k_en;
        hit_score[up * H + lane] = k_sc;
    }
    if (lane == 0) {
        count[up * 2] = kept; count[up * 2 + 1] = total;
        best_score[up] = reached ? best_sc : -INFINITY; best_span[up * 2] = best_st; best_span[up * 2 + 1] = best_en;
    }
    if (es) for (int t = T + lane; t < Tp; t += 64) { es[t] = -INFINITY; et[t] = -1; }
}

}  // namespace

extern "C" size_t las_kws_workspace_bytes(int n, int Tp) {
    if (n <= 0 || Tp <= 0) return 0;
    return align256((size_t)n * Tp * 4);
}

extern "C" int las_kws_search(const float* lp, int Vc, int Tp, const int* enc_len, int n, const int* y, int ldy, const int* y_len,
                              const float* thr, int P, int U, int H, int* hit_start, int* hit_end, double* hit_score, int* count,
                              double* best_score, int* best_span, double* end_score, int* end_start, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(lp && enc_len && y && y_len && thr, "las_kws_search: lp, enc_len, y, y_len and thr must be given");
    LAS_ARG(hit_start && hit_end && hit_score && count && best_score && best_span,
            "las_kws_search: hit_start, hit_end, hit_score, count, best_score and best_span must be given");
    LAS_ARG(U >= 1 && U <= KW_MAX_L, "las_kws_search: U=%d tokens per phrase, 1 to %d", U, KW_MAX_L);
    LAS_ARG(Tp > 0 && Tp <= KW_MAX_TP, "las_kws_search: 1 <= T' <= %d (got %d)", KW_MAX_TP, Tp);
    LAS_ARG(H >= 1 && H <= KW_MAX_H, "las_kws_search: H=%d kept hits per utterance and phrase, 1 to %d", H, KW_MAX_H);
    LAS_ARG(n > 0 && n <= 65535 && P > 0 && P <= 65535 && Vc >= 2 && ldy >= U, "las_kws_search: bad sizes (n=%d P=%d Vc=%d U=%d ldy=%d)", n, P,
            Vc, U, ldy);
    LAS_ARG((end_score == nullptr) == (end_start == nullptr), "las_kws_search: end_score and end_start are given together or not at all");
    LAS_ARG(ws && ws_bytes >= las_kws_workspace_bytes(n, Tp), "las_kws_search: workspace too small (%zu < %zu)", ws_bytes,
            las_kws_workspace_bytes(n, Tp));
    hipStream_t s = (hipStream_t)stream;
    float* m = (float*)ws;
    hipLaunchKernelGGL(kws_frame_max_kernel, dim3(cdiv(Tp, 64), n), dim3(64, KW_FM_Y), 0, s, lp, Vc, Tp, enc_len, m);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(kws_search_kernel, dim3(cdiv(P, KW_WAVES), n), dim3(64 * KW_WAVES), 0, s, lp, (const float*)m, Vc, Tp, enc_len, y, ldy,
                       y_len, thr, P, U, H, hit_start, hit_end, hit_score, count, best_score, best_span, end_score, end_start);
    LAS_LAUNCHED();
    return 0;
}
