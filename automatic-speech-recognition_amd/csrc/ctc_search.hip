// ctc_search.hip -- K10h: CTC-only decoding: a transcript from the CTC head alone, without the Speller.
//
// las_ctc_frame_topk   one workgroup of 256 lanes per (utterance, frame) over the head's frame-major logits [n, Tp, Vc] (Vc = V + 1,
//                      blank = class V): max, sum of exp, lse = m + logf(s); the argmax class over all Vc (ties: the lower id); the C
//                      non-blank classes of largest logit (ties: the lower id) LISTED IN ASCENDING TOKEN ID.  Selection: bisection over
//                      the order-preserving bits of the logits for the C-th largest key (32 counting passes; the first 20 keys of a
//                      lane stay in registers, classes from 5120 on are re-read), then one pass that compacts {key > cut} and the first C - count of {key == cut} in lane
//                      order.  Log-probabilities are z - lse.  C = 0 selects nothing.  Frames t >= T'_u are neither read nor written.
// las_ctc_greedy       one workgroup per utterance: emit best[t] where it is no blank and differs from best[t - 1], compacted in frame
//                      order; the score is the float64 sum of best_lp in frame order (one lane).
// las_ctc_beam_search  one workgroup of 512 lanes per utterance, sequential over its frames: CTC prefix beam search (Hannun et al. 2014)
//                      with an optional back-off n-gram (ngram_trie.h: the tables of las/ngram.py, pre-scaled) and a length bonus.
//   Mass at or below LOGZERO (-1e10) is no mass: a sum with such a term is LOGZERO and logaddexp ignores it.
//   Beam state (LDS, K slots, best first): trie node, p_b, p_nb, last token, n-gram node, length.  A frame:
//     stay      slot j keeps p_b' = y_blank + tot_j and p_nb' = [last_j is a candidate] (y + p_nb_j); if its PARENT prefix is in the beam
//               too, the parent's extension by last_j is this same prefix: its mass is gathered here, (+) p_nb', by the slot's own lane
//               (a prefix has one parent, so at most two terms meet and no scatter is needed).
//     extend    K C lanes of work: slot j by candidate i, unless j is closed (last = EOS) or the child is in the beam (gathered above):
//               y + (c == last_j ? p_b_j : tot_j) + g,  g = lm(c | node_j) + len_bonus.  The child's trie node is looked up in a hash
//               table keyed (parent node, token); the n-gram descent is done by the lane itself.
//     prune     up to K rounds of a workgroup arg-max over the K (C + 1) entries in LDS, key (total, lower entry index): entries that
//               were in the beam come first in slot order, then extensions by (parent slot, candidate position).  Entries at or below
//               LOGZERO never enter: the beam may hold fewer than K.
//     insert    only survivors get trie nodes, one lane, at most K per frame; there is ONE node per (parent, token) ever: a prefix that
//               left the beam and comes back finds its old node through the table, so a descendant that stayed still points at it.
//   After the last frame the slots are the ranked hypotheses; their tokens are walked back through the trie.
//   Workspace per utterance: NN = K Tp + 1 nodes x (parent, token, length, slot) and a table of H = the power of two >= 2 NN entries.
//   Bounds: T'_u is clamped to [0, Tp]; candidate tokens outside [0, V) are skipped; every n-gram access goes through ngram_trie.h's
//   clamps, a next outside [0, M) is the root; node numbers never exceed NN - 1.  No atomics: two runs give the same bits.
#include "las_common.h"
#include "ngram_trie.h"
#include <math.h>

namespace {

constexpr int CTC_MAX_K = 64;
constexpr int CTC_MAX_C = 64;
constexpr int TOPK_NT = 256;
constexpr int TOPK_REGS = 20;                         // keys a lane keeps in registers across the bisection: 5120 classes in all
constexpr int BEAM_NT = 512;
constexpr int BEAM_MAX_E = CTC_MAX_K * (CTC_MAX_C + 1);
#define CTC_LOGZERO (-1e10f)

typedef unsigned long long u64;

// float -> unsigned whose order is the floats' (-0 and +0 are one key).  The mapping is las_common.h's order_key bit for bit; it stays
// written out as a select here because the compiler turns the two spellings into different code, and with order_key's the beam kernel
// measured 1 % slower (3375 against 3345 us per 64 utterances x 150 frames, tools/bench_ctc_search.py, alternating runs)
__device__ __forceinline__ unsigned okey(float f) {
    if (f == 0.f) f = 0.f;
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <int NT> __device__ __forceinline__ int block_isum(int v, int* red) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) s += red[i];
    return s;
}
template <int NT> __device__ __forceinline__ u64 block_u64max(u64 v, u64* red) {
    for (int o = 32; o; o >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, o), hi = __shfl_xor((unsigned)(v >> 32), o);
        const u64 w = ((u64)hi << 32) | lo;
        v = w > v ? w : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) s = red[i] > s ? red[i] : s;
    return s;
}

// ---- frame summary ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TOPK_NT) void ctc_frame_topk_kernel(const float* __restrict__ logits, const int* __restrict__ enc_len, int Tp,
                                                                 int Vc, int C, int* __restrict__ cand_tok, float* __restrict__ cand_lp,
                                                                 float* __restrict__ blank_lp, int* __restrict__ best,
                                                                 float* __restrict__ best_lp) {
    __shared__ float redf[TOPK_NT / 64];
    __shared__ int redi[TOPK_NT / 64];
    __shared__ u64 redu[TOPK_NT / 64];
    __shared__ int wg[TOPK_NT / 64], we[TOPK_NT / 64];
    const int u = blockIdx.x / Tp, t = blockIdx.x - u * Tp, tid = threadIdx.x;
    const int Tu = clampi(enc_len[u], 0, Tp);
    if (t >= Tu) return;
    const size_t f = (size_t)u * Tp + t;
    const float* z = logits + f * Vc;
    const int V = Vc - 1;

    float m = -INFINITY;
    u64 bk = 0;
    for (int v = tid; v < Vc; v += TOPK_NT) {
        const float zv = z[v];
        m = fmaxf(m, zv);
        const u64 k = ((u64)okey(zv) << 32) | (0xffffffffu - (unsigned)v);
        bk = k > bk ? k : bk;
    }
    m = block_max<TOPK_NT>(m, redf);
    float s = 0.f;
    for (int v = tid; v < Vc; v += TOPK_NT) s += expf(z[v] - m);
    s = block_sum<TOPK_NT>(s, redf);
    const float lse = m + logf(s);
    bk = block_u64max<TOPK_NT>(bk, redu);
    if (tid == 0) {
        const int b = clampi((int)(0xffffffffu - (unsigned)bk), 0, V);
        best[f] = b;
        best_lp[f] = z[b] - lse;
        blank_lp[f] = z[V] - lse;
    }
    if (C == 0) return;                                                // (greedy needs no candidates)

    // the C-th largest key of the non-blank classes
    unsigned kreg[TOPK_REGS];
#pragma unroll
    for (int j = 0; j < TOPK_REGS; ++j) {
        const int v = tid + TOPK_NT * j;
        kreg[j] = v < V ? okey(z[v]) : 0u;                             // (a counted key is >= 1: 0 never counts)
    }
    unsigned cut = 0;
    for (int b = 31; b >= 0; --b) {
        const unsigned probe = cut | (1u << b);
        int c = 0;
#pragma unroll
        for (int j = 0; j < TOPK_REGS; ++j) c += kreg[j] >= probe;
        for (int v = tid + TOPK_NT * TOPK_REGS; v < V; v += TOPK_NT) c += okey(z[v]) >= probe;
        if (block_isum<TOPK_NT>(c, redi) >= C) cut = probe;
    }
    int above = 0;
#pragma unroll
    for (int j = 0; j < TOPK_REGS; ++j) above += kreg[j] > cut;
    for (int v = tid + TOPK_NT * TOPK_REGS; v < V; v += TOPK_NT) above += okey(z[v]) > cut;
    const int need = C - block_isum<TOPK_NT>(above, redi);             // how many of the keys equal to the cut are taken, lowest ids first

    // compaction in lane order: ascending token id
    const int lane = tid & 63, w = tid >> 6;
    const u64 below = (1ull << lane) - 1ull;
    int run_gt = 0, run_eq = 0;
    for (int base = 0; base < V; base += TOPK_NT) {
        const int v = base + tid;
        const bool ok = v < V;
        const float zv = ok ? z[v] : 0.f;
        const unsigned k = ok ? okey(zv) : 0u;
        const bool gt = ok && k > cut, eq = ok && k == cut;
        const u64 bg = __ballot(gt), be = __ballot(eq);
        __syncthreads();
        if (lane == 0) { wg[w] = __popcll(bg); we[w] = __popcll(be); }
        __syncthreads();
        int gb = run_gt + __popcll(bg & below), eb = run_eq + __popcll(be & below);
        for (int i = 0; i < TOPK_NT / 64; ++i) {
            if (i < w) { gb += wg[i]; eb += we[i]; }
            run_gt += wg[i]; run_eq += we[i];
        }
        const int pos = gb + (eb < need ? eb : need);
        if ((gt || (eq && eb < need)) && pos >= 0 && pos < C) {
            cand_tok[f * C + pos] = v;
            cand_lp[f * C + pos] = zv - lse;
        }
    }
}

// ---- greedy -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const int* __restrict__ best, const float* __restrict__ best_lp,
                                                         const int* __restrict__ enc_len, int Tp, int blank, int* __restrict__ tokens,
                                                         int* __restrict__ lens, double* __restrict__ scores) {
    __shared__ int wc[4];
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int Tu = clampi(enc_len[u], 0, Tp);
    const int* b = best + (size_t)u * Tp;
    const u64 below = (1ull << lane) - 1ull;
    int run = 0;
    for (int base = 0; base < Tu; base += 256) {
        const int t = base + tid;
        const bool ok = t < Tu;
        const int c = ok ? b[t] : blank;
        const bool emit = ok && c != blank && (t == 0 || c != b[t - 1]);
        const u64 bm = __ballot(emit);
        __syncthreads();
        if (lane == 0) wc[w] = __popcll(bm);
        __syncthreads();
        int pos = run + __popcll(bm & below);
        for (int i = 0; i < 4; ++i) {
            if (i < w) pos += wc[i];
            run += wc[i];
        }
        if (emit && pos < Tp) tokens[(size_t)u * Tp + pos] = c;
    }
    if (tid == 0) {
        double s = 0.0;
        for (int t = 0; t < Tu; ++t) s += (double)best_lp[(size_t)u * Tp + t];
        scores[u] = s;
        lens[u] = run;
    }
}

// ---- prefix beam search -------------------------------------------------------------------------------------------------------------
struct CtcBeamDev {
    NgramTrie lm; int has_lm, lm_start;
    const int* cand_tok; const float* cand_lp; const float* blank_lp; const int* enc_len;
    int Tp, V, K, C, eos; float beta;
    int* tokens; int* lens; float* totals; int* nhyp;
    long long* hkey; int* hval; int *nd_parent, *nd_tok, *nd_len, *nd_slot; int NN, H;
};

__device__ __forceinline__ bool live(float x) { return x > CTC_LOGZERO; }            // (NaN is no mass)
__device__ __forceinline__ float zadd(float a, float b) {
    if (!live(a) || !live(b)) return CTC_LOGZERO;
    const float r = __fadd_rn(a, b);
    return live(r) ? r : CTC_LOGZERO;
}
__device__ __forceinline__ float lae(float a, float b) {
    if (!live(a)) return live(b) ? b : CTC_LOGZERO;
    if (!live(b)) return a;
    const float mx = fmaxf(a, b), mn = fminf(a, b);
    return __fadd_rn(mx, log1pf(expf(__fsub_rn(mn, mx))));
}

// the pre-scaled back-off score of token c (inside [0, V)) from n-gram node `node` (inside [0, M)), and the node it leads to: the descent
// of las_ngram_step, for one token
__device__ __forceinline__ float lm_gain(const NgramTrie& L, int node, int c, int& next) {
    float acc = 0.f;
    int q = node;
    for (int lvl = 0; lvl < L.order && q != 0; ++lvl) {
        int lo, hi;
        trie_range(L.child_off, L.E, q, lo, hi);
        const int k = trie_find(L.child_tok, lo, hi, c);
        if (k >= 0) {
            next = L.child_next[k];
            if (next < 0 || next >= L.M) next = 0;
            return __fadd_rn(acc, L.child_lp[k]);
        }
        acc = __fadd_rn(acc, L.bow[q]);
        q = ngram_backoff(L, q);
    }
    next = L.uni_next[c];
    if (next < 0 || next >= L.M) next = 0;
    return __fadd_rn(acc, L.uni_lp[c]);
}
__device__ __forceinline__ float gain(const CtcBeamDev& a, int node, int c, int& next) {
    next = 0;
    return a.has_lm ? __fadd_rn(lm_gain(a.lm, node, c, next), a.beta) : a.beta;
}

__device__ __forceinline__ unsigned hash_home(int parent, int tok, int H) {
    unsigned h = (unsigned)parent * 0x9E3779B1u ^ (unsigned)tok * 0x85EBCA6Bu;
    h ^= h >> 15;
    return h & (unsigned)(H - 1);
}
__device__ __forceinline__ long long hash_key(int parent, int tok) { return ((long long)parent << 32) | (long long)(unsigned)tok; }
__device__ __forceinline__ int hash_lookup(const long long* hkey, const int* hval, int H, int parent, int tok) {
    const long long key = hash_key(parent, tok);
    unsigned h = hash_home(parent, tok, H);
    for (int i = 0; i < H; ++i, h = (h + 1) & (unsigned)(H - 1)) {
        const long long k = hkey[h];
        if (k == key) return hval[h];
        if (k == -1) return -1;
    }
    return -1;
}

__global__ __launch_bounds__(BEAM_NT) void ctc_beam_kernel(CtcBeamDev a) {
    __shared__ float e_tot[BEAM_MAX_E];
    __shared__ int e_nid[BEAM_MAX_E];
    __shared__ float s_pb[CTC_MAX_K], s_pnb[CTC_MAX_K], n_pb[CTC_MAX_K], n_pnb[CTC_MAX_K], t_pb[CTC_MAX_K], t_pnb[CTC_MAX_K], sel_tot[CTC_MAX_K];
    __shared__ int s_node[CTC_MAX_K], s_last[CTC_MAX_K], s_lm[CTC_MAX_K], s_len[CTC_MAX_K];
    __shared__ int t_node[CTC_MAX_K], t_last[CTC_MAX_K], t_lm[CTC_MAX_K], t_len[CTC_MAX_K], t_par[CTC_MAX_K], sel[CTC_MAX_K];
    __shared__ int c_tok[CTC_MAX_C];
    __shared__ float c_lp[CTC_MAX_C];
    __shared__ u64 redu[BEAM_NT / 64];
    const int u = blockIdx.x, tid = threadIdx.x;
    const int K = a.K, C = a.C, V = a.V, Tp = a.Tp, NN = a.NN, H = a.H;
    long long* hkey = a.hkey + (size_t)u * H;
    int* hval = a.hval + (size_t)u * H;
    int* nd_parent = a.nd_parent + (size_t)u * NN;
    int* nd_tok = a.nd_tok + (size_t)u * NN;
    int* nd_len = a.nd_len + (size_t)u * NN;
    int* nd_slot = a.nd_slot + (size_t)u * NN;
    const int Tu = clampi(a.enc_len[u], 0, Tp);

    for (int i = tid; i < H; i += BEAM_NT) hkey[i] = -1;
    if (tid == 0) {
        nd_parent[0] = -1; nd_tok[0] = -1; nd_len[0] = 0; nd_slot[0] = 0;
        s_node[0] = 0; s_pb[0] = 0.f; s_pnb[0] = CTC_LOGZERO; s_last[0] = -1; s_len[0] = 0;
        s_lm[0] = (a.has_lm && a.lm_start >= 0 && a.lm_start < a.lm.M) ? a.lm_start : 0;
    }
    int nlive = 1, nnodes = 1;                                         // (uniform: every lane keeps its own copy)
    __syncthreads();

    for (int t = 0; t < Tu && nlive > 0; ++t) {
        const size_t f = (size_t)u * Tp + t;
        if (tid < C) { c_tok[tid] = a.cand_tok[f * C + tid]; c_lp[tid] = a.cand_lp[f * C + tid]; }
        const float yb = a.blank_lp[f];
        __syncthreads();

        // ---- stay: the slot's own prefix, with the mass its parent's extension brings
        if (tid < K) {
            float tot = CTC_LOGZERO;
            int nid = -1;
            if (tid < nlive) {
                const int j = tid, node = s_node[j], last = s_last[j];
                const float pb = s_pb[j], pnb = s_pnb[j];
                int rep = -1;
                if (last >= 0) {
                    int lo = 0, hi = C;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1, tk = c_tok[mid];
                        if (tk == last) { rep = mid; break; }
                        if (tk < last) lo = mid + 1; else hi = mid;
                    }
                }
                const float npb = zadd(yb, lae(pb, pnb));
                float npnb = CTC_LOGZERO;
                if (rep >= 0 && last < V) {
                    const float y = c_lp[rep];
                    npnb = lae(npnb, zadd(y, pnb));
                    const int par = nd_parent[node];
                    const int ps = (par >= 0 && par < NN) ? nd_slot[par] : -1;
                    if (ps >= 0 && ps < nlive && s_node[ps] == par && s_last[ps] != a.eos) {
                        const float base = (last == s_last[ps]) ? s_pb[ps] : lae(s_pb[ps], s_pnb[ps]);
                        int nx;
                        const float g = gain(a, s_lm[ps], last, nx);
                        npnb = lae(npnb, zadd(zadd(y, base), g));
                    }
                }
                n_pb[j] = npb; n_pnb[j] = npnb;
                tot = lae(npb, npnb);
                nid = node;
            }
            e_tot[tid] = tot;
            e_nid[tid] = nid;
        }
        // ---- extend
        for (int e = tid; e < K * C; e += BEAM_NT) {
            const int j = e / C, i = e - j * C;
            float val = CTC_LOGZERO;
            int nid = -1;
            if (j < nlive && s_last[j] != a.eos) {
                const int c = c_tok[i];
                if (c >= 0 && c < V) {
                    nid = hash_lookup(hkey, hval, H, s_node[j], c);
                    if (nid < 0 || nid >= NN) nid = -1;
                    if (nid < 0 || nd_slot[nid] < 0) {                  // (a child in the beam gathered this mass itself)
                        const float base = (c == s_last[j]) ? s_pb[j] : lae(s_pb[j], s_pnb[j]);
                        int nx;
                        const float g = gain(a, s_lm[j], c, nx);
                        val = zadd(zadd(c_lp[i], base), g);
                    }
                }
            }
            e_tot[K + e] = val;
            e_nid[K + e] = nid;
        }
        __syncthreads();

        // ---- prune: up to K rounds of arg-max over the entries, key (total, lower index)
        const int E = K + K * C;
        int nnew = 0;
        for (; nnew < K; ++nnew) {
            u64 bk = 0;
            for (int e = tid; e < E; e += BEAM_NT) {
                const float tv = e_tot[e];
                if (live(tv)) {
                    const u64 k = ((u64)okey(tv) << 32) | (0xffffffffu - (unsigned)e);
                    bk = k > bk ? k : bk;
                }
            }
            bk = block_u64max<BEAM_NT>(bk, redu);
            if (bk == 0) break;
            if (tid == 0) {
                const int idx = (int)(0xffffffffu - (unsigned)bk);
                sel[nnew] = idx;
                sel_tot[nnew] = e_tot[idx];
                e_tot[idx] = CTC_LOGZERO;
            }
            __syncthreads();
        }
        __syncthreads();

        // ---- the new beam
        if (tid < nnew) {
            const int idx = sel[tid];
            if (idx < K) {
                t_node[tid] = s_node[idx]; t_pb[tid] = n_pb[idx]; t_pnb[tid] = n_pnb[idx]; t_last[tid] = s_last[idx];
                t_lm[tid] = s_lm[idx]; t_len[tid] = s_len[idx]; t_par[tid] = -1;
            } else {
                const int e = idx - K, j = e / C, i = e - j * C, c = c_tok[i];
                int nx;
                gain(a, s_lm[j], c, nx);
                t_node[tid] = e_nid[idx]; t_pb[tid] = CTC_LOGZERO; t_pnb[tid] = sel_tot[tid]; t_last[tid] = c;
                t_lm[tid] = nx; t_len[tid] = s_len[j] + 1; t_par[tid] = s_node[j];
            }
        }
        if (tid < nlive) nd_slot[s_node[tid]] = -1;
        __syncthreads();
        int created = 0;
        for (int r = 0; r < nnew; ++r) created += t_node[r] < 0;          // (uniform: every lane counts the same LDS words)
        __syncthreads();
        if (tid == 0) {
            int id = nnodes;
            for (int r = 0; r < nnew; ++r) {
                if (t_node[r] >= 0) continue;
                const int nid = id < NN ? id : NN - 1;                    // (K Tp + 1 nodes always suffice: at most K per frame)
                ++id;
                nd_parent[nid] = t_par[r]; nd_tok[nid] = t_last[r]; nd_len[nid] = t_len[r];
                const long long key = hash_key(t_par[r], t_last[r]);
                unsigned h = hash_home(t_par[r], t_last[r], H);
                for (int i = 0; i < H; ++i, h = (h + 1) & (unsigned)(H - 1))
                    if (hkey[h] == -1) { hval[h] = nid; hkey[h] = key; break; }
                t_node[r] = nid;
            }
        }
        nnodes += created;
        __syncthreads();
        if (tid < nnew) {
            s_node[tid] = t_node[tid]; s_pb[tid] = t_pb[tid]; s_pnb[tid] = t_pnb[tid]; s_last[tid] = t_last[tid];
            s_lm[tid] = t_lm[tid]; s_len[tid] = t_len[tid];
            nd_slot[t_node[tid]] = tid;
        }
        nlive = nnew;
        __syncthreads();
    }

    // ---- the ranked hypotheses
    if (tid == 0) a.nhyp[u] = nlive;
    if (tid < nlive) {
        const size_t row = (size_t)u * K + tid;
        a.totals[row] = lae(s_pb[tid], s_pnb[tid]);
        const int len = clampi(s_len[tid], 0, Tp);
        a.lens[row] = len;
        int node = s_node[tid];
        for (int pos = len - 1; pos >= 0 && node > 0 && node < NN; --pos) {
            a.tokens[row * Tp + pos] = nd_tok[node];
            node = nd_parent[node];
        }
    }
}

void beam_geometry(int Tp, int K, long long& NN, long long& H) {
    NN = (long long)K * Tp + 1;
    H = 2;
    while (H < 2 * NN) H <<= 1;
}

}  // namespace

extern "C" int las_ctc_frame_topk(const float* logits, const int* enc_len, int n, int Tp, int Vc, int C, int* cand_tok, float* cand_lp,
                                  float* blank_lp, int* best, float* best_lp, void* stream) {
    LAS_ARG(logits && enc_len && blank_lp && best && best_lp && (C == 0 || (cand_tok && cand_lp)), "las_ctc_frame_topk: null pointer");
    LAS_ARG(n > 0 && Tp > 0 && Vc >= 2 && (long long)n * Tp <= 0x7fffffffLL, "las_ctc_frame_topk: bad dims");
    LAS_ARG(C >= 0 && C <= CTC_MAX_C && C <= Vc - 1, "las_ctc_frame_topk: 0 <= C <= min(%d, V) (got %d, V = %d)", CTC_MAX_C, C, Vc - 1);
    hipLaunchKernelGGL(ctc_frame_topk_kernel, dim3(n * Tp), dim3(TOPK_NT), 0, (hipStream_t)stream, logits, enc_len, Tp, Vc, C, cand_tok,
                       cand_lp, blank_lp, best, best_lp);
    LAS_LAUNCHED();
    return 0;
}

extern "C" int las_ctc_greedy(const int* best, const float* best_lp, const int* enc_len, int n, int Tp, int blank, int* tokens, int* lens,
                              double* scores, void* stream) {
    LAS_ARG(best && best_lp && enc_len && tokens && lens && scores, "las_ctc_greedy: null pointer");
    LAS_ARG(n > 0 && Tp > 0 && (long long)n * Tp <= 0x7fffffffLL, "las_ctc_greedy: bad dims");
    hipLaunchKernelGGL(ctc_greedy_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, best, best_lp, enc_len, Tp, blank, tokens, lens,
                       scores);
    LAS_LAUNCHED();
    return 0;
}

extern "C" size_t las_ctc_beam_workspace_bytes(int n, int Tp, int K, int C) {
    (void)C;
    if (n <= 0 || Tp <= 0 || K <= 0) return 0;
    long long NN, H;
    beam_geometry(Tp, K, NN, H);
    return (size_t)n * ((size_t)H * (sizeof(long long) + sizeof(int)) + (size_t)NN * 4 * sizeof(int));
}

extern "C" int las_ctc_beam_search(const int* cand_tok, const float* cand_lp, const float* blank_lp, const int* enc_len, int n, int Tp,
                                   int V, int K, int C, int eos, float len_bonus, const int* child_off, const int* child_tok,
                                   const float* child_lp, const int* child_next, const float* bow, const int* bo, const float* uni_lp,
                                   const int* uni_next, int nnodes, int nchild, int order, int lm_start, int* tokens, int* lens,
                                   float* totals, int* nhyp, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(cand_tok && cand_lp && blank_lp && enc_len && tokens && lens && totals && nhyp && ws, "las_ctc_beam_search: null pointer");
    LAS_ARG(n > 0 && Tp > 0 && V >= 1 && (long long)n * Tp * (K > 0 ? K : 1) <= 0x7fffffffLL, "las_ctc_beam_search: bad dims");
    LAS_ARG(K >= 1 && K <= CTC_MAX_K, "las_ctc_beam_search: 1 <= K <= %d (got %d)", CTC_MAX_K, K);
    LAS_ARG(C >= 1 && C <= CTC_MAX_C && C <= V, "las_ctc_beam_search: 1 <= C <= min(%d, V) (got %d, V = %d)", CTC_MAX_C, C, V);
    LAS_ARG(isfinite(len_bonus), "las_ctc_beam_search: the length bonus is not finite");
    const bool has_lm = nnodes > 0;
    if (has_lm) {
        LAS_ARG(child_off && bow && bo && uni_lp && uni_next, "las_ctc_beam_search: n-gram tables: null pointer");
        LAS_ARG(nchild >= 0 && (nchild == 0 || (child_tok && child_lp && child_next)), "las_ctc_beam_search: %d children but no child tables", nchild);
        LAS_ARG(V > 1 && V <= TRIE_MAX_V, "las_ctc_beam_search: with an n-gram 1 < V <= %d (got %d)", TRIE_MAX_V, V);
        LAS_ARG(nnodes <= TRIE_MAX_NODES, "las_ctc_beam_search: 1 <= nodes <= %d (got %d)", TRIE_MAX_NODES, nnodes);
        LAS_ARG(order >= 1 && order <= NGRAM_MAX_ORDER, "las_ctc_beam_search: 1 <= order <= %d (got %d)", NGRAM_MAX_ORDER, order);
    } else {
        LAS_ARG(nnodes == 0, "las_ctc_beam_search: 1 <= nodes <= %d (got %d)", TRIE_MAX_NODES, nnodes);
    }
    const size_t need = las_ctc_beam_workspace_bytes(n, Tp, K, C);
    LAS_ARG(ws_bytes >= need, "las_ctc_beam_search: workspace of %zu bytes, %zu needed", ws_bytes, need);
    long long NN, H;
    beam_geometry(Tp, K, NN, H);
    CtcBeamDev a;
    a.lm.child_off = child_off; a.lm.child_tok = child_tok; a.lm.child_lp = child_lp; a.lm.child_next = child_next; a.lm.bow = bow;
    a.lm.bo = bo; a.lm.uni_lp = uni_lp; a.lm.uni_next = uni_next; a.lm.M = nnodes; a.lm.E = nchild; a.lm.order = order;
    a.has_lm = has_lm ? 1 : 0; a.lm_start = lm_start;
    a.cand_tok = cand_tok; a.cand_lp = cand_lp; a.blank_lp = blank_lp; a.enc_len = enc_len;
    a.Tp = Tp; a.V = V; a.K = K; a.C = C; a.eos = eos; a.beta = len_bonus;
    a.tokens = tokens; a.lens = lens; a.totals = totals; a.nhyp = nhyp;
    char* p = (char*)ws;
    a.hkey = (long long*)p; p += (size_t)n * H * sizeof(long long);
    a.hval = (int*)p; p += (size_t)n * H * sizeof(int);
    a.nd_parent = (int*)p; p += (size_t)n * NN * sizeof(int);
    a.nd_tok = (int*)p; p += (size_t)n * NN * sizeof(int);
    a.nd_len = (int*)p; p += (size_t)n * NN * sizeof(int);
    a.nd_slot = (int*)p;
    a.NN = (int)NN; a.H = (int)H;
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(n), dim3(BEAM_NT), 0, (hipStream_t)stream, a);
    LAS_LAUNCHED();
    return 0;
}
