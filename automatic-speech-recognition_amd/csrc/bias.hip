// bias.hip -- K10e: contextual biasing (hotword boosting) of the beam search by shallow fusion.
//
// A context is a set of phrases (token-id sequences) compiled on the host (las/bias.py, ContextGraph) into a token trie, node 0 = root:
//   child_off [M + 1], child_tok [E] (ascending inside a node), child_next [E]   one child list per node; child_next has rule 4 applied
//   gdef [M] = -pend(s), groot [M] = fl32(beta - pend(s))                        pend(s) = fl32(beta) * fl32(depth(s) - base(s))
// The transition on token v from node s (there are NO fail links: an occurrence that starts inside a failed partial match, other than
// at the failing token, is not seen):
//   1. v is a child of s:                            t = child(s, v),    gain = beta
//   2. else s != root and v is a child of the root:  t = child(root, v), gain = groot[s]   (the broken match is paid back, a new one starts)
//   3. else:                                         t = root,           gain = gdef[s]    (nothing from the root)
//   4. a t that ends a phrase and has no children is the root (already folded into child_next); the bonus is kept.
//
// las_bias_step, once per search step, behind the step's logits (and behind las_ctc_prefix_step when that runs) and in front of
// las_beam_loop_step.  One workgroup of 256 lanes per hypothesis row, live rows only (search_rows.h):
//   advance   the gathered parent's node (state_in[row][0], a float that holds an integer < 2^24; the root at step 0 or when the value
//             is not a node) is advanced by the entering token into state_out[row][0]; every lane walks the same two binary searches.
//   score     scores[row][v] receives exactly ONE fp32 add of its gain for the advanced node s, and none where the gain is 0:
//               s = root:            the root's children get beta -- the row's other V - fan-out values are neither read nor written
//                                    (almost every row of a real search: a few KB per step instead of 2 x 4 V bytes per row);
//               pend(s) = 0, s != 0: (a phrase end with children) its children get beta, the root's other children groot[s] = beta;
//               pend(s) != 0:        one pass over V.  Every token's class (2: child of s, 1: child of the root, 0: neither) comes from
//                                    a byte table in LDS, zeroed, marked with the root's list, then with s's list (barriers in between:
//                                    a token in both lists is a child of s); the pass adds beta / groot[s] / gdef[s] accordingly.
//             -inf + gain = -inf: a token outside the CTC bank stays outside.
// The ranking of las_beam_loop_step (K10) relies on the per-hypothesis top-64 cut not binding while beam < topn; with the biased scores
// that holds when the cut is read as a cut on the RANKED, biased score (it is the biased score the pruning sees).
//
// Limits (checked on the host, here and in las/bias.py): V <= 16384 (the LDS class table; hence root fan-out <= 16384), M <= 2^22 nodes
// (exact in the fp32 state word).  Bounds: a node value outside [0, M) or not finite is the root; an entering token outside [0, V) is
// no child of anything (rule 3); child lists are clamped to [0, E), child tokens outside [0, V) are skipped and a child_next outside
// [0, M) is the root (the host refuses to build such tables) -- no input makes the kernel index outside its buffers.
// No atomics and no reductions: two runs give the same bits, and numpy float32 gives them too (tests/bias_ref.py).
#include "las_common.h"
#include "ngram_trie.h"
#include "search_rows.h"
#include <math.h>

namespace {

struct BiasDev : SearchRows {                                          // (the rows and search_row_live / search_parent_node: search_rows.h;
    const int *child_off, *child_tok, *child_next; const float *gdef, *groot; float beta; int M, E;        // the walk over
    float* scores; int V;                                              //  the child lists, trie_range / trie_find: ngram_trie.h)
};

__global__ __launch_bounds__(256) void bias_step_kernel(BiasDev a) {
    __shared__ unsigned char cls[TRIE_MAX_V];
    const int row = blockIdx.x, tid = threadIdx.x;
    int t_step, u;
    if (!search_row_live(a, row, t_step, u)) return;
    const int V = a.V, M = a.M;
    int r_lo, r_hi;
    trie_range(a.child_off, a.E, 0, r_lo, r_hi);

    // ---- advance (uniform over the workgroup)
    const int p = search_parent_node(a, row, t_step, M);
    const int c = a.token[row];
    int s = 0;
    if (c >= 0 && c < V) {
        int lo, hi;
        trie_range(a.child_off, a.E, p, lo, hi);
        int k = trie_find(a.child_tok, lo, hi, c);
        if (k < 0 && p != 0) k = trie_find(a.child_tok, r_lo, r_hi, c);
        if (k >= 0) s = a.child_next[k];
        if (s < 0 || s >= M) s = 0;
    }
    if (tid == 0) a.st_out[(size_t)row * a.width] = (float)s;

    // ---- score, in place
    float* sc = a.scores + (size_t)row * V;
    const float beta = a.beta;
    if (s == 0) {
        for (int k = r_lo + tid; k < r_hi; k += 256) {
            const int v = a.child_tok[k];
            if (v >= 0 && v < V) sc[v] = __fadd_rn(sc[v], beta);
        }
        return;
    }
    int s_lo, s_hi;
    trie_range(a.child_off, a.E, s, s_lo, s_hi);
    const float gd = a.gdef[s], gr = a.groot[s];
    if (gd == 0.f) {                                                    // a phrase end with children: nothing to pay back, no pass over V
        for (int k = s_lo + tid; k < s_hi; k += 256) {
            const int v = a.child_tok[k];
            if (v >= 0 && v < V) sc[v] = __fadd_rn(sc[v], beta);
        }
        if (gr != 0.f)
            for (int k = r_lo + tid; k < r_hi; k += 256) {
                const int v = a.child_tok[k];
                if (v >= 0 && v < V && trie_find(a.child_tok, s_lo, s_hi, v) < 0) sc[v] = __fadd_rn(sc[v], gr);
            }
        return;
    }
    for (int v = tid; v < V; v += 256) cls[v] = 0;
    __syncthreads();
    for (int k = r_lo + tid; k < r_hi; k += 256) {
        const int v = a.child_tok[k];
        if (v >= 0 && v < V) cls[v] = 1;
    }
    __syncthreads();
    for (int k = s_lo + tid; k < s_hi; k += 256) {
        const int v = a.child_tok[k];
        if (v >= 0 && v < V) cls[v] = 2;
    }
    __syncthreads();
    for (int v = tid; v < V; v += 256) {
        const int cl = cls[v];
        const float g = cl == 2 ? beta : (cl == 1 ? gr : gd);
        if (g != 0.f) sc[v] = __fadd_rn(sc[v], g);
    }
}

}  // namespace

extern "C" int las_bias_step(const int* child_off, const int* child_tok, const int* child_next, const float* gdef, const float* groot,
                             float beta, int nnodes, int nchild, float* scores, int nutt, int beam, int V, const float* state_in,
                             float* state_out, int state_width, const int* token, const int* step, const int* nlive, const int* done,
                             const int* dec_step, int Umax, void* stream) {
    BiasDev a;
    if (search_rows_args(a, "las_bias_step", 1, nutt, beam, state_in, state_out, state_width,
                         token, step, nlive, done, dec_step, Umax)) return -1;
    LAS_ARG(child_off && gdef && groot && scores && token, "las_bias_step: null pointer");
    LAS_ARG(nchild >= 0 && (nchild == 0 || (child_tok && child_next)), "las_bias_step: %d children but no child tables", nchild);
    LAS_ARG(V > 1 && V <= TRIE_MAX_V, "las_bias_step: 1 < V <= %d (got %d)", TRIE_MAX_V, V);
    LAS_ARG(nnodes >= 1 && nnodes <= TRIE_MAX_NODES, "las_bias_step: 1 <= nodes <= %d (got %d)", TRIE_MAX_NODES, nnodes);
    LAS_ARG(beta > 0.f && beta <= 3.0e38f, "las_bias_step: the weight must be positive and finite (got %g)", (double)beta);
    a.child_off = child_off; a.child_tok = child_tok; a.child_next = child_next; a.M = nnodes; a.E = nchild;
    a.gdef = gdef; a.groot = groot; a.beta = beta; a.scores = scores; a.V = V;
    hipLaunchKernelGGL(bias_step_kernel, dim3(nutt * beam), dim3(256), 0, (hipStream_t)stream, a);
    LAS_LAUNCHED();
    return 0;
}
