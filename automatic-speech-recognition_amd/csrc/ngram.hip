// ngram.hip -- K10f: shallow fusion of a back-off n-gram language model into the beam search.
//
// The model (order n <= 6 over token ids [0, V)) is compiled on the host (las/ngram.py, NgramLM) into a trie, node 0 = root = the empty
// context; every stored n-gram of order 1 .. n - 1 is a node, highest-order n-grams are entries only.  All values arrive PRE-SCALED,
// fl32(w ln10 log10 x), rounded once on the host:
//   child_off [M + 1], child_tok [E] (ascending inside a node), child_lp [E], child_next [E]   one child list per node; the root's is
//                                                                                             empty (the unigrams are dense)
//   bow [M], bo [M]        back-off weight of a node and the node of its longest proper suffix that is a node (the root's is the root)
//   uni_lp [V], uni_next [V]   the unigrams and the node each leads to
// Transition on token c from node p: descend p, bo(p), ... to the first node that has c as a child and take that entry's next; the root
// always has c (uni_next).  A token outside [0, V) goes to the root.  At most `order` levels are descended, then the root is taken: a
// cyclic bo table cannot spin.
//
// las_ngram_step, once per search step, behind the step's logits (and the RNN LM's) and in front of las_ctc_prefix_step, las_bias_step
// and las_beam_loop_step.  One workgroup of 256 lanes per hypothesis row, live rows only (search_rows.h):
//   advance   the gathered parent's node (state_in[row][0], a float that holds an integer < 2^24; the root at step 0 or when the value
//             is not a node) is advanced by the entering token into state_out[row][0]; every lane walks the same binary searches.
//   score     over the chain s0 = s, s1 = bo(s0), ..., root with acc0 = 0: every child v of s_i that no deeper level held gets
//             g = fl32(acc_i + child_lp) and scores[row][v] = fl32(scores[row][v] + g) and is marked in a byte table in LDS (a barrier
//             between levels: a token stored at two levels takes the deeper one); acc_{i+1} = fl32(acc_i + bow[s_i]); then one pass over V
//             gives every unmarked token fl32(acc + uni_lp[v]) the same way.  Two fp32 adds per token, nothing contracted.  A row at the
//             root (a unigram model, an unseen context) makes the dense pass alone and needs no table.  -inf + g = -inf.
//
// Limits (checked on the host, here and in las/ngram.py): V <= 16384 (the LDS mark table), M <= 2^22 nodes (exact in the fp32 state
// word), order <= 6.  Bounds: a node value outside [0, M) or NaN is the root; child lists are clamped to [0, E), child tokens outside
// [0, V) are skipped, a next or bo outside [0, M) is the root (the host refuses to build such tables) -- no input makes the kernel
// index outside its buffers.  No atomics and no reductions: two runs give the same bits, and numpy float32 gives them too
// (tests/ngram_ref.py).
#include "las_common.h"
#include "ngram_trie.h"
#include "search_rows.h"
#include <math.h>

namespace {

struct NgramDev : SearchRows, NgramTrie {                              // (the rows and search_row_live / search_parent_node: search_rows.h;
    float* scores; int V;                                              //  the tables and trie_range / trie_find / ngram_backoff: ngram_trie.h)
};

__global__ __launch_bounds__(256) void ngram_step_kernel(NgramDev a) {
    __shared__ unsigned char mark[TRIE_MAX_V];
    const int row = blockIdx.x, tid = threadIdx.x;
    int t_step, u;
    if (!search_row_live(a, row, t_step, u)) return;
    const int V = a.V, M = a.M;

    // ---- advance (uniform over the workgroup)
    const int p = search_parent_node(a, row, t_step, M);
    const int c = a.token[row];
    int s = 0;
    if (c >= 0 && c < V) {
        int k = -1, q = p;
        for (int lvl = 0; lvl < a.order && q != 0 && k < 0; ++lvl) {
            int lo, hi;
            trie_range(a.child_off, a.E, q, lo, hi);
            k = trie_find(a.child_tok, lo, hi, c);
            q = ngram_backoff(a, q);
        }
        s = k >= 0 ? a.child_next[k] : a.uni_next[c];
        if (s < 0 || s >= M) s = 0;
    }
    if (tid == 0) a.st_out[(size_t)row * a.width] = (float)s;

    // ---- score, in place
    float* sc = a.scores + (size_t)row * V;
    float acc = 0.f;
    if (s == 0) {                                                       // the dense pass alone
        for (int v = tid; v < V; v += 256) sc[v] = __fadd_rn(sc[v], __fadd_rn(acc, a.uni_lp[v]));
        return;
    }
    for (int v = tid; v < V; v += 256) mark[v] = 0;
    __syncthreads();
    int q = s;
    for (int lvl = 0; lvl < a.order && q != 0; ++lvl) {                // (q is the same in every lane: so is the number of barriers)
        int lo, hi;
        trie_range(a.child_off, a.E, q, lo, hi);
        for (int k = lo + tid; k < hi; k += 256) {
            const int v = a.child_tok[k];
            if (v >= 0 && v < V && !mark[v]) {                          // (a node's child tokens are distinct: one lane per byte)
                sc[v] = __fadd_rn(sc[v], __fadd_rn(acc, a.child_lp[k]));
                mark[v] = 1;
            }
        }
        acc = __fadd_rn(acc, a.bow[q]);
        q = ngram_backoff(a, q);
        __syncthreads();
    }
    for (int v = tid; v < V; v += 256)
        if (!mark[v]) sc[v] = __fadd_rn(sc[v], __fadd_rn(acc, a.uni_lp[v]));
}

}  // namespace

extern "C" int las_ngram_step(const int* child_off, const int* child_tok, const float* child_lp, const int* child_next,
                              const float* bow, const int* bo, const float* uni_lp, const int* uni_next, int nnodes, int nchild,
                              int order, float* scores, int nutt, int beam, int V, const float* state_in, float* state_out,
                              int state_width, const int* token, const int* step, const int* nlive, const int* done,
                              const int* dec_step, int Umax, void* stream) {
    NgramDev a;
    if (search_rows_args(a, "las_ngram_step", 1, nutt, beam, state_in, state_out, state_width,
                         token, step, nlive, done, dec_step, Umax)) return -1;
    LAS_ARG(child_off && bow && bo && uni_lp && uni_next && scores && token, "las_ngram_step: null pointer");
    LAS_ARG(nchild >= 0 && (nchild == 0 || (child_tok && child_lp && child_next)), "las_ngram_step: %d children but no child tables", nchild);
    LAS_ARG(V > 1 && V <= TRIE_MAX_V, "las_ngram_step: 1 < V <= %d (got %d)", TRIE_MAX_V, V);
    LAS_ARG(nnodes >= 1 && nnodes <= TRIE_MAX_NODES, "las_ngram_step: 1 <= nodes <= %d (got %d)", TRIE_MAX_NODES, nnodes);
    LAS_ARG(order >= 1 && order <= NGRAM_MAX_ORDER, "las_ngram_step: 1 <= order <= %d (got %d)", NGRAM_MAX_ORDER, order);
    a.child_off = child_off; a.child_tok = child_tok; a.child_lp = child_lp; a.child_next = child_next; a.bow = bow; a.bo = bo;
    a.uni_lp = uni_lp; a.uni_next = uni_next; a.M = nnodes; a.E = nchild; a.order = order; a.scores = scores; a.V = V;
    hipLaunchKernelGGL(ngram_step_kernel, dim3(nutt * beam), dim3(256), 0, (hipStream_t)stream, a);
    LAS_LAUNCHED();
    return 0;
}
