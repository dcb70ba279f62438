// ngram_trie.h -- the device side of the host-built token tries: the one bounded walk over the child lists that las/bias.py's and
// las/ngram.py's tables share -- child_off [M + 1], child_tok [E] (ascending inside a node) -- for bias.hip, ngram.hip and ctc_search.hip,
// and NgramTrie, the n-gram model's tables (ngram.hip's las_ngram_step and ctc_search.hip's las_ctc_beam_search).  Whatever the tables
// hold, nothing here indexes outside them as long as the node handed in is inside [0, M).
#pragma once
#include "las_common.h"

constexpr int TRIE_MAX_V = 16384;                     // a byte per token in LDS (the scorers' class / mark tables)
constexpr int TRIE_MAX_NODES = 1 << 22;               // exact in the fp32 state word
constexpr int NGRAM_MAX_ORDER = 6;

struct NgramTrie {
    const int *child_off, *child_tok, *child_next, *bo, *uni_next; const float *child_lp, *bow, *uni_lp; int M, E, order;
};

// the child list of node s as [lo, hi), inside [0, E) whatever the table holds
__device__ __forceinline__ void trie_range(const int* child_off, int E, int s, int& lo, int& hi) {
    lo = clampi(child_off[s], 0, E);
    hi = clampi(child_off[s + 1], lo, E);
}
// position of token v in the sorted list [lo, hi), or -1
__device__ __forceinline__ int trie_find(const int* child_tok, int lo, int hi, int v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int tk = child_tok[mid];
        if (tk == v) return mid;
        if (tk < v) lo = mid + 1; else hi = mid;
    }
    return -1;
}
// bo[s], the root where the table holds no node
__device__ __forceinline__ int ngram_backoff(const NgramTrie& a, int s) {
    const int q = a.bo[s];
    return (q < 0 || q >= a.M) ? 0 : q;
}
