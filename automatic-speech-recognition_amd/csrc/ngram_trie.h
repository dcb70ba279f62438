// ngram_trie.h -- the device side of las/ngram.py's trie tables, shared by ngram.hip (las_ngram_step) and ctc_search.hip
// (las_ctc_beam_search): the tables and the three bounded accessors.  Whatever the tables hold, nothing here indexes outside them as
// long as the node handed in is inside [0, M).
#pragma once
#include "las_common.h"

constexpr int NGRAM_MAX_V = 16384;
constexpr int NGRAM_MAX_NODES = 1 << 22;
constexpr int NGRAM_MAX_ORDER = 6;

struct NgramTrie {
    const int *child_off, *child_tok, *child_next, *bo, *uni_next; const float *child_lp, *bow, *uni_lp; int M, E, order;
};

// the child list of node s as [lo, hi), inside [0, E) whatever the table holds
__device__ __forceinline__ void ngram_range(const NgramTrie& a, int s, int& lo, int& hi) {
    lo = a.child_off[s]; hi = a.child_off[s + 1];
    lo = lo < 0 ? 0 : (lo > a.E ? a.E : lo);
    hi = hi < lo ? lo : (hi > a.E ? a.E : hi);
}
// position of token v in the sorted list [lo, hi), or -1
__device__ __forceinline__ int ngram_find(const NgramTrie& a, int lo, int hi, int v) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const int tk = a.child_tok[mid];
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
