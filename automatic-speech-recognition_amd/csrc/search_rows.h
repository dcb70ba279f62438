// search_rows.h -- what every per-step scorer of the beam search shares (las_ngram_step, las_ctc_prefix_step, las_bias_step,
// las_coverage_step; a new scorer starts from here): the rows part of its kernel argument, the liveness rule, the parent-node read of
// the trie scorers and the host checks of the arguments that las/beam_step.py's Scorer hands to every entry.
//
// THE CONTRACT with beam_loop_kernel (beam.hip).  A scorer runs once per search step in front of the pruning, one workgroup per
// hypothesis row = (utterance u, slot j), and reads the step counter, the utterance's done word and its live count on the device: the
// launch is the same every step and is captured into the search's HIP graph.  The pruning of step t ranks the candidates of exactly
// these rows, and a scorer writes a row (its scores, its state_out row) exactly when the pruning will rank it:
//   t < Umax                         the search is still running;
//   !done[u] && t < dec_step[u]      the utterance is: the pruning ignores the rows of a finished one;
//   j < (t == 0 ? 1 : nlive[u])      the slot holds a hypothesis: at step 0 only [SOS] in slot 0, whatever nlive holds.
// A row that is not live is neither read nor written.  state_in is the parents' state gathered into row order by the pruning of the
// step before (at step 0 it holds nothing), state_out the rows' own; both are [nutt beam, width] fp32 and must differ.
#pragma once
#include "las_common.h"

// First in the kernel argument.  The first branch reads step (first 64-byte line of the argument) and Umax (second line), so both
// lines are requested at entry; with every liveness word in the first line the rest of the argument became a second, dependent miss
// behind the liveness test (measured: + 1.5 us on las_ctc_prefix_step's 73 us at 256 rows, tools/bench_ctc_decode.py).
struct SearchRows {
    const float* st_in; float* st_out;
    const int *token, *step, *nlive, *done, *dec_step;
    int nutt, beam, width, Umax;
};

// true where row is live, with the step and the row's utterance.  Called at the top of the kernel with row = blockIdx.x: the result is
// the workgroup's, which returns as a whole before any barrier.
__device__ __forceinline__ bool search_row_live(const SearchRows& a, int row, int& t_step, int& u) {
    t_step = __hip_atomic_load(a.step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t_step >= a.Umax) return false;
    u = row / a.beam;
    const int j = row - u * a.beam;
    if (a.done[u] || t_step >= a.dec_step[u]) return false;
    return j < (t_step == 0 ? 1 : a.nlive[u]);
}

// the gathered parent's trie node, state_in[row][0] (a float that holds an integer < 2^24): the root at step 0, for NaN and for values
// outside [0, M)
__device__ __forceinline__ int search_parent_node(const SearchRows& a, int row, int t_step, int M) {
    if (t_step == 0) return 0;
    const float f = a.st_in[(size_t)row * a.width];
    return (f >= 0.f && f < (float)M) ? (int)f : 0;                    // (NaN fails both compares)
}

// host: the checks on the arguments every entry is handed, then the rows part of its kernel argument.  `entry` prefixes the message;
// min_width: the floats of the entry's state row.  token is not checked: an entry that reads it checks it with its own pointers.
inline int search_rows_args(SearchRows& r, const char* entry, int min_width, int nutt, int beam, const float* state_in, float* state_out,
                            int state_width, const int* token, const int* step, const int* nlive, const int* done, const int* dec_step,
                            int Umax) {
    LAS_ARG(state_in && state_out && step && nlive && done && dec_step, "%s: null pointer", entry);
    LAS_ARG(nutt > 0 && beam > 0 && Umax > 0 && (long long)nutt * beam <= 0x7fffffffLL, "%s: bad dims", entry);
    LAS_ARG(state_width >= min_width, "%s: state_width %d < %d", entry, state_width, min_width);
    LAS_ARG(state_in != state_out, "%s: state_in and state_out must differ", entry);
    r.st_in = state_in; r.st_out = state_out; r.token = token; r.step = step; r.nlive = nlive; r.done = done; r.dec_step = dec_step;
    r.nutt = nutt; r.beam = beam; r.width = state_width; r.Umax = Umax;
    return 0;
}
