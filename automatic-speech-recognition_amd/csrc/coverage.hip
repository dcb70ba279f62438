// coverage.hip -- K10i: attention coverage of the beam search's hypotheses: scored, reported and rescored.
//
// For a hypothesis with alignments alpha_1 .. alpha_t over its utterance's T'_u encoder frames (enc_len, clamped to [0, Tp]):
//   cum_t[j]  = fl32(cum_{t-1}[j] + alpha_t[j]), cum_0 = 0       one fp32 add per step and frame, in step order, for every j < Tp
//   covered_t = #{ j < T'_u : cum_t[j] > tau },  over_t = #{ j < T'_u : cum_t[j] > kappa }      (a NaN never counts)
//   dc = covered_t - covered_{t-1},  do = over_t - over_{t-1}     (the parent's counts are the fp32 words of its state row)
//   g  = fl32( fl32(w_c dc) - fl32(w_o do) ),  score_row = fl32(score_row + g)     (no score write when w_c = w_o = 0)
// Rounding: every operation above is an explicit round-to-nearest intrinsic (__fadd_rn, __fsub_rn, __fmul_rn), which the compiler
// does not contract into an fma; the file needs no -ffp-contract switch.  numpy float32 gives the same bits (tests/coverage_ref.py).
//
// las_coverage_step, once per search step, behind the Speller step (which writes the step's alignments) and in front of
// las_beam_loop_step: the gain does not depend on the candidate token, so it goes to the PARENT's running sum `score`, which the
// pruning adds every candidate's logit to -- nothing [rows, V] is touched and the short form of the step stays on.  One workgroup of
// 256 lanes per hypothesis row, live rows only (search_rows.h).  State row of `width`
// >= Tp + 2 floats: cum[0, Tp), covered, over (fp32 values, exact below 2^24), zeros up to width.  16-byte loads and stores of the
// state rows where width % 4 == 0 and the buffers are 16-byte aligned, of the alignments where Tp % 4 == 0 too.  Counts: one ballot
// and popcount per wave and pass, the four waves' sums added in wave order by one lane through LDS -- integers, no atomics: two runs
// give the same bits.  That lane writes the counts, the optional per-step record `hist` and the score.
//
// las_coverage_rows: the same counts for FINISHED alignments alphas [U, R, Tp] (what the teacher-forced las_speller_fwd writes):
// steps[r] (clamped to [0, U]) additions per frame in step order through the same device functions, counts int32 [R, 2].
//
// Bounds: enc_len is clamped to [0, Tp] and steps to [0, U]; every index is < Tp, < width or < the row count by construction -- no
// input makes a kernel index outside its buffers.
#include "las_common.h"
#include "search_rows.h"
#include <math.h>

namespace {

// ---- the accumulate-and-count functions shared by both kernels
__device__ __forceinline__ float cov_add(float cum, float alpha) { return __fadd_rn(cum, alpha); }

// adds the wave's number of lanes with (inside && cum > tau) / (inside && cum > kappa) to nc / no; EVERY lane of the wave calls it
__device__ __forceinline__ void cov_count(float cum, bool inside, float tau, float kappa, int& nc, int& no) {
    nc += __popcll(__builtin_amdgcn_ballot_w64(inside && cum > tau));         // (NaN > x is false)
    no += __popcll(__builtin_amdgcn_ballot_w64(inside && cum > kappa));
}

// the four waves' counts, added in wave order; the result is valid in thread 0 only.  red: int [4][2] in LDS
__device__ __forceinline__ void cov_block_sum(int (*red)[2], int& nc, int& no) {
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) { red[tid >> 6][0] = nc; red[tid >> 6][1] = no; }
    __syncthreads();
    if (tid == 0) {
        nc = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        no = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
}

struct CovDev : SearchRows {                                           // (the rows and search_row_live: search_rows.h; token is not read)
    const float* alphas; const int* enc_len; float* score; float* hist;
    float w_c, w_o, tau, kappa;
    int Tp, vec_state, vec_alpha;
};

__global__ __launch_bounds__(256) void coverage_step_kernel(CovDev a) {
    __shared__ int red[4][2];
    const int row = blockIdx.x, tid = threadIdx.x;
    int t_step, u;
    if (!search_row_live(a, row, t_step, u)) return;
    const int Tp = a.Tp, W = a.width;
    const int L = clampi(a.enc_len[row], 0, Tp);
    const bool first = t_step == 0;                                    // the parent is all zeros, whatever state_in holds
    const float* al = a.alphas + (size_t)row * Tp;
    const float* pr = a.st_in + (size_t)row * W;
    float* cu = a.st_out + (size_t)row * W;
    const float tau = a.tau, kappa = a.kappa;
    int nc = 0, no = 0;

    // ---- whole groups of four frames, 16 bytes per access (the loop bounds are uniform: every lane takes part in the ballots)
    const int n4 = a.vec_state ? Tp >> 2 : 0;
    for (int c0 = 0; c0 < n4; c0 += 256) {
        const int c = c0 + tid;
        const bool on = c < n4;
        float4 p = {0.f, 0.f, 0.f, 0.f}, x = {0.f, 0.f, 0.f, 0.f};
        if (on) {
            if (!first) p = reinterpret_cast<const float4*>(pr)[c];
            if (a.vec_alpha) x = reinterpret_cast<const float4*>(al)[c];
            else { x.x = al[4 * c]; x.y = al[4 * c + 1]; x.z = al[4 * c + 2]; x.w = al[4 * c + 3]; }
        }
        const float4 s = {cov_add(p.x, x.x), cov_add(p.y, x.y), cov_add(p.z, x.z), cov_add(p.w, x.w)};
        if (on) reinterpret_cast<float4*>(cu)[c] = s;
        cov_count(s.x, on && 4 * c < L, tau, kappa, nc, no);
        cov_count(s.y, on && 4 * c + 1 < L, tau, kappa, nc, no);
        cov_count(s.z, on && 4 * c + 2 < L, tau, kappa, nc, no);
        cov_count(s.w, on && 4 * c + 3 < L, tau, kappa, nc, no);
    }
    // ---- the frames behind them, one at a time (at most three with 16-byte state rows)
    for (int j0 = 4 * n4; j0 < Tp; j0 += 256) {
        const int f = j0 + tid;
        const bool on = f < Tp;
        float s = 0.f;
        if (on) { s = cov_add(first ? 0.f : pr[f], al[f]); cu[f] = s; }
        cov_count(s, on && f < L, tau, kappa, nc, no);
    }
    for (int f = Tp + 2 + tid; f < W; f += 256) cu[f] = 0.f;            // padding
    cov_block_sum(red, nc, no);
    if (tid != 0) return;
    // ---- one lane: the counts, the record of the step and the row's running sum
    const float fc = (float)nc, fo = (float)no;
    cu[Tp] = fc; cu[Tp + 1] = fo;
    if (a.hist) {
        float* h = a.hist + ((size_t)t_step * a.nutt * a.beam + row) * 2;
        h[0] = fc; h[1] = fo;
    }
    if (a.w_c != 0.f || a.w_o != 0.f) {
        const float dc = __fsub_rn(fc, first ? 0.f : pr[Tp]), dov = __fsub_rn(fo, first ? 0.f : pr[Tp + 1]);
        const float g = __fsub_rn(__fmul_rn(a.w_c, dc), __fmul_rn(a.w_o, dov));
        a.score[row] = __fadd_rn(a.score[row], g);
    }
}

struct CovRowsDev { const float* alphas; const int *steps, *enc_len; int* counts; float tau, kappa; int U, R, Tp; };

__global__ __launch_bounds__(256) void coverage_rows_kernel(CovRowsDev a) {
    __shared__ int red[4][2];
    const int row = blockIdx.x, tid = threadIdx.x, Tp = a.Tp;
    const int n = clampi(a.steps[row], 0, a.U), L = clampi(a.enc_len[row], 0, Tp);
    const size_t stride = (size_t)a.R * Tp;
    const float* al = a.alphas + (size_t)row * Tp;
    int nc = 0, no = 0;
    for (int j0 = 0; j0 < Tp; j0 += 256) {
        const int f = j0 + tid;
        const bool on = f < Tp;
        float s = 0.f;
        if (on)
            for (int t = 0; t < n; ++t) s = cov_add(s, al[(size_t)t * stride + f]);
        cov_count(s, on && f < L, a.tau, a.kappa, nc, no);
    }
    cov_block_sum(red, nc, no);
    if (tid == 0) { a.counts[2 * (size_t)row] = nc; a.counts[2 * (size_t)row + 1] = no; }
}

bool cov_thresholds_ok(float tau, float kappa) { return tau > 0.f && kappa > tau && kappa <= 3.0e38f; }

}  // namespace

extern "C" int las_coverage_step(const float* alphas, const int* enc_len, int nutt, int beam, int Tp, float* score, float w_c, float w_o,
                                 float tau, float kappa, float* hist, const float* state_in, float* state_out, int state_width,
                                 const int* token, const int* step, const int* nlive, const int* done, const int* dec_step, int Umax,
                                 void* stream) {
    LAS_ARG(Tp > 0 && Tp <= (1 << 24) - 2, "las_coverage_step: bad dims (Tp = %d)", Tp);
    CovDev a;                                           // (token: one of the loop words every scorer is handed; not read, may be NULL)
    if (search_rows_args(a, "las_coverage_step", Tp + 2, nutt, beam, state_in, state_out, state_width,
                         token, step, nlive, done, dec_step, Umax)) return -1;
    LAS_ARG(alphas && enc_len && score, "las_coverage_step: null pointer");
    LAS_ARG(w_c >= 0.f && w_c <= 3.0e38f && w_o >= 0.f && w_o <= 3.0e38f,
            "las_coverage_step: the weights must be finite and >= 0 (got %g, %g)", (double)w_c, (double)w_o);
    LAS_ARG(cov_thresholds_ok(tau, kappa), "las_coverage_step: thresholds 0 < tau < kappa, finite (got %g, %g)", (double)tau, (double)kappa);
    a.alphas = alphas; a.enc_len = enc_len; a.score = score; a.hist = hist;
    a.w_c = w_c; a.w_o = w_o; a.tau = tau; a.kappa = kappa; a.Tp = Tp;
    a.vec_state = (state_width % 4 == 0 && (((size_t)state_in | (size_t)state_out) & 15) == 0) ? 1 : 0;
    a.vec_alpha = (Tp % 4 == 0 && ((size_t)alphas & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(coverage_step_kernel, dim3(nutt * beam), dim3(256), 0, (hipStream_t)stream, a);
    LAS_LAUNCHED();
    return 0;
}

extern "C" int las_coverage_rows(const float* alphas, int U, int R, int Tp, const int* steps, const int* enc_len, float tau, float kappa,
                                 int* counts, void* stream) {
    LAS_ARG(alphas && steps && enc_len && counts, "las_coverage_rows: null pointer");
    LAS_ARG(U > 0 && R > 0 && Tp > 0 && Tp <= (1 << 24) - 2, "las_coverage_rows: bad dims");
    LAS_ARG(cov_thresholds_ok(tau, kappa), "las_coverage_rows: thresholds 0 < tau < kappa, finite (got %g, %g)", (double)tau, (double)kappa);
    CovRowsDev a;
    a.alphas = alphas; a.steps = steps; a.enc_len = enc_len; a.counts = counts; a.tau = tau; a.kappa = kappa; a.U = U; a.R = R; a.Tp = Tp;
    hipLaunchKernelGGL(coverage_rows_kernel, dim3(R), dim3(256), 0, (hipStream_t)stream, a);
    LAS_LAUNCHED();
    return 0;
}
