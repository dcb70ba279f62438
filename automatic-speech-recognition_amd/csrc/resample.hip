// resample.hip -- the band-limited resampler in front of the audio front end: a batch of waveforms from fs_in to fs_out (= L / M in
// lowest terms) with a per-utterance gain, one launch.  sox's `speed s` is this with fs_in = fs * s: the reference's speed (and volume)
// augmentation (preprocess.py:157-167, utils/augmentation.py) without sox.  The arithmetic is preprocess.resample's, in fp32:
//   output m of a row reads n0 = (m M) / L and phase p = (m M) % L,   y[m] = gain * sum_{i < 2W} x[n0 - W + 1 + i] * table[p, i].
//
//   resample_kernel   a workgroup owns `tile` consecutive outputs of one utterance (blockIdx.x = tile, blockIdx.y = utterance).  It stages the
//                     input span those outputs read -- (tile - 1) M / L + 1 + 2W samples at most, int16 converted and samples outside
//                     the recording as zeros -- into LDS once; every thread then runs ONE fmaf chain per output over the taps in
//                     ascending order.  The chain of an output depends on (m, the row) only: not on where the tile boundaries fall, not
//                     on the other rows, so a row inside a batch gives the bits it gives alone and two runs give the same bits.
//                     m0 * M is formed in 64 bits once per workgroup (30 s at 44.1 kHz is already 6e8); inside the tile the offsets
//                     r0 + j * M stay below 2^31 (tile <= 1024, M <= 2^20: the entry's limits) and are divided in 32 bits.
//                     The table ([L, 2W]) is staged into LDS when it has at most 4096 entries (the speed and integer ratios: L <= 10);
//                     a rational ratio's table (44.1 kHz -> 16 kHz: 160 x 144, 90 KB) is read from global memory, two taps per load --
//                     the same rows are read by every workgroup and stay in cache.  Where the table sits does not change the result.
//   gain_kernel       L == M == 1: out = gain * in, one rounding (no fmaf with a zero addend, which would turn a -0 into +0); with no gain
//                     a bit copy of fp32 input.
// Every element of out [n, ld_out] is written: zeros behind n_out[u].
#include "las_common.h"

namespace {

constexpr int NT = 256;
constexpr int TILE_MAX = 1024;                        // outputs per workgroup: 4 per thread
constexpr int SPAN_MAX = 8192;                        // staged input samples (32 KB)
constexpr int TABLE_LDS_MAX = 4096;                   // table entries kept in LDS (16 KB)
constexpr int RATIO_MAX = 1 << 20;                    // L, M: (tile - 1) * M + L stays below 2^31
constexpr int TAPS_MAX = 1024;

// the input span of a tile of `tile` outputs: the first output reads from n0 - W + 1, the last up to n0' + W with n0' - n0 <= ((tile - 1) M + L - 1) / L
long long tile_span(int tile, int L, int M, int W) { return ((long long)(tile - 1) * M + L - 1) / L + 2LL * W; }

template <bool I16, bool TLDS>
__global__ __launch_bounds__(NT) void resample_kernel(const void* __restrict__ in, long long ld_in, const int* __restrict__ n_in, int L, int M, int W,
                                                      int tile, const float* __restrict__ table, const float* __restrict__ gain,
                                                      float* __restrict__ out, long long ld_out, int* __restrict__ n_out_dev) {
    __shared__ __attribute__((aligned(16))) float xs[SPAN_MAX];
    __shared__ __attribute__((aligned(16))) float ts[TLDS ? TABLE_LDS_MAX : 2];
    const int u = blockIdx.y, K = 2 * W;
    const long long n = max(min((long long)n_in[u], ld_in), 0LL);
    const long long n_out = min((n * L + M - 1) / M, ld_out);
    const long long m0 = (long long)blockIdx.x * tile;
    const long long m_end = min(m0 + tile, ld_out);
    if (blockIdx.x == 0 && threadIdx.x == 0 && n_out_dev) n_out_dev[u] = (int)n_out;
    float* orow = out + (long long)u * ld_out;
    if (m0 >= n_out) {                                // (uniform: the whole workgroup) a tile behind the utterance
        for (long long m = m0 + threadIdx.x; m < m_end; m += NT) orow[m] = 0.f;
        return;
    }
    const long long base = m0 * (long long)M;         // 64 bits
    const long long q0 = base / L;
    const unsigned r0 = (unsigned)(base - q0 * L);
    const long long s0 = q0 - W + 1;                  // the first staged sample (negative at the head of the recording)
    const int span = min((int)((r0 + (unsigned)(tile - 1) * (unsigned)M) / (unsigned)L) + K, SPAN_MAX);
    const char* irow = (const char*)in + (long long)u * ld_in * (I16 ? 2 : 4);
    for (int k = threadIdx.x; k < span; k += NT) {
        const long long i = s0 + k;
        xs[k] = (i >= 0 && i < n) ? sample_at<I16>(irow, i) : 0.f;
    }
    if (TLDS)
        for (int k = threadIdx.x; k < L * K; k += NT) ts[k] = table[k];
    __syncthreads();
    const float g = gain ? gain[u] : 1.f;
    for (int j = threadIdx.x; m0 + j < m_end; j += NT) {
        float y = 0.f;
        if (m0 + j < n_out) {
            const unsigned t = r0 + (unsigned)j * (unsigned)M;
            const unsigned dn = t / (unsigned)L, p = t - dn * (unsigned)L;
            const float* x = xs + dn;
            const float* h = (TLDS ? ts : table) + (long long)p * K;      // (K is even: a row starts on 8 bytes)
            float acc = 0.f;
            for (int i = 0; i < K; i += 2) {
                const float2 hh = *(const float2*)(h + i);
                acc = fmaf(x[i], hh.x, acc);
                acc = fmaf(x[i + 1], hh.y, acc);
            }
            y = gain ? g * acc : acc;
        }
        orow[m0 + j] = y;
    }
}

template <bool I16>
__global__ __launch_bounds__(NT) void gain_kernel(const void* __restrict__ in, long long ld_in, const int* __restrict__ n_in,
                                                  const float* __restrict__ gain, float* __restrict__ out, long long ld_out,
                                                  int* __restrict__ n_out_dev) {
    const int u = blockIdx.y;
    const long long n = max(min((long long)n_in[u], min(ld_in, ld_out)), 0LL);
    if (blockIdx.x == 0 && threadIdx.x == 0 && n_out_dev) n_out_dev[u] = (int)n;
    const char* irow = (const char*)in + (long long)u * ld_in * (I16 ? 2 : 4);
    float* orow = out + (long long)u * ld_out;
    const float g = gain ? gain[u] : 1.f;
    const long long m0 = (long long)blockIdx.x * TILE_MAX;
    const long long m_end = min(m0 + TILE_MAX, ld_out);
    for (long long m = m0 + threadIdx.x; m < m_end; m += NT) {
        float y = 0.f;
        if (m < n) {
            const float v = sample_at<I16>(irow, m);
            y = gain ? g * v : v;
        }
        orow[m] = y;
    }
}

}  // namespace

extern "C" long long las_resample_out_len(long long n_in, int L, int M) {
    if (n_in < 0 || L < 1 || M < 1) return -1;
    return (long long)(((__int128)n_in * L + (M - 1)) / M);
}

extern "C" int las_resample_tile(int L, int M, int W) {
    if (L < 1 || M < 1 || L > RATIO_MAX || M > RATIO_MAX || W < 1 || 2 * (long long)W > TAPS_MAX) return 0;
    for (int tile = TILE_MAX; tile >= NT; tile >>= 1)
        if (tile_span(tile, L, M, W) <= SPAN_MAX) return tile;
    return 0;
}

extern "C" int las_resample(const las_resample_args* a, void* stream) {
    LAS_ARG(a != nullptr, "las_resample: null argument struct");
    LAS_ARG(a->n >= 1 && a->n <= 65535, "las_resample: bad batch (n=%d, 1..65535)", a->n);
    LAS_ARG(a->L >= 1 && a->M >= 1 && a->L <= RATIO_MAX && a->M <= RATIO_MAX, "las_resample: ratio L/M = %d/%d (1..%d each)", a->L, a->M, RATIO_MAX);
    LAS_ARG(a->W >= 1 && 2LL * a->W <= TAPS_MAX, "las_resample: half width W=%d for ratio %d/%d (1 <= W, 2W <= %d taps)", a->W, a->L, a->M, TAPS_MAX);
    const int K = 2 * a->W;
    LAS_ARG((long long)a->L * K <= (1 << 20), "las_resample: table of ratio %d/%d has %d x %d entries (at most %d)", a->L, a->M, a->L, K, 1 << 20);
    const bool gain_only = a->L == 1 && a->M == 1;
    const int tile = las_resample_tile(a->L, a->M, a->W);
    LAS_ARG(gain_only || tile > 0, "las_resample: ratio %d/%d with W=%d: %d outputs read %lld input samples (staging holds %d)", a->L, a->M, a->W, NT,
            tile_span(NT, a->L, a->M, a->W), SPAN_MAX);
    LAS_ARG(a->in && a->n_in && a->n_in_host && a->out && (gain_only || a->table), "las_resample: null pointer");
    LAS_ARG(gain_only || ((uintptr_t)a->table & 7) == 0, "las_resample: table %p is not 8-byte aligned (its rows are read two taps per load)", (const void*)a->table);
    LAS_ARG(a->ld_in >= 1 && a->ld_out >= 1 && a->ld_out <= INT32_MAX, "las_resample: ld_in=%lld, ld_out=%lld (1..INT32_MAX)", a->ld_in, a->ld_out);
    for (int u = 0; u < a->n; ++u) {
        const int nu = a->n_in_host[u];
        LAS_ARG(nu >= 1 && nu <= a->ld_in, "las_resample: utterance %d has %d samples (1..pitch %lld)", u, nu, a->ld_in);
        const long long no = las_resample_out_len(nu, a->L, a->M);
        LAS_ARG(no <= a->ld_out, "las_resample: utterance %d gives %lld samples at ratio %d/%d, ld_out=%lld", u, no, a->L, a->M, a->ld_out);
    }
    hipStream_t st = (hipStream_t)stream;
    if (gain_only) {
        const dim3 grid(cdiv(a->ld_out, TILE_MAX), a->n);
        if (a->in_i16) hipLaunchKernelGGL(gain_kernel<true>, grid, dim3(NT), 0, st, a->in, a->ld_in, a->n_in, a->gain, a->out, a->ld_out, a->n_out);
        else           hipLaunchKernelGGL(gain_kernel<false>, grid, dim3(NT), 0, st, a->in, a->ld_in, a->n_in, a->gain, a->out, a->ld_out, a->n_out);
        LAS_LAUNCHED();
        return 0;
    }
    const dim3 grid(cdiv(a->ld_out, tile), a->n);
    const bool tlds = (long long)a->L * K <= TABLE_LDS_MAX;
#define LAS_RESAMPLE_LAUNCH(I16, TLDS)                                                                                                    \
    hipLaunchKernelGGL((resample_kernel<I16, TLDS>), grid, dim3(NT), 0, st, a->in, a->ld_in, a->n_in, a->L, a->M, a->W, tile, a->table, \
                       a->gain, a->out, a->ld_out, a->n_out)
    if (a->in_i16) { if (tlds) LAS_RESAMPLE_LAUNCH(true, true); else LAS_RESAMPLE_LAUNCH(true, false); }
    else           { if (tlds) LAS_RESAMPLE_LAUNCH(false, true); else LAS_RESAMPLE_LAUNCH(false, false); }
#undef LAS_RESAMPLE_LAUNCH
    LAS_LAUNCHED();
    return 0;
}
