// wave_aug.hip -- multi-condition training data on the device, between las_resample and las_frontend (las_hip.h K16): a room
// impulse response convolved into every utterance (las_reverb) and background noise mixed in at a drawn signal-to-noise ratio
// (las_noise_mix).  The arithmetic is preprocess.reverberate's and preprocess.mix_noise's, in fp32.
//
//   reverb_kernel       y[m] = sum_{k < K} h[k] x[m + delay - k], a direct-form FIR.  A workgroup owns TILE = 2048 consecutive outputs of
//                       one utterance (blockIdx.x = tile, blockIdx.y = utterance), every lane R = 8 CONSECUTIVE ones in registers.  The
//                       taps are taken CHUNK = 512 at a time: the workgroup stages the TILE + CHUNK input samples those taps reach
//                       (samples outside [0, n_u) as zeros: nothing behind a row's length is read) and the chunk's taps (zeros behind K)
//                       into LDS.  A block of U = 16 taps then costs a lane six ds_read_b128 of its 24-sample window, four ds_read_b128
//                       of the taps (one address for the whole wave: a broadcast) and 128 v_fma_f32 with static register indices --
//                       acc[r] += h[k] * w[16 + r - (k - kb)].  The windows of neighbouring lanes start 32 bytes apart, which puts the
//                       lanes of a 16-lane group of a ds_read_b128 on the same banks; the two 16-byte halves of every second group
//                       of eight 32-byte segments are swapped in LDS (an XOR on the address) so that they are not: measured, the
//                       launch of DESIGN 7m takes 1.93 ms with the swap and 6.57 ms without.
//                       SUMMATION ORDER (the contract): every output is ONE fmaf chain from +0 over the taps in ASCENDING k, then over
//                       the zero taps that pad the last chunk to a multiple of 16 (they add +-0).  It depends on (the row's samples, its
//                       response) only: not on the tile, not on the batch, not on the other rows' responses.
//                       Tiles of a row with rir_idx = -1 copy their input's bits; tiles behind n_u store zeros; neither stages anything.
//   noise_power_kernel  (tile of NOISE_TILE samples, utterance): sum s^2 and sum v^2, v[m] = noise[(off + m) mod len], in double over the
//                       fp32 samples: a thread sums its samples (m = t, t + 256, ...) in ascending order, then a fixed tree over the threads.
//   noise_gain_kernel   (utterance): the tile sums in ascending order by the same scheme, Ps = sum / n, Pn = sum / n, g = sqrt(Ps / (Pn
//                       10^(snr / 10))) in double, rounded to fp32 once; 0 when Ps or Pn is 0.
//   noise_mix_kernel    (tile, utterance): out = fmaf(g, v, s); a bit copy of s for a row without noise or with g == 0; zeros behind n_u.
//                       Element-wise behind the reductions, so in == out is allowed.
// No atomics anywhere: two calls give the same bits.  Every element of out [n, ld_out] is written.
#include "las_common.h"
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int R = 8;                                  // consecutive outputs a lane keeps in registers
constexpr int TILE = NT * R;                          // outputs per workgroup
constexpr int CHUNK = 512;                            // taps staged at a time (a multiple of U)
constexpr int U = 16;                                 // taps per block of the inner loop (a multiple of 8)
constexpr int RIR_MAX = 16384;                        // one second at 16 kHz
constexpr int NOISE_TILE = 4096;                      // samples per partial sum

// word i of the staged span -> its place in LDS: 8-word segments, the two 16-byte halves of a segment swapped where bit 3 of the segment
// index is set (lanes l and l + 8 / l + 24 of a ds_read_b128 group read segments 8 / 24 apart: one takes the even slot, one the odd)
__device__ __forceinline__ int swz(int i) { return i ^ ((i >> 4) & 4); }

__global__ __launch_bounds__(NT) void reverb_kernel(const float* __restrict__ in, long long ld_in, const int* __restrict__ n_in,
                                                    const float* __restrict__ rir, long long ld_rir, const int* __restrict__ rir_len,
                                                    const int* __restrict__ rir_delay, const int* __restrict__ rir_idx,
                                                    float* __restrict__ out, long long ld_out) {
    __shared__ float4 xs4[(TILE + CHUNK) / 4];        // (typed as the 16-byte slots the inner loop reads)
    __shared__ float4 hs4[CHUNK / 4];
    float* xs = (float*)xs4;
    float* hs = (float*)hs4;
    const int u = blockIdx.y, t = threadIdx.x;
    const long long n = max(min((long long)n_in[u], min(ld_in, ld_out)), 0LL);
    const long long m0 = (long long)blockIdx.x * TILE;
    const long long m_end = min(m0 + TILE, ld_out);
    const float* irow = in + (long long)u * ld_in;
    float* orow = out + (long long)u * ld_out;
    if (m0 >= n) {                                    // (uniform: the whole workgroup) a tile behind the utterance
        for (long long m = m0 + t; m < m_end; m += NT) orow[m] = 0.f;
        return;
    }
    const int idx = rir_idx[u];
    if (idx < 0) {                                    // (uniform) no response: the input's bits
        for (long long m = m0 + t; m < m_end; m += NT)
            ((unsigned*)orow)[m] = m < n ? ((const unsigned*)irow)[m] : 0u;
        return;
    }
    const int K = min(max(rir_len[idx], 1), RIR_MAX);
    const int D = min(max(rir_delay[idx], 0), K - 1);
    const float* h = rir + (long long)idx * ld_rir;
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += CHUNK) {           // (uniform)
        const int kc = min(CHUNK, K - k0);
        const int kc8 = (kc + U - 1) & ~(U - 1);          // (zero taps behind kc)
        // word i of the span is x[s0 + i]; output j of the tile and tap k0 + kk meet at i = j + CHUNK - kk
        const long long s0 = m0 + D - k0 - CHUNK;
        __syncthreads();                              // the previous chunk has been read
        for (int i = CHUNK - kc8 + t; i < TILE + CHUNK; i += NT) {
            const long long g = s0 + i;
            xs[swz(i)] = (g >= 0 && g < n) ? irow[g] : 0.f;
        }
        for (int kk = t; kk < kc8; kk += NT) hs[kk] = kk < kc ? h[k0 + kk] : 0.f;
        __syncthreads();
        for (int kb = 0; kb < kc8; kb += U) {
            const int base = R * t + CHUNK - kb - U;  // a multiple of 8: the window is the (R + U) / 8 segments from base / 8
            float w[R + U], hh[U];
#pragma unroll
            for (int s = 0; s < (R + U) / 8; ++s) {
                const int f = ((base + 8 * s) >> 6) & 1, s4 = (base >> 2) + 2 * s;
                const float4 lo = xs4[s4 + f], hi = xs4[s4 + (1 ^ f)];
                w[8 * s + 0] = lo.x; w[8 * s + 1] = lo.y; w[8 * s + 2] = lo.z; w[8 * s + 3] = lo.w;
                w[8 * s + 4] = hi.x; w[8 * s + 5] = hi.y; w[8 * s + 6] = hi.z; w[8 * s + 7] = hi.w;
            }
#pragma unroll
            for (int i = 0; i < U / 4; ++i) {
                const float4 h4 = hs4[(kb >> 2) + i];
                hh[4 * i + 0] = h4.x; hh[4 * i + 1] = h4.y; hh[4 * i + 2] = h4.z; hh[4 * i + 3] = h4.w;
            }
#pragma unroll
            for (int q = 0; q < U; ++q)
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = fmaf(hh[q], w[U + r - q], acc[r]);
        }
    }
    __syncthreads();                                  // through LDS once more, so that the stores of a wave are consecutive words
#pragma unroll
    for (int r = 0; r < R; ++r) xs[R * t + r] = acc[r];
    __syncthreads();
    for (int j = t; m0 + j < m_end; j += NT) orow[m0 + j] = m0 + j < n ? xs[j] : 0.f;
}

// sum over the workgroup's 256 threads in a fixed tree (every thread gets it); red holds NT doubles
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = NT / 2; o >= 1; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(NT) void noise_power_kernel(const float* in, long long ld_in, const int* __restrict__ n_in, long long ld_lim,
                                                         const float* __restrict__ noise, long long ld_noise, const int* __restrict__ noise_len,
                                                         const int* __restrict__ noise_idx, const int* __restrict__ noise_off,
                                                         double* __restrict__ part, int ntile) {
    __shared__ double red[NT];
    const int u = blockIdx.y, t = threadIdx.x;
    const int idx = noise_idx[u];
    const long long n = max(min((long long)n_in[u], ld_lim), 0LL);
    const long long m0 = (long long)blockIdx.x * NOISE_TILE;
    double ss = 0.0, vv = 0.0;
    if (idx >= 0 && m0 < n) {                         // (uniform)
        const float* srow = in + (long long)u * ld_in;
        const float* vrow = noise + (long long)idx * ld_noise;
        const unsigned len = (unsigned)max(noise_len[idx], 1);
        const unsigned b = (unsigned)(((unsigned long long)max(noise_off[u], 0) + (unsigned long long)m0) % len);      // 64 bits once per tile
        const int cnt = (int)min((long long)NOISE_TILE, n - m0);
        for (int j = t; j < cnt; j += NT) {           // (b < 2^31, j < 2^12: the sum fits 32 bits)
            const double s = (double)srow[m0 + j], v = (double)vrow[(b + (unsigned)j) % len];
            ss = fma(s, s, ss);
            vv = fma(v, v, vv);
        }
    }
    ss = block_sum_f64(ss, red);
    vv = block_sum_f64(vv, red);
    if (t == 0) {
        part[((long long)u * ntile + blockIdx.x) * 2] = ss;
        part[((long long)u * ntile + blockIdx.x) * 2 + 1] = vv;
    }
}

__global__ __launch_bounds__(NT) void noise_gain_kernel(const double* __restrict__ part, int ntile, const int* __restrict__ n_in, long long ld_lim,
                                                        const int* __restrict__ noise_idx, const float* __restrict__ snr_db,
                                                        float* __restrict__ gain, float* __restrict__ gain_out) {
    __shared__ double red[NT];
    const int u = blockIdx.x, t = threadIdx.x;
    const long long n = max(min((long long)n_in[u], ld_lim), 0LL);
    const int live = (int)((n + NOISE_TILE - 1) / NOISE_TILE);
    double ss = 0.0, vv = 0.0;
    for (int j = t; j < live && j < ntile; j += NT) {
        ss += part[((long long)u * ntile + j) * 2];
        vv += part[((long long)u * ntile + j) * 2 + 1];
    }
    ss = block_sum_f64(ss, red);
    vv = block_sum_f64(vv, red);
    if (t == 0) {
        float g = 0.f;
        if (noise_idx[u] >= 0 && n > 0 && ss > 0.0 && vv > 0.0) {
            const double Ps = ss / (double)n, Pn = vv / (double)n;
            g = (float)sqrt(Ps / (Pn * pow(10.0, (double)snr_db[u] / 10.0)));
        }
        gain[u] = g;
        if (gain_out) gain_out[u] = g;
    }
}

__global__ __launch_bounds__(NT) void noise_mix_kernel(const float* in, long long ld_in, const int* __restrict__ n_in,
                                                       const float* __restrict__ noise, long long ld_noise, const int* __restrict__ noise_len,
                                                       const int* __restrict__ noise_idx, const int* __restrict__ noise_off,
                                                       const float* __restrict__ gain, float* out, long long ld_out) {
    const int u = blockIdx.y, t = threadIdx.x;
    const long long n = max(min((long long)n_in[u], min(ld_in, ld_out)), 0LL);
    const long long m0 = (long long)blockIdx.x * NOISE_TILE;
    const long long m_end = min(m0 + NOISE_TILE, ld_out);
    const float* srow = in + (long long)u * ld_in;
    float* orow = out + (long long)u * ld_out;
    if (m0 >= n) {                                    // (uniform) a tile behind the utterance
        for (long long m = m0 + t; m < m_end; m += NT) orow[m] = 0.f;
        return;
    }
    const int idx = noise_idx[u];
    const float g = gain[u];
    if (idx < 0 || g == 0.f) {                        // (uniform) nothing to add: the input's bits
        for (long long m = m0 + t; m < m_end; m += NT) {
            const unsigned v = m < n ? ((const unsigned*)srow)[m] : 0u;
            ((unsigned*)orow)[m] = v;
        }
        return;
    }
    const float* vrow = noise + (long long)idx * ld_noise;
    const unsigned len = (unsigned)max(noise_len[idx], 1);
    const unsigned b = (unsigned)(((unsigned long long)max(noise_off[u], 0) + (unsigned long long)m0) % len);
    for (int j = t; m0 + j < m_end; j += NT) {
        float y = 0.f;
        if (m0 + j < n) y = fmaf(g, vrow[(b + (unsigned)j) % len], srow[m0 + j]);
        orow[m0 + j] = y;
    }
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

bool overlap(const void* a, long long a_bytes, const void* b, long long b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

}  // namespace

extern "C" int las_reverb_tile(void) { return TILE; }
extern "C" int las_reverb_tap_chunk(void) { return CHUNK; }
extern "C" int las_noise_mix_tile(void) { return NOISE_TILE; }

extern "C" int las_reverb(const float* in, long long ld_in, const int* n_in, const int* n_in_host, int n, const float* rir, long long ld_rir,
                          const int* rir_len, const int* rir_len_host, const int* rir_delay, const int* rir_delay_host, int n_rir,
                          const int* rir_idx, const int* rir_idx_host, float* out, long long ld_out, void* stream) {
    LAS_ARG(in && n_in && n_in_host && rir && rir_len && rir_len_host && rir_delay && rir_delay_host && rir_idx && rir_idx_host && out,
            "las_reverb: null pointer (in, n_in, n_in_host, rir, rir_len, rir_len_host, rir_delay, rir_delay_host, rir_idx, rir_idx_host, out)");
    LAS_ARG(n >= 1 && n <= 65535, "las_reverb: bad batch (n=%d, 1..65535)", n);
    LAS_ARG(n_rir >= 1, "las_reverb: a bank of %d responses (>= 1)", n_rir);
    LAS_ARG(ld_in >= 1 && ld_out >= 1 && ld_in <= INT32_MAX && ld_out <= INT32_MAX && ld_rir >= 1 && ld_rir <= INT32_MAX,
            "las_reverb: ld_in=%lld, ld_out=%lld, ld_rir=%lld (1..INT32_MAX)", ld_in, ld_out, ld_rir);
    for (int r = 0; r < n_rir; ++r) {
        const int K = rir_len_host[r], D = rir_delay_host[r];
        LAS_ARG(K >= 1 && K <= RIR_MAX && K <= ld_rir, "las_reverb: response %d has %d taps (1..%d, pitch %lld)", r, K, RIR_MAX, ld_rir);
        LAS_ARG(D >= 0 && D < K, "las_reverb: response %d has its direct path at %d (0..%d)", r, D, K - 1);
    }
    const long long lim = ld_in < ld_out ? ld_in : ld_out;
    for (int u = 0; u < n; ++u) {
        LAS_ARG(rir_idx_host[u] >= -1 && rir_idx_host[u] < n_rir, "las_reverb: utterance %d takes response %d (-1..%d)", u, rir_idx_host[u], n_rir - 1);
        LAS_ARG(n_in_host[u] >= 1 && n_in_host[u] <= lim, "las_reverb: utterance %d has %d samples (1..min(ld_in, ld_out)=%lld)", u, n_in_host[u], lim);
    }
    LAS_ARG(!overlap(in, 4LL * n * ld_in, out, 4LL * n * ld_out), "las_reverb: in and out overlap (every output reads up to %d inputs around it)", RIR_MAX);
    hipLaunchKernelGGL(reverb_kernel, dim3(cdiv(ld_out, TILE), n), dim3(NT), 0, (hipStream_t)stream, in, ld_in, n_in, rir, ld_rir, rir_len, rir_delay,
                       rir_idx, out, ld_out);
    LAS_LAUNCHED();
    return 0;
}

// the workspace: [tile sums f64 [n, ceil(ld / NOISE_TILE), 2] | gains f32 [n]]
extern "C" size_t las_noise_mix_workspace_bytes(int n, long long ld) {
    if (n < 1 || ld < 1 || ld > INT32_MAX) return 0;
    const size_t ntile = (size_t)((ld + NOISE_TILE - 1) / NOISE_TILE);
    return up256((size_t)n * ntile * 2 * sizeof(double)) + up256((size_t)n * sizeof(float));
}

extern "C" int las_noise_mix(const float* in, long long ld_in, const int* n_in, const int* n_in_host, int n, const float* noise,
                             long long ld_noise, const int* noise_len, const int* noise_len_host, int n_noise, const int* noise_idx,
                             const int* noise_idx_host, const int* noise_off, const int* noise_off_host, const float* snr_db,
                             const float* snr_db_host, float* out, long long ld_out, float* gain_out, void* ws, size_t ws_bytes,
                             void* stream) {
    LAS_ARG(in && n_in && n_in_host && noise && noise_len && noise_len_host && noise_idx && noise_idx_host && noise_off && noise_off_host &&
                snr_db && snr_db_host && out && ws,
            "las_noise_mix: null pointer (in, n_in, n_in_host, noise, noise_len, noise_len_host, noise_idx, noise_idx_host, noise_off, "
            "noise_off_host, snr_db, snr_db_host, out, ws)");
    LAS_ARG(n >= 1 && n <= 65535, "las_noise_mix: bad batch (n=%d, 1..65535)", n);
    LAS_ARG(n_noise >= 1, "las_noise_mix: a bank of %d noises (>= 1)", n_noise);
    LAS_ARG(ld_in >= 1 && ld_out >= 1 && ld_in <= INT32_MAX && ld_out <= INT32_MAX && ld_noise >= 1 && ld_noise <= INT32_MAX,
            "las_noise_mix: ld_in=%lld, ld_out=%lld, ld_noise=%lld (1..INT32_MAX)", ld_in, ld_out, ld_noise);
    for (int r = 0; r < n_noise; ++r)
        LAS_ARG(noise_len_host[r] >= 1 && noise_len_host[r] <= ld_noise, "las_noise_mix: noise %d has %d samples (1..pitch %lld)", r,
                noise_len_host[r], ld_noise);
    const long long lim = ld_in < ld_out ? ld_in : ld_out;
    long long longest = 1;
    for (int u = 0; u < n; ++u) {
        const int idx = noise_idx_host[u];
        LAS_ARG(idx >= -1 && idx < n_noise, "las_noise_mix: utterance %d takes noise %d (-1..%d)", u, idx, n_noise - 1);
        LAS_ARG(n_in_host[u] >= 1 && n_in_host[u] <= lim, "las_noise_mix: utterance %d has %d samples (1..min(ld_in, ld_out)=%lld)", u, n_in_host[u], lim);
        if (idx >= 0) {
            LAS_ARG(noise_off_host[u] >= 0 && noise_off_host[u] < noise_len_host[idx], "las_noise_mix: utterance %d starts at sample %d of noise %d (0..%d)",
                    u, noise_off_host[u], idx, noise_len_host[idx] - 1);
            LAS_ARG(isfinite(snr_db_host[u]), "las_noise_mix: utterance %d at snr_db=%g (finite)", u, (double)snr_db_host[u]);
        }
        if (n_in_host[u] > longest) longest = n_in_host[u];
    }
    const size_t need = las_noise_mix_workspace_bytes(n, longest);
    LAS_ARG(ws_bytes >= need, "las_noise_mix: workspace of %zu bytes, %zu needed", ws_bytes, need);
    LAS_ARG(((uintptr_t)ws & 7) == 0, "las_noise_mix: ws is 8-byte aligned");
    LAS_ARG(in == out || !overlap(in, 4LL * n * ld_in, out, 4LL * n * ld_out), "las_noise_mix: in and out overlap without being the same buffer");
    LAS_ARG(in != out || ld_in == ld_out, "las_noise_mix: in place with ld_in=%lld, ld_out=%lld (equal pitches)", ld_in, ld_out);
    const int ntile = cdiv(longest, NOISE_TILE);
    double* part = (double*)ws;
    float* gain = (float*)((char*)ws + up256((size_t)n * ntile * 2 * sizeof(double)));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(noise_power_kernel, dim3(ntile, n), dim3(NT), 0, st, in, ld_in, n_in, lim, noise, ld_noise, noise_len, noise_idx, noise_off, part, ntile);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(noise_gain_kernel, dim3(n), dim3(NT), 0, st, part, ntile, n_in, lim, noise_idx, snr_db, gain, gain_out);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(noise_mix_kernel, dim3(cdiv(ld_out, NOISE_TILE), n), dim3(NT), 0, st, in, ld_in, n_in, noise, ld_noise, noise_len, noise_idx,
                       noise_off, gain, out, ld_out);
    LAS_LAUNCHED();
    return 0;
}
