// frontend.hip -- the audio front end: waveform -> feature cube (reference preprocess.py:71-86: speechpy's mfcc / mfe, cmvn with variance
// normalisation, extract_derivative_feature), for a batch of utterances of different lengths in one call.  The arithmetic is the
// restatement in this build's preprocess.py, evaluated in fp32.
//
// Three launches, stream-ordered on the caller's stream, no atomics (every sum has a fixed order: bit-reproducible, and a row of the
// batch never reads another row, so an utterance extracted alone gives the bits it gives inside a batch):
//   frontend_frames_kernel  one wave per frame, four frames per workgroup.  The frame (fl <= 512 samples, zero-padded to 512) is packed
//                           into 256 complex points, a radix-2 FFT over them runs in the wave's own LDS slice (8 stages of 128 butterflies,
//                           two per lane; twiddles from the caller's double-precision table), the real-FFT split gives X[0..256],
//                           P = |X|^2 / 512 goes back to LDS.  Energy: four bins per lane (+ bin 256), then the wave butterfly.  Mel: lane j
//                           sums filter j over its non-zero bins on the VALU in fp32 (a triangle covers 3-60 of the 257 bins: the dense
//                           product would be 90% zeros).  mfcc: logf, lane c sums row c of the DCT table, c0 = log(energy).
//                           One wave per frame because every phase is 64-wide with no cross-wave traffic; a 16-frame MFMA tile would
//                           only speed up the mel product, which is a tenth of the frame's work.
//   frontend_stats_kernel   one workgroup per (utterance, column): mean over the T_u frames, then the ddof-0 standard deviation of
//                           the mean-subtracted column (two passes; per-thread partials in frame order, then a fixed-order block sum),
//                           both in double: an fp32 mean's rounding, divided by a small spread, is the one place fp32 does not do.
//   frontend_cmvn_delta_kernel
//                           one wave per frame row: (x - mean) / (std + 2^-30) in double, rounded to fp32, then derivative_extraction
//                           twice along the FEATURE axis with edge padding; rows behind T_u are written as zeros.
// Without cmvn the first kernel writes the raw features (and the zero rows) straight into the output.
#include "las_common.h"
#include <math.h>

namespace {

constexpr int NFFT = 512, NC = 256, NBINS = 257;      // real FFT length, complex points, power-spectrum bins
constexpr int MAX_FILTERS = 128;                      // mel filters (= feat_dim of fbank features)
constexpr int FRAMES_PER_WG = 4;
constexpr float ZERO_FLOOR = 2.220446049250313e-16f;  // np.finfo(float).eps = 2^-52: what an exact 0 becomes (_zero_handling)

struct FrameLds {
    float re[NC], im[NC];
    float P[NBINS + 3];
    float lm[MAX_FILTERS];
};

__device__ __forceinline__ int frames_of(int n_u, int fl, int step, int ld, int Tmax) {
    n_u = min(n_u, ld);
    const int T = n_u >= fl ? (n_u - fl) / step : 0;
    return min(T, Tmax);
}

template <bool I16>
__global__ __launch_bounds__(64 * FRAMES_PER_WG) void frontend_frames_kernel(
        const void* __restrict__ samples, long long ld, const int* __restrict__ n_samples, int Tmax, int fl, int step, int mfcc, int D, int NF,
        const float* __restrict__ tw, const float* __restrict__ fb, const int* __restrict__ fb_range, const float* __restrict__ dct,
        float* __restrict__ feat, int zero_tail) {
    __shared__ FrameLds lds[FRAMES_PER_WG];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int u = blockIdx.y;
    const int t = blockIdx.x * FRAMES_PER_WG + wv;
    const int T = frames_of(n_samples[u], fl, step, (int)min(ld, (long long)INT32_MAX), Tmax);
    const bool live = t < T;                 // (no early return: the barriers below are reached by every wave)
    FrameLds& s = lds[wv];
    float* row = feat + ((long long)u * Tmax + min(t, Tmax - 1)) * D;

    // ---- the frame as 256 complex points z[m] = x[2m] + i x[2m+1], stored bit-reversed for the decimation-in-time stages
    const long long base = (long long)u * ld + (long long)t * step;
#pragma unroll
    for (int i = 0; i < NC / 64; ++i) {
        const int m = lane + 64 * i;
        float a = 0.f, b = 0.f;
        if (live) {
            if (I16) {
                const short* x = (const short*)samples + base;
                if (2 * m < fl) a = (float)x[2 * m] / 32767.0f;
                if (2 * m + 1 < fl) b = (float)x[2 * m + 1] / 32767.0f;
            } else {
                const float* x = (const float*)samples + base;
                if (2 * m < fl) a = x[2 * m];
                if (2 * m + 1 < fl) b = x[2 * m + 1];
            }
        }
        const int r = (int)(__brev((unsigned)m) >> 24);
        s.re[r] = a;
        s.im[r] = b;
    }
    __syncthreads();
    // ---- 8 radix-2 stages; the twiddle of butterfly j in a group of 2 * half points is exp(-2 pi i j / (2 half)) = tw[j * (256 / half)]
#pragma unroll
    for (int st = 0; st < 8; ++st) {
        const int half = 1 << st;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int b = lane + 64 * i;
            const int j = b & (half - 1);
            const int i0 = ((b >> st) << (st + 1)) + j, i1 = i0 + half;
            const int k = j << (8 - st);
            const float c = tw[2 * k], sn = tw[2 * k + 1];
            const float xr = s.re[i1], xi = s.im[i1];
            const float vr = c * xr - sn * xi, vi = c * xi + sn * xr;
            const float ur = s.re[i0], ui = s.im[i0];
            s.re[i0] = ur + vr; s.im[i0] = ui + vi;
            s.re[i1] = ur - vr; s.im[i1] = ui - vi;
        }
        __syncthreads();
    }
    // ---- real-FFT split: X[k] = E + W^k O,  E = (Z[k] + conj Z[256-k]) / 2,  O = (Z[k] - conj Z[256-k]) / 2i;  P[k] = |X[k]|^2 / 512
    float esum = 0.f;
#pragma unroll
    for (int i = 0; i <= NC / 64; ++i) {
        const int k = lane + 64 * i;
        if (k <= NC) {                        // i == 4: lane 0 alone (bin 256)
            const int ka = k & (NC - 1), kb = (NC - k) & (NC - 1);
            const float ar = s.re[ka], ai = s.im[ka], br = s.re[kb], bi = s.im[kb];
            const float er = 0.5f * (ar + br), ei = 0.5f * (ai - bi);
            const float orr = 0.5f * (ai + bi), oi = -0.5f * (ar - br);
            const float c = tw[2 * k], sn = tw[2 * k + 1];
            const float xr = er + (c * orr - sn * oi), xi = ei + (c * oi + sn * orr);
            const float p = (xr * xr + xi * xi) * (1.0f / NFFT);
            s.P[k] = p;
            esum += p;
        }
    }
    const float energy = wave_sum(esum);      // every lane is active here
    __syncthreads();
    // ---- mel filters on the VALU, each over its own bin range, bins in ascending order
    for (int j = lane; j < NF; j += 64) {
        const int lo = max(fb_range[2 * j], 0), hi = min(fb_range[2 * j + 1], NBINS - 1);
        const float* w = fb + (long long)j * NBINS;
        float acc = 0.f;
        for (int k = lo; k <= hi; ++k) acc = fmaf(s.P[k], w[k], acc);
        if (acc == 0.f) acc = ZERO_FLOOR;
        if (mfcc) s.lm[j] = logf(acc);
        else if (live) row[j] = acc;          // fbank: D == NF
    }
    __syncthreads();
    if (mfcc && lane < D) {
        float acc = 0.f;
        const float* w = dct + lane * NF;
        for (int j = 0; j < NF; ++j) acc = fmaf(w[j], s.lm[j], acc);
        if (lane == 0) acc = logf(energy == 0.f ? ZERO_FLOOR : energy);
        if (live) row[lane] = acc;
    }
    if (zero_tail && !live && t < Tmax)
        for (int c = lane; c < D; c += 64) row[c] = 0.f;
}

// block-wide sum of doubles for blockDim.x == 256, in a fixed order; every thread calls it and gets the result
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// one workgroup per (column c = blockIdx.x, utterance u = blockIdx.y): stats[u, c] = {mean, std + 2^-30}, in DOUBLE.  An fp32 mean is
// off by up to ulp(sum) / 4, and CMVN divides that by the column's spread: a column whose frames differ by 5e-3 around 2.35 (the log
// energy of two overlapping frames) came out 4.4e-5 from the float64 result.  The fp32 features are summed exactly enough in double.
__global__ __launch_bounds__(256) void frontend_stats_kernel(const float* __restrict__ feat, const int* __restrict__ n_samples, long long ld,
                                                             int Tmax, int fl, int step, int D, double* __restrict__ stats) {
    __shared__ double red[4];
    const int c = blockIdx.x, u = blockIdx.y;
    const int T = frames_of(n_samples[u], fl, step, (int)min(ld, (long long)INT32_MAX), Tmax);
    if (T < 1) return;                        // (uniform: the whole workgroup)
    const float* x = feat + (long long)u * Tmax * D + c;
    double a = 0.0;
    for (int t = threadIdx.x; t < T; t += 256) a += (double)x[(long long)t * D];
    const double mean = block_sum_f64(a, red) / (double)T;
    double q = 0.0;
    for (int t = threadIdx.x; t < T; t += 256) { const double d = (double)x[(long long)t * D] - mean; q = fma(d, d, q); }
    const double var = block_sum_f64(q, red) / (double)T;
    if (threadIdx.x == 0) {
        stats[2 * ((long long)u * D + c)] = mean;
        stats[2 * ((long long)u * D + c) + 1] = sqrt(var) + 9.313225746154785e-10;       // 2^-30
    }
}

// derivative_extraction(DeltaWindows = 2) at column c of a row of D values: sum_r (r * f[c + r] - f[c - r]) / 10, indices clamped (edge
// padding) -- r scales the forward term only, as the reference writes it
__device__ __forceinline__ float delta_at(const float* f, int c, int D) {
    const float p1 = f[min(c + 1, D - 1)], m1 = f[max(c - 1, 0)], p2 = f[min(c + 2, D - 1)], m2 = f[max(c - 2, 0)];
    return ((p1 - m1) + (2.0f * p2 - m2)) / 10.0f;
}

__global__ __launch_bounds__(256) void frontend_cmvn_delta_kernel(const float* __restrict__ feat, const double* __restrict__ stats,
                                                                  const int* __restrict__ n_samples, long long ld, int Tmax, int fl, int step,
                                                                  int D, float* __restrict__ out) {
    __shared__ float xs[4][MAX_FILTERS], d1[4][MAX_FILTERS];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int u = blockIdx.y, t = blockIdx.x * 4 + wv;
    const int T = frames_of(n_samples[u], fl, step, (int)min(ld, (long long)INT32_MAX), Tmax);
    const bool live = t < T;
    if (live)
        for (int c = lane; c < D; c += 64) {
            const double* sp = stats + 2 * ((long long)u * D + c);
            xs[wv][c] = (float)(((double)feat[((long long)u * Tmax + t) * D + c] - sp[0]) / sp[1]);
        }
    __syncthreads();
    if (live)
        for (int c = lane; c < D; c += 64) d1[wv][c] = delta_at(xs[wv], c, D);
    __syncthreads();
    if (t < Tmax) {
        float* o = out + ((long long)u * Tmax + t) * D * 3;
        for (int c = lane; c < D; c += 64) {
            o[3 * c] = live ? xs[wv][c] : 0.f;
            o[3 * c + 1] = live ? d1[wv][c] : 0.f;
            o[3 * c + 2] = live ? delta_at(d1[wv], c, D) : 0.f;
        }
    }
}

size_t raw_bytes(int n, int Tmax, int D) { return (((size_t)n * Tmax * D * 4) + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t las_frontend_workspace_bytes(int n, int Tmax, int feat_dim, int cmvn) {
    if (n < 1 || Tmax < 1 || feat_dim < 1 || !cmvn) return 0;
    return raw_bytes(n, Tmax, feat_dim) + (size_t)n * feat_dim * 2 * sizeof(double);
}

extern "C" int las_frontend(const las_frontend_args* a, void* stream) {
    LAS_ARG(a != nullptr, "las_frontend: null argument struct");
    LAS_ARG(a->n >= 1 && a->n <= 65535 && a->Tmax >= 1, "las_frontend: bad batch (n=%d, Tmax=%d)", a->n, a->Tmax);
    LAS_ARG(a->fl >= 1 && a->fl <= NFFT && a->step >= 1, "las_frontend: frame of %d samples every %d (1..%d samples, step >= 1)", a->fl, a->step, NFFT);
    LAS_ARG(a->feat_type == LAS_FEAT_MFCC || a->feat_type == LAS_FEAT_FBANK, "las_frontend: bad feat_type %d", a->feat_type);
    LAS_ARG(a->num_filters >= 1 && a->num_filters <= MAX_FILTERS, "las_frontend: num_filters=%d (1..%d)", a->num_filters, MAX_FILTERS);
    if (a->feat_type == LAS_FEAT_MFCC)
        LAS_ARG(a->feat_dim >= 1 && a->feat_dim <= a->num_filters && a->feat_dim <= 64 && a->dct, "las_frontend: mfcc feat_dim=%d (1..min(num_filters, 64), with a DCT table)", a->feat_dim);
    else
        LAS_ARG(a->feat_dim == a->num_filters, "las_frontend: fbank feat_dim=%d must equal num_filters=%d", a->feat_dim, a->num_filters);
    LAS_ARG(a->samples && a->n_samples && a->n_samples_host && a->twiddle && a->fb && a->fb_range && a->out, "las_frontend: null pointer");
    LAS_ARG(a->ld_samples >= a->fl && a->ld_samples <= INT32_MAX, "las_frontend: ld_samples=%lld", a->ld_samples);
    for (int u = 0; u < a->n; ++u) {
        const int nu = a->n_samples_host[u];
        LAS_ARG(nu >= a->fl && nu <= a->ld_samples, "las_frontend: utterance %d has %d samples (frame %d, pitch %lld)", u, nu, a->fl, a->ld_samples);
        const int T = (nu - a->fl) / a->step;
        LAS_ARG(T >= 1 && T <= a->Tmax, "las_frontend: utterance %d has %d frames (1..Tmax=%d)", u, T, a->Tmax);
    }
    const int D = a->feat_dim;
    const size_t need = las_frontend_workspace_bytes(a->n, a->Tmax, D, a->cmvn);
    LAS_ARG(!need || (a->ws && a->ws_bytes >= need), "las_frontend: workspace of %zu bytes, %zu needed", a->ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    float* raw = a->cmvn ? (float*)a->ws : a->out;
    const dim3 gf(cdiv(a->Tmax, FRAMES_PER_WG), a->n);
    const int mfcc = a->feat_type == LAS_FEAT_MFCC;
    if (a->samples_i16)
        hipLaunchKernelGGL(frontend_frames_kernel<true>, gf, dim3(64 * FRAMES_PER_WG), 0, st, a->samples, a->ld_samples, a->n_samples, a->Tmax, a->fl,
                           a->step, mfcc, D, a->num_filters, a->twiddle, a->fb, a->fb_range, a->dct, raw, a->cmvn ? 0 : 1);
    else
        hipLaunchKernelGGL(frontend_frames_kernel<false>, gf, dim3(64 * FRAMES_PER_WG), 0, st, a->samples, a->ld_samples, a->n_samples, a->Tmax, a->fl,
                           a->step, mfcc, D, a->num_filters, a->twiddle, a->fb, a->fb_range, a->dct, raw, a->cmvn ? 0 : 1);
    LAS_LAUNCHED();
    if (a->cmvn) {
        double* stats = (double*)((char*)a->ws + raw_bytes(a->n, a->Tmax, D));      // (raw_bytes is a multiple of 256)
        hipLaunchKernelGGL(frontend_stats_kernel, dim3(D, a->n), dim3(256), 0, st, raw, a->n_samples, a->ld_samples, a->Tmax, a->fl, a->step, D, stats);
        LAS_LAUNCHED();
        hipLaunchKernelGGL(frontend_cmvn_delta_kernel, dim3(cdiv(a->Tmax, 4), a->n), dim3(256), 0, st, raw, stats, a->n_samples, a->ld_samples,
                           a->Tmax, a->fl, a->step, D, a->out);
        LAS_LAUNCHED();
    }
    return 0;
}
