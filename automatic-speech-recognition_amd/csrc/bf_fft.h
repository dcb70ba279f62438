// bf_fft.h -- the fp32 transform in LDS that beamform.hip (K18) and mvdr.hip (K19) share: a radix-2 decimation-in-time FFT of packed real
// input, the real-FFT split and its inverse.  The K18 functions stand here as they stood in beamform.hip (its tolerances were measured
// on this arithmetic); fft_lds_batch is the same butterfly over several buffers at once.
#pragma once
#include "las_common.h"

template <bool I16>
__device__ __forceinline__ float sample_at(const void* __restrict__ x, long long i) {
    if (I16) return (float)((const short*)x)[i] / 32767.0f;
    return ((const float*)x)[i];
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// in-place radix-2 decimation-in-time FFT of M = 2^lgM complex points in LDS (input bit-reversed, output in order); tw[k] = exp(-2 pi i
// k / NF), NF = 2^lgNF >= 2 M.  Every thread of the workgroup calls it; it ends with a barrier.
__device__ __forceinline__ void fft_lds(float2* z, int lgM, const float2* __restrict__ tw, int lgNF) {
    const int nb = 1 << (lgM - 1);
    for (int st = 0; st < lgM; ++st) {
        const int half = 1 << st;
        for (int b = threadIdx.x; b < nb; b += blockDim.x) {
            const int j = b & (half - 1);
            const int i0 = ((b >> st) << (st + 1)) + j, i1 = i0 + half;
            const float2 t = tw[j << (lgNF - 1 - st)];                // exp(-2 pi i j / (2 half))
            const float2 v = cmul(t, z[i1]), u = z[i0];
            z[i0] = make_float2(u.x + v.x, u.y + v.y);
            z[i1] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
}

// fft_lds over `count` buffers of M points, buffer c at z + c * stride: the butterflies of all buffers share the stages' barriers
__device__ __forceinline__ void fft_lds_batch(float2* z, int lgM, int count, int stride, const float2* __restrict__ tw, int lgNF) {
    const int nb = 1 << (lgM - 1), total = count << (lgM - 1);
    for (int st = 0; st < lgM; ++st) {
        const int half = 1 << st;
        for (int e = threadIdx.x; e < total; e += blockDim.x) {
            const int b = e & (nb - 1);
            float2* zc = z + (e >> (lgM - 1)) * stride;
            const int j = b & (half - 1);
            const int i0 = ((b >> st) << (st + 1)) + j, i1 = i0 + half;
            const float2 t = tw[j << (lgNF - 1 - st)];
            const float2 v = cmul(t, zc[i1]), u = zc[i0];
            zc[i0] = make_float2(u.x + v.x, u.y + v.y);
            zc[i1] = make_float2(u.x - v.x, u.y - v.y);
        }
        __syncthreads();
    }
}

// X[k], 0 <= k <= M, of the real sequence whose packed transform is Z: X = E + W^k O, E = (Z[k] + conj Z[M-k]) / 2, O = (Z[k] - conj Z[M-k]) / 2i
__device__ __forceinline__ float2 split_at(const float2* Z, int k, int M, const float2* __restrict__ tw) {
    const float2 a = Z[k & (M - 1)], b = Z[(M - k) & (M - 1)];
    const float2 e = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
    const float2 o = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));
    const float2 wo = cmul(tw[k], o);
    return make_float2(e.x + wo.x, e.y + wo.y);
}

// the packed point k of the inverse transform, conjugated: conj(E + i O), E = (Ga + conj Gb) / 2, O = (Ga - conj Gb) / 2 conj(tw[k]);
// Ga = G[k], Gb = G[M - k]
__device__ __forceinline__ float2 unsplit_conj(float2 ga, float2 gb, float2 t) {
    const float2 e = make_float2(0.5f * (ga.x + gb.x), 0.5f * (ga.y - gb.y));
    const float2 h = make_float2(0.5f * (ga.x - gb.x), 0.5f * (ga.y + gb.y));
    const float2 o = cmul(h, make_float2(t.x, -t.y));
    return make_float2(e.x - o.y, -(e.y + o.x));
}
