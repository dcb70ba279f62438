// bf_fft.h -- the windowed packed transform of the microphone-array units, beamform.hip (K18) and mvdr.hip (K19),
// in fp32 in LDS, and what their entry points share on the host.  Both units' test tolerances are measured on THIS arithmetic.
//   fft_tables_kernel  the caller's double tables (the window, exp(-2 pi i k / NF)) rounded to fp32 once, into the workspace
//   load_windowed      window times sample, two real samples to a complex point z[m] = x[2m] + i x[2m+1], zero-padded, stored bit-reversed
//   fft_lds[_batch]    a radix-2 decimation-in-time FFT of M = NF / 2 points, in place (input bit-reversed, output in order)
//   split_pt, split_at the real-FFT split: X[0 .. M] of the real sequence from its packed transform
//   unsplit_conj, store_unsplit, real_at   the way back: the Hermitian spectrum packed into M points (conjugated and bit-reversed: the
//                      inverse transform is the forward one between two conjugations), fft_lds again, and real sample i read out
// Everything here has internal linkage: each unit that includes the header gets its own tables kernel.
#pragma once
#include "las_common.h"
#include <limits.h>

namespace {

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// win [L] and tw [M + 1, 2] in double -> fp32; a grid of at least max(L, M + 1) threads
__global__ __launch_bounds__(256) void fft_tables_kernel(const double* __restrict__ win, const double* __restrict__ tw, int L, int M,
                                                         float* __restrict__ win_f, float2* __restrict__ tw_f) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < L) win_f[i] = (float)win[i];
    if (i <= M) tw_f[i] = make_float2((float)tw[2 * i], (float)tw[2 * i + 1]);
}

// the samples t0 .. t0 + 2 M - 1 of C rows (row c at x + row0 + c ld) times the window win_f [L], as C buffers of M = 2^lgM packed points,
// buffer c at z + c stride, stored bit-reversed.  Zero outside [0, n) of the row and beyond L; t0 may be negative.  (A caller with one
// row passes the literals C = 1, stride = 0, ld = 0: no row arithmetic is left in its loop.)
template <bool I16>
__device__ __forceinline__ void load_windowed(float2* z, int stride, int lgM, int C, const void* __restrict__ x, long long row0, long long ld,
                                              long long t0, long long n, int L, const float* __restrict__ win_f) {
    const int M = 1 << lgM;
    const long long end = min(n, t0 + L);             // the samples [max(0, t0), end) are read
    for (int e = threadIdx.x; e < (C << lgM); e += blockDim.x) {
        const int c = e >> lgM, m = e & (M - 1), i = 2 * m;
        const long long row = row0 + (long long)c * ld, s0 = t0 + i;
        float a = 0.f, b = 0.f;
        if (s0 >= 0 && s0 < end) a = win_f[i] * sample_at<I16>(x, row + s0);                         // (s0 < n <= ld: inside the row)
        if (s0 + 1 >= 0 && s0 + 1 < end) b = win_f[i + 1] * sample_at<I16>(x, row + s0 + 1);
        z[c * stride + (__brev((unsigned)m) >> (32 - lgM))] = make_float2(a, b);
    }
}

// butterfly b (0 <= b < M / 2) of stage st; tw[k] = exp(-2 pi i k / NF), NF = 2^lgNF >= 2 M
__device__ __forceinline__ void butterfly(float2* z, int b, int st, const float2* __restrict__ tw, int lgNF) {
    const int half = 1 << st, j = b & (half - 1);
    const int i0 = ((b >> st) << (st + 1)) + j, i1 = i0 + half;
    const float2 t = tw[j << (lgNF - 1 - st)];                        // exp(-2 pi i j / (2 half))
    const float2 v = cmul(t, z[i1]), u = z[i0];
    z[i0] = make_float2(u.x + v.x, u.y + v.y);
    z[i1] = make_float2(u.x - v.x, u.y - v.y);
}

// in-place FFT of M = 2^lgM complex points in LDS.  Every thread of the workgroup calls it; it ends with a barrier.
__device__ __forceinline__ void fft_lds(float2* z, int lgM, const float2* __restrict__ tw, int lgNF) {
    const int nb = 1 << (lgM - 1);
    for (int st = 0; st < lgM; ++st) {
        for (int b = threadIdx.x; b < nb; b += blockDim.x) butterfly(z, b, st, tw, lgNF);
        __syncthreads();
    }
}

// fft_lds over `count` buffers of M points, buffer c at z + c * stride: the butterflies of all buffers share the stages' barriers
__device__ __forceinline__ void fft_lds_batch(float2* z, int lgM, int count, int stride, const float2* __restrict__ tw, int lgNF) {
    const int nb = 1 << (lgM - 1), total = count << (lgM - 1);
    for (int st = 0; st < lgM; ++st) {
        for (int e = threadIdx.x; e < total; e += blockDim.x) butterfly(z + (e >> (lgM - 1)) * stride, e & (nb - 1), st, tw, lgNF);
        __syncthreads();
    }
}

// X[k] of the real sequence from the points a = Z[k], b = Z[M - k] of its packed transform and t = tw[k]: X = E + W^k O,
// E = (a + conj b) / 2, O = (a - conj b) / 2i
__device__ __forceinline__ float2 split_pt(float2 a, float2 b, float2 t) {
    const float2 e = make_float2(0.5f * (a.x + b.x), 0.5f * (a.y - b.y));
    const float2 o = make_float2(0.5f * (a.y + b.y), -0.5f * (a.x - b.x));
    const float2 wo = cmul(t, o);
    return make_float2(e.x + wo.x, e.y + wo.y);
}
// X[k], 0 <= k <= M, from the buffer
__device__ __forceinline__ float2 split_at(const float2* Z, int k, int M, const float2* __restrict__ tw) {
    return split_pt(Z[k & (M - 1)], Z[(M - k) & (M - 1)], tw[k]);
}

// the packed point k of the inverse transform, conjugated: conj(E + i O), E = (Ga + conj Gb) / 2, O = (Ga - conj Gb) / 2 conj(tw[k]);
// Ga = G[k], Gb = G[M - k]
__device__ __forceinline__ float2 unsplit_conj(float2 ga, float2 gb, float2 t) {
    const float2 e = make_float2(0.5f * (ga.x + gb.x), 0.5f * (ga.y - gb.y));
    const float2 h = make_float2(0.5f * (ga.x - gb.x), 0.5f * (ga.y + gb.y));
    const float2 o = cmul(h, make_float2(t.x, -t.y));
    return make_float2(e.x - o.y, -(e.y + o.x));
}
// the un-split points zk (of k, 0 <= k <= M / 2) and zm (of M - k) to their bit-reversed slots; k = 0 and k = M / 2 are one point each
__device__ __forceinline__ void store_unsplit(float2* B, int lgM, int k, float2 zk, float2 zm) {
    const int M = 1 << lgM;
    B[__brev((unsigned)k) >> (32 - lgM)] = zk;
    if (k > 0 && k < M - k) B[__brev((unsigned)(M - k)) >> (32 - lgM)] = zm;
}
// real sample i, 0 <= i < 2 M, of the inverse transform once fft_lds has run over the stored points: B = conj(M x), x[2m] = Re B[m] / M,
// x[2m+1] = -Im B[m] / M; scale = 1 / M
__device__ __forceinline__ float real_at(const float2* B, int i, float scale) {
    const float2 v = B[i >> 1];
    return ((i & 1) ? -v.y : v.x) * scale;
}

// ---- the host side of the entry points ------------------------------------------------------------------------------------------------
int log2_of(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
bool pow2_in(int v, int lo, int hi) { return v >= lo && v <= hi && (v & (v - 1)) == 0; }

// the tables' slice of a workspace: [tw fp32 [NF/2 + 1, 2] | win fp32 [NF]] from byte o on; -> the byte behind it
struct TableSlice { size_t tw, win; };
size_t table_slice(size_t o, int NF, TableSlice& s) {
    s.tw = o;  o += align256(((size_t)NF / 2 + 1) * sizeof(float2));
    s.win = o; o += align256((size_t)NF * sizeof(float));
    return o;
}
struct Tables { float2* tw; float* win; };
// rounds the caller's window [L] and twiddles [NF/2 + 1, 2] into the slice, on the stream
int tables_launch(const double* win, const double* twiddle, int L, int NF, void* ws, const TableSlice& s, hipStream_t st, Tables& t) {
    t.tw = (float2*)((char*)ws + s.tw);
    t.win = (float*)((char*)ws + s.win);
    hipLaunchKernelGGL(fft_tables_kernel, dim3(cdiv(NF, 256)), dim3(256), 0, st, win, twiddle, L, NF / 2, t.win, t.tw);
    LAS_LAUNCHED();
    return 0;
}

// the statement with I16 a constant: the instantiation of a <bool I16> kernel or launcher that the caller's x_i16 picks
#define WITH_I16(x_i16, ...)                                                          \
    do { if (x_i16) { constexpr bool I16 = true; __VA_ARGS__; } else { constexpr bool I16 = false; __VA_ARGS__; } } while (0)
// both instantiations of a <bool I16> kernel may use `bytes` of dynamic LDS: set once per process
#define RAISE_LDS_I16(kernel, bytes)                                                                                                        \
    do {                                                                                                                                    \
        static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                                   (int)(bytes)) |                                                                          \
                          (int)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                                   (int)(bytes));                                                                           \
        LAS_ARG(attr == 0, "hipFuncSetAttribute(" #kernel ") failed: %d", attr);                                                            \
    } while (0)
// the refusals every entry point words the same way; `name` is the entry point's
#define ARG_ROWS(name, n, ld) \
    LAS_ARG(n >= 1 && n <= ld && ld <= INT32_MAX, name ": n=%lld samples in rows of ld=%lld (1 <= n <= ld <= INT32_MAX)", n, ld)
#define ARG_REF(name, ref, C) LAS_ARG(ref >= 0 && ref < C, name ": ref=%d outside the %d channels", ref, C)
#define ARG_WS(name, ws, ws_bytes, need)                                                                          \
    do {                                                                                                          \
        LAS_ARG((need) && ws_bytes >= (need), name ": workspace of %zu bytes, %zu needed", ws_bytes, (size_t)(need)); \
        LAS_ARG(((uintptr_t)ws & 7) == 0, name ": ws is 8-byte aligned");                                         \
    } while (0)

}  // namespace
