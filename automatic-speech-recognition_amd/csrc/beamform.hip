// beamform.hip -- microphone arrays in front of everything else (las_hip.h K18): BeamformIt's scheme (Anguera et al. 2007)
// without its N-best lists.  One recording [C, n] per call, windows of L samples every H = L / 2:
//   las_gcc_phat    r[c, w, D + tau] = the PHAT-weighted cross-correlation of channel c with the reference channel at lag tau
//   las_tdoa_track  a Viterbi pass over the windows per channel (score r, a linear penalty on lag jumps) -> tau[c, w], and the
//                   channel weights a[c, w] from the correlation at the tracked lag
//   las_delay_sum   y[t] = the channels shifted by tau, weighted by a and summed, cross-faded linearly between window centres
// Everything runs on the caller's stream; no atomics, no cross-workgroup synchronisation: every output value is computed by one
// thread in a fixed order, so two calls give the same bits.
//
// The windowed transform (the fp32 tables, the packed loader, the FFT in LDS, the real-FFT split and the way back) is bf_fft.h's,
// shared with mvdr.hip.
//   bf_gcc_kernel      one workgroup per WINDOW, which keeps the window's channels to itself (the alternative -- spectra through the
//                      workspace, a grid over (window, channel) -- is in DESIGN 7v with what it would cost).  Two LDS buffers of NF / 2
//                      complex fp32 points (64 KiB each at NF = 16384): A holds the reference channel's spectrum X_ref[0 .. NF/2],
//                      computed once per window; B is the work buffer.  Per channel: the window is loaded and transformed in B, the
//                      split gives X_c[k] and X_c[NF/2 - k] in registers, G = X_c conj X_ref / max(|.|, 1e-12), the Hermitian G is
//                      packed back into B (through registers: B is source and destination), transformed again and the lags
//                      -D .. D are read out.  The reference channel's own row skips the forward transform (its spectrum is A) and
//                      is otherwise computed like any other.  2 C transforms per window.
//   bf_track_kernel    one WAVE per channel steps through the windows, score in LDS in double.  The linear penalty splits the
//                      maximisation into two sweeps: the best predecessor s' <= s maximises u[s'] = score[s'] + gamma s' (a prefix
//                      maximum), the best s' >= s maximises score[s'] - gamma s' (a suffix maximum).  Both are wave scans (six
//                      DPP steps per 64 states, a carry between the groups of 64) that carry the ARGUMENT: the scans only pick
//                      the two candidates, whose values are then computed as the contract writes them, score[s'] - gamma |s - s'|
//                      with ONE rounded product and ONE rounded difference, and compared.  The tie rule (smaller |s - s'|, then
//                      smaller s') is the scans' direction: the prefix scan keeps the last of equal maxima, the suffix scan the
//                      first, and of two equal candidates the nearer, then the left one wins.  Where gamma s' and the sums
//                      are exact (the exact-operand test: r in multiples of 2^-10, gamma = 2^-7) this is the plain maximum over
//                      all predecessors bit for bit, ties included; elsewhere u is rounded where the plain form is not, and
//                      two predecessors whose values differ by a rounding of u may swap -- the value kept is then within two
//                      roundings of the maximum (tests/test_beamform_host.py holds the paths of its recording 1e-4 away from such
//                      a swap).  Every product, sum and difference of the recursion is __dmul_rn / __dadd_rn / __dsub_rn: THAT is
//                      how this file keeps the compiler from contracting them into an fma (the exact-operand test depends on
//                      it).  One wave, because the windows are sequential and a wave needs no barrier to scan: the hour of 8
//                      channels takes 67 ms (profiles/beamform_bench.json), 6 times las_gcc_phat, all of it latency.  Rows of r are staged eight windows ahead (one memory round trip per
//                      eight windows); back-pointers go to the workspace as int16 (S <= 1025); the backtrack reads them back a
//                      chunk of windows at a time into LDS, where one lane walks the chunk, and all lanes write the chunk's lags.
//   bf_weights_kernel  one thread per window: q, the reference's share, the sum in channel order, all in double.
//   bf_sum_kernel      streaming: four outputs per thread, one 16-byte store.  Where the four outputs lie between the same two window
//                      centres (all but one thread per hop) the lags and weights are read once per channel and a lag that is a
//                      multiple of four samples reads its fp32 row with one 16-byte load; other lags read four dwords (a wave
//                      still covers whole cache lines).  A row is read twice, for the two windows of the cross-fade, the second
//                      time from cache.
#include "las_common.h"
#include "bf_fft.h"
#include <math.h>
#include <limits.h>

namespace {

constexpr int MAX_C = LAS_BF_MAX_CHANNELS, MAX_NF = LAS_BF_MAX_FFT, MAX_LAG = LAS_BF_MAX_LAG;
constexpr int NT_MAX = 1024;
constexpr int PAIRS = 5;                              // (k, NF/2 - k) pairs per thread: NF/4 + 1 pairs over max(64, NF/16) threads
constexpr int BP_CHUNK_ENTRIES = 16384;               // back-pointers staged per backtrack chunk (32 KiB of LDS)
constexpr int TRACK_ROWS = 8;                         // rows of r the tracker stages ahead
constexpr float PHAT_EPS = 1e-12f;

__device__ __forceinline__ float2 phat(float2 xc, float2 xr) {
    const float2 p = make_float2(xc.x * xr.x + xc.y * xr.y, xc.y * xr.x - xc.x * xr.y);      // xc conj(xr)
    const float inv = 1.0f / fmaxf(sqrtf(p.x * p.x + p.y * p.y), PHAT_EPS);
    return make_float2(p.x * inv, p.y * inv);
}

template <bool I16>
__global__ __launch_bounds__(NT_MAX) void bf_gcc_kernel(const void* __restrict__ x, long long ld, int C, long long n, int ref, int L, int D,
                                                        int lgNF, const float* __restrict__ hann_f, const float2* __restrict__ tw,
                                                        float* __restrict__ r, long long Wn) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bf_lds[];
    const int lgM = lgNF - 1, M = 1 << lgM, NF = 1 << lgNF, S = 2 * D + 1;
    float2* A = (float2*)bf_lds;                      // [M + 1] the reference spectrum (+ 1 of padding)
    float2* B = A + (M + 2);                          // [M]     the work buffer
    const long long w = blockIdx.x, t0 = w * (L / 2);
    const int tid = threadIdx.x, nt = blockDim.x;

    load_windowed<I16>(B, 0, lgM, 1, x, (long long)ref * ld, 0, t0, n, L, hann_f);
    __syncthreads();
    fft_lds(B, lgM, tw, lgNF);
    for (int k = tid; k <= M; k += nt) A[k] = split_at(B, k, M, tw);
    for (int c = 0; c < C; ++c) {                     // (uniform)
        __syncthreads();                              // B's readers (the split above, the previous channel's read-out) are through
        if (c != ref) {
            load_windowed<I16>(B, 0, lgM, 1, x, (long long)c * ld, 0, t0, n, L, hann_f);
            __syncthreads();
            fft_lds(B, lgM, tw, lgNF);
        }
        float2 zk[PAIRS], zm[PAIRS];
#pragma unroll
        for (int i = 0; i < PAIRS; ++i) {
            const int k = tid + i * nt;
            if (k <= M / 2) {
                const float2 xk = c == ref ? A[k] : split_at(B, k, M, tw), xm = c == ref ? A[M - k] : split_at(B, M - k, M, tw);
                const float2 gk = phat(xk, A[k]), gm = phat(xm, A[M - k]);
                zk[i] = unsplit_conj(gk, gm, tw[k]);
                zm[i] = unsplit_conj(gm, gk, tw[M - k]);
            }
        }
        __syncthreads();                              // every point of B has been read into registers
#pragma unroll
        for (int i = 0; i < PAIRS; ++i) {
            const int k = tid + i * nt;
            if (k <= M / 2) store_unsplit(B, lgM, k, zk[i], zm[i]);
        }
        __syncthreads();
        fft_lds(B, lgM, tw, lgNF);
        const float scale = 1.0f / (float)M;
        float* out = r + ((long long)c * Wn + w) * S;
        for (int j = tid; j < S; j += nt) out[j] = real_at(B, (j - D) & (NF - 1), scale);     // lag mod NF
    }
}

// one step of the prefix scan: the lane's partner (a DPP pattern; a lane without one keeps its own value) wins only when strictly greater
template <int CTRL, int ROWS>
__device__ __forceinline__ void scan_step(double& v, int& a) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const int plo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROWS, 0xf, false);
    const int phi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, ROWS, 0xf, false);
    const int pa = __builtin_amdgcn_update_dpp(a, a, CTRL, ROWS, 0xf, false);
    const double pv = __hiloint2double(phi, plo);
    if (pv > v) { v = pv; a = pa; }
}
// inclusive prefix maximum over the wave's lanes together with its argument; of equal values the one in the HIGHER lane stays.  Inside
// a row of 16 lanes by row_shr 1, 2, 4, 8; then lane 15 of rows 0 and 2 goes to rows 1 and 3 (row_bcast:15), then lane 31 to rows 2
// and 3 (row_bcast:31): VALU moves, no round trip through the LDS queue.  EVERY lane must be active.
__device__ __forceinline__ void wave_prefix_max(double& v, int& a) {
    scan_step<0x111, 0xf>(v, a); scan_step<0x112, 0xf>(v, a); scan_step<0x114, 0xf>(v, a); scan_step<0x118, 0xf>(v, a);
    scan_step<0x142, 0xa>(v, a); scan_step<0x143, 0xc>(v, a);
}
__device__ __forceinline__ double lane63(double v) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

struct TrackLds { size_t p, argf, argb, path, buf, total; };
__host__ __device__ inline TrackLds track_lds(int S, int K) {
    TrackLds t;
    size_t o = 0;
    t.p = o;    o += (size_t)2 * S * sizeof(double);                  // this window's scores and the next one's
    t.argf = o; o += (size_t)S * sizeof(int);
    t.argb = o; o += (size_t)S * sizeof(int);
    t.path = o; o += ((size_t)K + 2) * sizeof(int);
    t.buf = o;                                                        // TRACK_ROWS rows of r ahead; later a chunk of back-pointers
    const size_t rows = (size_t)TRACK_ROWS * S * sizeof(float), chunk = (size_t)K * S * sizeof(short);
    o += rows > chunk ? rows : chunk;
    t.total = (o + 15) & ~(size_t)15;
    return t;
}

__global__ __launch_bounds__(64) void bf_track_kernel(const float* __restrict__ r, long long Wn, int D, int ref, double gamma, int K,
                                                      short* __restrict__ bp, int* __restrict__ tau) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bf_lds[];
    const int S = 2 * D + 1, E = (S + 63) >> 6, lane = threadIdx.x, c = blockIdx.x;
    const TrackLds lay = track_lds(S, K);
    double* p = (double*)(bf_lds + lay.p);            // score of the previous window
    double* pn = p + S;                               // ... of this one
    int* argf = (int*)(bf_lds + lay.argf);
    int* argb = (int*)(bf_lds + lay.argb);
    int* path = (int*)(bf_lds + lay.path);            // [K] the chunk's lags, [K] the state carried between chunks
    float* rows = (float*)(bf_lds + lay.buf);
    short* chunk = (short*)(bf_lds + lay.buf);
    int* tc = tau + (long long)c * Wn;
    if (c == ref) {                                   // (uniform)
        for (long long w = lane; w < Wn; w += 64) tc[w] = 0;
        return;
    }
    const float* rc = r + (long long)c * Wn * S;
    short* bpc = bp + (long long)c * Wn * S;
    for (int s = lane; s < S; s += 64) p[s] = (double)rc[s];
    __syncthreads();
    for (long long w = 1; w < Wn; ++w) {
        const int slot = (int)((w - 1) % TRACK_ROWS);
        if (slot == 0) {                              // the next rows of r, one memory round trip for TRACK_ROWS windows
            const int nr = (int)min((long long)TRACK_ROWS, Wn - w);
#pragma unroll 8
            for (int i = lane; i < nr * S; i += 64) rows[i] = rc[w * S + i];      // (unrolled: eight loads in flight, not one)
            __syncthreads();
        }
        // from the left: the best predecessor s' <= s maximises u[s'] = score[s'] + gamma s'; of equal ones the LAST (the nearest)
        double cv = -INFINITY;
        int ca = 0;
        for (int i = 0; i < E; ++i) {                 // (uniform)
            const int s = i * 64 + lane;
            double v = s < S ? __dadd_rn(p[s], __dmul_rn(gamma, (double)s)) : -INFINITY;
            int a = s;
            wave_prefix_max(v, a);
            if (cv > v) { v = cv; a = ca; }
            if (s < S) argf[s] = a;
            cv = lane63(v);
            ca = __builtin_amdgcn_readlane(a, 63);
        }
        // from the right: s' >= s maximises score[s'] - gamma s'; of equal ones the FIRST (the nearest).  The lanes hold the states in
        // descending order, so the suffix maximum over the states is the same prefix scan over the lanes
        cv = -INFINITY;
        ca = 0;
        for (int i = E - 1; i >= 0; --i) {
            const int s = i * 64 + 63 - lane;
            double v = s < S ? __dsub_rn(p[s], __dmul_rn(gamma, (double)s)) : -INFINITY;
            int a = s;
            wave_prefix_max(v, a);
            if (cv > v) { v = cv; a = ca; }
            if (s < S) argb[s] = a;
            cv = lane63(v);
            ca = __builtin_amdgcn_readlane(a, 63);
        }
        lds_barrier();                                // argb[s] was written by the lane that held s in the descending order, not by its reader
        // the two candidates in the contract's arithmetic; equal values go to the nearer, then to the one on the left
        for (int s = lane; s < S; s += 64) {
            const int jf = argf[s], jb = argb[s];
            const double vf = __dsub_rn(p[jf], __dmul_rn(gamma, (double)(s - jf)));
            const double vb = __dsub_rn(p[jb], __dmul_rn(gamma, (double)(jb - s)));
            const bool right = vb > vf || (vb == vf && jb - s < s - jf);
            pn[s] = (double)rows[slot * S + s] + (right ? vb : vf);
            bpc[w * S + s] = (short)(right ? jb : jf);
        }
        lds_barrier();                                // (orders the LDS traffic only: the back-pointer stores stay in flight)
        double* t = p; p = pn; pn = t;
    }
    if (lane == 0) {                                  // the last window's best state: ties to the smaller |tau|, then the smaller tau
        int bs = 0;
        double bv = p[0];
        for (int s = 1; s < S; ++s) {
            const double v = p[s];
            const int da = abs(s - D), db = abs(bs - D);
            if (v > bv || (v == bv && (da < db || (da == db && s < bs)))) { bv = v; bs = s; }
        }
        path[K] = bs;
    }
    __syncthreads();                                  // (also: this workgroup's back-pointer stores are visible to all its threads)
    for (long long w1 = Wn; w1 > 0; w1 -= K) {
        const long long w0 = max(0ll, w1 - K);
        const int nr = (int)(w1 - w0);
#pragma unroll 8
        for (int i = lane; i < nr * S; i += 64) chunk[i] = bpc[w0 * S + i];   // (unrolled: eight loads in flight; window 0's row is never
        __syncthreads();                                                      //  written and never followed)
        if (lane == 0) {
            int cur = path[K];
            for (int i = nr - 1; i >= 0; --i) {
                path[i] = cur - D;
                if (w0 + i > 0) cur = chunk[i * S + cur];
            }
            path[K] = cur;
        }
        __syncthreads();
        for (int i = lane; i < nr; i += 64) tc[w0 + i] = path[i];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void bf_weights_kernel(const float* __restrict__ r, const int* __restrict__ tau, int C, long long Wn, int D, int ref,
                                                         float* __restrict__ a) {
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w >= Wn) return;
    const int S = 2 * D + 1;
    double q[MAX_C];
    double qref = 0.0;
#pragma unroll
    for (int c = 0; c < MAX_C; ++c) {
        q[c] = 0.0;
        if (c < C && c != ref) {
            const int t = tau[(long long)c * Wn + w];
            q[c] = fmax(0.0, (double)r[((long long)c * Wn + w) * S + D + t]);
            qref = fmax(qref, q[c]);
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int c = 0; c < MAX_C; ++c)
        if (c < C) { if (c == ref) q[c] = qref; sum += q[c]; }
#pragma unroll
    for (int c = 0; c < MAX_C; ++c)
        if (c < C) a[(long long)c * Wn + w] = sum > 0.0 ? (float)(q[c] / sum) : (c == ref ? 1.f : 0.f);
}

// the cross-fade of sample t: the window w0 on the left, its weight 1 - f; the window on the right is min(w0 + 1, Wn - 1)
__device__ __forceinline__ void fade_at(long long t, int H, long long Wn, long long& w0, float& f) {
    if (t < H) { w0 = 0; f = 0.f; return; }
    const long long q = t - H;
    w0 = q / H;
    f = (float)(q - w0 * H) / (float)H;
    if (w0 >= Wn - 1) { w0 = Wn - 1; f = 0.f; }
}

template <bool I16>
__device__ __forceinline__ float shifted(const void* __restrict__ x, long long row, long long i, long long n) {
    return (i >= 0 && i < n) ? sample_at<I16>(x, row + i) : 0.f;
}

template <bool I16>
__global__ __launch_bounds__(256) void bf_sum_kernel(const void* __restrict__ x, long long ld, int C, long long n, int H, long long Wn,
                                                     const int* __restrict__ tau, const float* __restrict__ a, float* __restrict__ y) {
    const long long t = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (t >= n) return;
    long long wa, wb;
    float fa, fb;
    fade_at(t, H, Wn, wa, fa);
    fade_at(min(t + 3, n - 1), H, Wn, wb, fb);
    float out[4];
    if (wa == wb && t + 3 < n) {                      // the four samples share their two windows
        const long long w0 = wa, w1 = min(w0 + 1, Wn - 1);
        float z0[4] = {0.f, 0.f, 0.f, 0.f}, z1[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < C; ++c) {
            const long long row = (long long)c * ld;
            const int t0 = tau[(long long)c * Wn + w0], t1 = tau[(long long)c * Wn + w1];
            const float a0 = a[(long long)c * Wn + w0], a1 = a[(long long)c * Wn + w1];
            float v0[4], v1[4];
            const long long i0 = t + t0, i1 = t + t1;
            if (!I16 && ((row + i0) & 3) == 0 && i0 >= 0 && i0 + 3 < n && (((uintptr_t)x) & 15) == 0) {
                const float4 v = *(const float4*)((const float*)x + row + i0);
                v0[0] = v.x; v0[1] = v.y; v0[2] = v.z; v0[3] = v.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v0[j] = shifted<I16>(x, row, i0 + j, n);
            }
            if (t1 == t0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) v1[j] = v0[j];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) v1[j] = shifted<I16>(x, row, i1 + j, n);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { z0[j] = fmaf(a0, v0[j], z0[j]); z1[j] = fmaf(a1, v1[j], z1[j]); }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            long long wj;
            float f;
            fade_at(t + j, H, Wn, wj, f);
            out[j] = (1.0f - f) * z0[j] + f * z1[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            out[j] = 0.f;
            if (t + j < n) {
                long long w0;
                float f;
                fade_at(t + j, H, Wn, w0, f);
                const long long w1 = min(w0 + 1, Wn - 1);
                float z0 = 0.f, z1 = 0.f;
                for (int c = 0; c < C; ++c) {
                    const long long row = (long long)c * ld;
                    z0 = fmaf(a[(long long)c * Wn + w0], shifted<I16>(x, row, t + j + tau[(long long)c * Wn + w0], n), z0);
                    z1 = fmaf(a[(long long)c * Wn + w1], shifted<I16>(x, row, t + j + tau[(long long)c * Wn + w1], n), z1);
                }
                out[j] = (1.0f - f) * z0 + f * z1;
            }
        }
    }
    if (t + 3 < n && (((uintptr_t)y) & 15) == 0) {
        *(float4*)(y + t) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
        for (int j = 0; j < 4 && t + j < n; ++j) y[t + j] = out[j];
    }
}

// the workspace: [back-pointers int16 [C, Wn, 2 D + 1] (las_tdoa_track) | tw fp32 [NF/2 + 1, 2] | hann fp32 [NF] (las_gcc_phat)]
struct Layout { size_t bp; TableSlice tab; size_t total; };
Layout layout(int C, long long Wn, int NF, int D) {
    Layout l;
    l.bp = 0;
    l.total = table_slice(align256((size_t)C * Wn * (2 * (size_t)D + 1) * sizeof(short)), NF, l.tab);
    return l;
}

bool geometry_ok(int C, int L, int D, int NF) {
    return C >= 2 && C <= MAX_C && L >= 2 && (L & 1) == 0 && D >= 1 && D <= MAX_LAG && pow2_in(NF, 4, MAX_NF) && (long long)L + D <= NF;
}
int track_chunk(int S) { return clampi(BP_CHUNK_ENTRIES / S, 1, 1024); }   // windows per backtrack chunk

}  // namespace

extern "C" long long las_bf_windows(long long n, int L) {
    if (n < 1 || L < 2 || (L & 1)) return -1;
    const long long H = L / 2;
    return n <= L ? 1 : (n - L + H - 1) / H + 1;
}

extern "C" size_t las_bf_workspace_bytes(int C, long long Wn, int NF, int D) {
    if (C < 2 || C > MAX_C || Wn < 1 || Wn > INT32_MAX || !pow2_in(NF, 4, MAX_NF) || D < 1 || D > MAX_LAG) return 0;
    return layout(C, Wn, NF, D).total;
}

extern "C" int las_gcc_phat(const void* x, int x_i16, long long ld, int C, long long n, int ref, int L, int D, int NF, const double* hann,
                            const double* twiddle, float* r, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(x && hann && twiddle && r && ws, "las_gcc_phat: null pointer (x, hann, twiddle, r, ws)");
    LAS_ARG(geometry_ok(C, L, D, NF), "las_gcc_phat: bad geometry (C=%d, 2..%d; L=%d, even, >= 2; D=%d, 1..%d; NF=%d, a power of two with "
            "L + D <= NF <= %d)", C, MAX_C, L, D, MAX_LAG, NF, MAX_NF);
    ARG_ROWS("las_gcc_phat", n, ld);
    ARG_REF("las_gcc_phat", ref, C);
    const long long Wn = las_bf_windows(n, L);
    ARG_WS("las_gcc_phat", ws, ws_bytes, las_bf_workspace_bytes(C, Wn, NF, D));
    const int M = NF / 2, lgNF = log2_of(NF);
    const size_t lds = (size_t)(2 * M + 2) * sizeof(float2);
    RAISE_LDS_I16(bf_gcc_kernel, (2 * (MAX_NF / 2) + 2) * sizeof(float2));
    hipStream_t st = (hipStream_t)stream;
    Tables t;
    if (const int rc = tables_launch(hann, twiddle, L, NF, ws, layout(C, Wn, NF, D).tab, st, t)) return rc;
    const int nt = clampi(M / 8, 64, NT_MAX);
    WITH_I16(x_i16, hipLaunchKernelGGL(bf_gcc_kernel<I16>, dim3((unsigned)Wn), dim3(nt), lds, st, x, ld, C, n, ref, L, D, lgNF, t.win, t.tw, r, Wn));
    LAS_LAUNCHED();
    return 0;
}

extern "C" int las_tdoa_track(const float* r, int C, long long Wn, int D, int ref, double gamma, int* tau, float* a, void* ws, size_t ws_bytes,
                              void* stream) {
    LAS_ARG(r && tau && a && ws, "las_tdoa_track: null pointer (r, tau, a, ws)");
    LAS_ARG(C >= 2 && C <= MAX_C && D >= 1 && D <= MAX_LAG && Wn >= 1 && Wn <= INT32_MAX, "las_tdoa_track: bad geometry (C=%d, 2..%d; D=%d, "
            "1..%d; Wn=%lld, >= 1)", C, MAX_C, D, MAX_LAG, Wn);
    ARG_REF("las_tdoa_track", ref, C);
    LAS_ARG(isfinite(gamma) && gamma >= 0.0, "las_tdoa_track: gamma=%g (finite, >= 0)", gamma);
    ARG_WS("las_tdoa_track", ws, ws_bytes, layout(C, Wn, 4, D).tab.tw);      // (the back-pointers lead the workspace, whatever NF it was sized for)
    short* bp = (short*)ws;
    const int S = 2 * D + 1, K = track_chunk(S);
    const size_t lds = track_lds(S, K).total;         // (at most 62 KiB, at 2 D + 1 = 1025: no attribute to raise)
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bf_track_kernel, dim3(C), dim3(64), lds, st, r, Wn, D, ref, gamma, K, bp, tau);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(bf_weights_kernel, dim3(cdiv(Wn, 256)), dim3(256), 0, st, r, tau, C, Wn, D, ref, a);
    LAS_LAUNCHED();
    return 0;
}

extern "C" int las_delay_sum(const void* x, int x_i16, long long ld, int C, long long n, int L, long long Wn, const int* tau, const float* a,
                             float* y, void* stream) {
    LAS_ARG(x && tau && a && y, "las_delay_sum: null pointer (x, tau, a, y)");
    LAS_ARG(C >= 2 && C <= MAX_C && L >= 2 && (L & 1) == 0, "las_delay_sum: bad geometry (C=%d, 2..%d; L=%d, even, >= 2)", C, MAX_C, L);
    ARG_ROWS("las_delay_sum", n, ld);
    LAS_ARG(Wn == las_bf_windows(n, L), "las_delay_sum: Wn=%lld, but %lld samples in windows of %d are %lld windows", Wn, n, L, las_bf_windows(n, L));
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)cdiv((n + 3) / 4, 256);
    WITH_I16(x_i16, hipLaunchKernelGGL(bf_sum_kernel<I16>, dim3(grid), dim3(256), 0, st, x, ld, C, n, L / 2, Wn, tau, a, y));
    LAS_LAUNCHED();
    return 0;
}
