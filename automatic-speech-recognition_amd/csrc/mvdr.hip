// mvdr.hip -- the adaptive counterpart of beamform.hip (las_hip.h K19): a mask-driven MVDR beamformer in the STFT domain, in
// Souden's reference-channel form (Souden et al. 2010): no array geometry, no delay estimate, no steering vector.  One recording
// [C, n] per call, frames of NF samples every Hs = NF / 2 under a sine window (analysis and synthesis), K = NF / 2 + 1 bins:
//   las_mvdr_mask     m[t] = the energy rule of las_vad on the reference channel's frames
//   las_mvdr_cov      phi_n[k] = the covariance of the frames the mask calls noise, phi_y[b][k] = of the speech frames of block b
//   las_mvdr_weights  w[b][k] = (A^-1 (phi_y - phi_n))[:, ref] / tr(...), A = phi_n + loading; a hold pass over the blocks per bin
//   las_mvdr_apply    y = the inverse STFT of sum_c conj(w_c) X_c
// Everything runs on the caller's stream; no atomics, no cross-workgroup synchronisation: every output value is computed by one
// thread or one workgroup in a fixed order, so two calls give the same bits.  The spectra are never stored: the covariance pass and
// the apply pass each transform their frames in LDS and read the samples once (the apply pass: 1 + 1 / 16 times).  The windowed
// transform (the fp32 tables, the packed loader, the FFT in LDS, the real-FFT split and the way back) is bf_fft.h's, shared with
// beamform.hip.
//
//   mvdr_energy_kernel   one thread per frame adds the frame's squared samples in ascending order in double (the contract's order).
//   mvdr_max_kernel      one workgroup: emax.  mvdr_mask_kernel: one thread per frame, the threshold and the dilation by `hang`.
//   mvdr_cov_kernel      THE SPLIT THAT WAS BUILT: over frame tiles, and over bin slices where the registers ask for it.  Workgroup
//                        (tile, slice): the tile is FT consecutive frames of ONE block (FT <= 256, chosen so that about a thousand
//                        workgroups exist); up to 8 frames at a time (as many as fit 128 KiB) the C channels are windowed into LDS,
//                        transformed together (frames x C packed transforms of NF / 2 points under shared barriers: the registers
//                        leave a compute unit ONE workgroup, so a barrier's wait is hidden by nobody; a frame at a time the pass
//                        took 9.6 ms for the timed hour), split in place into X_c[0 .. NF/2], and every thread
//                        adds its items' products s X_i conj(X_j) and q X_i conj(X_j) to fp32 accumulators in registers.  An item is
//                        (bin k, row i) with the CP / 2 + 1 columns j = (i + d) mod CP, d = 0 .. CP / 2 (CP = C rounded up to a
//                        power of two): every unordered pair lies in exactly one row but for d = CP / 2, which two rows hold as
//                        conjugates -- all rows carry the same load, where the upper triangle's rows carry 1 to C.  At CP = 16
//                        an item is 9 pairs x 2 sums = 36 accumulators and a thread holds 4 items (5 spill); 512 threads hold 128
//                        bins, so NF = 1024 takes 5 bin slices (each repeats the transforms), NF = 512 three, the 8 channels of
//                        the timed recording one.  On the VALU: the matrix cores (v_mfma_f32_16x16x4_f32) were not tried, the pass is
//                        measured in DESIGN 7w.  The tile's sums go to the workspace as fp32.
//   mvdr_counts_kernel   M_b and the block's noise count in ascending frame order, then N0 over the blocks in block order (double).
//   mvdr_phi_y_kernel / mvdr_phi_n_kernel   one thread per stored element adds the tiles' partial sums in tile order in double,
//                        divides, and writes both triangles from the same sums: Hermitian as stored, the diagonal's imaginary part 0.
//   mvdr_weights_kernel  workgroup (bin, a range of blocks): A = phi_n[k] + loading tn I is factorised ONCE per workgroup (Cholesky
//                        in LDS, a thread per row), then one thread per (block, column) solves L L^H g = P[:, column] with its
//                        vector in registers; the columns' diagonal entries meet in LDS for the trace, and the thread of column
//                        ref writes w_raw and valid.  mvdr_hold_kernel: one thread per (bin, channel) walks the blocks.
//   mvdr_apply_kernel    a workgroup owns 16 output segments: it transforms 17 frames (one halo frame), keeps the block's weights
//                        as fp32 in LDS, Y = sum_c conj(w_c) X_c in channel order, the inverse transform, the
//                        window, and every sample it owns is written once: f_j's second half (kept in LDS) plus f_j+1's first.
#include "las_common.h"
#include "bf_fft.h"
#include <math.h>
#include <limits.h>

namespace {

constexpr int MAX_C = LAS_BF_MAX_CHANNELS, MAX_NF = LAS_MVDR_MAX_FFT, MIN_NF = 64;
constexpr int COV_NT = 512;                           // largest workgroup of the covariance pass (256 VGPRs a thread)
constexpr int COV_FT = 256;                           // most frames a tile adds in fp32
constexpr int COV_WGS = 1024;                         // workgroups the tiling aims at
constexpr int COV_LDS = 128 * 1024;                   // LDS of the covariance pass: as many frames as fit (at most 8) are transformed together
constexpr int APPLY_SEG = 16;                         // output segments per workgroup of the apply pass
constexpr int WT_NT = 256;
constexpr double G_MIN = 1e-6;

__host__ __device__ constexpr int cov_items(int CP) { return CP == 16 ? 4 : CP == 8 ? 5 : CP == 4 ? 5 : 3; }   // items a thread holds

template <bool I16>
__global__ __launch_bounds__(64) void mvdr_energy_kernel(const void* __restrict__ x, long long row, long long n, int Hs, long long Tf,
                                                         double* __restrict__ e) {
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= Tf) return;
    const long long i0 = max(0ll, (t - 1) * Hs), i1 = min(n, (t + 1) * Hs);      // (samples outside [0, n) add an exact 0)
    double s = 0.0;
    for (long long i = i0; i < i1; ++i) {
        const double v = (double)sample_at<I16>(x, row + i);
        s += v * v;                                   // (v v is exact in double: one rounding per term, fused or not)
    }
    e[t] = s;
}

__global__ __launch_bounds__(1024) void mvdr_max_kernel(const double* __restrict__ e, long long Tf, double* __restrict__ emax) {
    __shared__ double red[1024];
    double v = 0.0;                                   // (energies are >= 0)
    for (long long t = threadIdx.x; t < Tf; t += 1024) v = fmax(v, e[t]);
    red[threadIdx.x] = v;
    __syncthreads();
    for (int h = 512; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) emax[0] = red[0];
}

__global__ __launch_bounds__(256) void mvdr_mask_kernel(const double* __restrict__ e, const double* __restrict__ emax, long long Tf, double ratio,
                                                        double floor_, int hang, float* __restrict__ m) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= Tf) return;
    const double thr = fmax(__dmul_rn(emax[0], ratio), floor_);
    const long long a = max(0ll, t - hang), b = min(Tf - 1, t + hang);
    bool on = false;
    for (long long u = a; u <= b && !on; ++u) {
        const double v = e[u];
        on = v >= thr && v > 0.0;
    }
    m[t] = on ? 1.f : 0.f;
}

// the C packed transforms in place to the spectra X_c[0 .. M] (buffers of stride >= M + 1); ends with a barrier
__device__ __forceinline__ void split_frames(float2* z, int stride, int lgM, int C, const float2* __restrict__ tw) {
    const int M = 1 << lgM, per = M / 2 + 1;
    for (int e = threadIdx.x; e < C * per; e += blockDim.x) {
        const int c = e / per, k = e - c * per;
        float2* Z = z + c * stride;
        const float2 a = Z[k], b = Z[(M - k) & (M - 1)];
        const float2 xk = split_pt(a, b, tw[k]), xm = split_pt(b, a, tw[M - k]);
        Z[k] = xk;
        if (k != M - k) Z[M - k] = xm;                // (k = 0 writes the slot M behind the packed points)
    }
    __syncthreads();
}

// partial sums of a tile: float2 [tile][2 (speech, noise)][K][CP][CP / 2 + 1]
__host__ __device__ inline size_t part_index(long long tile, int yn, int K, int CP, int k, int i, int d) {
    return ((((size_t)tile * 2 + yn) * K + k) * CP + i) * (CP / 2 + 1) + d;
}

template <bool I16, int CP>
__global__ __launch_bounds__(COV_NT) void mvdr_cov_kernel(const void* __restrict__ x, long long ld, int C, long long n, int lgNF, long long Tf,
                                                          long long Bf, int FT, int nsplit, int KS, int FB, const float* __restrict__ m,
                                                          const float* __restrict__ win_f, const float2* __restrict__ tw,
                                                          float2* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mv_lds[];
    constexpr int IT = cov_items(CP), ND = CP / 2 + 1;
    const int lgM = lgNF - 1, M = 1 << lgM, K = M + 1, stride = M + 1;
    float2* z = (float2*)mv_lds;                      // [FB][CP][M + 1]: FB frames share the transforms' barriers
    const long long tile = blockIdx.x, b = tile / nsplit;
    const int sp = (int)(tile - b * nsplit);
    const long long tb1 = min(Tf, (b + 1) * Bf), t0 = b * Bf + (long long)sp * FT, t1 = min(tb1, t0 + FT);
    const int k0 = blockIdx.y * KS, k1 = min(K, k0 + KS), tid = threadIdx.x, nt = blockDim.x;
    float2 ay[IT][ND], an[IT][ND];
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int d = 0; d < ND; ++d) ay[it][d] = an[it][d] = make_float2(0.f, 0.f);
    if (C < CP)                                       // the channels the array lacks: zeros, transformed along (their spectra stay zeros)
        for (int e = tid; e < FB * CP * stride; e += nt) z[e] = make_float2(0.f, 0.f);
    __syncthreads();
    for (long long tb = t0; tb < t1; tb += FB) {      // (uniform)
        const int nf = (int)min((long long)FB, t1 - tb);
        for (int f = 0; f < nf; ++f)                  // frame t: the samples from (t - 1) Hs on, Hs = M
            load_windowed<I16>(z + f * CP * stride, stride, lgM, C, x, 0, ld, (tb + f - 1) * M, n, 2 * M, win_f);
        __syncthreads();
        fft_lds_batch(z, lgM, nf * CP, stride, tw, lgNF);
        split_frames(z, stride, lgM, nf * CP, tw);
        for (int f = 0; f < nf; ++f) {                // in ascending t, as the contract has the tile's sums
            const float2* zf = z + f * CP * stride;
            const float s = m[tb + f], q = (float)(1.0 - (double)s);
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int item = tid + it * nt, k = k0 + item / CP, i = item & (CP - 1);
                if (k < k1 && i < C) {
                    const float2 xi = zf[i * stride + k];
#pragma unroll
                    for (int d = 0; d < ND; ++d) {
                        const float2 xj = zf[((i + d) & (CP - 1)) * stride + k];
                        const float pr = xi.x * xj.x + xi.y * xj.y, pi = xi.y * xj.x - xi.x * xj.y;  // X_i conj(X_j)
                        ay[it][d].x = fmaf(s, pr, ay[it][d].x); ay[it][d].y = fmaf(s, pi, ay[it][d].y);
                        an[it][d].x = fmaf(q, pr, an[it][d].x); an[it][d].y = fmaf(q, pi, an[it][d].y);
                    }
                }
            }
        }
        __syncthreads();                              // the spectra have been read: the next frames may overwrite them
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int item = tid + it * nt, k = k0 + item / CP, i = item & (CP - 1);
        if (k < k1) {                                 // (rows i >= C: zeros, so that the whole tile is defined)
#pragma unroll
            for (int d = 0; d < ND; ++d) {
                part[part_index(tile, 0, K, CP, k, i, d)] = ay[it][d];
                part[part_index(tile, 1, K, CP, k, i, d)] = an[it][d];
            }
        }
    }
}

// counts[1 + b] = M_b, nb[b] = the block's sum of q_t, both in ascending frame order
__global__ __launch_bounds__(256) void mvdr_counts_kernel(const float* __restrict__ m, long long Tf, long long Bf, long long Nb, double* __restrict__ counts,
                                                          double* __restrict__ nb) {
    const long long b = (long long)blockIdx.x * 256 + threadIdx.x;
    if (b >= Nb) return;
    const long long t1 = min(Tf, (b + 1) * Bf);
    double ms = 0.0, qs = 0.0;
    for (long long t = b * Bf; t < t1; ++t) {
        const double s = (double)m[t];
        ms += s;
        qs += 1.0 - s;
    }
    counts[1 + b] = ms;
    nb[b] = qs;
}
__global__ __launch_bounds__(64) void mvdr_n0_kernel(const double* __restrict__ nb, long long Nb, double* __restrict__ counts) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (long long b = 0; b < Nb; ++b) s += nb[b];
    counts[0] = s;
}

// where the product of the channels (i, j) is stored: row r, column slot d; conjugated when the stored row is not i
__device__ __forceinline__ void pair_slot(int i, int j, int CP, int& r, int& d, bool& conj) {
    if (i == j) { r = i; d = 0; conj = false; return; }
    const int lo = min(i, j), hi = max(i, j), dist = hi - lo;
    if (dist <= CP / 2) { r = lo; d = dist; } else { r = hi; d = CP - dist; }
    conj = r != i;
}

__global__ __launch_bounds__(256) void mvdr_phi_y_kernel(const float2* __restrict__ part, const double* __restrict__ counts, long long Nb, int K, int C,
                                                         int CP, int nsplit, double* __restrict__ phi_y) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x, total = Nb * K * C * C;
    if (e >= total) return;
    const int j = (int)(e % C), i = (int)((e / C) % C), k = (int)((e / ((long long)C * C)) % K);
    const long long b = e / ((long long)C * C * K);
    int r, d;
    bool conj;
    pair_slot(i, j, CP, r, d, conj);
    double sr = 0.0, si = 0.0;
    for (int sp = 0; sp < nsplit; ++sp) {
        const float2 p = part[part_index(b * nsplit + sp, 0, K, CP, k, r, d)];
        sr += (double)p.x;
        si += (double)p.y;
    }
    const double Mb = counts[1 + b];
    double re = 0.0, im = 0.0;
    if (Mb != 0.0) { re = sr / Mb; im = i == j ? 0.0 : (conj ? -si : si) / Mb; }
    phi_y[2 * e] = re;
    phi_y[2 * e + 1] = im;
}

__global__ __launch_bounds__(256) void mvdr_phi_n_kernel(const float2* __restrict__ part, const double* __restrict__ counts, long long ntiles, int K, int C,
                                                         int CP, double* __restrict__ phi_n) {
    const int e = blockIdx.x * 256 + threadIdx.x, total = K * C * C;
    if (e >= total) return;
    const int j = e % C, i = (e / C) % C, k = e / (C * C);
    int r, d;
    bool conj;
    pair_slot(i, j, CP, r, d, conj);
    double sr = 0.0, si = 0.0;
#pragma unroll 8
    for (long long tile = 0; tile < ntiles; ++tile) {
        const float2 p = part[part_index(tile, 1, K, CP, k, r, d)];
        sr += (double)p.x;
        si += (double)p.y;
    }
    const double N0 = counts[0];
    double re = 0.0, im = 0.0;
    if (N0 != 0.0) { re = sr / N0; im = i == j ? 0.0 : (conj ? -si : si) / N0; }
    phi_n[2 * e] = re;
    phi_n[2 * e + 1] = im;
}

struct cd { double x, y; };
__device__ __forceinline__ cd cd_make(double x, double y) { cd r; r.x = x; r.y = y; return r; }

// workgroup (bin k, blocks [blockIdx.y * per, ...)): see the head of the file
__global__ __launch_bounds__(WT_NT) void mvdr_weights_kernel(const double* __restrict__ phi_n, const double* __restrict__ phi_y,
                                                             const double* __restrict__ counts, int C, int K, long long Nb, long long per, int ref,
                                                             double loading, double* __restrict__ w, int* __restrict__ valid) {
    __shared__ cd Ls[MAX_C][MAX_C + 1];               // A, then its Cholesky factor in the lower triangle
    __shared__ cd Pn[MAX_C][MAX_C + 1];
    __shared__ double dg[WT_NT];
    const int k = blockIdx.x, tid = threadIdx.x;
    const long long b0 = (long long)blockIdx.y * per, b1 = min(Nb, b0 + per);
    const double* pn = phi_n + (size_t)k * C * C * 2;
    double tr = 0.0;
    for (int c = 0; c < C; ++c) tr += pn[2 * (c * C + c)];
    const double tn = tr / (double)C, N0 = counts[0];
    const bool bin_ok = N0 > 0.0 && tn > 0.0;         // (uniform)
    if (!bin_ok) {
        for (long long b = b0 + tid; b < b1; b += WT_NT) valid[b * K + k] = 0;
        return;
    }
    for (int e = tid; e < C * C; e += WT_NT) {
        const int i = e / C, j = e - i * C;
        const cd v = cd_make(pn[2 * e], pn[2 * e + 1]);
        Pn[i][j] = v;
        Ls[i][j] = cd_make(v.x + (i == j ? loading * tn : 0.0), v.y);
    }
    __syncthreads();
    for (int j = 0; j < C; ++j) {                     // column j of L: thread i owns row i
        cd s = cd_make(0.0, 0.0);
        if (tid >= j && tid < C) {
            s = Ls[tid][j];
            for (int p = 0; p < j; ++p) {             // s -= L[i][p] conj(L[j][p])
                const cd a = Ls[tid][p], c = Ls[j][p];
                s.x -= a.x * c.x + a.y * c.y;
                s.y -= a.y * c.x - a.x * c.y;
            }
            if (tid == j) Ls[j][j] = cd_make(sqrt(s.x), 0.0);     // (not positive: NaN, and every block of the bin comes out not valid)
        }
        __syncthreads();
        if (tid > j && tid < C) {
            const double dinv = Ls[j][j].x;
            Ls[tid][j] = cd_make(s.x / dinv, s.y / dinv);
        }
        __syncthreads();
    }
    const int G = WT_NT / C, bl = tid / C, j = tid - bl * C;
    for (long long base = b0; base < b1; base += G) {  // (uniform)
        const long long b = base + bl;
        const bool act = bl < G && b < b1;
        cd v[MAX_C];
        if (act) {
            const double* py = phi_y + ((size_t)b * K + k) * C * C * 2;
#pragma unroll
            for (int r = 0; r < MAX_C; ++r) {
                v[r] = cd_make(0.0, 0.0);
                if (r < C) { const cd p = Pn[r][j]; v[r] = cd_make(py[2 * (r * C + j)] - p.x, py[2 * (r * C + j) + 1] - p.y); }
            }
#pragma unroll
            for (int r = 0; r < MAX_C; ++r) {         // L u = P[:, j]
                if (r < C) {
                    cd s = v[r];
#pragma unroll
                    for (int p = 0; p < r; ++p) {
                        const cd l = Ls[r][p];
                        s.x -= l.x * v[p].x - l.y * v[p].y;
                        s.y -= l.x * v[p].y + l.y * v[p].x;
                    }
                    const double dd = Ls[r][r].x;
                    v[r] = cd_make(s.x / dd, s.y / dd);
                }
            }
#pragma unroll
            for (int r = MAX_C - 1; r >= 0; --r) {    // L^H g = u
                if (r < C) {
                    cd s = v[r];
#pragma unroll
                    for (int p = r + 1; p < MAX_C; ++p) {
                        if (p < C) {
                            const cd l = Ls[p][r];    // conj(L[p][r]) v[p]
                            s.x -= l.x * v[p].x + l.y * v[p].y;
                            s.y -= l.x * v[p].y - l.y * v[p].x;
                        }
                    }
                    const double dd = Ls[r][r].x;
                    v[r] = cd_make(s.x / dd, s.y / dd);
                }
            }
            double own = 0.0;
#pragma unroll
            for (int r = 0; r < MAX_C; ++r) if (r == j) own = v[r].x;
            dg[tid] = own;
        }
        __syncthreads();
        if (act && j == ref) {
            double g = 0.0;
            for (int c = 0; c < C; ++c) g += dg[bl * C + c];
            const bool ok = counts[1 + b] > 0.0 && g > G_MIN;
            valid[b * K + k] = ok ? 1 : 0;
            if (ok) {
                double* wo = w + ((size_t)b * K + k) * C * 2;
#pragma unroll
                for (int r = 0; r < MAX_C; ++r)
                    if (r < C) { wo[2 * r] = v[r].x / g; wo[2 * r + 1] = v[r].y / g; }
            }
        }
        __syncthreads();
    }
}

// per bin over the blocks: a block that is not valid takes the weights of the nearest valid block before it, else of the first valid
// block behind it, else e_ref
__global__ __launch_bounds__(256) void mvdr_hold_kernel(const int* __restrict__ valid, int C, int K, long long Nb, int ref, double* __restrict__ w) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= K * C) return;
    const int k = e / C, c = e - k * C;
    bool seen = false;
    double hx = c == ref ? 1.0 : 0.0, hy = 0.0;
    for (long long b = 0; b < Nb; ++b) {
        double* wo = w + (((size_t)b * K + k) * C + c) * 2;
        if (valid[b * K + k]) {
            hx = wo[0]; hy = wo[1];
            if (!seen) {
                for (long long a = 0; a < b; ++a) {
                    double* wa = w + (((size_t)a * K + k) * C + c) * 2;
                    wa[0] = hx; wa[1] = hy;
                }
                seen = true;
            }
        } else if (seen) {
            wo[0] = hx; wo[1] = hy;
        }
    }
    if (!seen)
        for (long long b = 0; b < Nb; ++b) {
            double* wo = w + (((size_t)b * K + k) * C + c) * 2;
            wo[0] = hx; wo[1] = hy;
        }
}

template <bool I16>
__global__ __launch_bounds__(512) void mvdr_apply_kernel(const void* __restrict__ x, long long ld, int C, long long n, int lgNF, long long Tf, long long Bf,
                                                         const double* __restrict__ w, const float* __restrict__ win_f, const float2* __restrict__ tw,
                                                         float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mv_lds[];
    const int lgM = lgNF - 1, M = 1 << lgM, K = M + 1, stride = M + 1, tid = threadIdx.x, nt = blockDim.x;
    float2* z = (float2*)mv_lds;                      // [C][M + 1] the spectra
    float2* wl = z + C * stride;                      // [C][M + 1] the block's weights, fp32
    float2* Y = wl + C * stride;                      // [M + 1]
    float2* B = Y + stride;                           // [M] the inverse transform's buffer
    float* prev = (float*)(B + M);                    // [M] the previous frame's second half, windowed
    const long long j0 = (long long)blockIdx.x * APPLY_SEG, tl = min(Tf - 1, j0 + APPLY_SEG);     // frames j0 .. tl
    long long cur = -1;
    const float scale = 1.0f / (float)M;
    for (long long t = j0; t <= tl; ++t) {            // (uniform)
        const long long b = t / Bf;
        load_windowed<I16>(z, stride, lgM, C, x, 0, ld, (t - 1) * M, n, 2 * M, win_f);
        if (b != cur) {                               // (uniform; the previous frame's readers of wl passed the barriers below)
            const double* wb = w + (size_t)b * K * C * 2;
            for (int e = tid; e < K * C; e += nt) {
                const int k = e / C, c = e - k * C;
                wl[c * stride + k] = make_float2((float)wb[2 * e], (float)wb[2 * e + 1]);
            }
            cur = b;
        }
        __syncthreads();
        fft_lds_batch(z, lgM, C, stride, tw, lgNF);
        split_frames(z, stride, lgM, C, tw);
        for (int k = tid; k < K; k += nt) {
            float yr = 0.f, yi = 0.f;
            for (int c = 0; c < C; ++c) {             // conj(w_c) X_c, in channel order
                const float2 wc = wl[c * stride + k], xc = z[c * stride + k];
                yr += wc.x * xc.x + wc.y * xc.y;
                yi += wc.x * xc.y - wc.y * xc.x;
            }
            Y[k] = make_float2(yr, (k == 0 || k == M) ? 0.f : yi);     // (the Hermitian extension has real ends)
        }
        __syncthreads();
        for (int k = tid; k <= M / 2; k += nt) {
            const float2 gk = Y[k], gm = Y[M - k];
            store_unsplit(B, lgM, k, unsplit_conj(gk, gm, tw[k]), unsplit_conj(gm, gk, tw[M - k]));
        }
        __syncthreads();
        fft_lds(B, lgM, tw, lgNF);                    // B holds the frame f_t for real_at
        for (int i = tid; i < M; i += nt) {           // the first half of f_t closes the segment t - 1
            const float f = real_at(B, i, scale) * win_f[i];
            const long long s = (t - 1) * M + i;
            if (t > j0 && s < n) y[s] = prev[i] + f;
        }
        __syncthreads();                              // prev has been read
        for (int i = tid; i < M; i += nt) prev[i] = real_at(B, M + i, scale) * win_f[M + i];
        __syncthreads();
    }
}

// the workspace: [tw fp32 [NF/2 + 1, 2] | win fp32 [NF] | e double [Tf] | emax double | nb double [Nb] | the tiles' partial sums]
struct Tiling { int CP, FT, nsplit, KS, slices, nt; long long Nb, ntiles; };
struct Layout { TableSlice tab; size_t e, emax, nb, part, total; };

long long frames_of(long long n, int NF) { return (n + NF / 2 - 1) / (NF / 2) + 1; }
long long blocks_of(long long Tf, long long Bf) { return (Tf + Bf - 1) / Bf; }
bool fft_ok(int NF) { return pow2_in(NF, MIN_NF, MAX_NF); }

Tiling tiling(int C, long long Tf, int NF, long long Bf) {
    Tiling t;
    t.CP = C <= 2 ? 2 : C <= 4 ? 4 : C <= 8 ? 8 : 16;
    t.Nb = blocks_of(Tf, Bf);
    const long long Bfe = Bf < Tf ? Bf : Tf, want = (COV_WGS + t.Nb - 1) / t.Nb;
    long long FT = (Bfe + want - 1) / want;
    if (FT < 8) FT = Bfe < 8 ? Bfe : 8;
    if (FT > COV_FT) FT = COV_FT;
    t.FT = (int)FT;
    t.nsplit = (int)((Bfe + FT - 1) / FT);
    t.ntiles = t.Nb * t.nsplit;
    const int K = NF / 2 + 1, most = COV_NT * cov_items(t.CP) / t.CP;     // bins a workgroup's registers hold
    t.slices = (K + most - 1) / most;
    t.KS = (K + t.slices - 1) / t.slices;
    const int threads = (t.KS * t.CP + cov_items(t.CP) - 1) / cov_items(t.CP);
    t.nt = clampi((threads + 63) / 64 * 64, 64, COV_NT);
    return t;
}

Layout layout(int C, long long Tf, int NF, long long Bf) {
    const Tiling t = tiling(C, Tf, NF, Bf);
    Layout l;
    size_t o = table_slice(0, NF, l.tab);
    l.e = o;    o += align256((size_t)Tf * sizeof(double));
    l.emax = o; o += 256;
    l.nb = o;   o += align256((size_t)t.Nb * sizeof(double));
    l.part = o; o += align256((size_t)t.ntiles * 2 * (NF / 2 + 1) * t.CP * (t.CP / 2 + 1) * sizeof(float2));
    l.total = o;
    return l;
}

template <bool I16>
int launch_cov(const Tiling& t, int C, const void* x, long long ld, long long n, int lgNF, long long Tf, long long Bf, const float* m, const float* win_f,
               const float2* tw_f, float2* part, hipStream_t st) {
    const size_t frame = (size_t)t.CP * ((1 << (lgNF - 1)) + 1) * sizeof(float2);    // at most 16 x 513 x 8 = 64 KiB + 128
    const int FB = clampi((int)(COV_LDS / frame), 1, 8);                             // frames transformed together
    const size_t lds = FB * frame;
    const dim3 grid((unsigned)t.ntiles, (unsigned)t.slices), block(t.nt);
#define MVDR_COV(CPV)                                                                                                                          \
    do {                                                                                                                                       \
        static int attr = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(mvdr_cov_kernel<I16, CPV>),                                   \
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, COV_LDS);                                        \
        LAS_ARG(attr == 0, "hipFuncSetAttribute(mvdr_cov_kernel) failed: %d", attr);                                                           \
        hipLaunchKernelGGL((mvdr_cov_kernel<I16, CPV>), grid, block, lds, st, x, ld, C, n, lgNF, Tf, Bf, t.FT, t.nsplit, t.KS, FB, m, win_f,    \
                           tw_f, part);                                                                                                        \
    } while (0)
    switch (t.CP) {
        case 2: MVDR_COV(2); break;
        case 4: MVDR_COV(4); break;
        case 8: MVDR_COV(8); break;
        default: MVDR_COV(16); break;
    }
#undef MVDR_COV
    LAS_LAUNCHED();
    return 0;
}

size_t apply_lds(int C, int NF) {
    const size_t M = NF / 2;
    return ((size_t)2 * C * (M + 1) + (M + 1) + M) * sizeof(float2) + M * sizeof(float);
}

}  // namespace

extern "C" long long las_mvdr_frames(long long n, int NF) {
    if (n < 1 || n > INT32_MAX || !fft_ok(NF)) return -1;
    return frames_of(n, NF);
}

extern "C" long long las_mvdr_blocks(long long Tf, int Bf) {
    if (Tf < 1 || Bf < 1) return -1;
    return blocks_of(Tf, Bf);
}

extern "C" size_t las_mvdr_workspace_bytes(int C, long long Tf, int NF, int Bf) {
    if (C < 2 || C > MAX_C || Tf < 1 || Tf > INT32_MAX || !fft_ok(NF) || Bf < 1) return 0;
    return layout(C, Tf, NF, Bf).total;
}

#define MVDR_GEOMETRY(name) \
    LAS_ARG(C >= 2 && C <= MAX_C && fft_ok(NF), name ": bad geometry (C=%d, 2..%d; NF=%d, a power of two, %d..%d)", C, MAX_C, NF, MIN_NF, MAX_NF)

extern "C" int las_mvdr_mask(const void* x, int x_i16, long long ld, int C, long long n, int ref, int NF, double ratio, double floor, int hang,
                             float* m, double* energy, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(x && m && ws, "las_mvdr_mask: null pointer (x, m, ws)");
    MVDR_GEOMETRY("las_mvdr_mask");
    ARG_ROWS("las_mvdr_mask", n, ld);
    ARG_REF("las_mvdr_mask", ref, C);
    LAS_ARG(ratio > 0.0 && ratio <= 1.0, "las_mvdr_mask: ratio=%g (in (0, 1])", ratio);
    LAS_ARG(isfinite(floor) && floor >= 0.0 && hang >= 0, "las_mvdr_mask: floor=%g (finite, >= 0), hang=%d (>= 0)", floor, hang);
    const long long Tf = frames_of(n, NF);
    const Layout l = layout(C, Tf, NF, 1);
    ARG_WS("las_mvdr_mask", ws, ws_bytes, l.nb);
    double* e = energy ? energy : (double*)((char*)ws + l.e);
    double* emax = (double*)((char*)ws + l.emax);
    hipStream_t st = (hipStream_t)stream;
    WITH_I16(x_i16, hipLaunchKernelGGL(mvdr_energy_kernel<I16>, dim3(cdiv(Tf, 64)), dim3(64), 0, st, x, (long long)ref * ld, n, NF / 2, Tf, e));
    LAS_LAUNCHED();
    hipLaunchKernelGGL(mvdr_max_kernel, dim3(1), dim3(1024), 0, st, e, Tf, emax);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(mvdr_mask_kernel, dim3(cdiv(Tf, 256)), dim3(256), 0, st, e, emax, Tf, ratio, floor, hang, m);
    LAS_LAUNCHED();
    return 0;
}

extern "C" int las_mvdr_cov(const void* x, int x_i16, long long ld, int C, long long n, int NF, int Bf, const float* m, const double* win,
                            const double* twiddle, double* counts, double* phi_n, double* phi_y, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(x && m && win && twiddle && counts && phi_n && phi_y && ws, "las_mvdr_cov: null pointer (x, m, win, twiddle, counts, phi_n, phi_y, ws)");
    MVDR_GEOMETRY("las_mvdr_cov");
    ARG_ROWS("las_mvdr_cov", n, ld);
    LAS_ARG(Bf >= 1, "las_mvdr_cov: Bf=%d frames per block (>= 1)", Bf);
    const long long Tf = frames_of(n, NF);
    const Layout l = layout(C, Tf, NF, Bf);
    ARG_WS("las_mvdr_cov", ws, ws_bytes, l.total);
    const Tiling t = tiling(C, Tf, NF, Bf);
    const int K = NF / 2 + 1, lgNF = log2_of(NF);
    LAS_ARG(t.ntiles <= INT32_MAX && t.Nb * K * C * C / 256 < INT32_MAX, "las_mvdr_cov: %lld blocks of %d bins are more than one launch takes", t.Nb, K);
    double* nb = (double*)((char*)ws + l.nb);
    float2* part = (float2*)((char*)ws + l.part);
    hipStream_t st = (hipStream_t)stream;
    Tables tab;
    int rc = tables_launch(win, twiddle, NF, NF, ws, l.tab, st, tab);
    if (rc) return rc;
    WITH_I16(x_i16, rc = launch_cov<I16>(t, C, x, ld, n, lgNF, Tf, Bf, m, tab.win, tab.tw, part, st));
    if (rc) return rc;
    hipLaunchKernelGGL(mvdr_counts_kernel, dim3(cdiv(t.Nb, 256)), dim3(256), 0, st, m, Tf, (long long)Bf, t.Nb, counts, nb);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(mvdr_n0_kernel, dim3(1), dim3(64), 0, st, nb, t.Nb, counts);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(mvdr_phi_y_kernel, dim3(cdiv(t.Nb * K * C * C, 256)), dim3(256), 0, st, part, counts, t.Nb, K, C, t.CP, t.nsplit, phi_y);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(mvdr_phi_n_kernel, dim3(cdiv((long long)K * C * C, 256)), dim3(256), 0, st, part, counts, t.ntiles, K, C, t.CP, phi_n);
    LAS_LAUNCHED();
    return 0;
}

extern "C" int las_mvdr_weights(const double* phi_n, const double* phi_y, const double* counts, int C, int NF, long long Nb, int ref, double loading,
                                double* w, int* valid, void* stream) {
    LAS_ARG(phi_n && phi_y && counts && w && valid, "las_mvdr_weights: null pointer (phi_n, phi_y, counts, w, valid)");
    MVDR_GEOMETRY("las_mvdr_weights");
    LAS_ARG(Nb >= 1 && Nb <= INT32_MAX, "las_mvdr_weights: Nb=%lld blocks (>= 1)", Nb);
    ARG_REF("las_mvdr_weights", ref, C);
    LAS_ARG(isfinite(loading) && loading > 0.0, "las_mvdr_weights: loading=%g (finite, > 0)", loading);
    const int K = NF / 2 + 1;
    const long long splits = clampi(cdiv(Nb * C, 4 * WT_NT), 1, 64), per = (Nb + splits - 1) / splits;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mvdr_weights_kernel, dim3(K, (unsigned)cdiv(Nb, per)), dim3(WT_NT), 0, st, phi_n, phi_y, counts, C, K, Nb, per, ref, loading, w,
                       valid);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(mvdr_hold_kernel, dim3(cdiv(K * C, 256)), dim3(256), 0, st, valid, C, K, Nb, ref, w);
    LAS_LAUNCHED();
    return 0;
}

extern "C" int las_mvdr_apply(const void* x, int x_i16, long long ld, int C, long long n, int NF, int Bf, const double* w, const double* win,
                              const double* twiddle, float* y, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(x && w && win && twiddle && y && ws, "las_mvdr_apply: null pointer (x, w, win, twiddle, y, ws)");
    MVDR_GEOMETRY("las_mvdr_apply");
    ARG_ROWS("las_mvdr_apply", n, ld);
    LAS_ARG(Bf >= 1, "las_mvdr_apply: Bf=%d frames per block (>= 1)", Bf);
    const long long Tf = frames_of(n, NF);
    const Layout l = layout(C, Tf, NF, Bf);
    ARG_WS("las_mvdr_apply", ws, ws_bytes, l.e);
    const int M = NF / 2, lgNF = log2_of(NF);
    const size_t lds = apply_lds(C, NF);              // at most (2 x 16 x 513 + 513 + 512) x 8 + 2048 = 138 KiB
    RAISE_LDS_I16(mvdr_apply_kernel, apply_lds(MAX_C, MAX_NF));
    hipStream_t st = (hipStream_t)stream;
    Tables tab;
    if (const int rc = tables_launch(win, twiddle, NF, NF, ws, l.tab, st, tab)) return rc;
    const int nt = clampi((C * M / 8 + 63) / 64 * 64, 64, 512);
    const unsigned grid = (unsigned)cdiv(Tf - 1, APPLY_SEG);
    WITH_I16(x_i16, hipLaunchKernelGGL(mvdr_apply_kernel<I16>, dim3(grid), dim3(nt), lds, st, x, ld, C, n, lgNF, Tf, (long long)Bf, w, tab.win, tab.tw, y));
    LAS_LAUNCHED();
    return 0;
}
