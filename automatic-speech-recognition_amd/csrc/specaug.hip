// specaug.hip -- SpecAugment (Park et al., 2019) on the feature cube, between the feeder and the Listener: one time warp, mF frequency
// masks and mT time masks per utterance, one launch.  The kernel APPLIES a plan (las_hip.h las_specaug_args: row b of plan [B, ldp] is
// {len, w0, w, 0, (f0, fw) x mF, (t0, tw) x mT}); it draws nothing -- las/specaug.py draws on the host.
//
//   specaug_kernel   a workgroup owns TILE consecutive frames of one utterance (blockIdx.x = tile, blockIdx.y = utterance): TILE * F*C
//                    consecutive floats of in and of out.  It loads the row's plan into LDS once, then one thread per frame of the tile
//                    works out where the frame comes from -- (i0, frac) of the piecewise-linear warp in 32-bit integers and ONE fp32
//                    division, or "zero" for a frame behind len or under a time mask -- into a TILE-entry LDS table: the divisions are per
//                    frame, not per element.  The element loop then runs over the tile's flat range in 16-byte stores: up to three
//                    scalar elements in front until the ADDRESS is 16-byte aligned (F*C is 39 or 117 in two of the three
//                    configurations: a frame, a tile and a row start on any 4-byte boundary), quads, up to three behind.  A quad
//                    inside one frame with no masked column reads its source frame(s) with one (unaligned) 16-byte load each; a quad
//                    across a frame boundary or a mask edge goes element by element, without branches, so that its loads are in
//                    flight together.  Masked elements are a select of +0.0f: the source under them is not read.  r == 0 (every
//                    frame of a row with w == 0, the control point, the last frame) is a bit copy of x[i0]; x[i0 + 1] is not read.
//                    TILE = 32: at B = 48, T = 1274 that is 1920 workgroups, all resident at once, of 1.2 (F*C = 39) to 3.75 (120)
//                    passes of the quad loop; 64 frames took 1.1x / 1.4x the time, 16 frames 1.03x.
// out[b, t, c] depends on (plan row b, t, c, the row's input) only: not on TILE, not on the alignment, not on the other rows.
// Every element of out is written.
#include "las_common.h"

namespace {

constexpr int NT = 256;
#ifndef LAS_SPECAUG_TILE
#define LAS_SPECAUG_TILE 32                           // (timing experiments: make ablf F=specaug D=-DLAS_SPECAUG_TILE=64)
#endif
constexpr int TILE = LAS_SPECAUG_TILE;                // frames per workgroup
constexpr int MASKS_MAX = 16;                         // mF, mT
constexpr int T_MAX = 32768;                          // t * w0 and its right-hand twin stay below 2^30

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));      // a 16-byte load from any 4-byte boundary

struct Frame { int i0; float frac; };                 // source of an output frame: i0 < 0 = zeros; frac == 0 = a bit copy of x[i0]

__device__ __forceinline__ bool col_masked(const int* cols, int mF, int c) {
    bool hit = false;
    for (int m = 0; m < mF; ++m) hit |= c >= cols[2 * m] && c < cols[2 * m + 1];
    return hit;
}

// One element, without a branch (a quad across a frame boundary or a mask edge issues its eight loads back to back): a masked element
// reads the row's element 0 instead of its source and drops it; with frac == 0 the second load repeats the first (x[i0 + 1] is not read).
__device__ __forceinline__ float element(const float* __restrict__ irow, int FC, Frame fr, int c, bool masked) {
    const bool ok = fr.i0 >= 0 && !masked;
    const int off = ok ? fr.i0 * FC + c : 0;
    const float x0 = irow[off], x1 = irow[off + ((ok && fr.frac != 0.f) ? FC : 0)];
    const float v = fr.frac == 0.f ? x0 : fmaf(fr.frac, x1 - x0, x0);
    return ok ? v : 0.f;
}

__global__ __launch_bounds__(NT) void specaug_kernel(const float* __restrict__ in, const int* __restrict__ plan, int ldp, int Tmax, int FC, int C,
                                                     int mF, int mT, float* __restrict__ out) {
    __shared__ int pl[4 + 4 * MASKS_MAX];
    __shared__ int cols[2 * MASKS_MAX];               // the frequency masks as flat column ranges [f0 C, (f0 + fw) C)
    __shared__ Frame frames[TILE];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int np = 4 + 2 * (mF + mT);
    for (int k = tid; k < np; k += NT) pl[k] = plan[(long long)b * ldp + k];
    __syncthreads();
    // (the entry validated the HOST copy of the plan; the clamps below keep every read inside the row whatever the device copy holds)
    const int len = min(max(pl[0], 0), Tmax), w0 = pl[1], w = pl[2];
    const bool warp = w != 0 && w0 >= 1 && w0 + w >= 1 && w0 <= len - 2 && w0 + w <= len - 2 && Tmax <= T_MAX;
    const int tbase = blockIdx.x * TILE;
    if (tid < 2 * mF) cols[tid] = (tid & 1) ? (pl[4 + tid - 1] + pl[4 + tid]) * C : pl[4 + tid] * C;
    static_assert(TILE <= NT, "one thread per frame of the tile");
    if (tid < TILE) {
        const int t = tbase + tid;
        Frame fr = {-1, 0.f};
        if (t < len) {
            bool hit = false;
            const int* tm = pl + 4 + 2 * mF;
            for (int m = 0; m < mT; ++m) hit |= t >= tm[2 * m] && t < tm[2 * m] + tm[2 * m + 1];
            if (!hit) {
                fr.i0 = t;
                if (warp) {
                    int num, den, off;
                    if (t <= w0 + w) { num = t * w0;                          den = w0 + w;           off = 0; }
                    else             { num = (t - (w0 + w)) * (len - 1 - w0); den = len - 1 - w0 - w; off = w0; }
                    const int q = num / den, r = num - q * den;
                    fr.i0 = off + q;
                    fr.frac = r ? (float)r / (float)den : 0.f;
                }
            }
        }
        frames[tid] = fr;
    }
    __syncthreads();
    const long long row = (long long)b * Tmax * FC;
    const float* irow = in + row;
    float* o = out + row + (long long)tbase * FC;
    const int n = min(TILE, Tmax - tbase) * FC;       // (Tmax * FC <= INT32_MAX: the entry's limit)
    const int head = min(n, (int)((4 - (((uintptr_t)o >> 2) & 3)) & 3));
    const int nq = (n - head) >> 2;

    auto one = [&](int j) {
        const int tl = j / FC, c = j - tl * FC;
        return element(irow, FC, frames[tl], c, col_masked(cols, mF, c));
    };
    if (tid < head) o[tid] = one(tid);
    for (int q = tid; q < nq; q += NT) {
        const int j = head + 4 * q;
        const int tl = j / FC, c = j - tl * FC;
        const Frame fr = frames[tl];
        float4 y;
        if (c + 3 < FC) {                             // inside one frame
            const bool m0 = col_masked(cols, mF, c), m1 = col_masked(cols, mF, c + 1), m2 = col_masked(cols, mF, c + 2),
                       m3 = col_masked(cols, mF, c + 3);
            if (fr.i0 < 0 || (m0 & m1 & m2 & m3)) y = make_float4(0.f, 0.f, 0.f, 0.f);
            else if (!(m0 | m1 | m2 | m3)) {
                const float* x = irow + fr.i0 * FC + c;
                const f4u x0 = *(const f4u*)x, x1 = *(const f4u*)(x + (fr.frac != 0.f ? FC : 0));
                if (fr.frac == 0.f) y = make_float4(x0.x, x0.y, x0.z, x0.w);
                else y = make_float4(fmaf(fr.frac, x1.x - x0.x, x0.x), fmaf(fr.frac, x1.y - x0.y, x0.y), fmaf(fr.frac, x1.z - x0.z, x0.z),
                                     fmaf(fr.frac, x1.w - x0.w, x0.w));
            } else {
                y = make_float4(element(irow, FC, fr, c, m0), element(irow, FC, fr, c + 1, m1), element(irow, FC, fr, c + 2, m2),
                                element(irow, FC, fr, c + 3, m3));
            }
        } else {
            y = make_float4(one(j), one(j + 1), one(j + 2), one(j + 3));
        }
        *(float4*)(o + j) = y;
    }
    const int jt = head + 4 * nq + tid;
    if (jt < n) o[jt] = one(jt);
}

}  // namespace

extern "C" int las_specaug_tile(void) { return TILE; }

extern "C" int las_specaug(const las_specaug_args* a, void* stream) {
    LAS_ARG(a != nullptr, "las_specaug: null argument struct");
    LAS_ARG(a->B >= 1 && a->B <= 65535, "las_specaug: bad batch (B=%d, 1..65535)", a->B);
    LAS_ARG(a->Tmax >= 1 && a->Tmax <= T_MAX, "las_specaug: Tmax=%d (1..%d: the warp's products are formed in 32 bits)", a->Tmax, T_MAX);
    LAS_ARG(a->F >= 1 && a->C >= 1, "las_specaug: F=%d, C=%d (>= 1 each)", a->F, a->C);
    LAS_ARG(a->mF >= 0 && a->mF <= MASKS_MAX && a->mT >= 0 && a->mT <= MASKS_MAX, "las_specaug: mF=%d, mT=%d masks (0..%d each)", a->mF, a->mT, MASKS_MAX);
    const long long per_row = (long long)a->Tmax * a->F * a->C;
    LAS_ARG((long long)a->F * a->C <= INT32_MAX && per_row <= INT32_MAX, "las_specaug: an utterance of Tmax x F x C = %d x %d x %d elements (at most INT32_MAX)",
            a->Tmax, a->F, a->C);
    const int need = 4 + 2 * (a->mF + a->mT);
    LAS_ARG(a->ldp >= need && a->ldp % 4 == 0, "las_specaug: ldp=%d (a multiple of 4, >= 4 + 2 (mF + mT) = %d)", a->ldp, need);
    LAS_ARG(a->in && a->out && a->plan && a->plan_host, "las_specaug: null pointer (in, out, plan, plan_host)");
    LAS_ARG(((uintptr_t)a->in & 3) == 0 && ((uintptr_t)a->out & 3) == 0 && ((uintptr_t)a->plan & 3) == 0, "las_specaug: in, out and plan are 4-byte aligned");
    const uintptr_t bytes = (uintptr_t)per_row * a->B * 4, pi = (uintptr_t)a->in, po = (uintptr_t)a->out;
    LAS_ARG(pi + bytes <= po || po + bytes <= pi, "las_specaug: in %p and out %p overlap (%llu bytes each): the warp reads frames other workgroups write",
            (const void*)a->in, (const void*)a->out, (unsigned long long)bytes);
    for (int b = 0; b < a->B; ++b) {
        const int* p = a->plan_host + (long long)b * a->ldp;
        const int len = p[0], w0 = p[1], w = p[2];
        LAS_ARG(len >= 0 && len <= a->Tmax, "las_specaug: row %d has len=%d (0..Tmax=%d)", b, len, a->Tmax);
        LAS_ARG(w == 0 || (w0 >= 1 && (long long)w0 + w >= 1 && (long long)w0 + w <= len - 2 && w0 <= len - 2),
                "las_specaug: row %d warp w0=%d, w=%d leaves an empty segment (len=%d: 1 <= w0, w0 + w <= len - 2)", b, w0, w, len);
        for (int m = 0; m < a->mF; ++m) {
            const int f0 = p[4 + 2 * m], fw = p[5 + 2 * m];
            LAS_ARG(f0 >= 0 && fw >= 0 && (long long)f0 + fw <= a->F, "las_specaug: row %d frequency mask %d f0=%d, fw=%d outside [0, F=%d]", b, m, f0, fw, a->F);
        }
        for (int m = 0; m < a->mT; ++m) {
            const int t0 = p[4 + 2 * a->mF + 2 * m], tw = p[5 + 2 * a->mF + 2 * m];
            LAS_ARG(t0 >= 0 && tw >= 0 && (long long)t0 + tw <= len, "las_specaug: row %d time mask %d t0=%d, tw=%d outside [0, len=%d]", b, m, t0, tw, len);
        }
    }
    const dim3 grid(cdiv(a->Tmax, TILE), a->B);
    hipLaunchKernelGGL(specaug_kernel, grid, dim3(NT), 0, (hipStream_t)stream, a->in, a->plan, a->ldp, a->Tmax, a->F * a->C, a->C, a->mF, a->mT, a->out);
    LAS_LAUNCHED();
    return 0;
}
