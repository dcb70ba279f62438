// vad.hip -- energy voice-activity detector and segmenter in front of the audio front end (las_hip.h K15): a batch of
// recordings of very different lengths (a ten-second clip next to a one-hour file) -> per recording the runs [a, b) of frames that hold
// speech.  The frames are the front end's (T_u = floor((n_u - fl) / step), frame t = samples [t step, t step + fl)).
//
// Six launches, stream-ordered on the caller's stream, no atomics.  TILE = 64 frames = one wave, so every per-tile scan is a ballot
// and bit arithmetic on a 64-bit mask; (tile, recording) grids parallelise over TIME within a row, the per-row kernels only walk
// per-tile summaries.
//   vad_energy_kernel   (tile, u), four waves.  Stages the tile's sample span ((nf - 1) step + fl samples: frames overlap fl / step = 2.5 x)
//                       into LDS once, rows of `step` samples at a pitch of step + pad words with the pitch ODD: lane l = frame l
//                       reads word (l + j) pitch + r at the same moment, 32 distinct banks per 32-lane group.  e[t] is the
//                       SEQUENTIAL double sum of x x over the frame (x x is exact in double: one rounding per sample, the bits
//                       of a numpy loop); the order is the contract, so the only parallelism is across frames: the first wave sums,
//                       the other three only help to keep loads in flight while the span is staged.  When the span of 64
//                       frames does not fit the staging buffer (48 kHz: 480-sample steps) the tile is done in passes of S frames.
//                       Writes e (0 behind T_u) and the tile's peak.
//   vad_peak_kernel     (u).  emax = max over the tile peaks in a fixed order, thr = max(emax ratio, floor).
//   vad_tiles_kernel    (tile, u).  raw = e >= thr && e > 0 as a 64-bit mask; the tile's first and last raw frame and the number of
//                       gaps of >= 2 hang + 2 between raw frames INSIDE the tile.  Dilating raw by hang and taking maximal stretches
//                       is the same as: a run starts hang frames before a raw frame whose predecessor raw frame is >= 2 hang + 2
//                       away (or absent), and ends hang + 1 behind a raw frame whose successor is that far away -- no window loop,
//                       whatever hang is.
//   vad_scan_kernel     (u).  Over the tile summaries, 1024 tiles per pass with a carry: the last raw frame in front of every tile
//                       (max-scan), the first one behind it (min-scan from the end), and the exclusive prefix sums of the
//                       tile's run starts and of its run ends, separately.
//   vad_emit_kernel     (tile, u).  Start flags and end flags again, now with the neighbours' raw frames; the k-th start of the row goes
//                       to starts[k], the k-th end to ends[k] (rank = tile prefix + popcount below the lane): a stream compaction.
//   vad_compact_kernel  (u).  Pairs starts[k] with ends[k], drops runs shorter than min_run, compacts what is left into runs (block
//                       prefix sums with a carry) and writes n_runs.
// Every value depends on (row u, its samples, the scalar arguments) only: not on TILE, not on the batch.
#include "las_common.h"
#include <math.h>
#include <limits.h>

namespace {

constexpr int TILE = 64;                              // frames per workgroup = lanes of a wave
constexpr int LDS_WORDS = 12288;                      // 48 KB staging buffer: 66 rows of 161 words at fl = 400, step = 160 (three workgroups per CU)
constexpr int NT_STAGE = 256;                         // threads of the energy kernel: four waves stage the span, the first one sums
constexpr int NT_ROW = 1024;                          // threads of the per-row kernels = tile summaries (runs) per pass
constexpr int NONE_NEXT = INT_MAX;                    // "no raw frame behind" (no raw frame in front: -1)

__device__ __forceinline__ int frames_of(int n_u, int fl, int step, long long ld, int Tmax) {
    n_u = (int)min((long long)n_u, ld);
    const int T = n_u >= fl ? (n_u - fl) / step : 0;
    return min(T, Tmax);
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// S: frames per staging pass (1..64), 0 = the span of one frame does not fit: frames read their samples from memory
template <bool I16>
__global__ __launch_bounds__(NT_STAGE) void vad_energy_kernel(const void* __restrict__ samples, long long ld, const int* __restrict__ n_samples,
                                                          int Tmax, int fl, int step, int S, int pitch, double* __restrict__ e,
                                                          double* __restrict__ tile_max, int ntile) {
    __shared__ float xs[LDS_WORDS];
    const int lane = threadIdx.x, u = blockIdx.y, tile = blockIdx.x;
    const int T = frames_of(n_samples[u], fl, step, ld, Tmax);
    const int t0 = tile * TILE;                       // (t0 < Tmax: the grid)
    const int live = min(max(T - t0, 0), TILE);       // live frames of this tile
    const long long row = (long long)u * ld;
    const int P = S > 0 ? S : TILE;
    double peak = 0.0;
    for (int f0 = 0; f0 < live; f0 += P) {            // (uniform)
        const int nf = min(P, live - f0);
        const long long base = row + (long long)(t0 + f0) * step;      // every sample read below is < row + (T - 1) step + fl <= row + n_u
        double acc = 0.0;
        if (S > 0) {
            const int span = (nf - 1) * step + fl;
            __syncthreads();                          // the previous pass has been read
#pragma unroll 8
            for (int g = lane; g < span; g += NT_STAGE) xs[g + (pitch - step) * (g / step)] = sample_at<I16>(samples, base + g);
            __syncthreads();
            if (lane < nf) {
                const float* rowp = xs + lane * pitch;
                for (int i = 0; i < fl; i += step, rowp += pitch) {
                    const int m = min(step, fl - i);
#pragma unroll 8
                    for (int r = 0; r < m; ++r) { const double x = (double)rowp[r]; acc = fma(x, x, acc); }
                }
            }
        } else if (lane < nf) {
            const long long b = base + (long long)lane * step;
            for (int i = 0; i < fl; ++i) { const double x = (double)sample_at<I16>(samples, b + i); acc = fma(x, x, acc); }
        }
        if (lane < nf) {
            e[(long long)u * Tmax + t0 + f0 + lane] = acc;
            peak = fmax(peak, acc);
        }
    }
    for (int f = live + lane; f < TILE && t0 + f < Tmax; f += NT_STAGE) e[(long long)u * Tmax + t0 + f] = 0.0;
    peak = wave_max_f64(peak);                        // (nf <= 64: the frames are the first wave's)
    if (lane == 0) tile_max[(long long)u * ntile + tile] = peak;
}

__global__ __launch_bounds__(NT_ROW) void vad_peak_kernel(const double* __restrict__ tile_max, int ntile, double ratio, double floor_,
                                                          double* __restrict__ thr, double* __restrict__ emax) {
    __shared__ double red[NT_ROW / 64];
    const int u = blockIdx.x;
    double m = 0.0;
    for (int j = threadIdx.x; j < ntile; j += NT_ROW) m = fmax(m, tile_max[(long long)u * ntile + j]);
    m = wave_max_f64(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = red[0];
        for (int i = 1; i < NT_ROW / 64; ++i) m = fmax(m, red[i]);
        thr[u] = fmax(m * ratio, floor_);
        if (emax) emax[u] = m;
    }
}

// the tile's raw frames as a mask (bit l = frame t0 + l); every lane of the wave calls it
__device__ __forceinline__ unsigned long long raw_mask(const double* __restrict__ e, long long erow, int t0, int T, double thr) {
    const int t = t0 + (int)threadIdx.x;
    const double v = t < T ? e[erow + t] : 0.0;
    return __ballot(v >= thr && v > 0.0);
}

struct TileSum { int first, last, gaps, pad; };       // first / last raw frame of the tile (-1: none), gaps >= G between raw frames inside it
struct TileOff { int prev, next, start_off, end_off; };   // last raw frame in front (-1) / first behind (NONE_NEXT); runs started / ended in front

__global__ __launch_bounds__(TILE) void vad_tiles_kernel(const double* __restrict__ e, const int* __restrict__ n_samples, long long ld, int Tmax,
                                                         int fl, int step, const double* __restrict__ thr, long long G,
                                                         TileSum* __restrict__ sums, int ntile) {
    const int lane = threadIdx.x, u = blockIdx.y, tile = blockIdx.x;
    const int T = frames_of(n_samples[u], fl, step, ld, Tmax);
    const unsigned long long M = raw_mask(e, (long long)u * Tmax, tile * TILE, T, thr[u]);
    const unsigned long long below = M & ((1ull << lane) - 1ull);
    const bool gap = ((M >> lane) & 1ull) && below && (long long)(lane - (63 - __clzll(below))) >= G;
    const unsigned long long gm = __ballot(gap);
    if (lane == 0) {
        TileSum s = {-1, -1, 0, 0};
        if (M) { s.first = tile * TILE + (__ffsll(M) - 1); s.last = tile * TILE + 63 - __clzll(M); s.gaps = __popcll(gm); }
        sums[(long long)u * ntile + tile] = s;
    }
}

// scan over the NT_ROW threads, every thread calls it: inside the wave by shuffles, across the waves through one LDS exchange (two
// barriers; integers: the order does not matter).  ident: the operation's identity.
struct Scan { int incl, excl, total; };
template <class Op>
__device__ __forceinline__ Scan block_scan(int v, int* buf, Op op, int ident) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(v, o);
        if (lane >= o) v = op(x, v);
    }
    const int below = __shfl_up(v, 1);
    __syncthreads();                                  // (buf's readers of the previous call are through)
    if (lane == 63) buf[w] = v;
    __syncthreads();
    int pre = ident, total = ident;
#pragma unroll
    for (int i = 0; i < NT_ROW / 64; ++i) {
        if (i == w) pre = total;
        total = op(total, buf[i]);
    }
    Scan r;
    r.incl = op(pre, v);
    r.excl = lane ? op(pre, below) : pre;
    r.total = total;
    return r;
}

__global__ __launch_bounds__(NT_ROW) void vad_scan_kernel(const TileSum* __restrict__ sums, TileOff* __restrict__ offs, int ntile, long long G,
                                                          int* __restrict__ n_raw_runs) {
    __shared__ int buf[NT_ROW / 64];
    const int tid = threadIdx.x, u = blockIdx.x;
    sums += (long long)u * ntile;
    offs += (long long)u * ntile;
    auto imin = [](int a, int b) { return min(a, b); };
    auto imax = [](int a, int b) { return max(a, b); };
    auto iadd = [](int a, int b) { return a + b; };
    // from the end: the first raw frame behind every tile
    int carry = NONE_NEXT;
    for (int hi = ntile; hi > 0; hi -= NT_ROW) {      // (uniform)
        const int j = hi - 1 - tid;
        const int f = j >= 0 ? sums[j].first : -1;
        const Scan sc = block_scan(f >= 0 ? f : NONE_NEXT, buf, imin, NONE_NEXT);
        if (j >= 0) offs[j].next = min(carry, sc.excl);
        carry = min(carry, sc.total);
    }
    __syncthreads();                                  // offs[].next is read below by other threads than wrote it
    // from the front: the last raw frame in front of every tile, then the runs started and ended in front of it
    int prev_c = -1, start_c = 0, end_c = 0;
    for (int lo = 0; lo < ntile; lo += NT_ROW) {
        const int j = lo + tid;
        TileSum s = {-1, -1, 0, 0};
        if (j < ntile) s = sums[j];
        const Scan sp = block_scan(s.last, buf, imax, -1);
        const int prev = max(prev_c, sp.excl);
        prev_c = max(prev_c, sp.total);
        int ns = 0, ne = 0;
        if (s.first >= 0) {
            const int next = offs[j].next;
            ns = s.gaps + ((prev < 0 || (long long)s.first - prev >= G) ? 1 : 0);
            ne = s.gaps + ((next == NONE_NEXT || (long long)next - s.last >= G) ? 1 : 0);
        }
        const Scan ss = block_scan(ns, buf, iadd, 0);
        const Scan se = block_scan(ne, buf, iadd, 0);
        if (j < ntile) { offs[j].prev = prev; offs[j].start_off = start_c + ss.excl; offs[j].end_off = end_c + se.excl; }
        start_c += ss.total;
        end_c += se.total;
    }
    if (tid == 0) n_raw_runs[u] = start_c;            // (== end_c: every run has one start and one end)
}

__global__ __launch_bounds__(TILE) void vad_emit_kernel(const double* __restrict__ e, const int* __restrict__ n_samples, long long ld, int Tmax,
                                                        int fl, int step, const double* __restrict__ thr, long long G, int hang,
                                                        const TileOff* __restrict__ offs, int ntile, int* __restrict__ starts,
                                                        int* __restrict__ ends, long long cap) {
    const int lane = threadIdx.x, u = blockIdx.y, tile = blockIdx.x;
    const int T = frames_of(n_samples[u], fl, step, ld, Tmax);
    const unsigned long long M = raw_mask(e, (long long)u * Tmax, tile * TILE, T, thr[u]);
    if (!M) return;                                   // (uniform)
    const TileOff o = offs[(long long)u * ntile + tile];
    const int t = tile * TILE + lane;
    const bool raw = (M >> lane) & 1ull;
    const unsigned long long below = M & ((1ull << lane) - 1ull), above = lane == 63 ? 0ull : M & ~((2ull << lane) - 1ull);
    const long long prev = below ? tile * TILE + 63 - __clzll(below) : o.prev;
    const long long next = above ? tile * TILE + (__ffsll(above) - 1) : o.next;
    const bool is_start = raw && (prev < 0 || t - prev >= G);
    const bool is_end = raw && (next == NONE_NEXT || next - t >= G);
    const unsigned long long sm = __ballot(is_start), em = __ballot(is_end);
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (is_start) {
        const long long k = o.start_off + __popcll(sm & lt);
        if (k < cap) starts[(long long)u * cap + k] = (int)max((long long)t - hang, 0ll);
    }
    if (is_end) {
        const long long k = o.end_off + __popcll(em & lt);
        if (k < cap) ends[(long long)u * cap + k] = (int)min((long long)t + hang + 1, (long long)T);
    }
}

__global__ __launch_bounds__(NT_ROW) void vad_compact_kernel(const int* __restrict__ starts, const int* __restrict__ ends, long long cap,
                                                             const int* __restrict__ n_raw_runs, int min_run, int* __restrict__ runs,
                                                             int max_runs, int* __restrict__ n_runs) {
    __shared__ int buf[NT_ROW / 64];
    const int tid = threadIdx.x, u = blockIdx.x;
    const int R = (int)min((long long)n_raw_runs[u], cap);
    auto iadd = [](int a, int b) { return a + b; };
    int kept = 0;
    for (int c0 = 0; c0 < R; c0 += NT_ROW) {          // (uniform)
        const int k = c0 + tid;
        int a = 0, b = 0;
        if (k < R) { a = starts[(long long)u * cap + k]; b = ends[(long long)u * cap + k]; }
        const int keep = (k < R && b - a >= min_run) ? 1 : 0;
        const Scan sc = block_scan(keep, buf, iadd, 0);
        const int pos = kept + sc.excl;
        if (keep && pos < max_runs) {
            runs[((long long)u * max_runs + pos) * 2] = a;
            runs[((long long)u * max_runs + pos) * 2 + 1] = b;
        }
        kept += sc.total;
    }
    if (tid == 0) n_runs[u] = min(kept, max_runs);
}

size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the workspace: [e f64 [n, Tmax] | tile peaks f64 [n, ntile] | thr f64 [n] | sums [n, ntile] | offs [n, ntile] | raw runs i32 [n] |
// starts i32 [n, cap] | ends i32 [n, cap]], cap = ceil(Tmax / 2) = las_vad_max_runs(Tmax, 0)
struct Layout { size_t e, tmax, thr, sums, offs, nraw, starts, ends, total; long long ntile, cap; };
Layout layout(int n, long long Tmax) {
    Layout L;
    L.ntile = (Tmax + TILE - 1) / TILE;
    L.cap = (Tmax + 1) / 2;
    size_t o = 0;
    L.e = o;      o += up256((size_t)n * Tmax * sizeof(double));
    L.tmax = o;   o += up256((size_t)n * L.ntile * sizeof(double));
    L.thr = o;    o += up256((size_t)n * sizeof(double));
    L.sums = o;   o += up256((size_t)n * L.ntile * sizeof(TileSum));
    L.offs = o;   o += up256((size_t)n * L.ntile * sizeof(TileOff));
    L.nraw = o;   o += up256((size_t)n * sizeof(int));
    L.starts = o; o += up256((size_t)n * L.cap * sizeof(int));
    L.ends = o;   o += up256((size_t)n * L.cap * sizeof(int));
    L.total = o;
    return L;
}

}  // namespace

extern "C" int las_vad_tile(void) { return TILE; }

extern "C" long long las_vad_max_runs(long long T, int hang) {
    if (T < 0 || hang < 0) return -1;
    const long long G = 2ll * hang + 2;
    return (T + G - 1) / G;
}

extern "C" size_t las_vad_workspace_bytes(int n, long long Tmax) {
    if (n < 1 || Tmax < 1 || Tmax > INT32_MAX) return 0;
    return layout(n, Tmax).total;
}

extern "C" int las_vad(const void* samples, int samples_i16, long long ld_samples, const int* n_samples, const int* n_samples_host, int n,
                       int Tmax, int fl, int step, double ratio, double floor, int hang, int min_run, double* energy, double* emax,
                       int* runs, int max_runs, int* n_runs, void* ws, size_t ws_bytes, void* stream) {
    LAS_ARG(samples && n_samples && n_samples_host && runs && n_runs && ws, "las_vad: null pointer (samples, n_samples, n_samples_host, runs, n_runs, ws)");
    LAS_ARG(n >= 1 && n <= 65535 && Tmax >= 1, "las_vad: bad batch (n=%d, 1..65535; Tmax=%d, >= 1)", n, Tmax);
    LAS_ARG(fl >= 1 && step >= 1, "las_vad: frame of %d samples every %d (>= 1 each)", fl, step);
    LAS_ARG(hang >= 0, "las_vad: hang=%d (>= 0)", hang);
    LAS_ARG(min_run >= 2, "las_vad: min_run=%d (>= 2: a run of r frames yields r - 1 front-end frames)", min_run);
    LAS_ARG(ratio > 0.0 && ratio <= 1.0, "las_vad: ratio=%g (0 < ratio <= 1)", ratio);
    LAS_ARG(isfinite(floor) && floor >= 0.0, "las_vad: floor=%g (finite, >= 0)", floor);
    LAS_ARG(max_runs >= las_vad_max_runs(Tmax, hang), "las_vad: max_runs=%d, %lld runs fit Tmax=%d frames at hang=%d", max_runs,
            las_vad_max_runs(Tmax, hang), Tmax, hang);
    LAS_ARG(ld_samples >= 1 && ld_samples <= INT32_MAX, "las_vad: ld_samples=%lld", ld_samples);
    for (int u = 0; u < n; ++u) {
        const long long nu = n_samples_host[u];
        LAS_ARG(nu >= 1 && nu <= ld_samples, "las_vad: recording %d has %lld samples (1..ld_samples=%lld)", u, nu, ld_samples);
        const long long T = nu >= fl ? (nu - fl) / step : 0;
        LAS_ARG(T <= Tmax, "las_vad: recording %d has %lld frames (Tmax=%d)", u, T, Tmax);
    }
    const size_t need = las_vad_workspace_bytes(n, Tmax);
    LAS_ARG(ws_bytes >= need, "las_vad: workspace of %zu bytes, %zu needed", ws_bytes, need);
    LAS_ARG(((uintptr_t)ws & 7) == 0, "las_vad: ws is 8-byte aligned");
    const Layout L = layout(n, Tmax);
    char* w = (char*)ws;
    double* e = energy ? energy : (double*)(w + L.e);
    double* tmax = (double*)(w + L.tmax);
    double* thr = (double*)(w + L.thr);
    TileSum* sums = (TileSum*)(w + L.sums);
    TileOff* offs = (TileOff*)(w + L.offs);
    int* nraw = (int*)(w + L.nraw);
    int* starts = (int*)(w + L.starts);
    int* ends = (int*)(w + L.ends);
    const int ntile = (int)L.ntile;
    const long long G = 2ll * hang + 2;
    // staging: rows of `step` samples at an odd pitch; S frames per pass need S - 1 + ceil(fl / step) rows
    const long long pitch = (long long)step + ((step & 1) ? 0 : 1);
    const long long rows_fl = ((long long)fl + step - 1) / step;
    long long S = LDS_WORDS / pitch - rows_fl + 1;
    S = S < 1 ? 0 : (S > TILE ? TILE : S);
    hipStream_t st = (hipStream_t)stream;
    const dim3 gt(ntile, n);
    if (samples_i16)
        hipLaunchKernelGGL(vad_energy_kernel<true>, gt, dim3(NT_STAGE), 0, st, samples, ld_samples, n_samples, Tmax, fl, step, (int)S, (int)pitch, e, tmax, ntile);
    else
        hipLaunchKernelGGL(vad_energy_kernel<false>, gt, dim3(NT_STAGE), 0, st, samples, ld_samples, n_samples, Tmax, fl, step, (int)S, (int)pitch, e, tmax, ntile);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(vad_peak_kernel, dim3(n), dim3(NT_ROW), 0, st, tmax, ntile, ratio, floor, thr, emax);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(vad_tiles_kernel, gt, dim3(TILE), 0, st, e, n_samples, ld_samples, Tmax, fl, step, thr, G, sums, ntile);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(vad_scan_kernel, dim3(n), dim3(NT_ROW), 0, st, sums, offs, ntile, G, nraw);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(vad_emit_kernel, gt, dim3(TILE), 0, st, e, n_samples, ld_samples, Tmax, fl, step, thr, G, hang, offs, ntile, starts, ends, L.cap);
    LAS_LAUNCHED();
    hipLaunchKernelGGL(vad_compact_kernel, dim3(n), dim3(NT_ROW), 0, st, starts, ends, L.cap, nraw, min_run, runs, max_runs, n_runs);
    LAS_LAUNCHED();
    return 0;
}
