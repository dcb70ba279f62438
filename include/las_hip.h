/* las_hip.h -- C ABI of liblas_hip.so, the MI355X (gfx950) engine behind the LAS hot path.
 *
 * The reference (30stomercury/Automatic-Speech-Recognition) has no FFI: its hot path sits
 * behind the TensorFlow session boundary  sess.run(fetches, feed_dict)  (train.py:115-117,
 * test.py:107, las/beam_search.py:209,222).  This header is what replaces that boundary: each
 * entry point names the reference graph fragment (file:line) whose stock TF ops it stands in for.
 *
 * Conventions
 *   - extern "C"; raw DEVICE pointers owned by the caller; the library never allocates or frees
 *     caller tensors.  Scratch is passed in explicitly (ws, ws_bytes), sized by *_workspace_bytes.
 *   - every dimension / leading dimension is an explicit int; tensors are fp32 in HBM (speed mode: the Listener's
 *     activations are bf16, see LAS_DT_*), row-major,
 *     batch-major [B,T,C] exactly as the reference lays them out (time_major=False,
 *     las/layers.py:24,53).  Weights keep the TF layout [in,out] with the [x;h] row concat and
 *     gate order i,j,f,o.
 *   - `prec` selects the arithmetic of the contractions:  LAS_PREC_F32 = exact fp32 FMA chains
 *     (parity mode), LAS_PREC_BF16 = operands rounded to bf16 (RNE), fp32 MFMA accumulation
 *     (speed mode).  Recurrent state, accumulators, parameters, parameter gradients and optimiser math are always fp32.
 *   - `stream` is a hipStream_t (passed as void*); all work is enqueued asynchronously on it,
 *     no hidden synchronisation, no global mutable state besides an init-once attribute cache; the library
 *     reads no environment variables (development switches are explicit `flags` arguments).
 *   - return value: 0 ok; <0 invalid argument / unsupported shape (message via las_last_error());
 *     >0 a hipError_t.
 */
#ifndef LAS_HIP_H
#define LAS_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { LAS_PREC_F32 = 0, LAS_PREC_BF16 = 1 };
enum { LAS_CELL_RNN = 0, LAS_CELL_LSTM = 1 };   /* BasicRNNCell (las/layers.py:31) / BasicLSTMCell */
enum { LAS_ACT_NONE = 0, LAS_ACT_TANH = 1 };
enum { LAS_ATT_ADD = 0, LAS_ATT_LOC = 1 };      /* las/las.py:44-49 */
enum { LAS_DT_F32 = 0, LAS_DT_BF16 = 1 };       /* element type of a tensor in HBM (see las_gemm_kk) */

#define LAS_HIP_ABI_VERSION 611      /* bumped whenever an argument struct or a signature changes: las_version() of a library
                                        built from another header differs, and the Python loader refuses it */
int         las_version(void);
const char* las_last_error(void);

/* ------------------------------------------------------------------------------------------
 * K1/K3/K4  dense contractions  (tf.layers.dense / Tensordot->MatMul+BiasAdd(+Tanh):
 * las/layers.py:71-74, :89-93, :250-251, :305; the input half of the cell MatMul las/layers.py:31;
 * and every matmul gradient of those ops).
 *   C[b] = act( alpha * op(A[b]) . op(B[b]) + beta * C[b] + bias )      b = 0..batch-1
 * op(A) is M x K, op(B) is K x N.  transX=0: X stored row-major as written; transX=1: stored
 * transposed (A as K x M, B as N x K).  bias (length N) may be NULL.
 * a_mask_period > 0: logical rows r of the CONTRACTION index of a transA=1 product with
 * (r % a_mask_period) == a_mask_skip contribute zero -- used for dW_hh = sum_t h_{t-1}^T dG_t where
 * the t=0 (fw) / t=T-1 (bw) frame has no predecessor inside its utterance (needs lda > 1: an A of one column
 * at pitch 1 is refused).
 * ws (optional, may be NULL): scratch for a deterministic split-K of tall contractions
 * (partials [s][M][N] reduced in fixed order); without it the product runs unsplit.
 */
int las_gemm(int prec, int transA, int transB, int M, int N, int K,
             float alpha, const float* A, int lda, long long strideA,
             const float* B, int ldb, long long strideB,
             float beta, float* C, int ldc, long long strideC,
             const float* bias, int act, int batch,
             int a_mask_period, int a_mask_skip, void* ws, size_t ws_bytes, void* stream);

/* Scratch las_gemm's split-K wants for this product (0: it runs unsplit); at most LAS_GEMM_WS_CAP.  A caller that passes at least
 * this much gets the same split -- hence bit-identical sums -- whatever else its buffer could hold. */
#define LAS_GEMM_WS_CAP ((size_t)256 << 20)
size_t las_gemm_workspace_bytes(int prec, int M, int N, int K, int batch);

/* las_gemm with both operands in `in_dtype` (LAS_DT_F32 = las_gemm; LAS_DT_BF16: activations / gradients that already
 * live in HBM as bf16 -- the weight-gradient contractions X^T . dZ of the speed mode; branch-free path only: aligned
 * pitches, K resp. row counts multiples of 4, no contraction mask).  C, bias fp32. */
int las_gemm_dt(int prec, int transA, int transB, int M, int N, int K,
                float alpha, const void* A, int lda, long long strideA,
                const void* B, int ldb, long long strideB, int in_dtype,
                float beta, float* C, int ldc, long long strideC,
                const float* bias, int act, int batch,
                int a_mask_period, int a_mask_skip, void* ws, size_t ws_bytes, void* stream);

/* What a las_gemm_dt call with these arguments launches: every decision of the dispatch (kernel family, tile, loader, operand type,
 * grid order, split-K and the grid), made by the one host function the launch itself follows.  Pure host arithmetic, no GPU: the
 * operands enter as a_align / b_align, their addresses modulo 16, and the scratch as ws_bytes (0 = none).  Returns 0, or a negative
 * value with las_gemm_dt's las_last_error text wherever that would refuse the call (e.g. bf16 operands off the branch-free path).
 * M == 0 or N == 0: kernel = LAS_GEMM_K_NONE, nothing is launched.  A test can so name the kernel a case ran, and a table of cases can
 * be held to the set of plans that are reachable at all. */
enum { LAS_GEMM_K_NONE = 0, LAS_GEMM_K_BF16_GENERIC = 1, LAS_GEMM_K_BF16_FAST = 2, LAS_GEMM_K_TN_TR = 3, LAS_GEMM_K_MF32 = 4,
       LAS_GEMM_K_MF32_SKINNY = 5 };
typedef struct las_gemm_plan_info {
    int kernel;              /* LAS_GEMM_K_* */
    int tile_m, tile_n;      /* output tile of a workgroup: 48 / 64 / 128 x 64 / 128; skinny: 16 * row tiles x 32 */
    int loader;              /* BF16_FAST: bit 0 = A k-contiguous, bit 1 = B k-contiguous; MF32 / MF32_SKINNY: 0 = generic loader, 1 + (A k-
                                contiguous) + 2 (B k-contiguous) = branch-free loader; else 0 */
    int in_bf16;             /* operands are bf16 in HBM */
    int grid_order;          /* 0 = plain 3-D grid, 1 = all tiles of a k-chunk / batch entry on one XCD, 2 = the column tiles of a row block on one XCD */
    int splitk, kchunk;      /* k-chunks (1 = unsplit) of kchunk contraction rows each (whole 32-wide k-tiles when split) */
    int grid_x, grid_y, grid_z;
} las_gemm_plan_info;
int las_gemm_plan(int prec, int transA, int transB, int M, int N, int K,
                  int lda, long long strideA, int ldb, long long strideB, int in_dtype,
                  int batch, int a_mask_period, unsigned a_align, unsigned b_align,
                  size_t ws_bytes, las_gemm_plan_info* out);

/* Both weight gradients of a recurrent layer's direction(s) (the matmul gradient of the cell's kernel, las/layers.py:31 under
 * bidirectional_dynamic_rnn, las/layers.py:49-53) in one pass over d(pre-activation):
 *   dW[0:I, :] += X^T . dZ_d        dW[I:I+H, :] += sum over utterances and frames of h_prev^T . dZ_d
 * X bf16 [B*T, ldx] (layer input; columns >= I up to the next multiple of 8 must be zero), out bf16 [B, Tp, ld_out >= 2 H] (batch stride
 * out_bstride elements) and dZ bf16 [B*T, lddz >= 2 GH]: the layer's output / d(pre-activation) tensors of BOTH directions (direction d's
 * column block starts at d H / d GH).  dir 0: h_prev(b, t) = out_fw[b, t-1] (zero at t = 0); dir 1: out_bw[b, t+1] (zero at t = T-1);
 * dir 2: both directions in ONE launch (dW = forward, dW2 = backward direction's gradient; X2 = the backward direction's own input copy
 * -- input dropout draws one mask per direction -- or NULL = X).  dW fp32 [I + H, GH], accumulated.  Needs H % 128 == 0, GH % 128 == 0,
 * 16-byte aligned operands, pitches multiples of 8.  Deterministic split-K over the frames (scratch from
 * las_wgrad_ih_hh_workspace_bytes(.., ndir), reduced in fixed order). */
size_t las_wgrad_ih_hh_workspace_bytes(int I, int H, int GH, int B, int T, int ndir);
/* The same contraction over a WINDOW of `nframes` frames per utterance: frames [t0_fw, t0_fw + nframes) for the forward direction's gradient,
 * [t0_bw, t0_bw + nframes) for the backward direction's (dir as below); accumulates into dW / dW2 like las_wgrad_ih_hh, so consecutive
 * windows that tile [0, T) give the whole gradient.  max_workgroups > 0 caps the launch (longer k-chunks, fewer split-K partials): a window
 * that runs beside the sweep that is producing dZ should stay small.  Workspace: las_wgrad_ih_hh_workspace_bytes of the whole sequence. */
int las_wgrad_ih_hh_window(const void* X, const void* X2, int ldx, int I, const void* out, int ld_out, long long out_bstride, const void* dZ, int lddz,
                           int B, int T, int H, int GH, int dir, int t0_fw, int t0_bw, int nframes, int max_workgroups,
                           float* dW, float* dW2, void* ws, size_t ws_bytes, void* stream);
int las_wgrad_ih_hh(const void* X, const void* X2, int ldx, int I, const void* out, int ld_out, long long out_bstride, const void* dZ, int lddz,
                    int B, int T, int H, int GH, int dir, float* dW, float* dW2, void* ws, size_t ws_bytes, void* stream);

/* Speed-mode storage type of activations in HBM.  LAS_PREC_BF16 keeps the Listener's activations (x-projections /
 * saved gates, cell states, h, dense outputs and their gradients) as bf16 -- SURVEY 8(d)'s algorithmic bytes -- while
 * accumulators, recurrent state inside the sweeps and all parameters / optimiser state stay fp32. */
/* The dependency-chain products of the Listener in speed mode, both operands bf16 with the contraction index contiguous:
 *   C[M,N] = act( A[M,K] . B[N,K]^T + bias ),   C bf16 (c_dtype = LAS_DT_BF16) or fp32.
 * x-projection and dense layers pass the bf16 shadow of W^T as B, their input gradients the shadow of W
 * (las/layers.py:31,49-53,71-74,89-93 and the matmul gradients of those ops).  K % 64 == 0 (pad with zero columns),
 * N % 4 == 0, row pitches lda / ldb multiples of 8 elements, 16-byte aligned operands.  LDS-DMA staged, 128x128x64 tiles. */
int las_gemm_kk(int M, int N, int K, const void* A, long long lda, const void* B, long long ldb,
                void* C, int c_dtype, long long ldc, const float* bias, int act, void* stream);
/* ... with the Tanh gradient of the producer of the result's consumer fused into the epilogue: C[m,n] *= 1 - y[m,n]^2
 * (y bf16, pitch ldy; NULL = las_gemm_kk).  Used for dX of a recurrent layer whose input IS the tanh output of the dense
 * layer below (las/layers.py:71-74 feeding :80): the separate las_tanh_bwd pass over dX disappears. */
int las_gemm_kk_tanhgrad(int M, int N, int K, const void* A, long long lda, const void* B, long long ldb,
                         void* C, int c_dtype, long long ldc, const float* bias, int act, const void* y, long long ldy, void* stream);

/* out[j] = beta*out[j] + sum_r X[r*ldx + j],  r < rows, j < cols   (BiasAdd gradient);
 * fixed-order two-stage reduction, ws >= las_colsum_workspace_bytes(cols). */
size_t las_colsum_workspace_bytes(int cols);
int las_colsum(const float* X, int rows, int cols, int ldx, float beta, float* out,
               void* ws, size_t ws_bytes, void* stream);

int las_colsum_dt(const void* X, int dtype, int rows, int cols, int ldx, float beta, float* out,
                  void* ws, size_t ws_bytes, void* stream);            /* X fp32 or bf16 (LAS_DT_*) */

/* dX = dY * (1 - Y*Y)   elementwise over rows x cols (Tanh gradient of dense(.., tanh)). */
int las_tanh_bwd(const float* Y, int ldy, const float* dY, int lddy, float* dX, int lddx,
                 int rows, int cols, void* stream);
int las_tanh_bwd_dt(const void* Y, int y_dt, int ldy, const void* dY, int dy_dt, int lddy, void* dX, int dx_dt, int lddx,
                    int rows, int cols, void* stream);               /* each tensor fp32 or bf16 */

/* ------------------------------------------------------------------------------------------
 * K2/K2b  recurrent sweep of one bidirectional layer
 * (tf.nn.bidirectional_dynamic_rnn without sequence_length, las/layers.py:49-53: every padded
 * frame is run; zero initial state; bw runs t=T-1..0).
 *
 * Element type of gates / out / cstate / dout: las_rnn_seq_io_dtype(cell, prec, H) -- fp32 in parity mode, bf16 in speed
 * mode (the recurrent state, accumulators and gate math stay fp32 inside the kernel).
 * gates : [B,T,2,G*H]  (G=1 rnn, 4 lstm; dir 0 = fw, 1 = bw).
 *         fwd in : x_t . W_ih + bias (the K1 product).   fwd out (lstm): activated i,j,f,o.
 *         bwd in : what fwd left.                        bwd out: d(pre-activation) for K1's bwd.
 * whh_* : [H, G*H] recurrent half of the TF kernel (row stride ldw).
 * out   : h for both directions, element (b,t,dir*H+u) at out[b*out_bstride + t*ld_out + dir*H + u]
 *         (ld_out = 2H; out_bstride lets the caller keep a zero pad frame per utterance so the
 *         pyramid concat of las/layers.py:83-88 is a pure view).
 * cstate: lstm only, [B,T,2,H] cell states (saved for bwd).
 * dout  : gradient w.r.t. out, same addressing scheme.
 */
/* `flags` (development / test switches, 0 in normal use; explicit per call -- the library reads no environment):
 *   LAS_SEQ_AGENT_GRANULES   cluster members always exchange through agent-scope (write-through) granules,
 *                            as if they ran on different XCDs
 *   LAS_SEQ_NO_KSPLIT        BPTT uses the all-gather cluster kernel instead of the K-split reduce-scatter one
 *   LAS_SEQ_NO_HELPER_WAVES  forward sweep without the helper waves that own the bulk HBM traffic
 *   LAS_SEQ_ROWS16           clustered sweeps always use 16-row batch tiles (default: 8-row tiles, i.e. twice the CUs and half
 *                            the per-lane work of a dependent step, whenever the whole batch fits one launch that way)
 *   LAS_SEQ_NO_WARMERS       clustered sweeps without the per-cluster "L2 warmer" workgroup (one extra workgroup on the cluster's
 *                            XCD that touches the operands of the next steps so that the cluster's own loads hit in L2)
 *   LAS_SEQ_F32_VALU         LAS_PREC_F32: the round-1 VALU kernels (one workgroup per (direction, 8 rows), W_hh streamed from L2)
 *                            instead of the clustered exact-fp32 MFMA kernels (csrc/rnn_seq_f32.hip) -- tests cross-check the two
 *   LAS_SEQ_P(p)             cluster width override (1, 2, 4, 8 workgroups per (direction, 16-row tile)); a width with no kernel falls
 *                            back to the next narrower one, and las_rnn_seq_plan describes the width that runs
 *   LAS_SEQ_SPIN_LOG2(n)     bound of every exchange spin = 2^n polls (default 2^22)
 *   LAS_SEQ_PREPARED         NOT a development switch: `ws` was prepared by las_rnn_seq_prepare (below) for these weights, this cell / H /
 *                            direction of the pass / flags and a batch >= B, and no sweep has used it since -- the launch then skips its own
 *                            weight pack + exchange-state clear (one launch less on the dependency chain per sweep)
 * `status` (may be NULL): caller-owned, caller-zeroed int32 DEVICE word.  The clustered bf16 sweeps exchange h / dh
 *   between workgroups with bounded spins; if a partner does not publish within the bound (it is not co-resident:
 *   shared or partitioned device) the launch finishes with undefined results and stores LAS_SEQ_STATUS_* here.
 *   The word is sticky (never cleared by the library); the caller reads it at its next synchronisation point. */
enum { LAS_SEQ_AGENT_GRANULES = 1, LAS_SEQ_NO_KSPLIT = 2, LAS_SEQ_NO_HELPER_WAVES = 4, LAS_SEQ_ROWS16 = 8, LAS_SEQ_NO_WARMERS = 16,
       LAS_SEQ_F32_VALU = 32, LAS_SEQ_PREPARED = 64 };
#define LAS_SEQ_P(p) (((p) & 0xf) << 8)
#define LAS_SEQ_SPIN_LOG2(n) (((n) & 0x1f) << 16)
/* LAS_SEQ_ANNOUNCE(n), n in 1..1023 (las_rnn_seq_bwd, clustered kernels): `status` then points to TWO ints and the launch
 * stores n into status[1] as soon as its first cluster is resident on the device -- see las_wait_word. */
#define LAS_SEQ_ANNOUNCE(n) (((n) & 0x3ff) << 21)
enum { LAS_SEQ_STATUS_OK = 0, LAS_SEQ_STATUS_FWD_TIMEOUT = 1, LAS_SEQ_STATUS_BWD_TIMEOUT = 2 };

/* Workspace of a sweep.  MANDATORY for every clustered kernel: LAS_PREC_BF16 with H in {64,128,256,512}, and -- since round 4 -- LAS_PREC_F32 with
 * those H as well (the exact-fp32 MFMA sweeps; a NULL / smaller `ws` is refused with "workspace too small", it does not fall back).  Only the
 * round-1 VALU kernels (other H, or LAS_SEQ_F32_VALU) run the forward sweep without one.  The clustered kernels also need all their workgroups
 * resident at once: on a shared / partitioned device they report LAS_SEQ_STATUS_* instead (bounded spins); pass LAS_SEQ_F32_VALU there. */
size_t las_rnn_seq_workspace_bytes(int cell, int prec, int H, int B);
/* Everything a speed-mode sweep does in front of its persistent kernel depends on the weights only: W_hh of both directions re-packed into
 * MFMA fragment order (forward, BPTT and K-split BPTT layouts differ) and the cleared exchange state of the workspace.  The reference
 * rebuilds nothing per layer call either (its weights are graph variables, las/layers.py:28-54).  las_rnn_seq_prepare does that work for n
 * (layer, pass) pairs in ONE launch -- once per optimiser step, off the dependency chain -- each into a workspace of its own
 * (las_rnn_seq_workspace_bytes(cell, LAS_PREC_BF16, H, B)); the sweep that then gets such a workspace together with LAS_SEQ_PREPARED in
 * `flags` launches nothing but its persistent kernel.  A prepared workspace serves ONE sweep (the exchange state is dirty afterwards) with
 * the same cell / H / flags / direction of the pass (bwd = 0: las_rnn_seq_fwd, 1: las_rnn_seq_bwd) and any batch B' <= B.
 * whh_fw / whh_bw: as for las_rnn_seq_fwd.  Only LAS_PREC_BF16 shapes (H in {64,128,256,512}).  `descs` is HOST memory. */
typedef struct las_seq_prepare_desc {
    const float* whh_fw; const float* whh_bw; int ldw;
    int cell, H, B, bwd, flags;
    void* ws; size_t ws_bytes;
} las_seq_prepare_desc;
int las_rnn_seq_prepare(const las_seq_prepare_desc* descs, int n, void* stream);
/* Element type of gates / out / cstate / dout for (cell, prec, H): LAS_DT_BF16 when the speed-mode MFMA sweeps serve the
 * shape (prec = LAS_PREC_BF16 and H in {64,128,256,512}), else LAS_DT_F32 (parity mode, or a speed-mode shape that falls
 * back to the fp32 VALU sweep).  The caller allocates those tensors -- and makes the K1 product write them -- accordingly. */
int las_rnn_seq_io_dtype(int cell, int prec, int H);
/* Which kernel a sweep of (cell, prec, B, H, flags) launches and what that kernel serves -- the same plan as the launch reads, pure host
 * arithmetic; callers ask it before they use a mode of las_rnn_seq_args, and tests name, and assert, the kernel a case runs (as
 * las_speller_last_variant does for the Speller).  bwd: 0 the forward sweep, 1 BPTT.  mode: what the call asks of its kernel,
 * LAS_SWEEP_MODE_ROWS (row_T set), LAS_SWEEP_MODE_CHUNKS (dout_chunk_flag set), LAS_SWEEP_MODE_CHUNKS | LAS_SWEEP_MODE_PROGRESS (progress
 * set as well); it only picks `kernel`'s variant, and a mode the planned kernel does not serve leaves the kernel as it is (the calls
 * refuse such a configuration: read x_chunks / rows / dout_chunks / progress_words first).  LAS_SWEEP_NONE with zeros: the fp32 paths
 * (parity mode, H outside {64, 128, 256, 512}), or no kernel at the picked width or a narrower one. */
enum { LAS_SWEEP_NONE = 0,
       LAS_SWEEP_FWD_PLAIN = 1,       /* plain bf16 MFMA forward, 16-row tiles (P = 1, LAS_SEQ_NO_HELPER_WAVES) */
       LAS_SWEEP_FWD_HW16 = 2,        /* helper-wave forward, 16-row tiles */
       LAS_SWEEP_FWD_HW8 = 3,         /* helper-wave forward, 8-row tiles */
       LAS_SWEEP_FWD_HW8_RAGGED = 4,  /* ... honouring row_T */
       LAS_SWEEP_BWD_PLAIN = 5,       /* plain bf16 MFMA BPTT (all-gather of dZ), 16-row tiles */
       LAS_SWEEP_BWD_KS16 = 6,        /* K-split BPTT, 16-row tiles */
       LAS_SWEEP_BWD_KS8 = 7,         /* K-split BPTT, 8-row tiles */
       LAS_SWEEP_BWD_KS8_CH = 8,      /* ... waiting for chunks of dout */
       LAS_SWEEP_BWD_KS8_CH_PG = 9 }; /* ... and publishing its progress */
enum { LAS_SWEEP_MODE_ROWS = 1, LAS_SWEEP_MODE_CHUNKS = 2, LAS_SWEEP_MODE_PROGRESS = 4 };
typedef struct las_rnn_seq_plan_info {
    int kernel;              /* LAS_SWEEP_* */
    int P;                   /* cluster width */
    int rows_per_tile;       /* batch rows per tile (8 or 16) */
    int launches;            /* row-chunk launches the batch is swept in */
    int x_chunks;            /* forward: 1 = the kernel waits for x-projection chunks (x_chunk_flag); only the helper-wave kernels do */
    int rows;                /* forward: 1 = rows of different lengths are served (row_T); only the 8-row helper-wave kernel does */
    int dout_chunks;         /* BPTT: 1 = the kernel waits for chunks of dout (dout_chunk_flag); only the 8-row K-split cluster kernel does */
    int progress_words;      /* BPTT: ints `progress` must hold, one per cluster member; 0 = the configuration has no progress-publishing kernel */
} las_rnn_seq_plan_info;
int las_rnn_seq_plan(int cell, int prec, int B, int H, int flags, int bwd, int mode, las_rnn_seq_plan_info* out);

/* One sweep: las_rnn_seq_fwd reads the first two groups of fields, las_rnn_seq_bwd the first and the third.  A zero / NULL field switches
 * its mode off; a field of the other pass's group must be zero / NULL (refused otherwise, as is every combination named below).  The
 * struct is HOST memory and is read before the call returns. */
typedef struct las_rnn_seq_args {
    int cell, prec, B, T, H;
    void* gates; const float* whh_fw; const float* whh_bw; int ldw;         /* BPTT overwrites gates with d(pre-activation) */
    void* out; int ld_out; long long out_bstride; void* cstate;             /* written by the forward sweep, read by BPTT */
    float forget_bias; int flags; int* status;
    void* ws; size_t ws_bytes;                                              /* las_rnn_seq_workspace_bytes */
    /* ---- forward only ----
     * x_chunk_flag: the x-projection is still being computed.  `gates` is filled in time chunks of x_chunk_steps (> 0) sweep steps, chunk
     * k = frames [k*cs, (k+1)*cs) and [T-(k+1)*cs, T-k*cs) of every utterance (both ends of the sequence first: the forward direction
     * consumes t = 0, 1, .., the backward direction t = T-1, T-2, ..), e.g. by las_gemm_kk_frames launches on ANOTHER stream, each
     * followed by las_set_word(x_chunk_flag, k+1).  The sweep reads a frame only after *x_chunk_flag has reached its chunk (bounded wait
     * -> LAS_SEQ_STATUS_FWD_TIMEOUT).  Chunk 0 must be complete IN STREAM ORDER in front of this call (produced on `stream`, or on a
     * stream `stream` has waited for): the sweep never waits for it and the value of *x_chunk_flag only matters from 2 on -- no flag
     * launch is needed between chunk 0's product and the sweep (round 5).  Needs las_rnn_seq_plan's x_chunks; not together with row_T. */
    const int* x_chunk_flag; int x_chunk_steps;
    /* row_T: a batch whose rows have DIFFERENT lengths (beam search encodes utterances the reference feeds one at a time, unpadded -- its
     * encoder has no length mask): row_T [B] device ints, row_T[b] <= T frames of row b.  At frames t >= row_T[b] the row's state and
     * outputs are forced to ZERO: the backward direction reaches the row's last real frame with the zero state of an unpadded run, the
     * forward direction's real frames come first, and the zero pad frame is the one the pyramid appends to an odd-length utterance --
     * every real frame equals the one-utterance-at-a-time result.  Needs las_rnn_seq_plan's rows. */
    const int* row_T;
    /* ---- BPTT only ----
     * dout: gradient w.r.t. out, addressed like out with ld_dout (>= 2H) and dout_bstride. */
    const void* dout; int ld_dout; long long dout_bstride;
    /* dbias_fw / dbias_bw (either may be NULL): the sweep additionally accumulates (+=) the bias gradients of the two directions, [G*H]
     * fp32 = column sums of d(pre-activation) over all B*T frames (the bias of the TF cell kernel, las/layers.py:31).  The cluster BPTT
     * kernel sums them in fp32 registers while it sweeps (before the bf16 rounding of the stored gradient). */
    float* dbias_fw; float* dbias_bw;
    /* dout_chunk_flag: the upstream gradient is still being computed.  dout [B, Tp, 2H] is the input gradient of the dense layer above,
     * whose rows are pyramid frame pairs (dout_rows = ceil(T/2)) or single frames (dout_rows = T); it is filled in chunks of
     * dout_chunk_rows (a power of two) of those rows from both ends of the sequence (chunk k = rows [k*c, (k+1)*c) and
     * [dout_rows-(k+1)*c, dout_rows-k*c) of every utterance), e.g. by las_gemm_kk_frames launches on another stream each followed by
     * las_set_word(dout_chunk_flag, k+1).  The sweep reads a frame of dout only after *dout_chunk_flag has reached the chunk of its row
     * (bounded wait -> LAS_SEQ_STATUS_BWD_TIMEOUT); chunk 0 must be complete in stream order in front of this call and is never waited
     * for.  Needs las_rnn_seq_plan's dout_chunks. */
    const int* dout_chunk_flag; int dout_chunk_rows, dout_rows;
    /* progress (with dout_chunk_flag only; round 5): the sweep PUBLISHES ITS PROGRESS.  d(pre-activation) leaves the sweep with
     * agent-scope (write-through) stores, and every progress_steps (> 0) sweep steps -- and at the end -- member m of cluster c stores the
     * number of steps whose dZ has reached memory into progress[c * P + m] (las_rnn_seq_plan's progress_words caller-zeroed device ints,
     * P its cluster width).  After s steps the forward direction's dZ exists for frames [T - s, T), the backward direction's for [0, s):
     * the layer's weight gradients can follow the sweep window by window on another stream (las_wait_words_min, las_wgrad_ih_hh_window)
     * instead of starting when it ends -- the bottom layer's are the end-of-step tail of the reference's train step (las/las.py:272-283
     * can only run behind them). */
    int* progress; int progress_steps;
} las_rnn_seq_args;
int las_rnn_seq_fwd(const las_rnn_seq_args* a, void* stream);
int las_rnn_seq_bwd(const las_rnn_seq_args* a, void* stream);

/* C = act(A . B^T + bias) like las_gemm_kk, restricted to the frames [lo0, lo0+nlo) and [hi0, hi0+nhi) of every utterance of
 * [nb, T, *] tensors A and C (row pitches lda / ldc per frame); las_set_word: stream-ordered store of a device word. */
int las_gemm_kk_frames(int nb, int T, int lo0, int nlo, int hi0, int nhi, int N, int K, const void* A, long long lda,
                       const void* B, long long ldb, void* C, int c_dtype, long long ldc, const float* bias, int act,
                       const void* y_tanh, long long ldy, void* stream);       /* y_tanh as in las_gemm_kk_tanhgrad (may be NULL) */
int las_set_word(int* word, int value, void* stream);

/* ------------------------------------------------------------------------------------------
 * K4-K7  Speller: the whole decode loop of Speller.__call__ (las/las.py:72-143) with
 * Speller.decode (las/las.py:145-160), AdditiveAttention / LocationAwareAttention
 * (las/layers.py:234-257 / :281-311), BaseAttention.mask/attend (las/layers.py:172-213).
 * One call enqueues all U steps (per step: one fused row kernel = finish previous cell +
 * [vocab logits/argmax/sample] + query projection + energies + mask + softmax + context + cell
 * input assembly, then the cell contraction through las_gemm).  All pointers device.  Layouts:
 *   enc   [B,Tp,Hd]   encoder output h           keys [B,Tp,A]  hoisted dense(hidden) (K4, las_gemm)
 *   enc_len int32 [B] (already int-cast as las/layers.py:193 does)
 *   Ws [S,A] (S=D*NL)  u [A]   emb [V,E]   Wv [D,V]  bv [V]
 *   loc_w [Kc,C], loc_b [C], Wf [C,A] (mode LOC only, else NULL)
 *   cellW[l] [(I_l+D), G*D], cellb[l] [G*D]  with I_0 = E+Hd, I_l = D   (HOST arrays of device ptrs)
 *   tokens_in int32 [U,B]: the token whose embedding enters step t (t=0: SOS; teacher forcing:
 *   teacher[:,t-1]).  -1 = greedy argmax of step t-1 (inference, las/las.py:111); -2 = a sample
 *   from Categorical(logits of step t-1) (scheduled sampling, las/las.py:101-105,170-175; Gumbel
 *   arg-max driven by `seed`).  Resolved tokens are written back in place.  Any negative entry
 *   requires step_logits=1 or 2.
 * Time-major internal results (the Python boundary returns [B,U,.] views):
 *   logits [U,B,V]   alphas [U,B,Tp]   tokens_out int32 [U,B] (argmax per step; step_logits=1 only)
 *   step_logits=2 (training with scheduled sampling): in-loop logits + draws only at the steps whose entering token is device-resolved
 *   (tokens_in < 0), every step's logits from the batched product behind the loop; tokens_out is written at those steps only.
 * Saved for backward (caller-allocated):
 *   hs  [NL,U+1,B,D]  h states (slot 0 = initial state: zeroed by the call, or supplied by the
 *       caller when keep_state0=1 -- single-step use by beam search)   cs [NL,U+1,B,D] (lstm)
 *   gates [NL,U,B,G*D] activated gates (lstm) / pre-activation scratch (rnn)
 *   xin0 [U,B,E+Hd+D]  first-layer cell input rows  [emb(token) ; context ; h_prev]
 */
enum { LAS_SPELLER_STATUS_TIMEOUT = 3 };   /* (LAS_SEQ_STATUS_* are 1 and 2) */
enum { LAS_SPELLER_NO_PF_ROWS = 1,    /* speed mode without the fully prefetching row kernels (generic bf16 rows) */
       LAS_SPELLER_NO_BF_ROWS = 2,    /* speed mode with the fp32-operand row kernels */
       LAS_SPELLER_NO_FUSED_STEP = 4,   /* speed mode with two launches per step (row kernel, then the cell product)
                                           instead of the whole loop in one launch (product + row workgroups, granule hand-off) */
       LAS_SPELLER_REUSE_PREP = 8 };    /* (las_speller_bwd: operand copies only) the workspace still holds the bf16 copies of enc / keys / Ws and the
                                           packed cell weights that an earlier call made from the SAME tensors -- skip rebuilding
                                           them (beam search calls the step U = 1 at a time against a fixed encoder output) */
enum { LAS_SPELLER_NO_LOGITS = 16 };    /* (las_speller_fwd, U = 1, speed mode, one LSTM layer, D and E + Hd + D multiples of 32) the beam search's step:
                                           attention row kernel, then the cell in ONE launch (product + gate math: hs / cs slot 1 and the activated
                                           gates); NO vocabulary projection, logits / tokens_out are left alone -- the caller projects inside
                                           las_beam_loop_step (proj_*) */
enum { LAS_SPELLER_ROWS_SHARE4 = 32 };  /* (with LAS_SPELLER_NO_LOGITS; round 5) the caller vouches that rows 4g .. 4g+3 have IDENTICAL enc / keys / enc_len
                                           (beam search: the hypotheses of one utterance are consecutive rows, beam % 4 == 0): the attention rows of
                                           four hypotheses run in one workgroup that reads Ws, the keys and the encoder rows once -- a quarter of
                                           the step's L2 traffic; bit-identical to one row per workgroup.  B % 4 == 0, tokens >= 0. */
enum { LAS_SPELLER_WIDE = 64,           /* (round 6) take the wide per-step path (csrc/speller_wide.h: the query projection as one product over all rows, energies and
                                           context on (slice, utterance) workgroups, every layer's cell product on pre-packed MFMA fragments) wherever its
                                           geometry allows; by default it serves the multi-layer and location-aware calls of both modes
                                           outside the one-launch loop kernels' geometry (e.g. run.sh's 2 x 1024 decoder at T' = 319) */
       LAS_SPELLER_NO_WIDE = 128,       /* never take it (round 5's per-utterance row kernels) */
       LAS_SPELLER_SHARED_OPERANDS = 1 << 14 };  /* (with row_group > 0 and LAS_SPELLER_NO_LOGITS: a beam search's step) enc and keys hold ONE block per
                                           group of row_group rows -- enc [B / row_group, Tp, Hd], keys [B / row_group, Tp, A] -- instead of one copy per
                                           hypothesis row (the reference feeds np.tile(h), las/beam_search.py:216: 16 copies of every utterance's
                                           205 KB, each read through its own addresses -- 54 MB per step at 256 rows).  enc_len stays per row. */
#define LAS_SPELLER_SPIN_LOG2(n) (((n) & 31) << 8)   /* tests: the loop kernels' poll budget is 2^n instead of 2^21 */
typedef struct {
    int B, Tp, Hd, A, D, NL, E, V, U, cell, mode, prec, Kc, C, step_logits, keep_state0;
    int flags;                     /* LAS_SPELLER_* development / test switches, 0 in normal use */
    float forget_bias;
    unsigned long long seed;
    const float *enc, *keys; const int* enc_len;
    const float *Ws, *u, *emb, *Wv, *bv, *loc_w, *loc_b, *Wf;
    const float* const* cellW; const float* const* cellb;   /* host arrays [NL] of device ptrs */
    int* tokens_in; int* tokens_out;
    float *logits, *alphas;
    const float* align0;           /* optional [B,Tp]: previous alignment entering step 0 (else zeros) */
    const float* emb_mask;         /* optional [U,B,E]: inverted-dropout mask on the embedded input token
                                      (tf.layers.dropout, las/las.py:107-108), already scaled by 1/keep */
    const float* emb_noise;        /* optional [U,V,E]: variational noise (--add_vn): the reference adds a fresh N(0, 0.075)
                                      draw to the WHOLE embedding matrix at every look-up (las/las.py:164-166), i.e. one
                                      [V,E] noise matrix per decode step, shared by the rows that look up the same token */
    float *hs, *cs, *gates, *xin0;
    void* act_save;                /* optional, saved for backward like the four above (las_speller_act_save_bytes): speed mode's row kernels keep
                                      tanh(keys + q [+ f . Wf]) of every step here (fp16 [U,B,Tp,A] behind a 32-byte header; location-aware: also
                                      the conv outputs f, fp32 [U,B,Tp,C]) and the gradient rows read them instead of recomputing the conv, C FMAs
                                      and a tanh per (frame, column) of every step; NULL (or a forward
                                      that ran another kernel family: the header says so) = recompute */
    void* ws; size_t ws_bytes;
    int* status;                   /* optional device int (the sweeps' status word): the one-launch loop kernels need all their
                                      workgroups co-resident (one per compute unit); a workgroup that does not see a partner
                                      within the poll bound stores LAS_SPELLER_STATUS_TIMEOUT here and the launch DRAINS
                                      (every workgroup finishes its steps without waiting) instead of hanging or trapping --
                                      results of that call are invalid, the host checks the word at its next synchronisation */
    const struct las_lstm_cell_args* companion;   /* optional, LAS_SPELLER_NO_LOGITS calls only: ANOTHER cell step (the LM's first layer in a beam
                                      search -- it depends on the tokens only) that is launched together with the Speller's cell, as
                                      the second problem of one grid: two dependent-launch slots of a search step become one */
    int row_group;                 /* optional (0 = none; round 6): rows g row_group .. (g + 1) row_group - 1 have IDENTICAL enc / keys / enc_len -- a beam
                                      search's hypotheses of one utterance (las/beam_search.py:216 tiles the encoder output over them).  The
                                      per-step attention-row launches then place an utterance's rows on ONE XCD (workgroup id -> row mapping,
                                      csrc/speller.hip xcd_local_row), so that its keys and encoder rows enter one L2 instead of eight.
                                      B % row_group == 0, else ignored.  Results do not depend on it. */
} las_speller_fwd_args;
size_t las_speller_workspace_bytes(int B, int Tp, int Hd, int A, int D, int NL, int E, int V, int U, int cell);
size_t las_speller_act_save_bytes(int U, int B, int Tp, int A, int C);   /* C = location-aware channels (0: additive attention) */
int las_speller_fwd(const las_speller_fwd_args* a, void* stream);

/* Backward of the loop above for the tokens recorded in tokens_in (gradients do not flow through
 * sampled tokens, as with tf.distributions.Categorical.sample, las/las.py:170-175).
 *   dlogits [U,B,V] in.   `gates` is overwritten with d(pre-activation).
 *   Accumulates (+=) into caller-zeroed gradient buffers:
 *   d_enc [B,Tp,Hd], d_keys [B,Tp,A], dWs, du, demb [V,E], dWv, dbv, dcellW[l], dcellb[l],
 *   dloc_w, dloc_b, dWf.
 */
typedef struct {
    las_speller_fwd_args f;           /* the forward arguments, with saved buffers filled in */
    const float* dlogits;
    float *d_enc, *d_keys, *dWs, *du, *demb, *dWv, *dbv, *dloc_w, *dloc_b, *dWf;
    float* const* dcellW; float* const* dcellb;              /* host arrays [NL] of device ptrs */
} las_speller_bwd_args;
int las_speller_bwd(const las_speller_bwd_args* a, void* stream);
/* The same in two launches so that the caller can take the parameter gradients off the dependency chain:
 *   part 1 = the reverse loop and the input gradients (d_enc, d_keys);
 *   part 2 = every parameter gradient (reads what part 1 left in `ws`, `gates`, `xin0`, `hs`; may run on another
 *            stream ordered after part 1);   part 3 = both (= las_speller_bwd). */
int las_speller_bwd_part(const las_speller_bwd_args* a, int part, void* stream);
/* Which kernel family served the process's LAST las_speller_fwd (which = 0) / las_speller_bwd* part 1 (which = 1): a bit mask.  The
 * reference has ONE Speller graph (las/las.py:72-160); this library picks among several kernel families by geometry, and a caller (bench.py,
 * the tests) must be able to say which one a number or a parity statement belongs to. */
enum { LAS_SPELLER_RAN_LOOP = 1,       /* the whole decode / gradient loop in one launch (dec_loop_*_kernel) */
       LAS_SPELLER_RAN_PF_ROWS = 2,    /* per-step launches, prefetching bf16 row kernels */
       LAS_SPELLER_RAN_BF_ROWS = 4,    /* per-step launches, generic bf16 row kernels */
       LAS_SPELLER_RAN_F32_ROWS = 8,   /* per-step launches, fp32-operand row kernels (parity mode; speed mode outside the other families' geometry) */
       LAS_SPELLER_RAN_SKINNY = 16,    /* layer 0's per-step cell product: pre-packed bf16 MFMA fragments (las_skinny_gemm_bf16) */
       LAS_SPELLER_RAN_LOC = 32,       /* location-aware attention */
       LAS_SPELLER_RAN_UPPER_SKINNY = 64,    /* layers >= 1: per-step cell products on pre-packed bf16 fragments (round 6) */
       LAS_SPELLER_RAN_WIDE = 128 };         /* the wide per-step path (csrc/speller_wide.h, round 6) */
int las_speller_last_variant(int which);

/* ------------------------------------------------------------------------------------------
 * K8  LAS._get_loss (las/las.py:320-333) + label_smoothing (las/utils.py:5-12), forward and
 * gradient in one pass.  logits element (b,t,v) at logits[b*sb + t*st + v] (so the Speller's
 * time-major [U,B,V] buffer is consumed in place: sb=V, st=B*V); dlogits uses the same strides.
 * y int32 [B,ldy] (first U columns used).  `smooth`: bit 0 = label smoothing with `epsilon`; bit 1 = no PAD mask, every
 * position counts (the RNNLM's mean sparse cross entropy, lang/char_rnn_model.py:146-149).
 * sums[0] += sum(ce*mask), sums[1] += sum(mask)   (caller zeroes sums; the division
 * sum/(n+1e-9) is the caller's so that data-parallel ranks can all-reduce both terms first).
 * bit 2 of `smooth` (needs scale_ptr; sums then has THREE floats): sums[0] = sum(ce*mask), sums[1] = sum(mask),
 * sums[2] = sums[0] * scale_ptr[0] are WRITTEN -- the scaled loss without a fill in front and a multiply behind.
 * dlogits = scale_ptr[0] * mask * (softmax - smoothed_onehot)    (scale = 1/(n_total+1e-9), a
 * device scalar; NULL dlogits skips the gradient).
 */
size_t las_ce_loss_workspace_bytes(int B, int U);
int las_ce_loss(const float* logits, long long sb, long long st, const int* y, int ldy,
                int B, int U, int V, float epsilon, int smooth,
                float* sums, const float* scale_ptr, float* dlogits,
                void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K8c  CTC term of joint CTC-attention training (las/las.py:75-77, 259-261, 335-349; tf.nn.ctc_loss, ctc_merge_repeated,
 * blank = class Vc - 1, softmax inside the loss).  logits fp32 [B, Tp, Vc] through strides sb / st (elements, last axis
 * contiguous).  The labels of row b are the nonzero entries of y[b, 0:U] (int32, pitch ldy >= U), in order; on row
 * drop_last_row (or none: -1) the last of them is dropped (the reference's `[:-1]` over the whole batch).
 * enc_len int32 [B]: frames t >= enc_len[b] contribute nothing.  U <= 511.
 *   nll[b]   = -log p(labels_b | logits_b)   (+inf for a row that cannot be aligned, or that holds a label outside [0, Vc-2])
 *   loss[0]  = scale_ptr[0] * sum_b nll[b]    (loss may be NULL; fixed-order sum)
 *   grad     = scale_ptr[0] * (softmax - posterior) per (b, t) row, element type grad_dtype (LAS_DT_F32 / LAS_DT_BF16), strides
 *              gsb / gst; zero rows at t >= enc_len[b] and for rows with nll = +inf.  NULL skips the gradient.
 * No atomics: two calls on the same inputs give the same bits.  ws >= las_ctc_workspace_bytes(B, Tp, U).
 */
size_t las_ctc_workspace_bytes(int B, int Tp, int U);
int las_ctc_loss(const float* logits, long long sb, long long st, int Vc, const int* y, int ldy, int U,
                 const int* enc_len, int B, int Tp, int drop_last_row,
                 float* nll, float* loss, const float* scale_ptr,
                 void* grad, int grad_dtype, long long gsb, long long gst,
                 void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K9  tf.clip_by_global_norm + tf.train.AdamOptimizer.apply_gradients (las/las.py:272-283) on one
 * flat fp32 parameter bucket.  las_sumsq: out[0] = sum g^2 (deterministic two-stage reduction;
 * ws >= las_sumsq_workspace_bytes(n)).  las_clip_adam: theta,m,v updated in place;
 * g *= clip/max(sqrt(sumsq[0]),clip) when clip>0;  lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the
 * caller;  theta -= lr_t * m / (sqrt(v) + eps)   (TF "epsilon-hat" placement).
 * status / guard (either may be NULL): device words checked by the kernel itself -- when status[0] != 0 (a recurrent sweep
 * of this step reported an exchange time-out, LAS_SEQ_STATUS_*) or guard[0] != 0 (the same, summed over the data-parallel
 * ranks with the gradient bucket) the update is SKIPPED: theta, m, v keep their values, no host synchronisation needed.
 * applied (may be NULL; round 6): a device int that the kernel increments when -- and only when -- it DOES apply the update.  The status
 * word is sticky until the host clears it, so after a time-out every later step is skipped too: when the host finally notices (its
 * polls are asynchronous), applied[0] tells it exactly which step was the first one lost, and LAS.train re-runs from there
 * (las/las.py LAS._recover).
 */
/* Stream-ordered, BOUNDED wait on a device word: work enqueued behind it on `stream` starts once *word == value or after
 * max_us microseconds.  A scheduling aid (never a correctness dependency): the weight-gradient GEMMs of a side stream are
 * held back until the next recurrent sweep has announced itself (LAS_SEQ_ANNOUNCE), so that they neither delay its start nor
 * compete with the chain GEMMs in front of it.  No reference counterpart (the reference has one stream). */
int las_wait_word(const int* word, int value, int max_us, void* stream);
/* ... for the announcement word itself (status[1] of LAS_SEQ_ANNOUNCE): passes once the word HAS REACHED n in the cyclic order of
 * 1..1023 -- also when later sweeps have announced themselves meanwhile (a hold enqueued late must not sit out its bound). */
int las_wait_announce(const int* word, int n, int max_us, void* stream);
/* Stream-ordered wait until EVERY one of n device words is >= need (las_rnn_seq_args' progress words).  Unlike las_wait_announce this
 * is a correctness dependency: on a time-out (max_us) `code` is stored into status[0] (may be NULL) -- the step is invalid, las_clip_adam skips it. */
int las_wait_words_min(const int* words, int n, int need, int max_us, int* status, int code, void* stream);
/* Diagnostics (round 5): a "foreign" kernel that stays RESIDENT -- n workgroups of 256 threads (workgroup L on XCD L % 8), `lds` bytes of LDS
 * and 32 or 64 VGPRs per lane each: the footprint of a collective's channel -- until *stop != 0 (or max_ms).  resident[0] (caller-zeroed)
 * counts the workgroups that have started.  The recurrent sweeps and the one-launch Speller loops need all THEIR workgroups resident at
 * once (LAS_SEQ_STATUS_*, LAS_SPELLER_STATUS_TIMEOUT): tests run a train step beside this kernel to show what they tolerate. */
int las_occupy(const int* stop, int* resident, int n, int lds, int vgprs, int max_ms, void* stream);

/* bf16 (or fp32) weight shadows of the speed mode, rebuilt after every optimiser step by ONE launch over a device-resident
 * descriptor table: D = zero-pad(op([src0 | src1])), op = transpose or identity; src1 may be NULL (cols1 = 0).
 * max_tiles >= max over the descriptors of ceil(dst_rows/32) * ceil(dst_cols/32).  (No reference counterpart: the
 * reference's fp32 graph has no operand copies; this replaces ~50 small copy / cat / cast kernels per step.) */
typedef struct las_shadow_desc {
    const float* src0; const float* src1;
    int ld0, ld1, rows, cols0, cols1, transpose;
    void* dst;
    int dst_rows, dst_cols, dst_ld, dst_bf16;
} las_shadow_desc;
int las_build_shadows(const las_shadow_desc* descs_dev, int n, int max_tiles, void* stream);

/* Input dropout of a bidirectional recurrent layer (las/layers.py:37-47: fw_cell and bw_cell in separate DropoutWrappers, input_keep_prob =
 * 1 - dropout_rate): ONE launch leaves the two directions' operand blocks y_fw / y_bw [rows, ldy] = x * mask_d / keep with INDEPENDENT
 * Bernoulli(keep) masks, in fp32 or bf16 (x_dt / y_dt: LAS_DT_*), columns K .. ldy - 1 zero (the product's K padding; ldy % 4 == 0).  The
 * masks are a counter-based function of (seed, direction, row, column) -- 16 bits of a splitmix64 word per element -- and are never stored:
 * las_dropout_pair_bwd regenerates them,  dx = (mask_fw * g_fw + mask_bw * g_bw) / keep  (g_*: [rows, ldg], the first K columns).
 * (tf.nn.dropout draws from TF's Philox stream; the reference fixes no seed, so only the distribution is contractual.) */
int las_dropout_pair_fwd(const void* x, int x_dt, long long rows, int K, int ldx, void* y_fw, void* y_bw, int y_dt, int ldy,
                         float keep, unsigned long long seed, void* stream);
int las_dropout_pair_bwd(const void* g_fw, const void* g_bw, int g_dt, int ldg, long long rows, int K, void* dx, int dx_dt, int lddx,
                         float keep, unsigned long long seed, void* stream);

/* tf.layers.batch_normalization over the last axis of a [rows, C] block in TRAINING mode, with the ReLU the CNN listener puts behind it
 * (las/layers.py:114-116,155-161; momentum 0.99 -> `momentum` 0.01 here, epsilon 1e-3):
 *   fwd: mean / rstd [C] = batch statistics (biased variance; kept by the caller for backward), y = [relu](gamma (x - mean) rstd + beta);
 *        moving_mean / moving_var (both or neither): m = (1 - momentum) m + momentum {mean, unbiased variance}   (UPDATE_OPS, las/las.py:272)
 *   bwd: dx; dgamma / dbeta (either may be NULL) are ACCUMULATED (+=).  relu: y is the forward's output (its sign is the mask).
 * C % 4 == 0, 16-byte aligned pointers, ws >= las_bn_workspace_bytes(rows, C).  Deterministic (fixed-order reductions, no atomics). */
size_t las_bn_workspace_bytes(long long rows, int C);
int las_bn_relu_fwd(const float* x, long long rows, int C, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
                    float* moving_mean, float* moving_var, float momentum, int relu, float* y, void* ws, size_t ws_bytes, void* stream);
int las_bn_relu_bwd(const float* x, const float* y, const float* dy, long long rows, int C, const float* gamma, const float* mean,
                    const float* rstd, int relu, float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);

size_t las_sumsq_workspace_bytes(long long n);
int las_sumsq(const float* g, long long n, float* out, void* ws, size_t ws_bytes, void* stream);
int las_clip_adam(float* theta, const float* g, float* m, float* v, long long n,
                  const float* sumsq, float clip, float lr_t, float beta1, float beta2, float eps,
                  const int* status, const float* guard, int* applied, void* stream);

/* ------------------------------------------------------------------------------------------
 * R1  one BasicLSTMCell step of the char RNNLM used for shallow fusion (lang/char_rnn_model.py:57-66 with
 * forget_bias 0, driven from las/beam_search.py:226-236): gate math on z = [x,h].kernel + bias [N,4H]
 * (the contraction itself is las_gemm): c' = c*sigmoid(f+fb) + sigmoid(i)*tanh(j), h' = tanh(c')*sigmoid(o).
 */
int las_lstm_pointwise(const float* z, const float* c_prev, int N, int H, float forget_bias,
                       float* c_out, float* h_out, void* stream);
/* ... with the input half of a ONE-HOT input (the LM's first layer: the reference feeds tf.one_hot ids, lang/char_rnn_model.py:106-112)
 * added on the way in: z[n] + xrows[max(ids[n] - id_shift, 0)], xrows [V,4H] = the input rows of the cell kernel.  id_shift / the clamp
 * are the LAS-id -> LM-id map of the shallow fusion (las/beam_search.py:109-116: LM ids = LAS ids - 2, SOS fed as id 0), so that the
 * beam search's next_token buffer is read as it is. */
int las_lstm_pointwise_rows(const float* z, const float* xrows, const int* ids, int id_shift, const float* c_prev, int N, int H,
                            float forget_bias, float* c_out, float* h_out, void* stream);
/* The whole cell for a block of rows in ONE launch (the beam search's LM step, M = utterances x beam rows): z = [x ; h] . kernel + bias
 * with the kernel's input rows / recurrent rows given as las_gemm_skinny_pack fragments (Wx_packed: [I, 4H], Wh_packed: [H, 4H]; operands
 * rounded to bf16, fp32 accumulation), then the gate math of las_lstm_pointwise.  Dense input: x [M, I] (I % 32 == 0) and Wx_packed; one-hot
 * input (lang/char_rnn_model.py:106-112): x = NULL and ids / id_shift / xrows as in las_lstm_pointwise_rows (fp32 row look-up, no rounding
 * inside the kernel).  H % 32 == 0; c_out / h_out [M, H] may not alias h / c_prev (other workgroups still read them). */
int las_lstm_cell_rows(const float* x, int ldx, int I, const int* ids, int id_shift, const float* xrows, const float* h, int ldh,
                       const void* Wx_packed, const void* Wh_packed, const float* bias, const float* c_prev, int M, int H,
                       float forget_bias, float* c_out, float* h_out, void* stream);
/* The same call with its arguments in a struct (what las_speller_fwd_args.companion points to): x fp32 or, with x_bf16, bf16; either
 * of x / h may be NULL (with its packed weights); fast = the Speller's approximated transcendentals instead of expf / tanhf;
 * gates_out (optional [M, 4H]) receives the ACTIVATED gates i, j, f, o. */
typedef struct las_lstm_cell_args {
    const void* x; int x_bf16, ldx, I;
    const int* ids; int id_shift; const float* xrows;
    const void* h; int ldh;          /* fp32 rows, or bf16 rows when h_bf16 (below) */
    const void *Wx, *Wh;
    const float *bias, *c_prev;
    float fb;
    float *c_out, *h_out, *gates_out;
    int M, H, fast;
    int h_bf16;                      /* (round 5) h holds bf16 rows: the copy a previous launch left in h_out_bf16.  Served by the pipelined
                                        body only (M >= 128, x absent or bf16 too; as is h_out_bf16): the beam search's LM cells */
    void* h_out_bf16;                /* optional [M, H] bf16: h' rounded as the next launch's operand staging would round it (RNE) -- the
                                        next layer's x and, gathered, the next step's h, at half the bytes */
} las_lstm_cell_args;
int las_lstm_cell_rows_args(const las_lstm_cell_args* a, void* stream);
/* Two independent cell steps as the two problems of ONE grid (what las_speller_fwd does with its companion): a = the Speller's (fast,
 * bf16 x), b = the LM's (exact; fp32 or bf16 rows, or a one-hot input).  Two problems no pair kernel is compiled for are served as two
 * single launches, a then b; the results are those of las_lstm_cell_rows_args(a) and las_lstm_cell_rows_args(b), bit for bit. */
int las_lstm_cell_rows_pair_args(const las_lstm_cell_args* a, const las_lstm_cell_args* b, void* stream);
/* What las_lstm_cell_rows_args(a) (b = NULL) or las_lstm_cell_rows_pair_args(a, b) launches: host arithmetic, no launch, callable
 * without a device (the pointers count by being NULL or not, and by their alignment).  Negative: the launch refuses these arguments.
 * Otherwise a code of the bits below.  One problem: 0 below 128 rows and for fp32 x AND h at <= 256 rows, else 32 rows per workgroup
 * up to 256 rows, 64 up to 512, 128 above.  A pair: PAIR with 0 (either problem below 128 rows or not of one element type), 32 (both
 * <= 256 rows) or 64 rows; TWO where a is not fast, b is fast, or the unpipelined pair kernel would meet fp32 x in a, bf16 x in b, or
 * bf16 h / h_out_bf16 in either. */
enum {
    LAS_LSTM_CELL_PLAN_ROWS = 0xff,      /* rows per workgroup of the pipelined body (32, 64, 128); 0: the unpipelined 32-row body */
    LAS_LSTM_CELL_PLAN_PAIR = 0x100,     /* both problems in one grid */
    LAS_LSTM_CELL_PLAN_B_BF16 = 0x200,   /* with PAIR and rows > 0: the second problem's rows are bf16 */
    LAS_LSTM_CELL_PLAN_TWO = 0x400       /* two single launches, each as the query with b = NULL says; no other bit is set */
};
int las_lstm_cell_rows_plan(const las_lstm_cell_args* a, const las_lstm_cell_args* b /* may be NULL */);
/* ... and its gradient, for training the RNNLM (lang/char_rnn_model.py:177-190, truncated BPTT over num_unrollings steps):
 * dz [N,4H] and dc_prev [N,H] from z, c_prev, dh (gradient w.r.t. h') and dc_in (gradient w.r.t. c', may be NULL). */
int las_lstm_pointwise_bwd(const float* z, const float* c_prev, const float* dh, const float* dc_in, int N, int H,
                           float forget_bias, float* dz, float* dc_prev, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10  one pruning step of BeamSearch.decode (las/beam_search.py:119-152, :297-312) for `nutt`
 * utterances at once.  Per utterance: nlive live hypotheses with raw logits [nlive,V] (raw logits
 * are the scores, las/beam_search.py:123-124), running float32 score (0 + np.float32 sums stay
 * float32 in BeamState.update, :27) and length (tokens after SOS so far).  Only hypothesis 0 is
 * expanded at t=0 (:119); SOS is skipped after t=0 (:127-128); candidates are ranked by
 * (score+logit)/(length+1) in float32 (:306) and the best `beam` are returned in ASCENDING order
 * (best last, :310-312).  Ties follow a stable ascending sort of the reference's candidate bank:
 * (key, hypothesis index, logit, token id).  The per-hypothesis top-`topn` cut (:123, 64) cannot
 * bind while beam < topn, which this entry point requires, AS LONG AS the ranked scores are monotone in the logit within a
 * hypothesis.  The joint CTC-attention scores of las_ctc_prefix_step (K10c) are not: that entry point applies the cut itself and
 * gives every token outside a row's bank a -inf score, which never ranks above the bank's >= beam finite candidates.
 *   logits [nutt,beam,V]   score f32 [nutt,beam]   length int32 [nutt,beam]   nlive int32 [nutt]
 * Outputs (count in out_n[nutt]): out_parent, out_token int32 [nutt,beam]; out_score f32 [nutt,beam]
 * = new running sums.
 */
int las_beam_step(const float* logits, const float* score, const int* length, const int* nlive,
                  int nutt, int beam, int V, int topn, int t, int start_id,
                  int* out_parent, int* out_token, float* out_score, int* out_n, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10c  CTC prefix scores for joint CTC-attention beam search (Watanabe et al. 2017, Algorithm 2).  blank = class V of the
 * head's V + 1 classes; token id c is CTC class c; SOS is never a label; EOS is scored as an ordinary final label.
 *
 * las_ctc_log_softmax: logits fp32 [n, Tp, Vc] (contiguous; the head's enc . Wc + bc) -> out fp32 [n, Vc, Tp] = log_softmax over
 * the Vc classes, CLASS-MAJOR (a candidate's column is contiguous over t).  Once per batch: 4 n Vc Tp bytes (410 MB at n = 64,
 * Vc = 5001, Tp = 319).
 *
 * las_ctc_prefix_step: one search step, launched between the step's logits and las_beam_loop_step; all arguments are fixed across
 * the search (the step is read from *step: hipGraph friendly).  For every live row = u * beam + j (j < nlive[u], j = 0 at step 0;
 * utterances with done[u] or *step >= dec_step[u], and every row once *step >= Umax, are skipped) with entering token c = token[row]:
 *   - state_in[row] is the parent g's state (as gathered by las_beam_loop_step); it is advanced by c into state_out[row]
 *     (at step 0: the empty prefix's state, r^n = LOGZERO, r^b_t = sum_{tau <= t} y_tau[blank], psi = 0).  Row layout, state_width
 *     >= 2 Tp + 2 floats: [0, Tp) r^n_t, [Tp, 2 Tp) r^b_t, [2 Tp] psi(h), [2 Tp + 1] last label of h (-1: empty); t < T'_u only.
 *   - joint[row][v] = logits[row][v] + lam * (psi(h.v) - psi(h)), fp32 in this order, for v in the row's candidate bank (top-64 of
 *     logits[row] by (logit, token id); every token when V <= 64), -inf for every other token.  psi(h.EOS) = full-sequence
 *     log-probability of h.EOS.  Impossible prefixes get ~LOGZERO = -1e10, not -inf.
 * lp: las_ctc_log_softmax's output; enc_len [nutt]: T'_u (clamped to [1, Tp]).  Tp <= 2048, V <= 16384, state_in != state_out.
 * No atomics: two runs give the same bits.
 */
int las_ctc_log_softmax(const float* logits, int n, int Tp, int Vc, float* out, void* stream);
int las_ctc_prefix_step(const float* lp, const int* enc_len, int nutt, int beam, int Tp, int V, int end_id,
                        const float* logits, float* joint, float lam, const float* state_in, float* state_out,
                        int state_width, const int* token, const int* step, const int* nlive, const int* done,
                        const int* dec_step, int Umax, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10e  contextual biasing (hotword boosting) of the search by shallow fusion.  A context is a set of phrases (non-empty
 * token-id sequences without SOS / PAD) with one per-token weight beta > 0, compiled on the host (las/bias.py, ContextGraph) into a
 * token trie with node 0 = root.  depth(s); base(s) = depth of the deepest phrase-end node on the path root .. s (s included), 0 if
 * none; pend(s) = fl32(beta) * fl32(depth(s) - base(s)) = the bonus paid out for a match that is not complete yet.  Tables:
 *   child_off int32 [nnodes + 1], child_tok int32 [nchild] (ascending inside a node), child_next int32 [nchild] (rule 4 applied),
 *   gdef fp32 [nnodes] = -pend, groot fp32 [nnodes] = fl32(beta - pend).
 * Transition on token v from node s:  1. v is a child of s: t = child(s, v), gain beta;  2. else s != root and v is a child of the
 * root: t = child(root, v), gain groot[s];  3. else t = root, gain gdef[s] (nothing, and no add, from the root);  4. a t that ends a
 * phrase and has no children is the root, the bonus is kept (a phrase end WITH children stays, pend = 0).  EOS is an ordinary token.
 * No fail links: an occurrence that starts inside a failed partial match, other than at the failing token, is not seen.
 *
 * las_bias_step: one search step, launched behind the step's logits (behind las_ctc_prefix_step when that runs) and in front of
 * las_beam_loop_step; all arguments are fixed across the search (the step is read from *step: hipGraph friendly).  Live rows as for
 * las_ctc_prefix_step: row = u * beam + j with j < nlive[u] (j = 0 at step 0); utterances with done[u] or *step >= dec_step[u], and
 * every row once *step >= Umax, are skipped; rows that are not live are not written.  Per live row:
 *   - state_in[row][0] is the gathered parent's node as a float (the root at step 0 whatever the buffer holds; a value outside
 *     [0, nnodes) or not finite is the root); it is advanced by the entering token token[row] (outside [0, V): rule 3) and written to
 *     state_out[row][0].  state_width floats per row, only the first is used (the search passes 4: rows of 16 bytes keep the 16-byte
 *     path of las_beam_loop_step's gather for all the state tensors).
 *   - scores [nutt * beam, V] (the logits, or las_ctc_prefix_step's joint scores) in place: scores[row][v] receives exactly one fp32
 *     add of the gain of v from the advanced node, and none where the gain is 0; -inf stays -inf (a boosted token still has to make
 *     the CTC bank by its attention logit).  A row at the root touches only the root's children; a row with pend != 0 makes one pass
 *     over V.  The result is bit-identical to numpy float32 (tests/bias_ref.py).
 * K10's note that the top-`topn` cut cannot bind while beam < topn still holds when the cut is read as a cut on the ranked, biased score.
 * V <= 16384, nnodes <= 2^22, beta finite and > 0, state_in != state_out: refused (< 0, las_last_error) before anything is launched.
 * No atomics: two runs give the same bits.
 */
int las_bias_step(const int* child_off, const int* child_tok, const int* child_next, const float* gdef, const float* groot,
                  float beta, int nnodes, int nchild, float* scores, int nutt, int beam, int V, const float* state_in,
                  float* state_out, int state_width, const int* token, const int* step, const int* nlive, const int* done,
                  const int* dec_step, int Umax, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10f  shallow fusion of a back-off n-gram language model into the search.  The model -- order n <= 6 over token ids
 * [0, V), a log10 probability per stored n-gram and a log10 back-off weight per stored n-gram of order < n, dense unigrams -- is compiled
 * on the host (las/ngram.py, NgramLM) into a trie with node 0 = root = the empty context; every stored n-gram of order 1 .. n - 1 is a
 * node, highest-order n-grams are entries only.  Tables, every value PRE-SCALED on the host to fl32(w ln10 log10 x), one rounding:
 *   child_off int32 [nnodes + 1] (the root's list is empty), child_tok int32 [nchild] (ascending inside a node), child_lp fp32 [nchild],
 *   child_next int32 [nchild] = the node of the longest suffix of (context . token) that is a node,
 *   bow fp32 [nnodes], bo int32 [nnodes] = the node of the longest proper suffix that is a node (the root's is the root),
 *   uni_lp fp32 [V], uni_next int32 [V].
 * Transition on token c from node p: descend p, bo(p), ... to the first node that has c as a child and take that entry's next; the root
 * always has c (uni_next); a token outside [0, V) goes to the root.  At most `order` levels are descended before the root is taken.
 *
 * las_ngram_step: one search step, launched behind the step's logits (and the RNN LM's addition) and in front of las_ctc_prefix_step,
 * las_bias_step and las_beam_loop_step, so that the CTC bank cut and the hotword bonus see LM-fused logits; all arguments are fixed
 * across the search (the step is read from *step: hipGraph friendly).  Live rows exactly as for las_bias_step; rows that are not live
 * are not written.  Per live row:
 *   - state_in[row][0] is the gathered parent's node as a float (the root at step 0 whatever the buffer holds -- the entering token is
 *     then SOS, so the state becomes <s>'s node; a value outside [0, nnodes) or NaN is the root); it is advanced by token[row] and
 *     written to state_out[row][0].  state_width floats per row, only the first is used (the search passes 4, as for las_bias_step).
 *   - scores [nutt * beam, V] (the logits) in place, over the chain s0 = s, s1 = bo(s0), ..., root with acc0 = 0: every child v of s_i
 *     that no deeper level held gets scores[row][v] = fl32(scores[row][v] + fl32(acc_i + child_lp)); acc_{i+1} = fl32(acc_i +
 *     bow[s_i]); at the root every remaining v takes uni_lp[v] the same way.  Two fp32 adds per token in this order, nothing
 *     contracted; -inf stays -inf; EOS is an ordinary token.  The result is bit-identical to numpy float32 (tests/ngram_ref.py).
 * Bounds: child ranges are clamped to [0, nchild), child tokens outside [0, V) are skipped, a next or bo outside [0, nnodes) is the root.
 * 1 < V <= 16384, 1 <= nnodes <= 2^22, 1 <= order <= 6, state_in != state_out: refused (< 0, las_last_error) before anything is
 * launched.  No atomics and no reductions: two runs give the same bits.
 */
int las_ngram_step(const int* child_off, const int* child_tok, const float* child_lp, const int* child_next, const float* bow,
                   const int* bo, const float* uni_lp, const int* uni_next, int nnodes, int nchild, int order, float* scores,
                   int nutt, int beam, int V, const float* state_in, float* state_out, int state_width, const int* token,
                   const int* step, const int* nlive, const int* done, const int* dec_step, int Umax, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10k  attention coverage of the search's hypotheses (Chorowski & Jaitly 2017): how many of its utterance's encoder frames
 * a hypothesis has attended to, and how many it has over-attended -- a score term against skipping and looping, and a report.  For
 * alignments alpha_1 .. alpha_t over T'_u frames:  cum_t[j] = fl32(cum_{t-1}[j] + alpha_t[j]), cum_0 = 0 (one fp32 add per step and
 * frame, in step order);  covered_t = #{j < T'_u : cum_t[j] > tau};  over_t = #{j < T'_u : cum_t[j] > kappa};  a NaN never counts.
 *
 * las_coverage_step: one search step, launched behind the Speller step (las_speller_fwd, which writes alphas) and in front of the
 * other scorers and las_beam_loop_step; all arguments are fixed across the search (the step is read from *step: hipGraph friendly).
 * Live rows exactly as for las_bias_step; rows that are not live are not written.  Per live row:
 *   - state_in[row] is the gathered parent's state (all zeros at step 0 whatever the buffer holds); state_out[row] receives
 *     cum_t[0, Tp), then covered_t and over_t as fp32 values (exact below 2^24), then zeros up to state_width >= Tp + 2.  The search
 *     passes 4 ceil((Tp + 2) / 4): rows of whole 16-byte groups, read and written 16 bytes at a time when the buffers are aligned.
 *   - with dc = covered_t - covered_{t-1} and do = over_t - over_{t-1} (the parent's counts: the fp32 words of its row),
 *     score[row] = fl32(score[row] + fl32(fl32(w_c dc) - fl32(w_o do))): the gain goes to the PARENT's running sum that
 *     las_beam_loop_step adds every candidate's logit to -- a per-row constant, so the ranking inside a row, the top-64 cut and the
 *     CTC bank are unchanged and no [rows, V] tensor is touched.  Nothing is contracted into an fma.  w_c = w_o = 0: the counts are
 *     kept, score is neither read nor written.
 *   - hist (may be NULL) fp32 [Umax, nutt * beam, 2]: hist[*step][row] = (covered_t, over_t), the record the host reads a finished
 *     hypothesis' counts from.
 * alphas fp32 [nutt * beam, Tp]; enc_len int32 [nutt * beam] = T'_u of the row's utterance, clamped to [0, Tp]; `token` is unused.
 * Weights finite and >= 0, 0 < tau < kappa finite, state_width >= Tp + 2, state_in != state_out: refused (< 0, las_last_error)
 * before anything is launched.  Counts by ballot and popcount, the waves' sums added in wave order; no atomics: two runs give the
 * same bits, and numpy float32 gives them too (tests/coverage_ref.py).
 *
 * las_coverage_rows: the same counts for finished alignments alphas fp32 [U, R, Tp] (the layout the teacher-forced las_speller_fwd
 * writes): row r accumulates its first steps[r] (int32 [R], clamped to [0, U]) alignments in step order with the step kernel's own
 * accumulate-and-count functions -> counts int32 [R, 2] = (covered, over) against enc_len int32 [R] (clamped to [0, Tp]).
 */
int las_coverage_step(const float* alphas, const int* enc_len, int nutt, int beam, int Tp, float* score, float w_c, float w_o,
                      float tau, float kappa, float* hist, const float* state_in, float* state_out, int state_width,
                      const int* token, const int* step, const int* nlive, const int* done, const int* dec_step, int Umax,
                      void* stream);
int las_coverage_rows(const float* alphas, int U, int R, int Tp, const int* steps, const int* enc_len, float tau, float kappa,
                      int* counts, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10h CTC-only decoding: greedy and prefix beam search over the CTC head's logits, without the Speller.  Classes as in
 * K10c: Vc = V + 1, blank = class V.  enc_len int32 [n] (device) = T'_u, clamped to [0, Tp]; frames t >= T'_u are neither read nor written.
 *
 * las_ctc_frame_topk: logits fp32 [n, Tp, Vc] frame-major (the head product, before any softmax) ->
 *   best int32 [n, Tp]        the argmax class over all Vc, ties to the lower id;       best_lp fp32 [n, Tp]   its z - lse
 *   cand_tok int32 [n, Tp, C] the C non-blank classes of largest logit (ties to the lower id), LISTED IN ASCENDING TOKEN ID
 *   cand_lp fp32 [n, Tp, C]   their z - lse;                                            blank_lp fp32 [n, Tp]  the blank's
 *   lse = m + logf(sum expf(z - m)).  0 <= C <= min(64, V); C = 0 selects no candidates (cand_tok / cand_lp may be NULL).  The integer outputs are read off
 *   the raw logits: they do not depend on libm.
 * las_ctc_greedy: best / best_lp as above -> tokens int32 [n, Tp] (best[t] where it is not `blank` and differs from best[t - 1]; entries
 *   beyond lens[u] are not written), lens int32 [n], scores fp64 [n] = the sum of best_lp over the frames, in frame order.
 * las_ctc_beam_search: cand_tok / cand_lp / blank_lp as above -> per utterance up to K hypotheses, best first:
 *   tokens int32 [n, K, Tp], lens int32 [n, K], totals fp32 [n, K] = log(p_b + p_nb), nhyp int32 [n]; nothing is written beyond
 *   nhyp[u] or beyond a length.  The standard CTC prefix beam search; a prefix whose last token is `eos` is closed (never extended);
 *   a new token adds g = lm + len_bonus, lm = the pre-scaled back-off score las_ngram_step would add for it from the prefix' node
 *   (tables as K10f; nnodes = 0 and NULL tables: no n-gram, lm = 0; lm_start = the node of <SOS>).  Mass at or below -1e10 is no mass.
 *   Pruning keeps the K largest totals; ties: entries already in the beam in slot order, then extensions by (parent slot, candidate
 *   position).  Candidate tokens outside [0, V) are skipped; the n-gram bounds are K10f's.
 *   ws: las_ctc_beam_workspace_bytes(n, Tp, K, C) bytes (a prefix trie of K Tp + 1 nodes and its (parent, token) table per utterance).
 * 1 <= K <= 64, 1 <= C <= min(64, V), with an n-gram K10f's limits, a workspace of the full size: otherwise < 0 with a las_last_error
 * text before anything is launched.  No atomics: two runs give the same bits.  One launch each on `stream`, no synchronisation.
 */
int las_ctc_frame_topk(const float* logits, const int* enc_len, int n, int Tp, int Vc, int C, int* cand_tok, float* cand_lp,
                       float* blank_lp, int* best, float* best_lp, void* stream);
int las_ctc_greedy(const int* best, const float* best_lp, const int* enc_len, int n, int Tp, int blank, int* tokens, int* lens,
                   double* scores, void* stream);
size_t las_ctc_beam_workspace_bytes(int n, int Tp, int K, int C);
int las_ctc_beam_search(const int* cand_tok, const float* cand_lp, const float* blank_lp, const int* enc_len, int n, int Tp, int V,
                        int K, int C, int eos, float len_bonus, const int* child_off, const int* child_tok, const float* child_lp,
                        const int* child_next, const float* bow, const int* bo, const float* uni_lp, const int* uni_next, int nnodes,
                        int nchild, int order, int lm_start, int* tokens, int* lens, float* totals, int* nhyp, void* ws,
                        size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10i two-pass decoding: the attention decoder's log-likelihood of given token strings from the teacher-forced Speller's
 * logits, and the re-ranking of a first pass' N-best list with it.
 *
 * las_rescore_score: logits fp32, element (r, t, v) at logits[r*sb + t*st + v] (strides in elements, last axis contiguous, as
 *   las_ce_loss: the Speller's time-major [U, R, V] buffer is sb = V, st = R*V; a batch-major [R, U, V] one is sb = U*V, st = V).  No
 *   alignment beyond the floats' own is asked of the row bases.  y int32 [R, ldy] (ldy >= U), len int32 [R] clamped to [0, U].  For t < len[r]:
 *     term(r, t) = z[y] - lse,  lse = m + logf(s),  m = the row maximum,  s = sum_v expf(z[v] - m), all fp32;
 *     m = -inf (no class has mass): term = -inf, never NaN;  y outside [0, V): term = -inf, and nothing is read for it.
 *   Order of s (part of the contract; tests/rescore_ref.py's float32 mode repeats it): 256 lanes, lane i adds classes i, i + 256, ... in
 *   ascending order from 0.f, one rounding per add; inside each 64-lane wave a xor butterfly (distances 32, 16, 8, 4, 2, 1); the four
 *   wave sums added in order from 0.f (las_ctc_frame_topk's order).  Every load is one dword per lane: the order, and with it every bit
 *   of the result, does not depend on where the logits lie.
 *   att fp64 [R] = the sum of the row's fp32 terms in step order from 0.0; 0 for len = 0; -inf if a term is.
 *   step_lp fp32 [R, ldy] or NULL: receives the terms; entries at t >= len[r] are not written.  With step_lp = NULL the terms pass
 *   through ws, las_rescore_workspace_bytes(R, U) bytes (with step_lp, ws may be NULL).
 *   One workgroup per (row, step), then one wave per row: two launches on `stream`, no synchronisation.
 * las_rescore_rank: n utterances of K <= 64 slots, nhyp int32 [n] clamped to [0, K]; first fp32 [n, K] the first pass' scores, att fp64
 *   [n, K]; w inside [0, 1].  For k < nhyp[u]:
 *     total[u, k] = (float)((1 - w) * att + w * (double)first), every operation rounded on its own;
 *     order[u, 0 : nhyp[u]] = the slots by descending total; equal totals: the lower slot (the first pass' rank) first; NaN totals
 *     last, in slot order.  Slots k >= nhyp[u] are neither read nor written.  One launch.
 * Null pointers, R, U, V, n < 1, V > 2^30, R*U > 2^31 - 1, ldy < U, a negative stride, K outside [1, 64], w outside [0, 1] or NaN, a missing or
 * short workspace: < 0 with a las_last_error text before anything is launched.  No atomics: two runs give the same bits.
 */
size_t las_rescore_workspace_bytes(int R, int U);
int las_rescore_score(const float* logits, long long sb, long long st, const int* y, int ldy, const int* len, int R, int U, int V,
                      double* att, float* step_lp, void* ws, size_t ws_bytes, void* stream);
int las_rescore_rank(const float* first, const double* att, const int* nhyp, int n, int K, double w, float* total, int* order,
                     void* stream);

/* ------------------------------------------------------------------------------------------
 * K10j minimum word error rate training: the expected number of word errors over the hypotheses of every utterance, from the
 * Speller's logits of those hypotheses, and its gradient with respect to the logits (Prabhavalkar et al. 2018).
 *
 * las_mwer_loss: n utterances of K <= 64 slots; row r = u*K + k is slot k of utterance u.  logits fp32, element (r, t, v) at
 *   logits[r*sb + t*st + v] (strides in elements, last axis contiguous, as las_ce_loss / las_rescore_score: the Speller's time-major
 *   buffer is consumed in place); dlogits has the same strides.  y int32 [n K, ldy >= U]: the token scored at each step; len int32 [n K]
 *   clamped to [0, U]: steps t >= len[r] are never read; nhyp int32 [n] clamped to [0, K]: slots k >= nhyp[u] are absent, nothing of them
 *   (logits, y, len, err) is read and their seq_lp / post / coef are not written; err fp32 [n K]: the row's word error count, the
 *   caller's; scale_ptr: one fp32 on the device.  mode 0: N-best renormalisation; 1: sampling estimate.
 *     term(r, t) = z[y] - lse,  lse = m + logf(s),  m = the row maximum,  s = sum_v expf(z[v] - m), all fp32; m = -inf, or y outside
 *       [0, V): term = -inf (never NaN; nothing is read for such a label).  Order of s (part of the contract; tests/mwer_ref.py's float32
 *       mode repeats it): 64 lanes, lane i adds classes i, i + 64, ... in ascending order from 0.f, then a xor butterfly (32, 16, 8, 4, 2, 1).
 *     seq_lp[r] fp64 = the sum of the row's fp32 terms in step order from 0.0 (as las_rescore_score's att); 0 for len = 0.
 *   Everything per utterance is fp64, sums in slot order from 0.0 over the live slots, rounded to fp32 once where it is stored:
 *     mode 0: post = exp(seq_lp - max) / sum of those (all 0 if every live seq_lp is -inf);  risk[u] = sum_j post_j err_j;
 *             coef[r] = scale * post[r] * sum_j post_j (err[r] - err_j)   ( = scale post (err - risk), and exactly 0 when the errors are equal);
 *     mode 1: post = 1 / nhyp;  risk[u] = (sum_j err_j) / nhyp;  coef[r] = scale * (err[r] - risk[u]) / nhyp.
 *     risk[u] = 0 for nhyp[u] = 0.  loss[0] = (float)(scale * sum_u risk[u]): lane i of 64 adds utterances i, i + 64, ... in order, then
 *     the 64 partial sums in lane order.
 *   dlogits[r, t, v] = coef[r] * (onehot(y_t)[v] - expf(z[v] - lse)) in fp32 for t < len[r].  It is exactly 0.f -- stored without a look
 *   at the logits, so that no -inf / NaN of theirs leaks in -- for every v at t >= len[r], in every row of an absent slot, in every row
 *   whose fp32 coef or fp32 post is 0, and at a step without mass (lse = -inf).  Every element of [n K, U, V] is written; nothing else is.
 *   dlogits = NULL: no gradient.  seq_lp / post / coef / risk may each be NULL.
 * Refused before anything is launched (< 0 with a las_last_error text): a null pointer among the others, n or V < 1, K outside [1, 64], U
 * outside [1, 1024], n K U > 2^31 - 1, ldy < U, a negative stride, another mode, ws missing, not 8-byte aligned or shorter than
 * las_mwer_workspace_bytes(n, K, U).  Three launches on `stream` (one wave per (row, step); one workgroup per utterance; one wave per
 * (row, step)): the logits are read twice and written once.  No atomics: two runs give the same bits.
 */
size_t las_mwer_workspace_bytes(int n, int K, int U);
int las_mwer_loss(const float* logits, long long sb, long long st, int V, const int* y, int ldy, const int* len, const int* nhyp,
                  const float* err, int n, int K, int U, int mode, const float* scale_ptr, double* seq_lp, float* post, float* coef,
                  float* risk, float* loss, float* dlogits, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10d CTC Viterbi (forced) alignment of a token sequence to the encoder frames: token and word times.  The max-plus form
 * of las_ctc_loss's extended-label recursion (states 0 .. 2L: blank, label 0, blank, ..., label L-1, blank) with a back-trace.
 *   lp           las_ctc_log_softmax's output, fp32 [n, Vc, Tp] class-major, blank = class Vc - 1
 *   enc_len [n]  frames of row u, clamped to [1, Tp] (as las_ctc_prefix_step)
 *   y, y_len     the labels of row u are y[u, 0 : y_len[u]] (int32, pitch ldy >= U).  Any token id is a label, EOS included, and id 0 is
 *                NOT skipped (unlike las_ctc_loss): the caller passes exactly the sequence to align.
 *   score [n]    fp64: max over the paths pi that collapse to the labels of sum_{t < enc_len} lp[u, pi_t, t]
 *   first, last  int32 [n, U]: the inclusive frame range the best path spends on label j, j < y_len[u]; other entries are not written
 *   frame_state  int32 [n, Tp] or NULL: the state s in [0, 2L] of the best path at frame t, -1 for t >= enc_len[u]
 * Arithmetic (part of the contract): path scores are fp64; best(0, s) = (double)lp for s <= 1, -inf otherwise; best(t, s) = max(prev(s),
 * prev(s-1), prev(s-2) if s is a label that differs from the label before it) + (double)lp.  On equal values the smaller step wins (stay,
 * then s-1, then s-2); the final state is the larger of 2L and 2L-1, 2L on a tie.  One fp64 addition per frame and no products: a float64
 * restatement that adds in the same order along t gives the same bits (tests/ctc_align_ref.py), and so do two runs (no atomics).
 * A row that cannot be aligned -- y_len[u] outside [0, U], a label outside [0, Vc-2], or no path (L + repeats > enc_len) -- gets score =
 * -inf, first = last = -1 for j < min(max(y_len[u], 0), U) and frame_state = -1; the other rows are unaffected and the call returns 0.
 * Refused on the host before anything is launched: U > 511, Tp > 2048 (the limits of las_ctc_loss / las_ctc_prefix_step), n > 65535,
 * ws_bytes < las_ctc_align_workspace_bytes(n, Tp, U).  Three launches on `stream` (gather, recursion, back-trace), no synchronisation.
 */
size_t las_ctc_align_workspace_bytes(int n, int Tp, int U);
int las_ctc_align(const float* lp, int Vc, int Tp, const int* enc_len, int n, const int* y, int ldy, const int* y_len, int U,
                  int* first, int* last, int* frame_state, double* score, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10j keyword search (spoken-term detection) on the CTC head: where in a recording is a listed phrase said, and how sure
 * is the model?  It asks the posteriors, not a 1-best.  Plain arguments, no struct (as las_ctc_align).
 *   lp           las_ctc_log_softmax's output, fp32 [n, Vc, Tp] class-major, blank = class Vc - 1; finite values
 *   enc_len [n]  frames of utterance u, clamped to [1, Tp] (as las_ctc_align)
 *   y, y_len     P phrases shared by all utterances: the labels of phrase p are y[p, 0 : y_len[p]] (int32, pitch ldy >= U), L = y_len[p]
 *                in [1, min(U, 32)], labels in [0, Vc - 2]
 *   thr [P]      fp32, one threshold per phrase
 * The score (part of the contract).  m[u, t] = max_c lp[u, c, t] (fp32: exact in any order); e(c, t) = (double)lp[u, c, t] -
 * (double)m[u, t] <= 0, exactly 0.0 where c is the frame's arg-max.  A path's score is its log-likelihood ratio against the frame-wise
 * best path over the same window: <= 0, and exactly 0.0 when the phrase IS the greedy path there.  States s = 0 .. 2L - 2: even s = 2j
 * is label j, odd s the blank between labels j and j + 1; no leading or trailing blank (the window starts on the first label and ends
 * on the last), S = 2L - 1 <= 63.  Every state carries a pair (best, start).  In front of t = 0 every state is (-inf, -1).  For
 * t < T_u the candidates are taken in this order, a later one replacing an earlier one only if it is STRICTLY greater:
 *   1. stay (best(t-1, s), start(t-1, s));   2. s - 1, for s >= 1;   3. s - 2, for even s >= 2 whose label differs from the label
 *   before it;   4. the fresh start (0.0, t), for s = 0 only;
 * then best(t, s) = chosen + e(label_s, t) and the start is carried (at t = 0 only state 0 is alive, from the fresh start (0.0, 0)).
 * One fp64 subtraction and one fp64 addition per state and frame, in frame order, no products: a float64 restatement that does the same
 * gives the same bits (tests/kws_ref.py), and so do two runs (no atomics).  The tie rule gives a phrase that is the greedy path over
 * frames [a, b] start = a: staying in a 0-scoring first label beats a fresh start on the tie.
 *   end_score fp64 [n, P, Tp], end_start int32 [n, P, Tp], or both NULL: best(t, 2L - 2) and its start; -inf / -1 for t >= T_u.
 * Hits, from the end series while it is produced.  Frame t is a candidate (sc, st, t) when sc = end_score[t] > -inf and sc >=
 * (double)thr[p].  One open hit is kept at a time.  A candidate overlaps it when st <= open.end: it then replaces the open hit if sc >=
 * open.score (the later end on a tie: a hit ends on the last frame of its last label's run) and is dropped otherwise.  A candidate that
 * does not overlap (or finds no open hit) closes the open hit and opens a new one; at t = T_u the open hit is closed.  Closed hits go into
 * a kept list of capacity H in [1, 8], in time order; when it is full, the closing hit replaces the weakest kept hit (the smallest score,
 * the earliest among equals) only if it scores strictly greater -- the survivors are shifted and the new hit is appended -- and is
 * dropped otherwise.
 *   hit_start, hit_end int32 [n, P, H], hit_score fp64 [n, P, H]: the kept hits; entries at or beyond `kept` are not written
 *   count int32 [n, P, 2] = (kept, total closed)
 *   best_score fp64 [n, P], best_span int32 [n, P, 2]: independently of thr, the maximum of the end series with its (start, end); on
 *   equal values the later end; -inf, -1, -1 when no end state is ever reached (L + repeats > T_u)
 * A phrase that cannot be searched -- y_len[p] outside [1, min(U, 32)] or a label outside [0, Vc - 2] -- gets count = (0, 0), best =
 * -inf / -1 / -1 and a -inf / -1 series in every utterance; the other phrases are unaffected and the call returns 0.
 * Refused on the host with a las_last_error text before anything is launched: U > 32, Tp > 2048, H outside [1, 8], n > 65535, P > 65535,
 * exactly one of end_score / end_start NULL, ws_bytes < las_kws_workspace_bytes(n, Tp) (the frame maxima).  Two launches on `stream`
 * (frame maxima; one wavefront per utterance and phrase), no synchronisation.
 */
size_t las_kws_workspace_bytes(int n, int Tp);
int las_kws_search(const float* lp, int Vc, int Tp, const int* enc_len, int n, const int* y, int ldy, const int* y_len, const float* thr,
                   int P, int U, int H, int* hit_start, int* hit_end, double* hit_score, int* count, double* best_score, int* best_span,
                   double* end_score, int* end_start, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10g  consensus over the N-best list a search ends with: minimum-Bayes-risk choice and token confidences from the
 * unit-cost Levenshtein distances and alignments among the hypotheses of an utterance.  Plain arguments, no struct (as las_ctc_align).
 * A batch is n utterances with K hypothesis slots of at most U tokens:
 *   tok  int32 [n, K, U]  token ids; positions at or beyond a length hold anything
 *   len  int32 [n, K]     0 <= len <= U (clamped); an empty hypothesis is legal
 *   nhyp int32 [n]        0 <= nhyp <= K (clamped); slots k >= nhyp[u] are absent: nothing of them is read but their len, nothing written
 *   w    fp32  [n, K]     the posteriors, computed by the host (las/nbest.py); the kernels never exponentiate
 *
 * las_nbest_risk
 *   dist int32 [n, K, K]  the Levenshtein distance of every two live slots (insertion, deletion, substitution cost 1): each unordered
 *                         pair is computed once and both entries are written, the diagonal is 0; entries of absent slots are not written
 *   risk fp32  [n, K]     risk[u, i] = sum_k w[u, k] * float(dist[u, i, k]) for live i, added in the order k = 0 .. nhyp - 1 from 0.f, the
 *                         product and the sum separate fp32 operations (nothing contracted): bit-identical to sequential numpy float32
 *   pick int32 [n]        the live slot of least risk; on equal risk the larger w, then the lower index (comparisons on the fp32 values as
 *                         stored; a slot replaces the best so far only by risk < best or risk == best and w > best's); -1 where nhyp = 0
 *
 * las_nbest_confidence
 *   pivot int32 [n]       DEVICE array (las_nbest_risk's pick can be passed straight in): the slot every hypothesis is aligned to; -1, or
 *                         any value outside [0, nhyp[u]), writes nothing for the utterance
 *   Every live hypothesis b is aligned to the pivot a by D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1,
 *   D[i-1][j-1] + (a[i-1] != b[j-1])), traced back from (len_a, len_b) by ONE rule at (i, j), checked in this order:
 *     1. i, j > 0, a[i-1] == b[j-1] and D[i][j] == D[i-1][j-1]: a match, to (i-1, j-1);   2. i, j > 0 and D[i][j] == D[i-1][j-1] + 1: a
 *     substitution, to (i-1, j-1);   3. i > 0 and D[i][j] == D[i-1][j] + 1: the pivot token stays unmatched, to (i-1, j);   4. to (i, j-1).
 *   match int8 [n, K, U]  1 where pivot token i was matched in hypothesis k, else 0, for i < len of the pivot and live k (row k = pivot is
 *                         all ones); entries at or beyond the pivot's length and rows of absent slots are not written
 *   conf  fp32 [n, U]     conf[u, i] = sum_k w[u, k] * float(match[u, k, i]), same order and separate operations as risk; i < len of the pivot
 *
 * Both: integer outputs are exact, no atomics, one wavefront per dynamic programme whatever the batch, so two runs -- and the same
 * utterance at another place in another batch -- give the same bits; the distances behind the two entry points come from one routine.
 * CEILING: 1 <= U <= 1024 (a wave keeps the pivot's tokens and one boundary column of D in LDS; the search's Umax for a --max_segment_s
 * = 17 s recording is 282), 1 <= K <= 64, n <= 65535.  Outside that, or with ws_bytes < las_nbest_workspace_bytes(n, K, U) (the packed
 * 2-bit directions, n K ceil(U/16) 64 ceil(U/64) words; las_nbest_risk needs none), the call returns < 0 with a las_last_error text
 * before anything is launched.  Two launches each on `stream`, no synchronisation.
 */
size_t las_nbest_workspace_bytes(int n, int K, int U);
int las_nbest_risk(const int* tok, const int* len, const int* nhyp, const float* w, int n, int K, int U, int* dist, float* risk,
                   int* pick, void* stream);
int las_nbest_confidence(const int* tok, const int* len, const int* nhyp, const float* w, const int* pivot, int n, int K, int U,
                         signed char* match, float* conf, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10h  confusion network over the N-best list: the hypotheses of an utterance merged one after the other into a word
 * transition network (ROVER, Fiscus 1997) by a minimum-cost alignment with 0/1 costs; per bin the symbol of largest posterior mass.
 * Plain arguments; sym / len / nhyp / w as tok / len / nhyp / w of K10g (len and nhyp clamped the same way), except that symbols are
 * >= 0: a negative value is read as 0.  EPS = -1 is "no word here".  max_bins = the bins an utterance's network may have.
 * Per utterance the live slots are merged in the order k = 0 .. nhyp - 1 (the host passes them best first), starting from an empty
 * network, B = 0 bins.  To merge hypothesis b (length L) into B bins, with has(i, s) = symbol s was put into bin i by a hypothesis
 * merged before, cup(i) = 0 if has(i, EPS) else 1:
 *   D[0][j] = j,  D[i][0] = D[i-1][0] + cup(i),
 *   D[i][j] = min(D[i-1][j] + cup(i), D[i][j-1] + 1, D[i-1][j-1] + (has(i, b[j-1]) ? 0 : 1)),
 * traced back from (B, L) by ONE rule at (i, j), checked in this order:
 *   1. i, j > 0, has(i, b[j-1]) and D[i][j] == D[i-1][j-1]: b's token joins bin i as a match, to (i-1, j-1);
 *   2. i, j > 0 and D[i][j] == D[i-1][j-1] + 1: b's token becomes a new alternative of bin i, to (i-1, j-1);
 *   3. i > 0 and D[i][j] == D[i-1][j] + cup(i): b contributes EPS to bin i, to (i-1, j);
 *   4. otherwise a NEW BIN is inserted directly behind bin i, holding b's token for this slot and EPS for every slot merged before, to
 *      (i, j-1).
 * Overflow: with ins = the number of rule-4 steps, if B + ins > max_bins the hypothesis is NOT merged: the network stays as it is,
 * merged[u, k] = 0, and the later hypotheses are still tried.
 *   cols   int32 [n, K, max_bins]  cols[u, k, i] = the symbol slot k put into bin i, or EPS: the multi-alignment matrix.  Row k without its
 *                                  EPS entries is hypothesis k.  Rows of slots that were not merged are not written
 *   nbins  int32 [n]               the bins of the utterance's network (0 where nhyp = 0)
 *   merged int8  [n, K]            1 where the live slot was merged, else 0
 *   best   int32 [n, max_bins]     per bin the symbol (EPS included) of largest mass, mass(s) = sum over merged k with cols[k][i] == s of
 *   post   fp32  [n, max_bins]     w[k], added in k order from 0.f, one fp32 add each (bit-identical to sequential numpy float32); on equal
 *                                  mass the symbol whose first contributing slot is lower wins; post = that mass
 * Nothing is written beyond nbins[u], for absent slots, or -- but nbins = 0 -- for an utterance with nhyp = 0.  Integer outputs are
 * exact, no atomics, one wavefront per utterance whatever the batch: two runs, and the same utterance anywhere in any batch, give the
 * same bits.  CEILING: 1 <= K <= 64, 1 <= U <= 1024, 1 <= max_bins <= 2048, n <= 65535; outside that, or with ws_bytes <
 * las_nbest_network_workspace_bytes(n, K, U, max_bins) (per utterance the packed directions of the one table in flight, ceil(max_bins/16)
 * 64 ceil(U/64) words, and max_bins 8 ceil(K/4) words of network) or a workspace that is not 16-byte aligned, the call returns < 0 with
 * a las_last_error text before anything is launched.  One launch on `stream`, no synchronisation.
 */
size_t las_nbest_network_workspace_bytes(int n, int K, int U, int max_bins);
int las_nbest_network(const int* sym, const int* len, const int* nhyp, const float* w, int n, int K, int U, int max_bins, int* cols,
                      int* nbins, signed char* merged, int* best, float* post, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K10b device-resident BeamSearch.decode loop (las/beam_search.py:94-158) for `nutt` utterances at once: ONE call per
 * step prunes every utterance exactly as las_beam_step does AND keeps the reference's bookkeeping on the device, so
 * the host never waits inside the loop:
 *   - live hypotheses: score / length [nutt,beam] and nlive [nutt] updated in place (compacted, ascending rank);
 *   - back-pointer records of step t = *step: hist_parent (live slot of step t), hist_token, hist_score [Umax,nutt,beam],
 *     hist_n [Umax,nutt] picks, hist_slot [Umax,nutt,beam] (live slot k of step t+1 = pick hist_slot[t][u][k]);
 *   - retired hypotheses (EOS, :148-152; the live ones on step exhaustion, :155-156) appended as (sel_t, sel_j)
 *     references into the records, nsel [nutt]; selcap >= 3*beam;
 *   - done[u] set when `t+1 == dec_step[u]`, `nsel >= beam` (:94) or no live hypothesis is left; a done utterance is
 *     skipped by later calls;
 *   - src_row [nutt,beam] (global row the new live slot continues) and next_token [nutt*beam] for the next step, and
 *     the `ntens` recurrent-state tensors gathered accordingly: state_out[k][row] = state_in[k][src_row[row]]
 *     (state_width[k] floats per row; decoder h/c, previous alignment, LM states);
 *   - optionally the logits themselves are computed by the call (proj_*, below) instead of being read;
 *   - optionally a per-step record of one row tensor (the step's alignments): file_out[t][r] = file_in[r] for the nutt*beam rows of
 *     file_width floats (file_in NULL = none);
 *   - finally *step += 1 (device-resident step counter: the launch sequence is identical every step, hipGraph friendly).
 * All state is caller-owned and caller-initialised (score 0, length 0, nlive = beam, nsel = done = 0, *step = 0,
 * next_token = start_id).  The host reads the records once after the last step and rebuilds token ids by back-tracking.
 */
typedef struct {
    float* logits; float* score; int* length; int* nlive; int* nsel; int* done; const int* dec_step; int* step;
    int *hist_parent, *hist_token, *hist_slot; float* hist_score; int* hist_n;
    int *sel_t, *sel_j; int* src_row; int* next_token;
    int nutt, beam, V, Umax, selcap, topn, start_id, end_id;
    int ntens; const float* state_in[16]; float* state_out[16]; int state_width[16];
    const float* file_in; float* file_out; int file_width;
    /* optional: the vocabulary projection inside the step (two launches less per decode step): with proj_w != NULL
     * logits[row] = proj_b + bf16([proj_h0[row] ; proj_h1[row]]) . proj_w, proj_w = las_gemm_skinny_pack fragments of a [proj_k0 + proj_k1, V]
     * matrix (the Speller's output kernel on top of the LM's softmax kernel, pre-scaled by lm_weight and shifted to its token columns;
     * proj_h1 NULL = no second part), proj_h0 / proj_h1 fp32 [nutt*beam, proj_k0 / proj_k1] (multiples of 32), fp32 accumulation.
     * ceil(beam/16) * ceil(V/16) <= 8.  `logits` (may be NULL then) additionally receives the values. */
    const float* proj_h0; int proj_k0; const float* proj_h1; int proj_k1; const void* proj_w; const float* proj_b;
} las_beam_loop_args;
int las_beam_loop_step(const las_beam_loop_args* a, void* stream);
/* After the last step: walk the back-pointer records of every retired hypothesis on the device (the reference carries whole token
 * lists in its BeamState objects, las/beam_search.py:38-45).  For selection slot w = u*selcap + s (s < min(nsel[u], selcap)):
 * len[w] = tokens after SOS, ids[w][p] / rows[w][p] (p < len[w]; arrays [nutt*selcap, Umax]) = token and global state row
 * (u*beam + live slot) at step p, score[w] = running float32 sum; unused slots get len 0.  Only the record pointers and
 * nutt / beam / Umax / selcap of `a` are read. */
int las_beam_backtrack(const las_beam_loop_args* a, int* ids, int* rows, int* len, float* score, void* stream);

/* ------------------------------------------------------------------------------------------
 * Skinny-M product for per-step recurrences driven from the host (the char RNNLM step inside beam search,
 * lang/char_rnn_model.py:57-66 / las/beam_search.py:226-236; the Speller's own cell product uses the same kernel inside
 * las_speller_fwd): the weight W [K, N] (row-major fp32, leading dimension ldw) is packed ONCE into bf16 MFMA fragments
 * (las_gemm_skinny_pack_bytes(K, N) bytes), then every call computes C[M, N] = bf16(A[M, K]) . bf16(W) + bias (accumulate = 0) or
 * C += ... (accumulate = 1) with fp32 accumulation, for 1 <= M <= 1024 rows: grid = (N / 16 column tiles) x (M / 16 row tiles),
 * eight waves split K with every load in flight at once.  Same arithmetic as las_gemm in LAS_PREC_BF16 (operands rounded to
 * bf16, fp32 sums) at a fifth of the time for M = 256.
 */
size_t las_gemm_skinny_pack_bytes(int K, int N);
int las_gemm_skinny_pack(const float* W, int ldw, int K, int N, void* packed, void* stream);
int las_gemm_skinny(const float* A, int lda, int M, int K, const void* packed, int N, float* C, int ldc, const float* bias,
                    int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------
 * F1  input side of the step loop: TFRecord reader + bucket_by_sequence_length + pinned batch ring + H2D upload
 * (reference tfrecord_data_loader.py:54-109: list_files / parallel_interleave(cycle_length 16) / map(data_parser) /
 * bucket_by_sequence_length(pad_to_bucket_boundary) / shuffle(64) / repeat / prefetch -- TensorFlow's C++ input threads in the
 * reference, one producer thread per reader here; train.py:45-55,114-117 is the consumer).  Host code; the only device
 * interaction is the asynchronous copy of las_input_upload.  Batch order is a pure function of (files, seed) and equals the
 * Python restatement in tfrecord_data_loader.py (same splitmix64 stream).  rank / world: lock-step data parallelism -- a bucket
 * emits when it holds world x batch_limit utterances and this rank keeps rows rank, rank + world, ... of that global batch, so
 * every rank runs the same bucket shape at every step.
 */
typedef struct las_input_config {
    int feat_dim;                 /* MFCC coefficients per channel (13): a frame is feat_dim x 3 floats */
    int is_training;              /* 1: shuffle + repeat forever; 0: one pass, then las_input_next returns 1 */
    int n_bounds;                 /* number of bucket boundaries (<= 16) */
    int bounds[16];               /* tfrecord_data_loader.py:75,80 */
    int batch_limit[17];          /* tfrecord_data_loader.py:83, per rank */
    int max_tokenlen;             /* token rows are padded to this (219 train / 227 eval, :76,:81) */
    int shuffle_buffer;           /* batches (64 train, 0 eval) */
    int cycle_length;             /* files read round robin (16) */
    unsigned long long seed;
    int rank, world;
    int slots;                    /* pinned batches in flight (>= 2) */
} las_input_config;

typedef struct las_input_batch {
    int slot, B, T, bucket, global_B, max_tokenlen;
    const float* feat;            /* [B, T, feat_dim, 3] zero padded, pinned host memory (valid until the slot is released) */
    const int* token;             /* [B, max_tokenlen] zero padded */
    const int* featlen;           /* [B] */
    const int* tokenlen;          /* [B] */
} las_input_batch;

unsigned int las_crc32c(const void* data, size_t n);              /* CRC-32C (Castagnoli) of a host buffer: the TFRecord framing's checksum */
void* las_input_open(const char* const* files, int nfiles, const las_input_config* cfg);   /* NULL on error (las_last_error) */
int las_input_next(void* reader, las_input_batch* out);          /* blocks; 0 = a batch, 1 = end of data, < 0 = error */
/* asynchronous copy of the slot's features / tokens to caller-owned device buffers on `stream`; the reader does not refill the
 * slot before that copy has executed.  Follow with las_input_release. */
int las_input_upload(void* reader, int slot, float* d_feat, int* d_token, void* stream);
int las_input_release(void* reader, int slot);
long long las_input_records(void* reader);                       /* records parsed so far */
void las_input_close(void* reader);

/* ------------------------------------------------------------------------------------------
 * K12  audio front end: waveform -> feature cube (preprocess.py:71-86: speechpy.feature.mfcc / mfe at :71-80,
 * speechpy.processing.cmvn(variance_normalization=True) at :84, speechpy.feature.extract_derivative_feature at :85), for a batch
 * of n utterances of different lengths in one call.  Arithmetic of the restatement in this build's preprocess.py:
 *   frames    T_u = floor((n_u - fl) / step) frames of fl <= 512 samples every `step` samples, rectangular window, no padding of the
 *             signal (the last full frame is dropped, as speechpy does)
 *   spectrum  frame zero-padded to 512, real FFT, P[k] = |X[k]|^2 / 512 (k = 0..256); frame energy = sum_k P[k]
 *   mel       P . fb^T in fp32 over each filter's non-zero bins; an exact 0 (filter output or energy) becomes 2^-52
 *   mfcc      logf, orthonormal DCT-II (table dct [feat_dim, num_filters]), coefficient 0 replaced by log(energy)
 *   fbank     the filter outputs as they are (feat_dim == num_filters; no log, as the reference)
 *   cmvn != 0 per utterance and column: mean over its T_u frames, ddof-0 standard deviation of the mean-subtracted column (two
 *             fixed-order passes, in double over the fp32 features), x = (x - mean) / (std + 2^-30); then derivative_extraction twice, window 2, ALONG THE FEATURE
 *             AXIS with edge padding (the reference's quirk).  out fp32 [n, Tmax, feat_dim, 3], zeros behind T_u.
 *   cmvn == 0 out fp32 [n, Tmax, feat_dim]: the raw features, zeros behind T_u.
 * The tables are the caller's (built in double, rounded to fp32): twiddle [257][2] = (cos, -sin)(2 pi k / 512); fb [num_filters, 257];
 * fb_range int32 [num_filters][2] = first and last non-zero bin of each filter (first > last: an empty filter); dct (mfcc only).
 * samples: fp32 or int16 (samples_i16: value / 32767, what read_audio does to 16-bit files) [n, ld_samples]; n_samples int32 [n] on
 * the device, n_samples_host the same values on the host (what the entry validates: fl <= n_u <= ld_samples, 1 <= T_u <= Tmax).
 * No atomics: two calls on the same inputs give the same bits.  ws >= las_frontend_workspace_bytes(n, Tmax, feat_dim, cmvn).
 */
enum { LAS_FEAT_MFCC = 0, LAS_FEAT_FBANK = 1 };
typedef struct las_frontend_args {
    const void* samples; int samples_i16; long long ld_samples;
    const int* n_samples; const int* n_samples_host;
    int n, Tmax, fl, step, feat_type, feat_dim, num_filters, cmvn;
    const float* twiddle; const float* fb; const int* fb_range; const float* dct;
    float* out;
    void* ws; size_t ws_bytes;
} las_frontend_args;
size_t las_frontend_workspace_bytes(int n, int Tmax, int feat_dim, int cmvn);
int las_frontend(const las_frontend_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * K13  band-limited resampler in front of las_frontend: a batch of n waveforms from one sample rate to another (fs_out / fs_in =
 * L / M in lowest terms), with a per-utterance gain in the same pass.  sox's `speed s` is this with fs_in = fs * s (the reference's
 * augmentation, preprocess.py:157-167 through utils/augmentation.py).  The arithmetic is preprocess.resample's, in fp32:
 *   n_out[u] = ceil(n_in[u] * L / M);  output m reads n0 = (m M) / L, phase p = (m M) % L (64-bit products) and is
 *   out[u, m] = gain[u] * sum_{i = 0 .. 2W-1} x[u, n0 - W + 1 + i] * table[p, i],  x zero outside [0, n_in[u]),
 *   ONE fmaf chain over the taps in ascending order: a row gives the bits it gives alone, and the same bits on every run.
 * table [L, 2W] is the caller's (preprocess.resample_table in double, rounded to fp32), 8-byte aligned.  L == M == 1 is the gain-only path
 * out = gain * in (one rounding; with gain NULL a bit copy of fp32 input; table may be NULL).
 * One launch on `stream`, no atomics, no synchronisation.  Every element of out [n, ld_out] is written, zeros behind n_out[u].
 * The entry validates on the host before it launches: 1 <= n <= 65535, 1 <= L, M <= 2^20, 1 <= W, 2W <= 1024, L * 2W <= 2^20,
 * a workgroup's input span (tile - 1) M / L + 1 + 2W fits its staging buffer (las_resample_tile > 0),
 * 1 <= n_in_host[u] <= ld_in, las_resample_out_len(n_in_host[u], L, M) <= ld_out <= INT32_MAX.
 */
typedef struct las_resample_args {
    const void* in; int in_i16; long long ld_in;      /* [n, ld_in] fp32 or int16 (value / 32767, as las_frontend) */
    const int* n_in; const int* n_in_host;            /* samples per row, device and host copies */
    int n, L, M, W;                                   /* K = 2W taps */
    const float* table;                               /* [L, 2W] fp32, device, 8-byte aligned */
    const float* gain;                                /* [n] fp32 on the device, or NULL = 1 */
    float* out; long long ld_out;                     /* [n, ld_out] fp32; every element written, zeros behind n_out[u] */
    int* n_out;                                       /* [n] int32 on the device, or NULL */
} las_resample_args;
long long las_resample_out_len(long long n_in, int L, int M);     /* ceil(n_in * L / M); < 0 for bad arguments */
int las_resample_tile(int L, int M, int W);           /* consecutive outputs of one utterance a workgroup owns; <= 0: ratio refused */
int las_resample(const las_resample_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * K14  SpecAugment (Park et al., 2019) on the feature cube in front of the Listener: one piecewise-linear time warp, mF frequency
 * masks and mT time masks per utterance.  The entry APPLIES a plan and draws nothing (las/specaug.py draws on the host).
 *   in, out  fp32 [B, Tmax, F, C], contiguous, 4-byte aligned; they must not overlap (refused on the host).
 *   plan     int32 [B, ldp] on the device, plan_host the same values on the host (what the entry validates); ldp a multiple of 4,
 *            >= 4 + 2 (mF + mT).  Row b = {len, w0, w, 0, (f0, fw) x mF, (t0, tw) x mT}.
 * Time warp (w == 0: none): output frames [0, w0 + w] read source [0, w0], output frames [w0 + w, len - 1] read source [w0, len - 1].
 * The source position of output frame t is an exact rational in 32-bit integers: on the left i0 = (t w0) / (w0 + w), r = (t w0) %
 * (w0 + w); on the right i0 = w0 + ((t - w0 - w) (len - 1 - w0)) / (len - 1 - w0 - w), r the remainder.  frac = r / den is ONE fp32
 * division and the value is fmaf(frac, x[i0 + 1] - x[i0], x[i0]); with r == 0 it is a bit copy of x[i0] and x[i0 + 1] is not read (so a
 * row with w == 0 is a bit copy).  Masked elements -- frames [t0, t0 + tw) of a time mask, bins [f0, f0 + fw) of a frequency mask in
 * every channel, frames t >= len -- are +0.0f by a select: the source is not read there, a NaN underneath does not survive.
 * Zero-width masks do nothing.  One launch on `stream`, no atomics, no synchronisation; every element of out is written; a row gives
 * the bits it gives alone, whatever the tile (las_specaug_tile frames per workgroup) and the batch.
 * Validated on the host before the launch: 1 <= B <= 65535, 1 <= Tmax <= 32768, F, C >= 1, Tmax F C <= INT32_MAX, mF, mT <= 16, ldp;
 * per row 0 <= len <= Tmax; w == 0 or both segments non-empty (1 <= w0, 1 <= w0 + w, w0 + w <= len - 2, w0 <= len - 2); masks inside
 * [0, F] and [0, len].
 */
typedef struct las_specaug_args {
    const float* in; float* out;                      /* [B, Tmax, F, C] fp32 */
    const int* plan; const int* plan_host; int ldp;   /* [B, ldp] int32, device and host copies */
    int B, Tmax, F, C, mF, mT;
} las_specaug_args;
int las_specaug_tile(void);                           /* consecutive frames of one utterance a workgroup owns */
int las_specaug(const las_specaug_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * K15  energy voice-activity detector and segmenter in front of las_frontend: a batch of n recordings of very different
 * lengths -> per recording the runs of frames that hold speech.  Plain arguments, no struct (as las_ctc_align).
 *   frames    the front end's: T_u = floor((n_u - fl) / step) (0 when n_u < fl), frame t covers samples [t step, t step + fl).  samples
 *             fp32 or int16 (samples_i16: value / 32767 in fp32, as las_frontend) [n, ld_samples], finite; n_samples int32 [n] on the
 *             device, n_samples_host the same values on the host (what the entry validates).
 *   energy    e[u, t] is a DOUBLE: the sum over the frame's samples, in ascending order, of x x, starting at 0, x the fp32 sample widened
 *             to double -- the product is exact in double, every step is one rounding, a numpy loop gives the same bits.
 *   peak      emax[u] = max_t e[u, t] (0 for T_u = 0);  thr[u] = max(emax[u] * ratio, floor), ONE double multiply.
 *   raw       raw[t] = e[t] >= thr && e[t] > 0
 *   dilation  s[t] = any raw[t'] with |t' - t| <= hang, clipped to [0, T_u): pads the speech, joins gaps of at most 2 hang frames
 *   runs      a run is a maximal stretch [a, b) of s; runs shorter than min_run frames are dropped
 * Outputs: runs int32 [n, max_runs, 2]: runs[u, k] = (a, b) in ascending order for k < n_runs[u], entries behind the count are NOT
 * written; n_runs int32 [n] always written (0 for silence and for T_u = 0).  energy fp64 [n, Tmax] (frames t >= T_u written as 0) and
 * emax fp64 [n] may be NULL.  las_vad_max_runs(T, hang) = ceil(T / (2 hang + 2)) is the most runs T frames can hold (< 0: bad
 * arguments); las_vad_tile() the frames of one recording a workgroup owns.
 * Six launches on `stream` (energies + tile peaks, row peak, tile summaries, row scan, emit, filter + compact), no atomics, no
 * synchronisation: two calls give the same bits, and a row gives the result it gives alone, whatever the batch and the tile.
 * Refused on the host before anything is launched (< 0, las_last_error): a NULL samples / n_samples / n_samples_host / runs / n_runs /
 * ws; n outside 1..65535; Tmax < 1; fl < 1 or step < 1; hang < 0; min_run < 2 (a run of r frames yields r - 1 front-end frames, and
 * the front end needs one); ratio outside (0, 1]; floor < 0 or not finite; max_runs < las_vad_max_runs(Tmax, hang); ld_samples
 * outside [1, INT32_MAX]; n_samples_host[u] outside [1, ld_samples]; T_u > Tmax; ws_bytes < las_vad_workspace_bytes(n, Tmax).
 */
int       las_vad_tile(void);
long long las_vad_max_runs(long long T, int hang);
size_t    las_vad_workspace_bytes(int n, long long Tmax);
int       las_vad(const void* samples, int samples_i16, long long ld_samples,
                  const int* n_samples, const int* n_samples_host, int n, int Tmax, int fl, int step,
                  double ratio, double floor, int hang, int min_run,
                  double* energy, double* emax, int* runs, int max_runs, int* n_runs,
                  void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K16  multi-condition training data between las_resample and las_frontend: a room impulse response convolved into every
 * utterance, and background noise mixed in at a given signal-to-noise ratio.  Plain arguments, no struct (as las_vad).  The arithmetic
 * is preprocess.reverberate's and preprocess.mix_noise's, in fp32.  Both entries APPLY per-utterance choices and draw nothing
 * (las/augment.py draws on the host).  Every pointer but the *_host ones is a device pointer; a *_host array holds the same values
 * on the host and is what the entry validates.
 *
 * las_reverb   out[u, m] = sum_{k = 0 .. K-1} h[k] * in[u, m + delay - k] for m < n_in[u], `in` zero outside [0, n_in[u]); h = rir[r],
 *   K = rir_len[r], delay = rir_delay[r], r = rir_idx[u].  The output has the input's length and the direct path (tap `delay`) does
 *   not shift it.  Direct-form FIR; SUMMATION ORDER: ONE fmaf chain per output, from +0, over the taps in ASCENDING k, followed by up to
 *   15 zero taps (the last block of 16 taps is padded; they add +-0).  A row gives the bits it gives alone, and the same bits on every
 *   call: the tile, the batch and the other rows' responses do not matter.  A row with rir_idx[u] = -1 is a bit copy of its input.
 *   Every element of out [n, ld_out] is written, zeros behind n_in[u]; nothing behind n_in[u] is read.  One launch, no atomics.
 *   in fp32 [n, ld_in]; rir fp32 [n_rir, ld_rir]; out fp32 [n, ld_out].  las_reverb_tile(): the consecutive outputs of one utterance a
 *   workgroup owns; las_reverb_tap_chunk(): the taps it stages at a time.
 *   Refused on the host before the launch (< 0, las_last_error): a NULL pointer; n outside 1..65535; n_rir < 1; a pitch outside
 *   [1, INT32_MAX]; rir_len_host[r] outside [1, min(16384, ld_rir)]; rir_delay_host[r] outside [0, rir_len_host[r]); rir_idx_host[u]
 *   outside [-1, n_rir); n_in_host[u] outside [1, min(ld_in, ld_out)]; in and out overlapping.
 *
 * las_noise_mix   v[m] = noise[r, (noise_off[u] + m) mod noise_len[r]], r = noise_idx[u] (the index in 64 bits);  Ps = mean of in^2 and
 *   Pn = mean of v^2 over m < n_in[u], both fixed-order sums in double over the fp32 samples (per tile of las_noise_mix_tile() samples:
 *   a thread's samples in ascending order, then a fixed tree; then the tiles the same way);  g = sqrt(Ps / (Pn 10^(snr_db[u] / 10))) in
 *   double, rounded to fp32 once, 0 when Ps or Pn is 0;  out[u, m] = fmaf(g, v[m], in[u, m]).  A row with noise_idx[u] = -1 or g = 0 is
 *   a bit copy of its input.  Every element of out is written, zeros behind n_in[u]; in == out (with equal pitches) is allowed.
 *   gain_out fp32 [n] (g; 0 for rows without noise) may be NULL.  Three launches, no atomics: the same bits on every call, and a row
 *   gives the bits it gives alone.  ws >= las_noise_mix_workspace_bytes(n, the longest n_in_host[u]) (any ld >= that will do), 8-byte
 *   aligned.
 *   Refused on the host before anything is launched: a NULL pointer (gain_out excepted); n outside 1..65535; n_noise < 1; a pitch
 *   outside [1, INT32_MAX]; noise_len_host[r] outside [1, ld_noise]; noise_idx_host[u] outside [-1, n_noise); n_in_host[u] outside
 *   [1, min(ld_in, ld_out)]; for a row with noise, noise_off_host[u] outside [0, noise_len) or snr_db_host[u] not finite; a workspace
 *   that is too small; in and out overlapping without being the same buffer.
 */
int    las_reverb_tile(void);
int    las_reverb_tap_chunk(void);
int    las_reverb(const float* in, long long ld_in, const int* n_in, const int* n_in_host, int n,
                  const float* rir, long long ld_rir, const int* rir_len, const int* rir_len_host,
                  const int* rir_delay, const int* rir_delay_host, int n_rir,
                  const int* rir_idx, const int* rir_idx_host, float* out, long long ld_out, void* stream);
int    las_noise_mix_tile(void);
size_t las_noise_mix_workspace_bytes(int n, long long ld);
int    las_noise_mix(const float* in, long long ld_in, const int* n_in, const int* n_in_host, int n,
                     const float* noise, long long ld_noise, const int* noise_len, const int* noise_len_host, int n_noise,
                     const int* noise_idx, const int* noise_idx_host, const int* noise_off, const int* noise_off_host,
                     const float* snr_db, const float* snr_db_host,
                     float* out, long long ld_out, float* gain_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K17  speaker diarization of long recordings without a trained model: the Bayesian information criterion between
 * full-covariance Gaussians (Chen & Gopalakrishnan 1998) finds the speaker changes inside a run of speech (las_bic_change) and
 * drives the agglomerative clustering of the pieces (las_bic_cluster).  Plain arguments, no struct (as las_vad).  All reals are
 * doubles unless stated.  Every pointer but the *_host ones is a device pointer; a *_host array holds the same values on the host
 * and is what the entry validates.
 *   inputs     feat fp32 [N, ld], a row = a frame, the first D columns are used (1 <= D <= LAS_BIC_MAX_DIM = 20); mask uint8 [N] or
 *              NULL (= all ones); S sequences, sequence s = the rows [seq_off[s], seq_off[s] + seq_len[s]).  Only rows inside a
 *              listed sequence are read, and of those only the columns < D.
 *   statistics of a set F of frames, over its frames with mask != 0 only: n = their number, S1 = sum x, S2 = sum x x^T, every fp32 x
 *              widened to double first (a product is exact; every sum runs in frame order);
 *              Sigma(F) = (S2 - S1 S1^T / n) / n + floor I;  L(F) = log det Sigma(F), by Cholesky.  floor > 0 keeps digital silence
 *              and constant frames from giving a singular matrix.  The statistics of a union are the sums of its parts'.
 *   dBIC(X, Y; lambda) = 1/2 [n L(X u Y) - n1 L(X) - n2 L(Y)] - lambda 1/2 (D + D (D + 1) / 2) log n,  n = n1 + n2
 *
 * las_bic_change   w >= 2, hop >= 1, nmin >= 1.  Sequence s has C_s = las_bic_candidates(seq_len[s], w, hop) candidates (0 when the
 *   sequence is shorter than 2 w, else (len - 2 w) / hop + 1; < 0: bad arguments), candidate c at the local frame t = w + c hop:
 *   v[c] = dBIC([t - w, t), [t, t + w); lambda), -inf when either window holds fewer than nmin masked frames.  With R = ceil(w / hop),
 *   c is a change point iff v[c] > 0, v[c] > v[c'] for every existing c' in [c - R, c) and v[c] >= v[c'] for every existing c' in
 *   (c, c + R]: the first of equal maxima wins, two change points are more than w frames apart.  cand_off int32 [S + 1] is the
 *   exclusive prefix of the C_s (the caller computes it); v fp64 and peak uint8 hold cand_off[S] entries, sequence s's from
 *   cand_off[s]; nothing behind the last candidate is written.  Two launches (none when there is no candidate), no workspace.
 *   Refused on the host before anything is launched (< 0, las_last_error): a NULL feat / seq_off / cand_off / seq_off_host /
 *   seq_len_host / v / peak; D outside 1..20; N < 1; ld < D; S < 1; a sequence outside [0, N); w < 2, hop < 1, nmin < 1; lambda or
 *   floor not finite, floor < 0; more than INT32_MAX candidates.
 *
 * las_bic_cluster  one problem per recording: recording r owns the units (sequences, as above) [rec_off[r], rec_off[r + 1]), S_r of
 *   them, 1 <= S_r <= LAS_BIC_MAX_UNITS; indices i, j below count inside the recording.  d(i, j) = dBIC of the two units' statistics
 *   with lambda.  Loop over the live units: take the pair i < j of least d (ties: the smallest i, then the smallest j); stop when one
 *   unit is left, when K > 0 and at most K are live (the sign of d is ignored), or when K = 0 and d >= 0; else add j's statistics
 *   to i's, retire j and recompute d(i, .).  Outputs: label int32 [S], the clusters of a recording numbered from 0 in the order of
 *   their earliest unit; n_clusters int32 [n_rec]; optionally dist fp64 [S, ldd], ldd = max_r S_r: dist[s, j] = the INITIAL d(i, j) of
 *   unit s = rec_off[r] + i for i < j < S_r (nothing else is written); optionally merges int32 [S, 2] and merge_val fp64 [S] (both or
 *   neither) and n_merges int32 [n_rec]: recording r's m-th merge (i, j) and its d at row rec_off[r] - r + m.
 *   Every unit needs a masked frame: n_masked_host int32 [S] states the units' masked frame counts on the host (NULL allowed iff mask
 *   is NULL); the kernels count for themselves.  Three launches (statistics, pairs, one workgroup per recording for the loop), no
 *   atomics.  ws >= las_bic_cluster_workspace_bytes(S, max_r S_r, D) (0: bad arguments), 8-byte aligned.
 *   Refused on the host before anything is launched: a NULL feat / seq_off / seq_len / rec_off / *_host / label / n_clusters / ws; a
 *   mask without n_masked_host; merges without merge_val or the reverse; D, N, ld, S, lambda, floor as above; an empty sequence or
 *   one outside [0, N); n_rec outside 1..S; K < 0; rec_off_host not running from 0 to S; S_r outside 1..LAS_BIC_MAX_UNITS; a unit
 *   without a masked frame; a workspace that is too small.
 * Both: a sequence gives the bits it gives alone, whatever else the call holds, and two calls give the same bits.
 */
#define LAS_BIC_MAX_DIM 20
#define LAS_BIC_MAX_UNITS 1024
long long las_bic_candidates(long long len, int w, int hop);
int       las_bic_change(const float* feat, long long N, long long ld, int D, const unsigned char* mask,
                         const int* seq_off, const int* cand_off, const int* seq_off_host, const int* seq_len_host, int S,
                         int w, int hop, int nmin, double lambda, double floor,
                         double* v, unsigned char* peak, void* stream);
size_t    las_bic_cluster_workspace_bytes(int S, int Smax, int D);
int       las_bic_cluster(const float* feat, long long N, long long ld, int D, const unsigned char* mask,
                          const int* seq_off, const int* seq_len, const int* rec_off,
                          const int* seq_off_host, const int* seq_len_host, const int* n_masked_host, int S,
                          const int* rec_off_host, int n_rec, int K, double lambda, double floor,
                          int* label, int* n_clusters, double* dist, int* merges, double* merge_val, int* n_merges,
                          void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * K18  microphone arrays: the delays of every channel against a reference channel from the peak of the PHAT-weighted
 * cross-correlation per window (las_gcc_phat), smoothed over the windows by a Viterbi pass (las_tdoa_track), then the channels
 * shifted, weighted and summed (las_delay_sum) -- BeamformIt's scheme (Anguera et al. 2007) without its N-best lists.  No trained
 * model.  Plain arguments, no struct (as las_vad).  One recording per call; every pointer is a device pointer.  All work goes on the
 * caller's stream, no atomics, no cross-workgroup synchronisation: two calls give the same bits.
 *   geometry   x [C, ld], int16 (x_i16 != 0; widened as v / 32767, as in las_vad) or fp32; 2 <= C <= LAS_BF_MAX_CHANNELS; n <= ld
 *              samples per row are read; ref = the reference channel.  Windows of L samples (even) every H = L / 2; the largest lag
 *              1 <= D <= LAS_BF_MAX_LAG; the FFT length NF a power of two, L + D <= NF <= LAS_BF_MAX_FFT.  Wn = las_bf_windows(n, L) =
 *              1 if n <= L, else ceil((n - L) / H) + 1 (< 0: bad arguments); window w covers the samples [w H, w H + L), samples at
 *              or behind n read as 0.  ws >= las_bf_workspace_bytes(C, Wn, NF, D) (0: bad arguments), 8-byte aligned: the tracker's
 *              back-pointers (int16 [C, Wn, 2 D + 1]) and las_gcc_phat's fp32 copies of its two tables.
 *
 * las_gcc_phat   r fp32 [C, Wn, 2 D + 1], column D + tau = lag tau:  X_c = FFT_NF(hann . x_c[window]);
 *   G_c[k] = X_c[k] conj(X_ref[k]) / max(|X_c[k] conj(X_ref[k])|, 1e-12);  r_c[tau] = Re IFFT_NF(G_c)[tau mod NF], -D <= tau <= D.
 *   A channel that lags the reference by tau samples (x_c[t] = s[t - tau]) peaks at +tau.  The row of ref is computed like any
 *   other: 1 at lag 0 where the window has signal.  hann: double [L], hann[i] = 0.5 - 0.5 cos(2 pi (i + 0.5) / L); twiddle: double
 *   [NF / 2 + 1, 2], (cos, -sin)(2 pi k / NF) -- the caller computes both in double, the call rounds them to fp32 once; the
 *   transforms run in fp32.  Two launches (the tables; one workgroup per window, which computes the reference spectrum once).
 *
 * las_tdoa_track   reads r, writes tau int32 [C, Wn] and a fp32 [C, Wn].  Per channel c != ref, all arithmetic in double on the widened r:
 *   score[0][s] = r[0][s];  score[w][s] = r[w][s] + max_s' (score[w-1][s'] - gamma |s - s'|), the product and the difference each
 *   rounded once (never contracted); ties at a back-pointer go to the smaller |s - s'|, then the smaller s'.  The last window takes
 *   the arg-max of score, ties to the smaller |tau|, then the smaller tau; the path is traced back from there.  tau[ref][w] = 0.
 *   Weights: q_c[w] = max(0, r_c[w][tau_c[w]]) for c != ref, q_ref[w] = max_{c != ref} q_c[w]; a_c[w] = q_c[w] / sum_c q_c[w], the sum
 *   in channel order; where the sum is 0 the reference gets 1 and the others 0.  gamma finite, >= 0.  Two launches (one wave per
 *   channel steps through the windows; the weights).  The kernel picks the two candidate predecessors of a state, one on either
 *   side, by a prefix and a suffix maximum of score[s'] +- gamma s' and evaluates and compares those two as written above: equal to the
 *   maximum over all predecessors wherever gamma s' and the sums are exact, within two roundings of it elsewhere.
 *
 * las_delay_sum   reads x, tau, a, writes y fp32 [n]:  z_w[t] = sum_c a_c[w] x_c[t + tau_c[w]] in channel order, reads outside [0, n)
 *   are 0;  p = clamp((t - H) / H, 0, Wn - 1), w0 = floor(p), f = p - w0;  y[t] = (1 - f) z_w0[t] + f z_min(w0 + 1, Wn - 1)[t]: a linear
 *   cross-fade between window centres, one window alone at both ends.  Integer delays only.  One launch, no workspace.
 *
 * Refused on the host before anything is launched (< 0, las_last_error): a NULL pointer; C, L, D, NF, n, ld, ref, Wn, gamma outside the
 * above; a workspace that is too small or misaligned; las_delay_sum's Wn != las_bf_windows(n, L).
 */
#define LAS_BF_MAX_CHANNELS 16
#define LAS_BF_MAX_FFT 16384
#define LAS_BF_MAX_LAG 512
long long las_bf_windows(long long n, int L);
size_t    las_bf_workspace_bytes(int C, long long Wn, int NF, int D);
int       las_gcc_phat(const void* x, int x_i16, long long ld, int C, long long n, int ref, int L, int D, int NF,
                       const double* hann, const double* twiddle, float* r, void* ws, size_t ws_bytes, void* stream);
int       las_tdoa_track(const float* r, int C, long long Wn, int D, int ref, double gamma, int* tau, float* a,
                         void* ws, size_t ws_bytes, void* stream);
int       las_delay_sum(const void* x, int x_i16, long long ld, int C, long long n, int L, long long Wn,
                        const int* tau, const float* a, float* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * K19  microphone arrays, adaptive: a mask-driven MVDR (minimum-variance distortionless-response) beamformer in the STFT
 * domain, in Souden's reference-channel form (Souden, Benesty, Affes 2010): the noise covariance from the frames an energy rule
 * calls non-speech, the speech covariance per block of frames, no array geometry, no delay estimate, no steering vector.  No trained
 * model.  Plain arguments, no struct (as K18).  One recording per call; every pointer is a device pointer.  All work goes on the
 * caller's stream, no atomics, no cross-workgroup synchronisation: every output value is computed by one thread or one workgroup in
 * a fixed order, and two calls give the same bits.  Samples at or behind n in a row are never read.
 *   geometry   x [C, ld], int16 (x_i16 != 0; widened as v / 32767) or fp32; 2 <= C <= LAS_BF_MAX_CHANNELS; n <= ld.  The frame length
 *              NF is a power of two, 64 <= NF <= LAS_MVDR_MAX_FFT; the hop Hs = NF / 2; K = NF / 2 + 1 bins.
 *              Tf = las_mvdr_frames(n, NF) = ceil(n / Hs) + 1 (< 0: bad arguments); frame t covers the samples [(t - 1) Hs, (t + 1) Hs),
 *              reads outside [0, n) are 0: every sample lies in exactly two frames.  The window win[i] = sin(pi (i + 0.5) / NF) serves
 *              analysis and synthesis (win[i]^2 + win[i + Hs]^2 = 1: the pair reconstructs exactly).  win: double [NF]; twiddle: double
 *              [NF / 2 + 1, 2], (cos, -sin)(2 pi k / NF) -- the caller computes both in double, a call rounds them to fp32 once (as
 *              las_gcc_phat); the transforms run in fp32: X_c[t, k] = FFT_NF(win . x_c[frame t])[k].  Blocks of Bf >= 1 frames: block b
 *              holds the frames [b Bf, min(Tf, (b + 1) Bf)), Nb = las_mvdr_blocks(Tf, Bf) = ceil(Tf / Bf) (< 0: bad arguments).
 *              Complex doubles are interleaved (re, im).  ws >= las_mvdr_workspace_bytes(C, Tf, NF, Bf) (0: bad arguments), 8-byte
 *              aligned, the same buffer for the calls of one recording: the fp32 tables, the frame energies of las_mvdr_mask, and
 *              the partial sums las_mvdr_cov's first launch hands to its last two.
 *
 * las_mvdr_mask   m fp32 [Tf] from channel ref alone, by las_vad's rule on these frames:  e[t] (double) = the sum over the frame's
 *   samples, in ascending order from 0, of x x with x widened to double (no window; reads outside [0, n) are 0);  emax = max_t e[t];
 *   thr = max(emax * ratio, floor), one multiply;  raw[t] = e[t] >= thr && e[t] > 0;  m[t] = 1 if any raw[t'] with |t' - t| <= hang,
 *   else 0.  energy: double [Tf] or NULL.  ratio in (0, 1]; floor >= 0, finite; hang >= 0.  Three launches.
 *
 * las_mvdr_cov   takes any m with values in [0, 1] (not checked: the array is on the device).  s_t = (double) m[t], q_t = 1.0 - s_t.
 *   counts double [1 + Nb]: counts[1 + b] = M_b = sum_{t in b} s_t in ascending t; counts[0] = N0 = sum_b (sum_{t in b} q_t), the
 *   inner sums in ascending t, the outer in ascending b.  phi_n [K, C, C] complex double:  phi_n[k][i][j] = (sum_t q_t X_i[t, k]
 *   conj(X_j[t, k])) / N0, zeros where N0 == 0;  phi_y [Nb, K, C, C]:  phi_y[b][k][i][j] = (sum_{t in b} s_t X_i conj(X_j)) / M_b,
 *   zeros where M_b == 0.  Both exactly Hermitian as stored (the lower triangle the conjugate of the upper, the diagonal's imaginary
 *   part 0).  WHERE THE SUMS ARE ROUNDED: s_t and q_t are rounded to fp32; a block's frames are cut into tiles of at most 256
 *   consecutive frames (fewer where that gives the device about a thousand tiles); within a tile the products and the sums are
 *   fp32 (fused multiply-adds, in ascending t); the tiles' sums are added in double, in ascending tile order, and divided in
 *   double.  Six launches (tables; tiles; the counts, two; phi_y; phi_n).
 *
 * las_mvdr_weights   w [Nb, K, C] complex double, valid int32 [Nb, K]; all in double, per (b, k):  tn = Re tr(phi_n[k]) / C;
 *   A = phi_n[k] + loading tn I (loading > 0, finite);  P = phi_y[b][k] - phi_n[k];  G = A^-1 P from a Cholesky factorisation of A;
 *   g = Re tr(G), the diagonal added in channel order;  valid = (N0 > 0 && M_b > 0 && tn > 0 && g > 1e-6) (an A that does not
 *   factorise gives g = NaN: not valid);  where valid, w_raw[c] = G[c][ref] / g.  A hold pass per bin over the blocks:  w[b][k] =
 *   w_raw of the nearest valid block b' <= b; if there is none, of the nearest valid b' > b; if bin k has no valid block, the unit
 *   vector e_ref.  valid reports the test, not the hold.  Two launches, no workspace.
 *
 * las_mvdr_apply   y fp32 [n]:  b(t) = t / Bf;  Y[t, k] = sum_c conj(w[b(t)][k][c]) X_c[t, k], in channel order in fp32, w rounded to
 *   fp32 once; the imaginary parts of Y[t, 0] and Y[t, NF / 2] are dropped;  f_t = win . IFFT_NF(Y[t, .]) (the Hermitian extension
 *   of the K bins);  output segment j, the samples [j Hs, (j + 1) Hs), is f_j's second half plus f_j+1's first half, in that
 *   order.  With w = e_ref everywhere y is x_ref up to the fp32 transforms' error.  Two launches.
 *
 * Refused on the host before anything is launched (< 0, las_last_error): a NULL pointer (but energy); C, NF, n, ld, ref, Bf, Nb, ratio,
 * floor, hang, loading outside the above; a workspace that is too small or misaligned.
 */
#define LAS_MVDR_MAX_FFT 1024
long long las_mvdr_frames(long long n, int NF);
long long las_mvdr_blocks(long long Tf, int Bf);
size_t    las_mvdr_workspace_bytes(int C, long long Tf, int NF, int Bf);
int       las_mvdr_mask(const void* x, int x_i16, long long ld, int C, long long n, int ref, int NF, double ratio, double floor,
                        int hang, float* m, double* energy, void* ws, size_t ws_bytes, void* stream);
int       las_mvdr_cov(const void* x, int x_i16, long long ld, int C, long long n, int NF, int Bf, const float* m,
                       const double* win, const double* twiddle, double* counts, double* phi_n, double* phi_y,
                       void* ws, size_t ws_bytes, void* stream);
int       las_mvdr_weights(const double* phi_n, const double* phi_y, const double* counts, int C, int NF, long long Nb, int ref,
                           double loading, double* w, int* valid, void* stream);
int       las_mvdr_apply(const void* x, int x_i16, long long ld, int C, long long n, int NF, int Bf, const double* w,
                         const double* win, const double* twiddle, float* y, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LAS_HIP_H */
