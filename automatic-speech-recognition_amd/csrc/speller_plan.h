// speller_plan.h -- which kernel family serves las_speller_fwd / las_speller_bwd (plan_speller, the one place that decides it for both
// passes) and the predicates it is built from.  Included by speller.hip behind bwd_layout.
#pragma once

// speed mode, additive attention: the row kernels read bf16 copies of Ws / keys / encoder rows (made once per call)
static bool bf_rows_ok(const DecDev& d) {
    return !(d.flags & LAS_SPELLER_NO_BF_ROWS) && d.mode == LAS_ATT_ADD && (d.A % 8) == 0 && (d.Hd % 8) == 0 && d.A <= 256;
}
// ... and, for the common single-layer geometry, the fully prefetching variants
static bool pf_geom_ok(const DecDev& d) {
    return d.NL == 1 && d.D <= 512 && d.A <= 128 && d.Hd <= 512 && d.Tp <= 224 && d.E <= 1024 && (d.E % 2) == 0 && (d.D % 2) == 0 &&
           (d.A % 8) == 0 && (d.Hd % 8) == 0;
}
static bool pf_rows_ok(const DecDev& d) { return !(d.flags & LAS_SPELLER_NO_PF_ROWS) && bf_rows_ok(d) && pf_geom_ok(d); }
// ... and the whole loop in one launch: 8 groups of pn product + R row workgroups, all co-resident (one per compute unit),
// tpw column tiles per product workgroup and kw k-steps per product wave as instantiated in the kernels
constexpr int LOOP_TPW_F = 5, LOOP_KW_F = 3, LOOP_TPW_B = 3, LOOP_KW_B = 4;
static bool loop_geom_ok(const DecDev& d, int ncols, int K, int tpw, int kw) {
    const int R = cdiv(d.B, 8), pn = las_device_cus() / 8 - R;
    // (U >= 4: a launch of the persistent grid costs ~100 us before its first step -- 256 workgroups, placement handshake -- which
    //  30 us saved per step only repays from the fourth step on; beam search calls the step with U = 1: 141 vs 43 us, r3 decode trace)
    return d.U >= 4 && (d.E % 4) == 0 && (d.D % 4) == 0 && (d.Hd % 4) == 0 && ((d.E + d.Hd + d.D) % 8) == 0 && (K % 8) == 0 && R <= 16 &&
           pn >= 1 && pn + R <= 32 && pn * tpw >= cdiv(ncols, 16) && 16 * kw >= cdiv(K, 32);
}
static bool loop_ok(const DecDev& d, int ncols, int K, int tpw, int kw) {
    return !(d.flags & LAS_SPELLER_NO_FUSED_STEP) && pf_rows_ok(d) && loop_geom_ok(d, ncols, K, tpw, kw);
}
// Location-aware attention (round 3): served by the SAME loop kernels (pf_fwd_row / pf_bwd_row with LOC = true: conv1d over the
// previous alignment from LDS, the f . Wf term in the energies, d f / d alpha_{t-1} in the gradient loop; keys / Wf / filter gradients
// contracted over the steps afterwards) when BOTH loops are eligible, so that forward and gradient stay in one arithmetic family
// (bf16 row operands); otherwise the wide path or the per-step fp32-operand row kernels dec_step_{fwd,bwd}_kernel<.,.,true>.
static bool loc_loop_ok(const DecDev& d, int G) {
    const int GD = G * d.D, I0D = d.E + d.Hd + d.D;
    return d.mode == LAS_ATT_LOC && !(d.flags & (LAS_SPELLER_NO_PF_ROWS | LAS_SPELLER_NO_BF_ROWS | LAS_SPELLER_NO_FUSED_STEP)) &&
           pf_geom_ok(d) && (d.A % 32) == 0 && d.C >= 1 && d.C <= 10 && d.Kc * d.C <= 4096 && cdiv(d.Tp, 8) <= RNG &&
           cdiv(d.Tp, 16) <= RNW && bf_lds_bytes(d) <= 128 * 1024 &&     // the MFMA convs: one wave per 16-frame tile; the row state in LDS
           loop_geom_ok(d, GD, I0D, LOOP_TPW_F, LOOP_KW_F) && loop_geom_ok(d, d.Hd + d.D, GD, LOOP_TPW_B, LOOP_KW_B);
}
static constexpr size_t LOOP_LDS_MAX = 159 * 1024;                 // a loop workgroup has its CU to itself (160 KB less the kernels' static LDS)

struct SpellerPlan {
    int family;          // LAS_SPELLER_RAN_{LOOP, PF_ROWS, BF_ROWS, F32_ROWS, WIDE}
    bool skinny;         // layer 0's per-step cell product on packed bf16 fragments (las_skinny_gemm_bf16)
    bool locloop;        // LOOP with location-aware attention
    bool bf_copies;      // the bf16 operand copies of Ws / keys / enc (make_bf_copies)
    bool act_save;       // the forward keeps its activations in act_save, the backward hands act_save to its kernels
    size_t lds_row;      // the fp32-operand rows' dynamic LDS (row_lds_bytes): <= 150 KB, above 64 KB location-aware only
    size_t lds_bf;       // the bf16 rows' (bf_lds_bytes): checked where LOOP / PF_ROWS / BF_ROWS run
    size_t lds_loop;     // LOOP: the launch's (row state + resident encoder slabs, or the product workgroups' partial tiles)
    int ran;             // the LAS_SPELLER_RAN_* word las_speller_last_variant reports
};

// The one place that decides which kernel family serves a pass.  What differs between the passes is their own work:
//  * the skinny cell product's operand: forward xin0 [B][I0D] . W0, backward gates [B][GD] . W0^T;
//  * the loop kernels' in-loop product: forward every gate column over K = I0D, backward the chain columns [E, I0D) over K = GD;
//  * the workspace: the forward may run without one (no skinny product below the embedding buckets' offset, no wide path below the
//    split-K region's); the backward has checked that it holds the whole layout.
// act_save (header word 0 says which forward filled it; every other forward clears it):
//  * forward LOOP / PF_ROWS (U > 1) -> LAS_ACT_MAGIC: the attention activations (+ the conv outputs f): read by a backward LOOP or
//    PF_ROWS (the same row code: the bench geometry at B = 64 runs the forward on PF_ROWS, the backward on LOOP);
//  * forward WIDE, location-aware (U > 1) -> LAS_ACT_MAGIC_WIDE: the conv outputs f only: read by a backward WIDE;
//  * BF_ROWS / F32_ROWS / additive WIDE neither leave nor read anything; a backward ignores a header it does not know.
template <int CELL, bool FAST>
static int plan_speller(const DecDev& d, bool bwd, const BwdWs& w, size_t ws_bytes, SpellerPlan& p) {
    constexpr int G = CELL == LAS_CELL_LSTM ? 4 : 1;
    const int GD = G * d.D, I0D = d.E + d.Hd + d.D;
    const bool loc = d.mode == LAS_ATT_LOC;
    const char* who = bwd ? "speller bwd" : "speller";
    p = SpellerPlan{};
    p.lds_row = row_lds_bytes(d, bwd);
    // (location-aware attention with the reference's K = 201, C = 10: the staged filter + Wf push the carve past 64 KB)
    LAS_ARG(p.lds_row <= 150 * 1024 && (p.lds_row <= 64 * 1024 || loc), "%s: row state does not fit LDS (%zu bytes)", who, p.lds_row);
    const int K0 = bwd ? GD : I0D, N0 = bwd ? I0D : GD;
    const void* A0 = bwd ? (const void*)d.gates : (const void*)d.xin0;
    p.skinny = FAST && ws_bytes >= w.embp && (K0 % 8) == 0 && las_skinny_ok(d.B, K0, N0, K0, A0);
    const bool bfrows = p.skinny && bf_rows_ok(d);
    const bool pf = bfrows && pf_rows_ok(d);
    p.locloop = p.skinny && loc_loop_ok(d, G);
    const bool loop = p.locloop || (pf && (bwd ? loop_ok(d, d.Hd + d.D, GD, LOOP_TPW_B, LOOP_KW_B) : loop_ok(d, GD, I0D, LOOP_TPW_F, LOOP_KW_F)));
    // round 6: the wide path (speller_wide.h), forced by LAS_SPELLER_WIDE wherever the geometry allows; by default the multi-layer and
    // location-aware calls that the loop kernels do not take (until round 5: the per-utterance fp32-operand row kernels) -- in BOTH modes:
    // in parity mode it is 62.4 against 85.2 ms (run.sh recipe, rnn cells), 90.0 against 112.3 (lstm), 50.4 against 58.2 (configs[3]);
    // the one-layer additive geometry keeps the per-utterance rows there (42.9 against 44.7 ms on the wide path).  In speed mode
    // LAS_SPELLER_NO_BF_ROWS asks for the fp32-operand rows.
    bool wide = !(d.flags & LAS_SPELLER_NO_WIDE) && ws_bytes >= w.gemm && wide_geom_ok(d) && (!FAST || p.skinny);
    if (wide && !(d.flags & LAS_SPELLER_WIDE))
        wide = !(FAST && (d.flags & LAS_SPELLER_NO_BF_ROWS)) && !loop && !pf && (d.NL >= 2 || loc);
    if (wide) p.locloop = false;
    p.family = wide ? LAS_SPELLER_RAN_WIDE : loop ? LAS_SPELLER_RAN_LOOP : pf ? LAS_SPELLER_RAN_PF_ROWS : bfrows ? LAS_SPELLER_RAN_BF_ROWS
                                                                                                           : LAS_SPELLER_RAN_F32_ROWS;
    const bool bf_family = !wide && (bfrows || p.locloop);             // LOOP, PF_ROWS, BF_ROWS
    p.bf_copies = bf_family || (wide && FAST);
    p.act_save = (bwd || d.U > 1) && (p.family == LAS_SPELLER_RAN_LOOP || p.family == LAS_SPELLER_RAN_PF_ROWS || (wide && loc));
    p.lds_bf = bf_lds_bytes(d);
    if (bf_family) LAS_ARG(p.lds_bf <= (p.locloop ? 128 : 64) * 1024, "%s: row state does not fit LDS (%zu bytes)", who, p.lds_bf);  // (loop launches: 96 KB attribute)
    if (p.family == LAS_SPELLER_RAN_LOOP) {
        const size_t lds_pr = (size_t)RNW * (bwd ? LOOP_TPW_B : LOOP_TPW_F) * 1024;          // the product workgroups' partial tiles
        const size_t lds_rw = p.lds_bf + enc_res_bytes(d, p.locloop, loop_ne(d.Tp), bwd);      // row state + resident encoder slabs
        p.lds_loop = lds_rw < lds_pr ? lds_pr : lds_rw;
        LAS_ARG(p.lds_loop <= LOOP_LDS_MAX, "%s: the loop's row state does not fit LDS (%zu bytes)", who, p.lds_loop);
    }
    p.ran = p.family | (p.skinny ? LAS_SPELLER_RAN_SKINNY : 0) | (loc ? LAS_SPELLER_RAN_LOC : 0) |
            (wide && FAST && d.NL > 1 ? LAS_SPELLER_RAN_UPPER_SKINNY : 0);
    return 0;
}
