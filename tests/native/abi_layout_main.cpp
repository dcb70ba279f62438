// Prints the layout of every argument struct include/las_hip.h declares, as the C++ compiler sees it:
//   struct <name> <sizeof>
//   field <struct> <field> <offsetof> <sizeof>
// tests/test_cabi_and_host.py compares the lines with the ctypes structures of las/_hip.py, which are laid out by hand.  The field lists
// below are written by hand next to the header: a struct or field added there is added here (the test names a struct that is missing).
#include <cstddef>
#include <cstdio>

#include "../../include/las_hip.h"

#define STRUCT(T) std::printf("struct %s %zu\n", #T, sizeof(T))
#define FIELD(T, f) std::printf("field %s %s %zu %zu\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))

int main() {
    STRUCT(las_seq_prepare_desc);
    FIELD(las_seq_prepare_desc, whh_fw); FIELD(las_seq_prepare_desc, whh_bw); FIELD(las_seq_prepare_desc, ldw); FIELD(las_seq_prepare_desc, cell);
    FIELD(las_seq_prepare_desc, H); FIELD(las_seq_prepare_desc, B); FIELD(las_seq_prepare_desc, bwd); FIELD(las_seq_prepare_desc, flags);
    FIELD(las_seq_prepare_desc, ws); FIELD(las_seq_prepare_desc, ws_bytes);
    STRUCT(las_gemm_plan_info);
    FIELD(las_gemm_plan_info, kernel); FIELD(las_gemm_plan_info, tile_m); FIELD(las_gemm_plan_info, tile_n); FIELD(las_gemm_plan_info, loader);
    FIELD(las_gemm_plan_info, in_bf16); FIELD(las_gemm_plan_info, grid_order); FIELD(las_gemm_plan_info, splitk); FIELD(las_gemm_plan_info, kchunk);
    FIELD(las_gemm_plan_info, grid_x); FIELD(las_gemm_plan_info, grid_y); FIELD(las_gemm_plan_info, grid_z);
    STRUCT(las_rnn_seq_plan_info);
    FIELD(las_rnn_seq_plan_info, kernel); FIELD(las_rnn_seq_plan_info, P); FIELD(las_rnn_seq_plan_info, rows_per_tile);
    FIELD(las_rnn_seq_plan_info, launches); FIELD(las_rnn_seq_plan_info, x_chunks); FIELD(las_rnn_seq_plan_info, rows);
    FIELD(las_rnn_seq_plan_info, dout_chunks); FIELD(las_rnn_seq_plan_info, progress_words);
    STRUCT(las_rnn_seq_args);
    FIELD(las_rnn_seq_args, cell); FIELD(las_rnn_seq_args, prec); FIELD(las_rnn_seq_args, B); FIELD(las_rnn_seq_args, T); FIELD(las_rnn_seq_args, H);
    FIELD(las_rnn_seq_args, gates); FIELD(las_rnn_seq_args, whh_fw); FIELD(las_rnn_seq_args, whh_bw); FIELD(las_rnn_seq_args, ldw);
    FIELD(las_rnn_seq_args, out); FIELD(las_rnn_seq_args, ld_out); FIELD(las_rnn_seq_args, out_bstride); FIELD(las_rnn_seq_args, cstate);
    FIELD(las_rnn_seq_args, forget_bias); FIELD(las_rnn_seq_args, flags); FIELD(las_rnn_seq_args, status); FIELD(las_rnn_seq_args, ws);
    FIELD(las_rnn_seq_args, ws_bytes); FIELD(las_rnn_seq_args, x_chunk_flag); FIELD(las_rnn_seq_args, x_chunk_steps); FIELD(las_rnn_seq_args, row_T);
    FIELD(las_rnn_seq_args, dout); FIELD(las_rnn_seq_args, ld_dout); FIELD(las_rnn_seq_args, dout_bstride); FIELD(las_rnn_seq_args, dbias_fw);
    FIELD(las_rnn_seq_args, dbias_bw); FIELD(las_rnn_seq_args, dout_chunk_flag); FIELD(las_rnn_seq_args, dout_chunk_rows);
    FIELD(las_rnn_seq_args, dout_rows); FIELD(las_rnn_seq_args, progress); FIELD(las_rnn_seq_args, progress_steps);
    STRUCT(las_speller_fwd_args);
    FIELD(las_speller_fwd_args, B); FIELD(las_speller_fwd_args, Tp); FIELD(las_speller_fwd_args, Hd); FIELD(las_speller_fwd_args, A);
    FIELD(las_speller_fwd_args, D); FIELD(las_speller_fwd_args, NL); FIELD(las_speller_fwd_args, E); FIELD(las_speller_fwd_args, V);
    FIELD(las_speller_fwd_args, U); FIELD(las_speller_fwd_args, cell); FIELD(las_speller_fwd_args, mode); FIELD(las_speller_fwd_args, prec);
    FIELD(las_speller_fwd_args, Kc); FIELD(las_speller_fwd_args, C); FIELD(las_speller_fwd_args, step_logits);
    FIELD(las_speller_fwd_args, keep_state0); FIELD(las_speller_fwd_args, flags); FIELD(las_speller_fwd_args, forget_bias);
    FIELD(las_speller_fwd_args, seed); FIELD(las_speller_fwd_args, enc); FIELD(las_speller_fwd_args, keys); FIELD(las_speller_fwd_args, enc_len);
    FIELD(las_speller_fwd_args, Ws); FIELD(las_speller_fwd_args, u); FIELD(las_speller_fwd_args, emb); FIELD(las_speller_fwd_args, Wv);
    FIELD(las_speller_fwd_args, bv); FIELD(las_speller_fwd_args, loc_w); FIELD(las_speller_fwd_args, loc_b); FIELD(las_speller_fwd_args, Wf);
    FIELD(las_speller_fwd_args, cellW); FIELD(las_speller_fwd_args, cellb); FIELD(las_speller_fwd_args, tokens_in);
    FIELD(las_speller_fwd_args, tokens_out); FIELD(las_speller_fwd_args, logits); FIELD(las_speller_fwd_args, alphas);
    FIELD(las_speller_fwd_args, align0); FIELD(las_speller_fwd_args, emb_mask); FIELD(las_speller_fwd_args, emb_noise);
    FIELD(las_speller_fwd_args, hs); FIELD(las_speller_fwd_args, cs); FIELD(las_speller_fwd_args, gates); FIELD(las_speller_fwd_args, xin0);
    FIELD(las_speller_fwd_args, act_save); FIELD(las_speller_fwd_args, ws); FIELD(las_speller_fwd_args, ws_bytes);
    FIELD(las_speller_fwd_args, status); FIELD(las_speller_fwd_args, companion);
    FIELD(las_speller_fwd_args, row_group);
    STRUCT(las_speller_bwd_args);
    FIELD(las_speller_bwd_args, f); FIELD(las_speller_bwd_args, dlogits); FIELD(las_speller_bwd_args, d_enc); FIELD(las_speller_bwd_args, d_keys);
    FIELD(las_speller_bwd_args, dWs); FIELD(las_speller_bwd_args, du); FIELD(las_speller_bwd_args, demb); FIELD(las_speller_bwd_args, dWv);
    FIELD(las_speller_bwd_args, dbv); FIELD(las_speller_bwd_args, dloc_w); FIELD(las_speller_bwd_args, dloc_b); FIELD(las_speller_bwd_args, dWf);
    FIELD(las_speller_bwd_args, dcellW); FIELD(las_speller_bwd_args, dcellb);
    STRUCT(las_shadow_desc);
    FIELD(las_shadow_desc, src0); FIELD(las_shadow_desc, src1); FIELD(las_shadow_desc, ld0); FIELD(las_shadow_desc, ld1);
    FIELD(las_shadow_desc, rows); FIELD(las_shadow_desc, cols0); FIELD(las_shadow_desc, cols1); FIELD(las_shadow_desc, transpose);
    FIELD(las_shadow_desc, dst); FIELD(las_shadow_desc, dst_rows); FIELD(las_shadow_desc, dst_cols); FIELD(las_shadow_desc, dst_ld);
    FIELD(las_shadow_desc, dst_bf16);
    STRUCT(las_lstm_cell_args);
    FIELD(las_lstm_cell_args, x); FIELD(las_lstm_cell_args, x_bf16); FIELD(las_lstm_cell_args, ldx); FIELD(las_lstm_cell_args, I);
    FIELD(las_lstm_cell_args, ids); FIELD(las_lstm_cell_args, id_shift); FIELD(las_lstm_cell_args, xrows); FIELD(las_lstm_cell_args, h);
    FIELD(las_lstm_cell_args, ldh); FIELD(las_lstm_cell_args, Wx); FIELD(las_lstm_cell_args, Wh); FIELD(las_lstm_cell_args, bias);
    FIELD(las_lstm_cell_args, c_prev); FIELD(las_lstm_cell_args, fb); FIELD(las_lstm_cell_args, c_out); FIELD(las_lstm_cell_args, h_out);
    FIELD(las_lstm_cell_args, gates_out); FIELD(las_lstm_cell_args, M); FIELD(las_lstm_cell_args, H); FIELD(las_lstm_cell_args, fast);
    FIELD(las_lstm_cell_args, h_bf16); FIELD(las_lstm_cell_args, h_out_bf16);
    STRUCT(las_beam_loop_args);
    FIELD(las_beam_loop_args, logits); FIELD(las_beam_loop_args, score); FIELD(las_beam_loop_args, length); FIELD(las_beam_loop_args, nlive);
    FIELD(las_beam_loop_args, nsel); FIELD(las_beam_loop_args, done); FIELD(las_beam_loop_args, dec_step); FIELD(las_beam_loop_args, step);
    FIELD(las_beam_loop_args, hist_parent); FIELD(las_beam_loop_args, hist_token); FIELD(las_beam_loop_args, hist_slot);
    FIELD(las_beam_loop_args, hist_score); FIELD(las_beam_loop_args, hist_n); FIELD(las_beam_loop_args, sel_t); FIELD(las_beam_loop_args, sel_j);
    FIELD(las_beam_loop_args, src_row); FIELD(las_beam_loop_args, next_token); FIELD(las_beam_loop_args, nutt); FIELD(las_beam_loop_args, beam);
    FIELD(las_beam_loop_args, V); FIELD(las_beam_loop_args, Umax); FIELD(las_beam_loop_args, selcap); FIELD(las_beam_loop_args, topn);
    FIELD(las_beam_loop_args, start_id); FIELD(las_beam_loop_args, end_id); FIELD(las_beam_loop_args, ntens); FIELD(las_beam_loop_args, state_in);
    FIELD(las_beam_loop_args, state_out); FIELD(las_beam_loop_args, state_width); FIELD(las_beam_loop_args, file_in);
    FIELD(las_beam_loop_args, file_out); FIELD(las_beam_loop_args, file_width); FIELD(las_beam_loop_args, proj_h0);
    FIELD(las_beam_loop_args, proj_k0); FIELD(las_beam_loop_args, proj_h1); FIELD(las_beam_loop_args, proj_k1); FIELD(las_beam_loop_args, proj_w);
    FIELD(las_beam_loop_args, proj_b);
    STRUCT(las_input_config);
    FIELD(las_input_config, feat_dim); FIELD(las_input_config, is_training); FIELD(las_input_config, n_bounds); FIELD(las_input_config, bounds);
    FIELD(las_input_config, batch_limit); FIELD(las_input_config, max_tokenlen); FIELD(las_input_config, shuffle_buffer);
    FIELD(las_input_config, cycle_length); FIELD(las_input_config, seed); FIELD(las_input_config, rank); FIELD(las_input_config, world);
    FIELD(las_input_config, slots);
    STRUCT(las_input_batch);
    FIELD(las_input_batch, slot); FIELD(las_input_batch, B); FIELD(las_input_batch, T); FIELD(las_input_batch, bucket);
    FIELD(las_input_batch, global_B); FIELD(las_input_batch, max_tokenlen); FIELD(las_input_batch, feat); FIELD(las_input_batch, token);
    FIELD(las_input_batch, featlen); FIELD(las_input_batch, tokenlen);
    STRUCT(las_frontend_args);
    FIELD(las_frontend_args, samples); FIELD(las_frontend_args, samples_i16); FIELD(las_frontend_args, ld_samples);
    FIELD(las_frontend_args, n_samples); FIELD(las_frontend_args, n_samples_host); FIELD(las_frontend_args, n); FIELD(las_frontend_args, Tmax);
    FIELD(las_frontend_args, fl); FIELD(las_frontend_args, step); FIELD(las_frontend_args, feat_type); FIELD(las_frontend_args, feat_dim);
    FIELD(las_frontend_args, num_filters); FIELD(las_frontend_args, cmvn); FIELD(las_frontend_args, twiddle); FIELD(las_frontend_args, fb);
    FIELD(las_frontend_args, fb_range); FIELD(las_frontend_args, dct); FIELD(las_frontend_args, out); FIELD(las_frontend_args, ws);
    FIELD(las_frontend_args, ws_bytes);
    STRUCT(las_resample_args);
    FIELD(las_resample_args, in); FIELD(las_resample_args, in_i16); FIELD(las_resample_args, ld_in); FIELD(las_resample_args, n_in);
    FIELD(las_resample_args, n_in_host); FIELD(las_resample_args, n); FIELD(las_resample_args, L); FIELD(las_resample_args, M);
    FIELD(las_resample_args, W); FIELD(las_resample_args, table); FIELD(las_resample_args, gain); FIELD(las_resample_args, out);
    FIELD(las_resample_args, ld_out); FIELD(las_resample_args, n_out);
    STRUCT(las_specaug_args);
    FIELD(las_specaug_args, in); FIELD(las_specaug_args, out); FIELD(las_specaug_args, plan); FIELD(las_specaug_args, plan_host);
    FIELD(las_specaug_args, ldp); FIELD(las_specaug_args, B); FIELD(las_specaug_args, Tmax); FIELD(las_specaug_args, F); FIELD(las_specaug_args, C);
    FIELD(las_specaug_args, mF); FIELD(las_specaug_args, mT);
    return 0;
}
