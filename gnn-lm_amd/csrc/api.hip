// C ABI of libgnnlm_hip.so (include/gnnlm.h): the one-line wrappers of the kernel launchers whose files have no extern "C" block of
// their own.  Process state lives in runtime.hip, the store in store.hip, the orchestrators in hgt_forward.hip, adaptive_logp.hip
// and the files named after what they run.
#include "host.h"

using namespace gnnlm;

extern "C" {

int gnnlm_gemm_nt(const gnnlm_gemm_t* d, void* stream) { GNNLM_DESC(d); return gemm_nt(*d, (hipStream_t)stream); }
int gnnlm_group_assign(const gnnlm_group_assign_t* d, void* stream) { GNNLM_DESC(d); return group_assign(*d, (hipStream_t)stream); }
int gnnlm_gather_rows_peer(const gnnlm_peer_gather_t* d, void* stream) { GNNLM_DESC(d); return gather_rows_peer(*d, (hipStream_t)stream); }
int gnnlm_enable_peer_access(int32_t peer_device) {
    const hipError_t e = hipDeviceEnablePeerAccess(peer_device, 0);
    if (e == hipErrorPeerAccessAlreadyEnabled) { (void)hipGetLastError(); return OK; }
    GNNLM_HIP(e);
    return OK;
}
int gnnlm_lse_reduce(const float* part, int32_t n_parts, int64_t rows, const int32_t* m_dev, float* lse, void* stream) {
    return lse_reduce(part, n_parts, rows, m_dev, lse, (hipStream_t)stream);
}
int gnnlm_pq_encode(const float* x, int64_t ldx, const float* centroids, const float* norm2, int32_t M, int32_t dsub,
                    int64_t n, uint8_t* codes, void* stream) {
    return pq_encode(x, ldx, centroids, norm2, M, dsub, n, codes, (hipStream_t)stream);
}
int gnnlm_bucket_rows(const int64_t* rows, int64_t n, int64_t n_store, int64_t rows_per_rank, int32_t world,
                      int32_t self_rank, int64_t* counts, int64_t* cursor, int64_t* send_rows, int32_t* inv, void* stream) {
    return bucket_rows(rows, n, n_store, rows_per_rank, world, self_rank, counts, cursor, send_rows, inv, (hipStream_t)stream);
}
int gnnlm_bucket_rows_padded(const int64_t* rows, int64_t n, int64_t n_store, int64_t rows_per_rank, int32_t world,
                             int64_t cap, int64_t* cursor, int64_t* send_rows, int32_t* inv, int64_t* overflow, void* stream) {
    return bucket_rows_padded(rows, n, n_store, rows_per_rank, world, cap, cursor, send_rows, inv, overflow, (hipStream_t)stream);
}
int gnnlm_pq_gather_decode(const gnnlm_gather_t* d, void* stream) { GNNLM_DESC(d); return gather_decode(*d, (hipStream_t)stream); }
int gnnlm_token_gather(const gnnlm_token_gather_t* d, void* stream) { GNNLM_DESC(d); return token_gather(*d, (hipStream_t)stream); }
int gnnlm_neighbor_labels(const int64_t* ids, int64_t n, int64_t n_store, const void* vals, int32_t vals_itemsize, int32_t n_vocab, int32_t* out,
                          void* stream) {
    return neighbor_labels(ids, n, n_store, vals, vals_itemsize, n_vocab, out, (hipStream_t)stream);
}
int gnnlm_star_attn(const gnnlm_star_attn_t* d, void* stream) { GNNLM_DESC(d); return star_attn(*d, (hipStream_t)stream); }
int gnnlm_chain_attn(const gnnlm_chain_attn_t* d, void* stream) { GNNLM_DESC(d); return chain_attn(*d, (hipStream_t)stream); }
int gnnlm_causal_softmax(float* S, int64_t n_mats, int32_t T, int64_t ld, int32_t max_ctx, void* stream) {
    return causal_softmax(S, n_mats, T, ld, max_ctx, (hipStream_t)stream);
}
int gnnlm_causal_attn(const float* Q, const float* K, const float* V, int64_t ld, float* out, int64_t ldo,
                      int32_t n_blocks, int32_t T, int32_t H, int32_t dk, int32_t max_ctx, void* stream) {
    return causal_attn_fused(Q, K, V, ld, out, ldo, n_blocks, T, H, dk, max_ctx, (hipStream_t)stream);
}
int64_t gnnlm_ragged_tiles(const int32_t* block_off, int32_t n_blocks, int32_t* tiles) { return ragged_tiles(block_off, n_blocks, tiles); }
int gnnlm_causal_attn_varlen(const float* Q, const float* K, const float* V, int64_t ld, float* out, int64_t ldo,
                             const gnnlm_ragged_t* blocks, int32_t H, int32_t dk, int32_t max_ctx, void* stream) {
    GNNLM_DESC(blocks);
    return causal_attn_varlen(Q, K, V, ld, out, ldo, *blocks, H, dk, max_ctx, (hipStream_t)stream);
}
int gnnlm_layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, float* out, int64_t ldo,
                    int64_t rows, int32_t d, float eps, const uint8_t* valid, void* stream) {
    return layernorm(x, ldx, gamma, beta, out, ldo, rows, d, eps, valid, (hipStream_t)stream);
}
int gnnlm_gelu(float* x, int64_t n, void* stream) { return gelu(x, n, (hipStream_t)stream); }
int gnnlm_filter_neighbors(const int64_t* ids, const int64_t* tok_pos, int64_t n_tok, int32_t kg, int64_t invalid_ctx, int64_t* out,
                           void* stream) {
    return filter_neighbors(ids, tok_pos, n_tok, kg, invalid_ctx, out, (hipStream_t)stream);
}
int gnnlm_half_to_float(const void* src, float* dst, int64_t n, void* stream) {
    return half_to_float(src, dst, n, (hipStream_t)stream);
}
int gnnlm_row_lse_pick(const float* logits, int64_t ld, int64_t rows, const int32_t* m_dev, int32_t n,
                       const int32_t* pick, float* lse, float* picked, void* stream) {
    return row_lse_pick(logits, ld, rows, m_dev, n, pick, lse, picked, (hipStream_t)stream);
}
int gnnlm_knn_interp(const gnnlm_knn_interp_t* d, void* stream) { GNNLM_DESC(d); return knn_interp(*d, (hipStream_t)stream); }
int gnnlm_knn_interp_grid(const gnnlm_knn_interp_grid_t* d, void* stream) { GNNLM_DESC(d); return knn_interp_grid(*d, 1, 0, (hipStream_t)stream); }
int gnnlm_knn_interp_grid_lm(const gnnlm_knn_interp_grid_t* d, int32_t n_lm, int64_t ld_lm, void* stream) {
    GNNLM_DESC(d);
    return knn_interp_grid(*d, n_lm, ld_lm, (hipStream_t)stream);
}
int gnnlm_logp_mix(const float* gnn_logp, const float* base_logp, int64_t n, const double* alphas, int32_t n_alphas, float* out, void* stream) {
    return logp_mix(gnn_logp, base_logp, n, alphas, n_alphas, out, (hipStream_t)stream);
}
int gnnlm_knn_recompute_sims(const gnnlm_knn_resim_t* d, void* stream) { GNNLM_DESC(d); return knn_recompute_sims(*d, (hipStream_t)stream); }
size_t gnnlm_knn_interp_scratch_bytes(int64_t n, int32_t k, int64_t n_local) { return knn_interp_scratch_bytes(n, k, n_local); }
int gnnlm_label_tags(const void* vals, int32_t vals_itemsize, int64_t n, uint8_t* tag, void* stream) { return label_tags(vals, vals_itemsize, n, tag, (hipStream_t)stream); }
int gnnlm_topk_merge(const gnnlm_topk_t* d, void* stream) { GNNLM_DESC(d); return topk_merge(*d, (hipStream_t)stream); }
int gnnlm_ivfpq_scan(const gnnlm_ivfpq_scan_t* d, void* stream) { GNNLM_DESC(d); return ivfpq_scan(*d, (hipStream_t)stream); }
int gnnlm_ivfpq_pack_codes(const uint8_t* codes, int64_t N, int32_t M, uint8_t* out, void* stream) {
    return ivfpq_pack_codes(codes, N, M, out, (hipStream_t)stream);
}
int gnnlm_ivfpq_pack_lut(const float* lut, int64_t ld_lut, int64_t n, int32_t M, float* out, void* stream) {
    return ivfpq_pack_lut(lut, ld_lut, n, M, out, (hipStream_t)stream);
}
int gnnlm_ivfpq_key_terms(const uint8_t* list_codes, const int64_t* list_off, int64_t N, int32_t nlist, const float* coarse, const float* pq,
                          int32_t M, int32_t dsub, float* key_term, void* stream) {
    return ivfpq_key_terms(list_codes, list_off, N, nlist, coarse, pq, M, dsub, key_term, (hipStream_t)stream);
}
int gnnlm_ivfpq_pack_tiles(const uint8_t* codes, int64_t N, int32_t M, uint8_t* out, void* stream) {
    return ivfpq_pack_tiles(codes, N, M, out, (hipStream_t)stream);
}
int gnnlm_ivfpq_build_groups(const int64_t* probe_list, int64_t ld_probe, int64_t n, int32_t P, int32_t nlist, int64_t seg, int32_t* grp_list,
                             int32_t* grp_q, int64_t* grp_out, int32_t* n_groups, int32_t* scratch, void* stream) {
    return ivfpq_build_groups(probe_list, ld_probe, n, P, nlist, seg, grp_list, grp_q, grp_out, n_groups, scratch, (hipStream_t)stream);
}
int gnnlm_ivfpq_quantize_lut(const float* lut, int64_t ld_lut, int64_t n, int32_t M, uint8_t* qlut, float* qmeta, void* stream) {
    return ivfpq_quantize_lut(lut, ld_lut, n, M, qlut, qmeta, (hipStream_t)stream);
}
int gnnlm_ivfpq_scan8(const gnnlm_ivfpq_scan8_t* d, void* stream) { GNNLM_DESC(d); return ivfpq_scan8(*d, (hipStream_t)stream); }
int gnnlm_ivfpq_rescore(const gnnlm_ivfpq_rescore_t* d, void* stream) { GNNLM_DESC(d); return ivfpq_rescore(*d, (hipStream_t)stream); }
int gnnlm_ivfpq_tables(const gnnlm_ivfpq_tables_t* d, void* stream) { GNNLM_DESC(d); return ivfpq_tables(*d, (hipStream_t)stream); }
int gnnlm_ivfpq_tau(const gnnlm_ivfpq_tau_t* d, void* stream) { GNNLM_DESC(d); return ivfpq_tau(*d, (hipStream_t)stream); }
int gnnlm_ivfpq_split_payload(int64_t* idx, int64_t n, int32_t label_bits, int32_t val_last, int32_t* out_vals, void* stream) { return ivfpq_split_payload(idx, n, label_bits, val_last, out_vals, (hipStream_t)stream); }
int gnnlm_ivfpq_select_probes(const gnnlm_ivfpq_select_probes_t* d, void* stream) { GNNLM_DESC(d); return ivfpq_select_probes(*d, (hipStream_t)stream); }
int gnnlm_ivfpq_select_final(const gnnlm_ivfpq_select_final_t* d, void* stream) { GNNLM_DESC(d); return ivfpq_select_final(*d, (hipStream_t)stream); }
int gnnlm_masked_sum_f64(const float* x, const uint8_t* mask, int64_t n, double* out, void* stream) {
    return masked_sum_f64(x, mask, n, out, (hipStream_t)stream);
}
int gnnlm_rows_sum_f64(const float* x, int64_t ld, int64_t rows, int64_t n, double* out, void* stream) {
    return rows_sum_f64(x, ld, rows, n, out, (hipStream_t)stream);
}

}  // extern "C"
