// Internal launcher declarations (C++).  The public C ABI is include/gnnlm.h.
#pragma once
#include "common.h"
#include "../../include/gnnlm.h"

namespace gnnlm {

// Descriptor structs are the public C structs of include/gnnlm.h.
typedef gnnlm_gemm_t GemmParams;
typedef gnnlm_gather_t GatherParams;
typedef gnnlm_star_attn_t StarAttnParams;
typedef gnnlm_chain_attn_t ChainAttnParams;
typedef gnnlm_knn_interp_t KnnInterpParams;
int topk_merge(const gnnlm_topk_t& d, hipStream_t stream);
int ivfpq_scan(const gnnlm_ivfpq_scan_t& d, hipStream_t stream);
int ivfpq_pack_codes(const uint8_t* codes, int64_t N, int M, uint8_t* out, hipStream_t stream);
int ivfpq_pack_lut(const float* lut, int64_t ld_lut, int64_t n, int M, float* out, hipStream_t stream);
int ivfpq_key_terms(const uint8_t* codes, const int64_t* list_off, int64_t N, int nlist, const float* coarse, const float* pq, int M, int dsub,
                    float* out, hipStream_t stream);

int ivfpq_pack_tiles(const uint8_t* codes, int64_t N, int M, uint8_t* out, hipStream_t stream);
int ivfpq_build_groups(const int64_t* pl, int64_t ld, int64_t n, int P, int nlist, int64_t seg, int32_t* grp_list, int32_t* grp_q,
                       int64_t* grp_out, int32_t* n_groups, int32_t* scratch, hipStream_t stream);
int ivfpq_quantize_lut(const float* lut, int64_t ld_lut, int64_t n, int M, uint8_t* qlut, float* qmeta, hipStream_t stream);
int ivfpq_scan8(const gnnlm_ivfpq_scan8_t& d, hipStream_t stream);
int ivfpq_rescore(const gnnlm_ivfpq_rescore_t& d, hipStream_t stream);
int ivfpq_tables(const gnnlm_ivfpq_tables_t& d, hipStream_t stream);
int ivfpq_split_payload(int64_t* idx, int64_t n, int label_bits, int32_t val_last, int32_t* out_vals, hipStream_t stream);
int ivfpq_tau(const gnnlm_ivfpq_tau_t& d, hipStream_t stream);
// the search's probe selection and final k-selection in kernels of their own (ivfpq_select.hip)
int ivfpq_select_probes(const gnnlm_ivfpq_select_probes_t& d, hipStream_t stream);
int ivfpq_select_final(const gnnlm_ivfpq_select_final_t& d, hipStream_t stream);
// adding keys: the residual encode of assigned rows and the merge behind the old rows of their lists (ivfpq_add.hip)
int ivfpq_encode_rows(const gnnlm_ivfpq_encode_t& d, hipStream_t stream);
int ivfpq_list_merge(const gnnlm_ivfpq_list_merge_t& d, hipStream_t stream);
// the coarse step without the score matrix: MFMA scores, a running k-best per row on chip, slabs folded by topk_merge (ivfpq_coarse.hip)
int ivfpq_coarse_probes(const gnnlm_ivfpq_coarse_t& d, hipStream_t stream);
// removing keys: the rows that survive a set of id ranges, and their compaction list by list (ivfpq_remove.hip)
int ivfpq_keep_flags(const gnnlm_ivfpq_keep_flags_t& d, hipStream_t stream);
size_t ivfpq_list_compact_workspace_bytes(int64_t N0, int nlist);
int ivfpq_list_compact(const gnnlm_ivfpq_list_compact_t& d, hipStream_t stream);

// gemm.hip: refusals, the route (gemm_route.h), one launch
int gemm_nt(const GemmParams& p, hipStream_t stream);
// the launchers of the kernel files, called by gemm_nt with a normalised descriptor, the route gemm_route() chose and its grid
enum class GemmRoute : int;
void gemm_launch_reg(GemmRoute route, const GemmParams& p, dim3 grid, hipStream_t stream);       // gemm_f32.hip: reg64, reg128
int gemm_launch_sched(const GemmParams& p, dim3 grid, hipStream_t stream);                       // gemm_f32_sched.hip: sched128
int gemm_launch_dma(GemmRoute route, const GemmParams& p, dim3 grid, hipStream_t stream);        // gemm_f32_dma.hip: dma128, dma256, astat128
void gemm_launch_skinny(const GemmParams& p, dim3 grid, hipStream_t stream);                     // gemm_f32_skinny.hip: skinny32
// gemm_split.hip (split128, split256): the plane images of both operands in the stream's scratch, then the GEMM over them
struct GemmPlanes { const void* A = nullptr; const void* W = nullptr; int KS = 0; };
int gemm_split_planes(GemmRoute route, const GemmParams& p, hipStream_t stream, GemmPlanes* out);
void gemm_launch_split(GemmRoute route, const GemmParams& p, const GemmPlanes& planes, dim3 grid, hipStream_t stream);
// precision used by gemm_nt for descriptors that leave `precision` at 0 (set by the orchestrators)
extern thread_local int g_default_gemm_precision;
struct GemmPrecisionScope {
    int saved;
    explicit GemmPrecisionScope(int prec) : saved(g_default_gemm_precision) { g_default_gemm_precision = prec; }
    ~GemmPrecisionScope() { g_default_gemm_precision = saved; }
};
int lse_reduce(const float* part, int n_parts, int64_t rows, const int32_t* m_dev, float* lse, hipStream_t stream);
int gather_decode(const GatherParams& p, hipStream_t stream);
int pq_encode(const float* x, int64_t ldx, const float* cen, const float* norm2, int M, int dsub, int64_t n, uint8_t* codes,
              hipStream_t stream);
// token-embedding rows of the slots' labels / labels of a neighbour-id matrix (token_gather.hip, `--reinit-nfeat`)
int token_gather(const gnnlm_token_gather_t& p, hipStream_t stream);
int neighbor_labels(const int64_t* ids, int64_t n, int64_t n_store, const void* vals, int itemsize, int n_vocab, int32_t* out,
                    hipStream_t stream);
int bucket_rows(const int64_t* rows, int64_t n, int64_t n_store, int64_t per, int world, int self, int64_t* counts,
                int64_t* cursor, int64_t* send_rows, int32_t* inv, hipStream_t stream);
int gather_rows_peer(const gnnlm_peer_gather_t& d, hipStream_t stream);
int bucket_rows_padded(const int64_t* rows, int64_t n, int64_t n_store, int64_t per, int world, int64_t cap, int64_t* cursor,
                       int64_t* send_rows, int32_t* inv, int64_t* overflow, hipStream_t stream);
// star_attn.hip: refusals, the route (star_route.h), one launch -- the generic kernel or one of the two launchers below
int star_attn(const StarAttnParams& p, hipStream_t stream);
struct StarPlan;
// table-resident formulation for the PQ source, k_g <= 128 (star_tab.hip), called by star_attn with the plan star_route() made
int star_attn_tab(const StarAttnParams& p, const StarPlan& plan, hipStream_t stream);

// Neighbour (i, j) takes part in the star softmax iff its id is a row of the store, the row is present on this
// shard (PQ source read from the store) and the caller's validity byte (exchange / gather_decode) says so: the
// rule of gather_decode_kernel, so layer-0 star attention and the ntgt states can never disagree.
// row `row` (>= 0) of a set of mapped shards: pointer to its M bytes, or nullptr if no shard holds it
__device__ __forceinline__ const uint8_t* shard_row_ptr(const gnnlm_shards_t* sh, int64_t row, int M) {
    const int64_t per = sh->rows_per_rank;
    // (a 64-bit division costs ~10x a 32-bit one; the stores of this path have fewer than 2^32 rows)
    const int64_t q = ((uint64_t)(row | per) >> 32) == 0 ? (int64_t)((uint32_t)row / (uint32_t)per) : row / per;
    const int g = (int)min((int64_t)sh->n - 1, q);
    const int64_t local = row - sh->row0[g];
    return local >= 0 && local < sh->rows[g] ? sh->base[g] + local * M : nullptr;
}
// group of neighbour (i, j): its own (i * kg + j), or the distinct-centre group of a de-duplicated batch (-1: none)
__device__ __forceinline__ int64_t star_group(const StarAttnParams& p, int i, int j) {
    const int64_t e = (int64_t)i * p.kg + j;
    return p.x_index ? (int64_t)p.x_index[e] : e;
}
__device__ __forceinline__ bool star_nb_ok(const StarAttnParams& p, int i, int j, int64_t id) {
    bool ok = id >= 0 && (p.n_store <= 0 || id < p.n_store);
    if (p.shards) ok = ok && shard_row_ptr(p.shards, id, p.M) != nullptr;
    else if (p.codes && !p.codes_direct) ok = ok && id - p.row0 >= 0 && id - p.row0 < p.n_local;
    if (ok && (p.nb_valid || p.x_index)) {
        const int64_t gi = star_group(p, i, j);
        ok = gi >= 0 && (!p.nb_valid || p.nb_valid[gi * p.nb_valid_stride] != 0);
    }
    return ok;
}
// row of the code table that holds neighbour (i, j) (store rows, or the slots of an exchange)
__device__ __forceinline__ int64_t star_code_row(const StarAttnParams& p, int i, int j, int64_t id) {
    if (!p.codes_direct) return id - p.row0;
    const int64_t s = ((int64_t)i * p.kg + j) * p.codes_direct;
    return p.codes_index ? (int64_t)p.codes_index[s] : s;
}
// pointer to the M code bytes of a VALID neighbour (i, j) (star_nb_ok): one table, the slots of an exchange, or mapped shards
__device__ __forceinline__ const uint8_t* star_code_ptr(const StarAttnParams& p, int i, int j, int64_t id) {
    if (p.shards) return shard_row_ptr(p.shards, id, p.M);
    return p.codes + star_code_row(p, i, j, id) * p.M;
}
// dense neighbour rows (layers >= 1), D in {256, 512, 1024}, H <= 8: one pass over the rows with a running softmax (star_dense.hip)
int star_attn_dense(const StarAttnParams& p, const StarPlan& plan, hipStream_t stream);
// chain_attn.hip
int chain_attn(const ChainAttnParams& p, hipStream_t stream);

// rows of S[b, h, w, :T] -> causal softmax (u <= w, and w-u < max_ctx if max_ctx > 0), in place (causal_attn.hip)
int causal_softmax(float* S, int64_t n_mats, int T, int64_t ld, int max_ctx, hipStream_t stream);
// fused scores + masked softmax + P.V for T = 256, d_k = 128 (causal_attn.hip); Q, K', V are [n_blocks * T, ld] with head h at
// column h * dk
bool causal_attn_fused_ok(int T, int dk);
int causal_attn_fused(const float* Q, const float* K, const float* V, int64_t ld, float* out, int64_t ldo,
                      int n_blocks, int T, int H, int dk, int max_ctx, hipStream_t stream, bool accumulate = false);

// the same attention over packed blocks of unequal length (causal_varlen.hip): one launch for any lengths, d_k in {16, 32, 64, 128}
bool causal_attn_varlen_ok(int dk);
int causal_attn_varlen(const float* Q, const float* K, const float* V, int64_t ld, float* out, int64_t ldo, const gnnlm_ragged_t& rg,
                       int H, int dk, int max_ctx, hipStream_t stream, bool accumulate = false);
// one new row per sequence against a K/V cache (decode_attn.hip): chunks of GNNLM_DECODE_CHUNK keys per wave, combined in order
bool decode_attn_ok(int dk);
int check_kv_cache(const gnnlm_kv_cache_t& c);
size_t decode_attn_workspace_bytes(int B, int H, int dk, int max_len);
// a table of cache slots (gnnlm_beam_attn): key row u < len of sequence b is row u of sequence src[b * ld + u]
struct SlotTable { const int32_t* src; int64_t ld; };
// tab == nullptr: every sequence reads its own rows (gnnlm_decode_attn); else through the table
int decode_attn(const gnnlm_decode_attn_t& d, const SlotTable* tab, hipStream_t stream);
// one beam-search step of every sentence (beam.hip)
int beam_select(const gnnlm_beam_select_t& d, hipStream_t stream);
int beam_select_diverse(const gnnlm_beam_select_diverse_t& d, hipStream_t stream);
// the K' and V' rows [n_tok, ld_src] of the packed tokens -> cache rows [0, min(len_b, max_rows)) of sequence b = block b of `layer`
int kv_cache_fill(const float* k, const float* v, int64_t ld_src, const gnnlm_kv_cache_t& c, int layer, const gnnlm_ragged_t& rg,
                  int max_rows, hipStream_t stream);
// len[b] = min(block_off[b + 1] - block_off[b], max_rows);  len[b] += 1 for rows that are not done and hold 0 <= len[b] < bound
int kv_len_set(const gnnlm_kv_cache_t& c, const int32_t* block_off, int max_rows, hipStream_t stream);
int kv_len_advance(const gnnlm_kv_cache_t& c, int bound, hipStream_t stream);
// the next token of every row from its sorted top-N (sample.hip)
int sample_topk(const gnnlm_sample_topk_t& d, hipStream_t stream);
int sample_topp(const gnnlm_sample_topp_t& d, hipStream_t stream);
// host: the (block, query tile) table of block_off [n_blocks + 1], heaviest tiles first; tiles == nullptr only counts.  -1: an empty block
int64_t ragged_tiles(const int32_t* block_off, int n_blocks, int32_t* tiles);

// out[r,:] = LayerNorm(x[r,:]) * gamma + beta ; optional row validity (invalid rows -> 0)
int layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, float* out, int64_t ldo,
              int64_t rows, int d, float eps, const uint8_t* valid, hipStream_t stream,
              const float* residual = nullptr, int64_t ldr = 0,      // out = LN(x + residual)
              const int32_t* rows_idx = nullptr,                     // only the rows rows_idx[0..rows) (of x, residual, out, valid)
              const int32_t* n_dev = nullptr, int n_mult = 1);       // device-side count: rows = min(rows, *n_dev * n_mult)
// idx[g * n_sel + j] = g * n_g + sel[j]
int group_rows(int32_t* idx, int64_t n_groups, int n_g, const int* sel, int n_sel, hipStream_t stream);
// dst[slots[g]][0..d) = src[g * ld_src][0..d) for g < n (rows of d floats, d % 4 == 0)
int scatter_rows(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, const int32_t* slots, int64_t n, int d, hipStream_t stream,
                 const int32_t* n_dev = nullptr);                    // device-side count: n = min(n, *n_dev)

// group assignment on the device (groups.hip, ABI 9)
int group_assign(const gnnlm_group_assign_t& d, hipStream_t stream);
// (ABI 11: row-keyed K / V of layer 0) slot -> datastore row of the first *n_dev groups, for the slots within `reach` of their centre
int slot_rows(const int64_t* centres, int64_t G, const int32_t* n_dev, int left, int right, int reach, int64_t n_store, int64_t* out, hipStream_t stream);
// counts[w * 8 + mult - 1] = rows of window w (groups [w * per, (w + 1) * per) of min(*n_dev, cap)) times mult, mult = 1 .. 8
int window_counts(const int32_t* n_dev, int64_t cap, int64_t per, int n_win, int32_t* counts, hipStream_t stream);
// out[e] = row of the fetched buffer that holds the centre code of neighbour e's group (-1: none)
int nb_code_rows(const int32_t* group_index, const int32_t* fetched_index, int n_g, int64_t n, int32_t* out, hipStream_t stream);
// dst[slots[g]] = src[index ? index[g * stride] : g * stride] (zero row if valid && !valid[g * stride]) for g < min(*n_dev, cap)
int scatter_code_rows(const uint8_t* src, const int32_t* index, int64_t stride, const uint8_t* valid, uint8_t* dst, const int32_t* slots,
                      const int32_t* n_dev, int64_t cap, int bytes, hipStream_t stream);

// out = 0.5 * (a + b)
int mean2(const float* a, const float* b, float* out, int64_t n, hipStream_t stream);

int gelu(float* x, int64_t n, hipStream_t stream);
// x = max(x, 0) in place, NaN kept (transformer_lm.hip)
int relu(float* x, int64_t n, hipStream_t stream);

// the --invalid-neighbor-context rule of token_block_dataset.py:360-362 applied to a batch of neighbour-id rows
int filter_neighbors(const int64_t* ids, const int64_t* pos, int64_t n, int kg, int64_t ctx, int64_t* out, hipStream_t stream);

// fp16 -> fp32 row convert
int half_to_float(const void* src, float* dst, int64_t n, hipStream_t stream);

// ---------------------------------------------------------------------------------------------
// adaptive softmax / kNN interpolation
// ---------------------------------------------------------------------------------------------
// lse[r] = logsumexp(logits[r, :n]); picked[r] = logits[r, pick[r]] (pick may be null; include/gnnlm.h: gnnlm_row_lse_pick)
int row_lse_pick(const float* logits, int64_t ld, int64_t rows, const int32_t* m_dev, int n,
                 const int32_t* pick, float* lse, float* picked, hipStream_t stream);

struct BandSplitParams {
    const int64_t* target = nullptr; int64_t n = 0;
    int n_bands = 0; int32_t cutoff[8] = {0};      // cutoff[0..n_bands-1], band b = [cutoff[b-1], cutoff[b])
    int32_t* head_pick = nullptr;          // [n] index into the head logits (target or cutoff0+band-1); -1 for a target outside
                                           // [0, cutoff[n_bands-1]), which joins no band either
    int32_t* band_rows = nullptr;          // [n_bands-1, n] compacted row lists of the tail bands
    int32_t* band_pick = nullptr;          // [n_bands-1, n] target - cutoff[band-1] for the compacted rows
    int32_t* band_count = nullptr;         // [n_bands-1]
};
int band_split(const BandSplitParams& p, hipStream_t stream);

// out[r] = picked[r] - lse[r], -inf where pick[r] < 0 (a target outside the vocabulary: BandSplitParams.head_pick)
int head_logp(const float* picked, const float* lse, const int32_t* pick, float* out, int64_t n, hipStream_t stream);
// lm_logp[rows[r]] += tail_picked[r] - tail_lse[r] for r < min(n_max, *count_dev)   (rows null: identity)
int tail_combine(const float* tail_picked, const float* tail_lse, const int32_t* rows,
                 const int32_t* count_dev, int64_t n_max, float* lm_logp, hipStream_t stream);

int knn_interp(const KnnInterpParams& p, hipStream_t stream);
int label_tags(const void* vals, int itemsize, int64_t n, uint8_t* tag, hipStream_t stream);
size_t knn_interp_scratch_bytes(int64_t n, int k, int64_t n_local);
bool knn_interp_bucketed_eligible(const KnnInterpParams& p);
int knn_interp_bucketed(const KnnInterpParams& p, float log_1ml, float log_l, hipStream_t stream);
// every point of ks x temperatures x lmbdas from one read of the search result (knn_grid.hip)
// lm_logp read as [n_lm, n] (row stride ld_lm), out_logp as [n_lm * G, n]; n_lm = 1 is the plain grid
int knn_interp_grid(const gnnlm_knn_interp_grid_t& d, int n_lm, int64_t ld_lm, hipStream_t stream);
// out[a, :] = logsumexp(log(alphas[a]) + base, log(1 - alphas[a]) + gnn) for up to 8 ratios from one read (logp_mix.hip)
int logp_mix(const float* gnn_logp, const float* base_logp, int64_t n, const double* alphas, int n_alphas, float* out, hipStream_t stream);
// similarities recomputed from the stored keys, one wave per (query, run of 64 neighbours) (knn_resim.hip)
int knn_recompute_sims(const gnnlm_knn_resim_t& d, hipStream_t stream);

// sum of x[start[b] : ] per ... simple masked sum in double: out[0] += sum(x[i] * (mask?mask[i]:1))
int masked_sum_f64(const float* x, const uint8_t* mask, int64_t n, double* out, hipStream_t stream);
// out[g] += sum(x[g * ld : g * ld + n]) for g < rows, each row in masked_sum_f64's summation order (knn_grid.hip)
int rows_sum_f64(const float* x, int64_t ld, int64_t rows, int64_t n, double* out, hipStream_t stream);

}  // namespace gnnlm
