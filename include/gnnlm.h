/* gnnlm.h -- C ABI of libgnnlm_hip.so: the MI355X (gfx950) implementation of the GNN+kNN eval hot
 * path of ShannonAI/GNN-LM (`fairseq-eval-lm --graph --use-precompute-feat --knnlm`).
 *
 * The reference has NO native / FFI boundary on this path (everything is Python over torch, DGL and
 * faiss: SURVEY.md section 8b), so each entry point below names the reference Python function it
 * replaces (paths relative to the reference tree).  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative errno-style code (GNNLM_E_*);
 *     gnnlm_last_error() returns a thread-local message for the last failure
 *   - all `const float*` / `void*` operands are DEVICE pointers unless the name says `host`
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls only enqueue work
 *   - the caller owns every buffer; descriptors are plain structs, zero-initialise them and fill
 *     what you need (0 / NULL always means "not used / default")
 *   - matrices are row-major; "ld" is the row stride in ELEMENTS
 *   - no call allocates or synchronises except gnnlm_store_* (explicitly documented)
 */
#ifndef GNNLM_H
#define GNNLM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GNNLM_ABI_VERSION 12
#define GNNLM_OK 0
#define GNNLM_E_INVALID (-22)
#define GNNLM_E_NOMEM (-12)
#define GNNLM_E_HIP (-5)

const char* gnnlm_last_error(void);
int gnnlm_abi_version(void);
/* name of the code object's target ("gfx950") -- lets a loader check it got the MI355X build */
const char* gnnlm_target_arch(void);
/* sizeof() of a descriptor struct by its typedef name ("gnnlm_gemm_t", ...), 0 if unknown: lets a
 * foreign-language binding verify its struct mirror */
size_t gnnlm_sizeof(const char* struct_name);

/* ------------------------------------------------------------------------------------------------
 * Dense contraction:  C[M,N] = alpha * A[M,K] . W[N,K]^T (+ gate[row] * bias) (+ R)
 * f32 operands, f32 MFMA accumulate (v_mfma_f32_32x32x2_f32: exact fmaf chain).
 * Replaces: nn.Linear of HGTLayer (fairseq/models/hgt.py:315-322,401), the relation einsum (:347-348),
 *           fn.v_dot_u / u_mul_e+sum on the dense tgt-tgt edges (:354,383-385),
 *           `x @ A` of TorchPQCodec.decode (knn/pq_wrapper.py:202),
 *           the head/tail matmuls of AdaptiveSoftmax (fairseq/modules/adaptive_softmax.py:184-203).
 *
 * Store flavour, for every logical row r < m = min(M, *m_dev) (m = M without m_dev; *m_dev >= 0) and every batch (b1, b2):
 *   C[b][c_rows[r], n] = alpha * <A[b][a_rows[r], :], W[b][n, :]> + gate[r] * bias + R[b][c_rows[r], n],   n < N
 *   with X[b] = X + b1 * sX1 + b2 * sX2; bias is bias[b][n] (bias_mode 1) or bias[b][r] (bias_mode 2).  a_rows, c_rows, gate and
 *   m_dev are shared by all batches.  a_rows[r] < 0 makes the product term of the row zero (bias and R still apply).  Nothing else
 *   of C is written: not the pad columns of ldc > N, not the rows from m on, not a row no c_rows entry names.  c_rows entries
 *   below m must be distinct.  R may be C itself with ldr = ldc (in place).
 * Alignment: A and W 16 bytes, lda, ldw, K and the A / W batch strides multiples of 4 elements; C, R, bias, gate and lse_picked need
 *   their natural 4 bytes only and ldc, ldr, the C / R / bias strides may be any number; lse_part needs 8 bytes.
 * tile_order, m_dev's presence and a_rows_bound choose among kernels and the order tiles are visited in.  tile_order never changes a
 *   bit of the result.  Kernels differ in the order they sum k in, so "the same bits" holds per kernel: the same problem with and
 *   without m_dev (or with and without a_rows_bound) may differ in the last bits.  Two identical calls give identical bits.
 * Refused with GNNLM_E_INVALID before anything is launched or written: a NULL A or W, C and lse_part both NULL, M < 0, N or K <= 0,
 *   K, lda, ldw or an A / W batch stride not a multiple of 4, A or W not 16-byte aligned, precision outside 0..3, tile_order outside
 *   0..66, and what the log-sum-exp flavour does not take (below).  M = 0 is accepted and touches nothing (m_out included).
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnlm_gemm {
    const float* A;  int64_t lda;
    const int32_t* a_rows;     /* optional gather: logical row r reads A row a_rows[r] (<0: zero row) */
    const float* W;  int64_t ldw;
    float* C;        int64_t ldc;
    const int32_t* c_rows;     /* optional scatter: logical row r is stored to C (and read from R) row c_rows[r] */
    const float* bias;         /* bias_mode 1: per column [N]; 2: per row [M] */
    int32_t bias_mode;
    const float* gate;         /* optional [M]: per-row multiplier of the bias */
    const float* R;  int64_t ldr;
    float alpha;               /* 0 is read as 1 */
    int32_t M, N, K;           /* K % 4 == 0 */
    const int32_t* m_dev;      /* optional device-side row count >= 0, read as min(M, *m_dev): rows from it on are neither read nor written */
    int32_t* m_out;            /* optional: receives that row count (M without m_dev) (device or host-mapped memory; while the library's
                                  profiler runs it records there instead) */
    int32_t batch1, batch2;    /* 0 is read as 1; batch index (b1, b2) */
    int64_t sA1, sA2, sW1, sW2, sC1, sC2, sB1, sB2, sR1, sR2;   /* batch strides in elements */
    int32_t precision;         /* 0: f32 MFMA (exact fmaf chain; or the enclosing orchestrator's setting);
                                  1: bf16x3 split emulation (~2^-16 per product); 2: bf16x6 (~2^-24, f32-level);
                                  3: fp16 -- both operands rounded to IEEE float16 (round-to-nearest-even; beyond +-65504
                                     -> +-inf, as torch.Tensor.half(), not clamped), exact products, f32 accumulation;
                                     every epilogue and every tensor in memory stays f32 */
    int32_t tile_order;        /* 0: auto (consecutive tiles share the larger operand's panel), 1: n fastest, 2: m fastest, 2 + GM (GM in
                                  1..64): bands of GM m-tiles, n slow inside a band.  Speed only: no bit of the result depends on it */
    /* log-sum-exp epilogue, taken when lse_part is given: instead of storing C (ignored, may be NULL), every row r < m and every
     * part p < 2*ceil(N/128) writes lse_part[r][p] = (alpha * max, sum exp(alpha * x - alpha * max)) over the logits x = (A.W^T)[r, n]
     * of the columns 64 p <= n < min(N, 64 p + 64); a part without a column (the last one when N mod 128 is in 1..64) holds
     * (-inf, 0).  With lse_pick, lse_picked[r] = alpha * x[r, lse_pick[r]] for r < m where 0 <= lse_pick[r] < N; any other entry of
     * lse_picked is left untouched, as are the rows of lse_part from m on.  Finish with gnnlm_lse_reduce.
     * a_rows, a_rows_bound, m_dev, m_out, precision and tile_order act as in the store flavour, except that every a_rows[r], r < m,
     * must be >= 0: a negative entry reads nothing out of bounds, but the row's result is unspecified.  Refused (GNNLM_E_INVALID):
     * batch1 * batch2 != 1, alpha < 0 or NaN (0 is read as 1), and bias, gate, R or c_rows -- the epilogue would drop them. */
    float* lse_part;           /* [M, 2*ceil(N/128), 2] */
    const int32_t* lse_pick;   /* optional [M] */
    float* lse_picked;         /* [M] (with lse_pick) */
    int64_t a_rows_bound;      /* ABI 5, optional with a_rows: every a_rows[r] < a_rows_bound (0: unknown) -- lets the kernels with
                                  32-bit row offsets take a gathered problem */
} gnnlm_gemm_t;
int gnnlm_gemm_nt(const gnnlm_gemm_t* desc, void* stream);
/* lse[row] = log sum exp over the row, from the n_parts (max, sum) pairs of the LSE epilogue: max_p + log sum_p s_p exp(m_p - max_p) for
 * row < min(rows, *m_dev); later rows are untouched.  A (-inf, 0) pair adds nothing; a row of such pairs only gives -inf.  rows = 0 is
 * accepted. */
int gnnlm_lse_reduce(const float* part, int32_t n_parts, int64_t rows, const int32_t* m_dev, float* lse, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PQ datastore row gather + decode (HBM-resident store).
 * Replaces: quant_neighbor_feats[offset] / neighbor_tokens[offset] row gathers and the context
 *           expansion of GraphTokenBlockDataset.new_build_graph
 *           (fairseq/data/token_block_dataset.py:354-394,407-410; PlasmaArray.__getitem__
 *           fairseq/data/new_plasma_utils.py:115-116; MmapDataset.__getitem__ fairseq/data/mmap_dataset.py:57-58)
 *           and the lookup half of TorchPQCodec.decode (knn/pq_wrapper.py:169-196).
 * Slot order inside a group: centre o, then o-left..o-1, then o+1..o+right (reference node order).
 * A slot is valid iff ids[g] != -1 and 0 <= row < n_store (the bound of :384) and the
 * row lies in the shard [row0, row0+n_local).
 * ---------------------------------------------------------------------------------------------- */
/* A range-sharded code table whose shards are ALL mapped into this process (the local one, the peers' through HIP IPC:
 * gnnlm_amd.dist.PeerMappedFetcher): the kernels that read code rows then take row r from shard min(n - 1, r /
 * rows_per_rank) -- over xGMI straight from the owner's HBM, no exchange and no copy.  The table lives in DEVICE memory;
 * the descriptors carry a pointer to it (NULL: not used, codes / row0 / n_local describe one table) -- by value it would
 * add 400 B of kernel arguments to every launch.  base[g] holds the rows [row0[g], row0[g] + rows[g]) (rank g's range plus its halo). */
typedef struct gnnlm_shards {
    int32_t n, reserved;
    int64_t rows_per_rank;
    const uint8_t* base[16];
    int64_t row0[16], rows[16];
} gnnlm_shards_t;

typedef struct gnnlm_gather {
    const uint8_t* codes;      /* [n_local, M] */
    const void* vals;          /* [n_local] int16 / int32 (optional) */
    int32_t vals_itemsize;     /* 2 or 4 with vals; ignored (0 is fine) when vals is NULL */
    int64_t n_store, row0, n_local;
    int32_t M, dsub;           /* dsub % 4 == 0; ksub is fixed to 256 (8-bit codes, pq_wrapper.py:33) */
    const float* centroids;    /* [M, 256, dsub] */
    const int64_t* ids;        /* [n_groups] */
    int64_t n_groups;
    int32_t left, right;
    float* out_x;  int64_t ld_x;   /* optional [n_groups*(1+left+right), M*dsub], zero rows for invalid slots */
    uint8_t* out_codes;        /* optional [n_slots, M] */
    int32_t* out_labels;       /* optional [n_slots], -1 for invalid */
    uint8_t* out_valid;        /* optional [n_slots] */
    int32_t direct;            /* 1: `codes` is an already-fetched [n_slots, M] buffer (slot s = row s), */
    const uint8_t* in_valid;   /*    validity comes from in_valid[n_slots]; ids is ignored */
    const int32_t* in_index;   /*    optional with direct: slot s reads row in_index[s] of `codes` */
    const gnnlm_shards_t* shards;  /* ABI 4 (DEVICE pointer): replaces codes / row0 / n_local for the code rows (not with direct, not for vals) */
    const int32_t* n_groups_dev;   /* ABI 9, optional (DEVICE int32): only the first min(n_groups, *n_groups_dev) groups are processed */
} gnnlm_gather_t;
int gnnlm_pq_gather_decode(const gnnlm_gather_t* desc, void* stream);

/* PQ encode of already-rotated rows: codes[r, m] = argmin_c norm2[m, c] - 2 x[r, m*dsub:(m+1)*dsub] . centroids[m, c]
 * (lowest index on ties).  Replaces the argmin of TorchPQCodec.encode (knn/pq_wrapper.py:131-167); the OPQ
 * rotation `x @ A.T + b` in front of it is a gnnlm_gemm_nt.  Offline producer in the reference
 * (knn/quantize_features.py:122-146), a "next" row of the hot-path table. */
int gnnlm_pq_encode(const float* x, int64_t ldx, const float* centroids, const float* norm2, int32_t M, int32_t dsub,
                    int64_t n, uint8_t* codes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * `--reinit-nfeat` ("use word embedding as neighbor node feature instead of cached representation",
 * fairseq/tasks/language_modeling.py:151-153): the datastore is the label table alone (no quantized-keys.npy is loaded,
 * :273-278; the graph builder attaches only `labels` to the ntgt nodes, fairseq/data/token_block_dataset.py:369-371,392-394,
 * 407-410) and a node's feature is the token embedding of its label,
 *     ntgt_feat = self.embed_tokens(graph.nodes["ntgt"].data["labels"])         fairseq/models/transformer.py:1046-1048
 * (embed_tokens called directly: no embed_scale, no positions, no project_in_dim).  `embed` is that table materialised once,
 * [n_vocab, d] f32 with row stride ld_embed (gnn-lm_amd/token_embed.py, imported as gnnlm_amd.token_embed: per band emb_i . proj_i^T of AdaptiveInput,
 * fairseq/modules/adaptive_input.py:63-74, or embed_tokens.weight itself).  Additive to ABI 12: a new struct and new entries.
 *
 * gnnlm_token_gather is the counterpart of gnnlm_pq_gather_decode: the same slot order (centre o, then o-left..o-1, then
 * o+1..o+right) and the same validity rule (ids[g] >= 0 and 0 <= row < n_store); in addition a slot whose label lies outside
 * [0, n_vocab) is invalid (memory safety only: the loader refuses such a table).  out_x [n_slots, d] (row stride ld_x) gets
 * embed[vals[row]] -- a copy, bit for bit -- and zero rows for invalid slots; out_labels the label (-1: invalid); out_valid
 * 1 / 0.  Each output is optional.  Only the first min(n_groups, *n_groups_dev) groups are processed; nothing else is written.
 * d % 4 == 0, ld_embed % 4 == 0, ld_x % 4 == 0, embed and out_x 16-byte aligned; vals is the WHOLE table [n_store].
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnlm_token_gather {
    const int64_t* ids;        /* [n_groups] centre rows */
    int64_t n_groups;
    int32_t left, right;
    int64_t n_store;
    const void* vals;          /* [n_store] int16 / int32 labels (neighbor_tokens, language_modeling.py:291-293) */
    int32_t vals_itemsize;     /* 2 or 4 */
    int32_t n_vocab, d;
    const float* embed;  int64_t ld_embed;   /* [n_vocab, d] */
    float* out_x;  int64_t ld_x;   /* optional [n_groups*(1+left+right), d], zero rows for invalid slots */
    int32_t* out_labels;       /* optional [n_slots], -1 for invalid */
    uint8_t* out_valid;        /* optional [n_slots] */
    const int32_t* n_groups_dev;   /* optional (DEVICE int32): only the first min(n_groups, *n_groups_dev) groups are processed */
} gnnlm_token_gather_t;
int gnnlm_token_gather(const gnnlm_token_gather_t* desc, void* stream);
/* out[e] = vals[ids[e]] for the n entries of a neighbour-id matrix, or -1 where ids[e] is not a neighbour (ids[e] < 0,
 * ids[e] >= n_store, or a label outside [0, n_vocab)): the index through which the star edges of layer 0 read the embedding
 * table directly (gnnlm_star_attn_t: X = embed, x_group_stride = 1, x_index = out) -- no [n_slots, d] buffer. */
int gnnlm_neighbor_labels(const int64_t* ids, int64_t n, int64_t n_store, const void* vals, int32_t vals_itemsize,
                          int32_t n_vocab, int32_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ('ntgt','inter','tgt') attention with the neighbour-side projections absorbed into the query:
 *   s[i,h,j] = x_j . U[i,h,:]  (valid j only),  alpha = softmax_j,  Z[i,h,:] = sum_j alpha x_j
 * x_j is decoded on the fly from PQ codes (codes != NULL) or read from dense rows (X != NULL).
 * Replaces: apply_edges(v_dot_u) + edge_softmax + u_mul_e/sum on the star edges
 *           (fairseq/models/hgt.py:354-356,383-385) fused with the gather/decode above.
 * D % 4 == 0, D <= 1024; U, Z, X (with ldx % 4 == 0), centroids, and codes when M % 16 == 0, are 16-byte aligned: other
 * operands are refused (GNNLM_E_INVALID).
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnlm_star_attn {
    const float* U;            /* [T, H, D] */
    const int64_t* ids;        /* [T, kg], -1 = no neighbour */
    int32_t T, H, D, kg;
    const uint8_t* codes;  int64_t row0, n_local;  int32_t M, dsub;
    int32_t codes_direct;      /* s > 0: `codes` is an already-fetched buffer, row of (i,j) = (i*kg+j)*s (sharded store) */
    const float* centroids;
    const float* X;  int64_t ldx;  int64_t x_group_stride;   /* dense row of (i,j) = X + (i*kg+j)*x_group_stride*ldx */
    float* Z;                  /* [T, H, D] */
    float* has_nb;             /* optional [T]: 1.0 if >= 1 valid neighbour */
    const int32_t* codes_index;   /* optional with codes_direct: row of (i,j) = codes_index[(i*kg+j)*codes_direct] */
    /* Neighbour validity (ABI 2).  (i,j) takes part in the softmax iff ids[i,j] >= 0, ids[i,j] < n_store (when
     * n_store > 0), the row lies in the shard [row0, row0+n_local) (PQ source read from the store itself) and
     * nb_valid[(i*kg+j)*nb_valid_stride] != 0 (when nb_valid is given: the validity bytes of an exchange / of
     * gnnlm_pq_gather_decode) -- the same rule as gnnlm_pq_gather_decode, so the star edges and the ntgt states
     * always agree.  The reference raises IndexError for rows >= n_store (token_block_dataset.py:370). */
    int64_t n_store;
    const uint8_t* nb_valid;  int64_t nb_valid_stride;
    const gnnlm_shards_t* shards;  /* ABI 4 (DEVICE pointer): replaces codes / row0 / n_local (PQ source, not with codes_direct) */
    /* ABI 6: optional [T, kg] group of neighbour (i, j) (-1: not a neighbour) when the dense rows / validity bytes are stored
     * once per DISTINCT centre row of the batch: row of (i,j) = X + x_index[i*kg+j]*x_group_stride*ldx, validity byte
     * nb_valid[x_index[i*kg+j]*nb_valid_stride] */
    const int32_t* x_index;
} gnnlm_star_attn_t;
int gnnlm_star_attn(const gnnlm_star_attn_t* desc, void* stream);

/* ('ntgt','intra','ntgt'): path graph with self loops over each group's slots
 * (build_ntgt_edges(context=1, bidirect=True), fairseq/data/token_block_dataset.py:395-398,545-584;
 *  attention math fairseq/models/hgt.py:354-356,383-385). */
typedef struct gnnlm_chain_attn {
    const float* Q;  const float* K;  const float* V;  int64_t ld;   /* [n_slots, d] */
    const uint8_t* valid;      /* [n_slots] */
    int64_t n_groups;  int32_t left, right, H, dk;
    const float* scale;        /* optional [H]; NULL = 1 (relation_pri/sqrt(dk) folded into K) */
    float* out;  int64_t ldo;
    int32_t radius_p1;         /* ABI 4.  0: every slot is computed; r + 1 > 0: only the slots within r positions of the centre
                                  are (Q is read for them, K / V up to r + 1 positions away; the other rows of `out` stay untouched) */
    const int32_t* n_groups_dev;   /* ABI 9, optional (DEVICE int32): only the first min(n_groups, *n_groups_dev) groups */
    const int32_t* kv_index;       /* ABI 11, optional [n_slots]: slot s reads row kv_index[s] of K and V (Q, valid and out stay slot-indexed) */
} gnnlm_chain_attn_t;
int gnnlm_chain_attn(const gnnlm_chain_attn_t* desc, void* stream);

/* masked row softmax of the dense ('tgt','intra','tgt') scores (auto_regressive_edges,
 * fairseq/data/token_block_dataset.py:586-594; edge_softmax fairseq/models/hgt.py:356).
 * S holds n_mats matrices of T rows, row stride ld; columns >= T are zeroed. */
int gnnlm_causal_softmax(float* S, int64_t n_mats, int32_t T, int64_t ld, int32_t max_ctx, void* stream);
/* The three steps above in one kernel for the recipe shape T = 256, d_k = 128 (other shapes: -EINVAL, use the GEMM +
 * gnnlm_causal_softmax + GEMM sequence): Q, K', V' are [n_blocks*T, ld] f32 with head h at columns [h*dk, (h+1)*dk);
 * out[blk*T + w, h*dk + :] = sum_{u <= w, w-u < max_ctx} softmax_u(Q_w . K'_u) V'_u.  The score matrix stays in
 * registers.  Replaces fn.v_dot_u + edge_softmax + u_mul_e/sum on ('tgt','intra','tgt') (hgt.py:354-356,383-385). */
int gnnlm_causal_attn(const float* Q, const float* K, const float* V, int64_t ld, float* out, int64_t ldo,
                      int32_t n_blocks, int32_t T, int32_t H, int32_t dk, int32_t max_ctx, void* stream);

/* Packed blocks of UNEQUAL length (`--sample-break-mode eos | complete | complete_doc`: a sample is a run of sentences,
 * fairseq/data/token_block_utils_fast.pyx:50-103; the collater batches the ragged samples' graphs as a disjoint union,
 * fairseq/data/monolingual_dataset.py:261).  Additive to ABI 12: no existing struct changes.
 *   block_off (DEVICE int32 [n_blocks + 1], ascending): block b holds the rows block_off[b] - block_off[0] ..
 *       block_off[b + 1] - block_off[0] of the call's operands.  Only differences are read, so a caller keeps ONE table for a
 *       whole split on the device and hands every batch a pointer into it (nothing per batch over PCIe).
 *   tiles (DEVICE int32 [n_tiles][2]): the (block, tile of 32 queries) work items of the causal attention, heaviest first --
 *       what gnnlm_ragged_tiles writes (host arrays: the lengths are host-known); n_tok = block_off[n_blocks] - block_off[0].
 * A table entry that does not describe rows of [0, n_tok) is skipped by the kernel, never followed. */
typedef struct gnnlm_ragged {
    const int32_t* block_off;
    const int32_t* tiles;
    int32_t n_blocks, n_tiles;
    int64_t n_tok;
} gnnlm_ragged_t;
/* HOST arrays.  Writes the tile table of block_off [n_blocks + 1] into tiles [n_tiles][2] (NULL: only counts) and returns
 * n_tiles = sum_b ceil(len_b / 32); -1 if a block is empty.  Order: descending query tile (a tile's work is the number of key
 * tiles below its diagonal), blocks in order among equals -- one 3000-token block beside a thousand sentences starts first. */
int64_t gnnlm_ragged_tiles(const int32_t* block_off, int32_t n_blocks, int32_t* tiles);
/* gnnlm_causal_attn for packed blocks of any length >= 1 in ONE launch: Q, K', V' are [n_tok, ld] f32 with head h at columns
 * [h*dk, (h+1)*dk), out[w, h*dk + :] = sum_{u in block(w), u <= w, (max_ctx == 0 or w-u < max_ctx)} softmax_u(Q_w . K'_u) V'_u.
 * f32 MFMA, running maximum / sum over tiles of 32 keys: no score matrix in memory.  d_k in {16, 32, 64, 128}, else -EINVAL.
 * Replaces fn.v_dot_u + edge_softmax + u_mul_e/sum on ('tgt','intra','tgt') (hgt.py:354-356,383-385) over the batched graph
 * of ragged samples (monolingual_dataset.py:261). */
int gnnlm_causal_attn_varlen(const float* Q, const float* K, const float* V, int64_t ld, float* out, int64_t ldo,
                             const gnnlm_ragged_t* blocks, int32_t H, int32_t dk, int32_t max_ctx, void* stream);

/* LayerNorm epilogue of HGTLayer (fairseq/models/hgt.py:404-405).  valid (optional): rows with 0 -> zeros */
int gnnlm_layernorm(const float* x, int64_t ldx, const float* gamma, const float* beta, float* out,
                    int64_t ldo, int64_t rows, int32_t d, float eps, const uint8_t* valid, void* stream);

/* `--invalid-neighbor-context c` (fairseq/data/token_block_dataset.py:360-362, switched on for the train split only:
 * fairseq/tasks/language_modeling.py:299): a neighbour whose datastore row lies within c positions of its own token
 * (`abs(offsets[tgt_idx] - offset) < c`) is skipped exactly like a -1 id -- so the rule is an id rewrite in front of the
 * graph consumers: out[i, j] = -1 if ids[i, j] != -1 and |tok_pos[i] - ids[i, j]| < c, else ids[i, j].
 * ids / out [n_tok, kg] int64 (out may alias ids), tok_pos [n_tok] int64 = the tokens' global offsets in the split. */
int gnnlm_filter_neighbors(const int64_t* ids, const int64_t* tok_pos, int64_t n_tok, int32_t kg, int64_t invalid_ctx,
                           int64_t* out, void* stream);

/* fp16 -> fp32 (precompute_feats[offsets].astype(np.float32), token_block_dataset.py:328) */
int gnnlm_half_to_float(const void* src, float* dst, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Tied adaptive softmax, target log-probability only
 * (AdaptiveSoftmax.get_log_prob with target, fairseq/modules/adaptive_softmax.py:170-206, +
 *  gather_target_probs fairseq/sequence_scorer.py:48-53,89).
 * ---------------------------------------------------------------------------------------------- */
/* lse[row] = log sum exp of logits[row * ld + e], e < n, for row < min(rows, *m_dev) (m_dev optional, a device-side count); later
 * rows of lse and picked are untouched.  An element of -inf adds nothing and a row of -inf only gives -inf; a row with a +inf gives
 * +inf; a NaN gives NaN (as torch.logsumexp).  With picked: picked[row] = logits[row * ld + pick[row]] where 0 <= pick[row] < n, and
 * untouched for any other pick (nothing out of bounds is read); without pick, picked[row] = 0.  n >= 1; rows = 0 is accepted. */
int gnnlm_row_lse_pick(const float* logits, int64_t ld, int64_t rows, const int32_t* m_dev, int32_t n,
                       const int32_t* pick, float* lse, float* picked, void* stream);

typedef struct gnnlm_adaptive_softmax {
    int32_t d, n_bands;
    int32_t cutoff[8];         /* cutoff[0..n_bands-1]; cutoff[n_bands-1] = vocab size */
    int32_t gemm_precision;    /* precision of the GEMMs (see gnnlm_gemm_t.precision); 0 = exact f32, 3 = fp16 operands
                                  (`eval_lm --fp16`; attention, LayerNorm and everything that is not a GEMM stay f32) */
    const float* head_w;       /* [cutoff[0] + n_bands - 1, d]: rows of E_0 followed by class_proj */
    const float* proj_t[8];    /* band b>=1: [dim_b, d] (embeddings.b.1.weight TRANSPOSED) */
    const float* emb[8];       /* band b>=1: [cutoff[b]-cutoff[b-1], dim_b] */
    int32_t dim[8];
} gnnlm_adaptive_softmax_t;
size_t gnnlm_adaptive_workspace_bytes(const gnnlm_adaptive_softmax_t* w, int64_t n);
/* lm_logp[r] = log p(target[r] | x[r]) for r < n: with b the band of t = target[r] (cutoff[b-1] <= t < cutoff[b], cutoff[-1] = 0),
 *   band 0:  head[t] - lse(head),                 head = x[r] . head_w^T   (cutoff[0] + n_bands - 1 logits)
 *   band b:  head[cutoff[0] + b - 1] - lse(head) + tail[t - cutoff[b-1]] - lse(tail),   tail = (x[r] . proj_t[b]^T) . emb[b]^T;
 *   the projection is a float32 tensor in the workspace, so at gemm_precision 1..3 it is rounded again as an operand of the band GEMM.
 * A target outside [0, cutoff[n_bands-1]) gives -INFINITY and nothing out of bounds is read; the 64-bit value is compared, so
 * 2^31 or 2^32 + 3 are outside too.  Nothing but lm_logp[0..n) and the workspace is written, and no bit of the result depends on
 * what the workspace held.  x, head_w, proj_t[b], emb[b] and the workspace are 16-byte aligned, ldx >= d, ldx % 4 == 0.
 * GNNLM_E_INVALID before anything is launched or any pointer is followed: n_bands outside 1..8, d or a tail dim not a positive
 * multiple of 4, gemm_precision outside 0..3, a NULL or misaligned head_w / proj_t[b] / emb[b] (b >= 1), cutoffs that are not
 * positive and strictly ascending, n < 0 or >= 2^31, a NULL x, target or lm_logp, ldx < d or ldx % 4 != 0, a misaligned x, and
 * (n > 0) a NULL, misaligned or too small workspace (gnnlm_adaptive_workspace_bytes).  n = 0 is accepted and touches nothing.
 * The call only enqueues on `stream`: no allocation, no synchronisation (graph-capturable). */
int gnnlm_adaptive_target_logp(const gnnlm_adaptive_softmax_t* w, const float* x, int64_t ldx,
                               const int64_t* target, int64_t n, float* lm_logp,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Plain (non-adaptive) output layer, target log-probability only.  Additive to ABI 12: a new struct and new entries.
 * Replaces: TransformerDecoder.output_layer with adaptive_softmax None (fairseq/models/transformer.py:843-852),
 *           get_normalized_probs' log_softmax (:1081-1085) + gather_target_probs (fairseq/sequence_scorer.py:48-53,89).
 *   lm_logp[r] = (x[r] . w[t]^T + bias[t]) - log sum_v exp(x[r] . w[v]^T + bias[v]),  t = target[r];  a target outside
 *   [0, vocab) gives -INFINITY and nothing out of bounds is read.
 * Routes: 1 = one launch (csrc/dense_logp.hip): a workgroup owns 32 rows and the whole vocabulary, no logit or partial reaches
 * memory, no workspace; vocab <= 512 and gemm_precision 0 or 3 only (at precision 0 the logits are those of gnnlm_gemm_nt bit for
 * bit).  2 = the general route, any vocab and precision: without a bias gnnlm_gemm_nt's log-sum-exp epilogue + gnnlm_lse_reduce;
 * with a bias the logits of a chunk of rows go through the workspace (gnnlm_gemm_nt with bias_mode 1 + gnnlm_row_lse_pick).
 * 0 = auto: route 1 for vocab <= 384 at gemm_precision 3, where it measured faster on the bias-free problem, else route 2.
 * gnnlm_dense_workspace_bytes sizes the workspace for chunks of at most 64 MiB of logits (0 on route 1);
 * gnnlm_dense_workspace_bytes_min is the least the call accepts (128-row chunks) -- in between, a chunk holds the multiple of
 * 128 rows that fits.  x and w are 16-byte aligned with ldx % 4 == 0, ldw % 4 == 0.  A bad d, vocab, precision or route, a null w
 * or a workspace that is too small is GNNLM_E_INVALID before anything is launched or any pointer is followed.  The call only
 * enqueues on `stream`: no allocation, no synchronisation (graph-capturable). */
typedef struct gnnlm_dense_softmax {
    int32_t d, vocab;          /* d % 4 == 0, vocab >= 1 */
    int32_t gemm_precision, route;
                               /* gemm_precision: as gnnlm_gemm_t.precision (0 f32, 1 / 2 split-bf16, 3 fp16 operands);
                                  route: 0 auto; 1 the one-launch kernel (vocab <= 512 and precision 0 or 3, else invalid); 2 the general route */
    const float* w;  int64_t ldw;   /* [vocab, d]: embed_tokens.weight or embed_out */
    const float* bias;         /* optional [vocab]: xl_bias; added in f32 and never rounded, under every precision */
} gnnlm_dense_softmax_t;
size_t gnnlm_dense_workspace_bytes(const gnnlm_dense_softmax_t* w, int64_t n);
size_t gnnlm_dense_workspace_bytes_min(const gnnlm_dense_softmax_t* w, int64_t n);
int gnnlm_dense_target_logp(const gnnlm_dense_softmax_t* w, const float* x, int64_t ldx, const int64_t* target,
                            int64_t n, float* lm_logp, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * kNN-LM distance-softmax + interpolation
 * (KNNModel.get_knn_prob knn/knn_model.py:192-217; SequenceScorer fairseq/sequence_scorer.py:55-68,110,121).
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnlm_knn_interp {
    const float* lm_logp;      /* [n] */
    const float* sims;         /* [n, k] similarities after sim_func (knn_model.py:137-177) */
    const int64_t* ids;        /* [n, k], -1 = padding (masked with -1e10, :193) */
    const void* vals;  int32_t vals_itemsize;  int64_t n_store, row0, n_local;
    const int32_t* knn_vals;   /* optional [n, k]: vals[ids] already fetched (sharded store) */
    const int64_t* targets;    /* [n] */
    int64_t n;  int32_t k;
    float temperature;
    double lmbda;
    float* out_logp;           /* [n] */
    float* out_pknn;           /* optional [n] */
    int64_t* out_recall;       /* optional [n] */
    /* ABI 7, optional: one TAG byte per label row, vals_tag[r] = gnnlm_label_tag(vals[r]) (built once per store by
     * gnnlm_label_tags).  A neighbour can only match the target when the tags match, so the k gathers of `vals[knns]`
     * (knn_model.py:198) read this 4x smaller table and the 4-byte label only on a tag match (1 in 256 + the true hits):
     * same result bit for bit, a quarter of the table behind the random reads. */
    const uint8_t* vals_tag;
    /* ABI 7, optional, with vals_tag: scratch of at least gnnlm_knn_interp_scratch_bytes(n, k, n_local) bytes (16-byte aligned,
     * contents irrelevant).  The k look-ups of every token are then ROUTED: sorted by region of the tag table (<= 128 KB each) and
     * looked up by one workgroup per region against the region's slice held in LDS, instead of costing one memory request each
     * (the memory system serves ~48 G requests/s whatever their size: 8192 x 1024 one-by-one look-ups take 176 us).  Same result
     * bit for bit (csrc/knn_bucket.hip).  Needs k <= 1024, n <= 2^16, n_local <= 2^27 (else the one-pass kernel runs). */
    void* scratch;  size_t scratch_bytes;
} gnnlm_knn_interp_t;
int gnnlm_knn_interp(const gnnlm_knn_interp_t* desc, void* stream);
size_t gnnlm_knn_interp_scratch_bytes(int64_t n, int32_t k, int64_t n_local);
/* The tuning grid of kNN-LM in one call: every point of ks x temperatures x lmbdas from ONE read of the search result.
 * Replaces: one whole `fairseq-eval-lm ... --lmbda $a` per setting (gnnlm_scripts/wiki103/hgt_lm_wiki103_reproduce.sh:137),
 * i.e. get_knn_prob (knn/knn_model.py:192-217) + combine_knn_and_vocab_probs (fairseq/sequence_scorer.py:55-68,121) once per
 * point.  Point (k', t, l), 1 <= k' <= k, t > 0, 0 <= l <= 1, is computed over the FIRST k' columns of sims / ids / knn_vals
 * (the search returns neighbours best first: what a k'-search returns) and is bit-identical to gnnlm_knn_interp on those
 * columns where that call is defined (0 < l < 1); l = 0 gives lm_logp back, l = 1 gives logf(p_knn + 1e-10f).
 * The grid values are HOST data inside the descriptor (the call neither allocates nor copies); more values than the arrays
 * hold, k > 1024 (gnnlm_knn_interp serves it, one setting per call) or a value out of range is GNNLM_E_INVALID and nothing is
 * launched.  Labels as in gnnlm_knn_interp_t (knn_vals, or vals with n_store / row0 / n_local); no tag table, no routed
 * look-ups.  Point index g = (ik * n_temperatures + it) * n_lmbdas + il: k slowest, lmbda fastest. */
typedef struct gnnlm_knn_interp_grid {
    const float* lm_logp;      /* [n] */
    const float* sims;         /* [n, k] */
    const int64_t* ids;        /* [n, k], -1 = padding */
    const void* vals;  int32_t vals_itemsize;  int64_t n_store, row0, n_local;
    const int32_t* knn_vals;   /* optional [n, k]: vals[ids] delivered by the search */
    const int64_t* targets;    /* [n] */
    int64_t n;  int32_t k;     /* k <= 1024 */
    int32_t n_ks, n_temperatures, n_lmbdas;
    int32_t ks[8];
    float temperatures[16];
    double lmbdas[16];
    float* out_logp;           /* [n_ks * n_temperatures * n_lmbdas, n]: a point's tokens are contiguous */
    float* out_pknn;           /* optional [n_ks * n_temperatures, n] */
    int64_t* out_recall;       /* optional [n_ks, n] */
} gnnlm_knn_interp_grid_t;
int gnnlm_knn_interp_grid(const gnnlm_knn_interp_grid_t* desc, void* stream);
/* The same grid for n_lm language-model rows at once, 1 <= n_lm <= 8: desc->lm_logp is read as [n_lm, n] with row stride ld_lm
 * (>= n) and desc->out_logp is [n_lm * G, n], G = n_ks * n_temperatures * n_lmbdas; the lm row varies slowest (row a * G + g).
 * Replaces: one whole `fairseq-eval-lm ... --model-overrides "{'orig_prob_ratio': $alpha, ...}" --lmbda $a` per (alpha, setting)
 * (gnnlm_scripts/wiki103/hgt_lm_wiki103_reproduce.sh:79-86,137): the kNN interpolation of fairseq/sequence_scorer.py:135 applied
 * on top of the base-LM / GNN mixture of fairseq/models/transformer.py:1056-1062,1075-1077 (gnnlm_logp_mix) at every ratio.
 * The exponentials, prefix sums and wave reductions of a (k', t) pair are computed once and serve every lm row; out_pknn and
 * out_recall do not depend on the lm row and keep their shapes.  Row block a equals gnnlm_knn_interp_grid called with lm row a,
 * bit for bit; gnnlm_knn_interp_grid is the n_lm = 1 call of this entry.  n_lm outside 1 .. 8 is GNNLM_E_INVALID. */
int gnnlm_knn_interp_grid_lm(const gnnlm_knn_interp_grid_t* desc, int32_t n_lm, int64_t ld_lm, void* stream);
/* out[a, i] = logsumexp(log(alphas[a]) + base_logp[i], log(1 - alphas[a]) + gnn_logp[i]) in float32, a < n_alphas <= 8: the
 * `orig_prob_ratio` mixture of the two target log-probabilities the tied adaptive softmax gives for the base-LM feature and for
 * the GNN output.  Replaces: TokenGraphTransformerDecoder.combinetow_probs (fairseq/models/transformer.py:1056-1062) as called
 * by get_normalized_probs (:1075-1077) on the gathered target column, once per ratio; here one read of the two inputs serves
 * every ratio.  The ratios are HOST data (the call neither allocates nor copies; graph-capturable, no scratch); the logs are
 * taken in float64 and rounded to float32, as math.log lands in the reference's float32 coeffs.  alphas[a] = 0 returns gnn_logp
 * and alphas[a] = 1 returns base_logp bit for bit (log 0 = -inf drops the term).  out is [n_alphas, n], rows contiguous.
 * A ratio outside 0 .. 1 or n_alphas outside 1 .. 8 is GNNLM_E_INVALID and nothing is launched. */
int gnnlm_logp_mix(const float* gnn_logp, const float* base_logp, int64_t n, const double* alphas, int32_t n_alphas, float* out,
                   void* stream);
/* Exact similarities: the similarity of every retrieved neighbour recomputed from its stored key in one kernel.
 * Replaces: the `ip` / `l2` branches of KNNModel.get_knn_prob's sim_func dispatch (knn/knn_model.py:161-175:
 * `self.keys[knns]` gathered on the host, then `-sum((q - key)^2)` or `sum(key * q)`, the keys divided by their norm when the
 * index file name says "cosine").  out[i, j] is a function of query row i and of the key row of neighbour (i, j) ONLY: one
 * fixed summation order per row, whatever n, k, the column, the strides, the mode.  fp16 / f32 values are widened exactly, the
 * sums (and the division by the key norm) run in float64 and a result is rounded to float32 once: within half a float32 ulp
 * of the exact value, where the reference's own float32 sums carry an error that grows with d and with what cancels.
 * An id < 0 reads row id + n_rows (numpy's wrap: -1 is the last row, as for the reference); an id outside [-n_rows, n_rows)
 * touches no memory and yields -FLT_MAX.  No scratch, no allocation, only enqueues on `stream` (graph-capturable). */
typedef struct gnnlm_knn_resim {
    const float* queries;  int64_t ldq;     /* [n, d], row stride in elements; already normalised for a cosine index (:181-184) */
    const int64_t* ids;  int64_t ld_ids;    /* [n, k]; NULL = direct mode: neighbour (i, j) is row i * k + j of keys (staged rows) */
    const void* keys;  int32_t keys_itemsize;   /* [n_rows, d] fp16 (2) or f32 (4) */
    int64_t ld_keys, n_rows;                /* row stride in elements; byte offsets are 64-bit */
    int32_t d;  int64_t n;  int32_t k;      /* d >= 1, n >= 0, k >= 1 */
    int32_t metric;                         /* 0: sum_e key[e] * q[e];  1: -sum_e (q[e] - key[e])^2   (:166-167) */
    int32_t normalize_keys;                 /* metric 0 only: divide by sqrt(sum_e key[e]^2) of the same row, same pass (:172-173) */
    float* out;  int64_t ld_out;            /* [n, k] */
} gnnlm_knn_resim_t;
int gnnlm_knn_recompute_sims(const gnnlm_knn_resim_t* desc, void* stream);
/* tag[r] = (uint32(vals[r]) * 2654435761) >> 24 for the n rows of a label table (int16 / int32) */
int gnnlm_label_tags(const void* vals, int32_t vals_itemsize, int64_t n, uint8_t* tag, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Next-token DISTRIBUTIONS: the dense [n, V] outputs of the scoring chain (csrc/dense_dist.hip).  Additive to ABI 12: one new
 * struct and new entries, no existing member moved.
 * Replaces: AdaptiveSoftmax.get_log_prob(input, target=None) (fairseq/modules/adaptive_softmax.py:170-206) as called by
 *           TokenGraphTransformerDecoder.get_normalized_probs (fairseq/models/transformer.py:1064-1085), the log_softmax of the
 *           plain head (:1081-1085), KNNModel.get_knn_prob(targets=None) (knn/knn_model.py:192-205) and
 *           combine_knn_and_vocab_probs over the whole row (fairseq/sequence_scorer.py:55-68,121).
 * ---------------------------------------------------------------------------------------------- */
/* out[r, v] = log p(v | x[r]) for r < n and EVERY v < V = cutoff[n_bands-1]; out is [n, V] with row stride ldo >= V:
 *   v < cutoff[0]:                   head[v] - lse(head)                                  head = x[r] . head_w^T
 *   cutoff[b-1] <= v < cutoff[b]:    tail_b[v - cutoff[b-1]] - lse(tail_b) + head[cutoff[0] + b - 1] - lse(head)
 * built from gnnlm_gemm_nt (the head's logits go to the workspace, a band's straight into its columns of out with ldc = ldo),
 * gnnlm_row_lse_pick without a pick, and one kernel that finishes the rows in place.  The columns ldo > V leaves behind a row
 * are not written.  Rows are worked in chunks -- at most 1024 rows, as many multiples of 128 as the workspace holds, and
 * chunk * max(ldo, ldx) < 2^31: the base pointers advance per chunk, so no kernel sees an element offset of 2^31 or more and
 * n * ldo may be any size.  gnnlm_adaptive_log_probs_workspace_bytes sizes the workspace for the largest chunk,
 * ..._workspace_bytes_min is the least the call accepts (chunks of min(n, 128) rows).  Two identical calls give identical bits.
 * x, the weights and the workspace are 16-byte aligned, ldx >= d, ldx % 4 == 0; out needs its natural 4 bytes only.
 * GNNLM_E_INVALID before anything is launched or written: what gnnlm_adaptive_target_logp refuses of w, x, ldx and n, a NULL
 * or misaligned out, ldo < V or >= 2^31, and (n > 0) a NULL, misaligned or too small workspace.  n = 0 is accepted and touches
 * nothing.  The call only enqueues on `stream`: no allocation, no synchronisation. */
size_t gnnlm_adaptive_log_probs_workspace_bytes(const gnnlm_adaptive_softmax_t* w, int64_t n);
size_t gnnlm_adaptive_log_probs_workspace_bytes_min(const gnnlm_adaptive_softmax_t* w, int64_t n);
int gnnlm_adaptive_log_probs(const gnnlm_adaptive_softmax_t* w, const float* x, int64_t ldx, int64_t n, float* out, int64_t ldo,
                             void* workspace, size_t workspace_bytes, void* stream);
/* The same for the plain head: out[r, v] = (x[r] . w[v]^T + bias[v]) - log sum_u exp(x[r] . w[u]^T + bias[u]), v < vocab.  The
 * logits of a chunk are written into out by gnnlm_gemm_nt (bias_mode 1 with a bias) and finished in place by the same kernel;
 * `route` is not read.  Chunks, alignment, refusals and the two workspace sizes as above. */
size_t gnnlm_dense_log_probs_workspace_bytes(const gnnlm_dense_softmax_t* w, int64_t n);
size_t gnnlm_dense_log_probs_workspace_bytes_min(const gnnlm_dense_softmax_t* w, int64_t n);
int gnnlm_dense_log_probs(const gnnlm_dense_softmax_t* w, const float* x, int64_t ldx, int64_t n, float* out, int64_t ldo,
                          void* workspace, size_t workspace_bytes, void* stream);

/* kNN distance-softmax aggregated by label and interpolated with a WHOLE row of language-model log-probabilities:
 *   p_j = softmax_j((ids[r, j] == -1 ? -1e10 : sims[r, j]) / temperature)                 (knn/knn_model.py:192-196)
 *   p_knn[r, v] = sum of p_j over the neighbours j whose label is v                       (:203-205, `weighted_probs`)
 *   out[r, v] = logaddexp(lm_logp[r, v] + log(1 - lmbda), logf(p_knn[r, v] + 1e-10f) + log(lmbda))   for EVERY v < V
 * -- the 1e-10 applies to labels without a neighbour too, so out[r, t] is what gnnlm_knn_interp gives for target t, whatever
 * t is (fairseq/sequence_scorer.py:55-68,121; up to the summation order of p_knn).  Labels as in gnnlm_knn_interp_t: knn_vals,
 * or vals with n_store / row0 / n_local (an id < 0 wraps to id + n_store; a row outside the shard has no label).  A neighbour
 * whose label lies outside [0, V) or is missing takes part in the softmax and contributes to no column; nothing is read or
 * written out of bounds.  The aggregation is deterministic: the k (label, p) pairs of a row are sorted by label in LDS and every
 * run is summed in sorted order (float64, rounded once); no floating-point atomics; two identical calls give identical bits.
 * Two launches ordered by the stream: an elementwise pass over [n, V] that writes the no-neighbour value (16-byte loads and
 * stores when lm_logp, out, out_pknn are 16-byte aligned and their row strides multiples of 4; any 4-byte alignment works),
 * then one workgroup per row that overwrites its at most k label columns from lm_logp.  The pad columns of ldo / ld_pknn > V
 * are not written.  out, out_pknn and lm_logp must not overlap.
 * GNNLM_E_INVALID before anything is launched or written: a NULL lm_logp / sims / ids / out, neither vals nor knn_vals, vals
 * without n_store / n_local or with an itemsize other than 2 / 4, k outside 1 .. 1024, temperature <= 0, lmbda outside (0, 1),
 * V < 1, n < 0, a row stride below V, a misaligned pointer (natural alignment), out == lm_logp.  n = 0 is accepted and touches
 * nothing.  The call only enqueues: no allocation, no synchronisation, no scratch. */
typedef struct gnnlm_knn_mix_dense {
    const float* lm_logp;  int64_t ld_lm;     /* [n, V], row stride ld_lm >= V */
    const float* sims;         /* [n, k] similarities after sim_func */
    const int64_t* ids;        /* [n, k], -1 = padding */
    const void* vals;  int32_t vals_itemsize;  int64_t n_store, row0, n_local;
    const int32_t* knn_vals;   /* optional [n, k]: vals[ids] already fetched */
    int64_t n;  int32_t k, V;  /* k <= 1024 */
    float temperature;
    double lmbda;
    float* out;  int64_t ldo;          /* [n, V] */
    float* out_pknn;  int64_t ld_pknn; /* optional [n, V]: p_knn itself, zero where no neighbour has the label */
} gnnlm_knn_mix_dense_t;
int gnnlm_knn_mix_dense(const gnnlm_knn_mix_dense_t* desc, void* stream);

/* rank[r] = the number of columns of logp[r, 0..V) that come before column target[r] in the order of gnnlm_topk_merge (largest
 * = 1): larger value first, then smaller id -- so target[r] is at position rank[r] of the row's full top-V list, and inside the
 * top-N that gnnlm_topk_merge (ncols = V, k = N) returns iff rank[r] < N.  As there, a NaN or -inf column is absent: it comes
 * before nothing, and a target whose own value is absent comes behind every present column.  A target outside [0, V) gives -1
 * and reads nothing.  logp [n, V] with row stride ld >= V; target int64 [n]; rank int32 [n].  NULL operands, ld < V, V < 1 and
 * n < 0 are GNNLM_E_INVALID; n = 0 is accepted and touches nothing. */
int gnnlm_row_rank(const float* logp, int64_t ld, int64_t n, int32_t V, const int64_t* target, int32_t* rank, void* stream);

/* ------------------------------------------------------------------------------------------------
 * On-device kNN search, selection half: fold one chunk of scores into a running top-k per query.
 * Replaces the k-selection of faiss `index.search` (knn/knn_model.py:87-101, knn/find_knn.py:55-70); the
 * scores of a chunk come from gnnlm_gemm_nt over a chunk of keys (exact search) or from gnnlm_ivfpq_scan.
 *   value of column c for row r:  v = col_bias[c] + alpha * col_scale[c] * scores[r, c]
 *   (cosine index: col_scale = 1/|key|;  L2: alpha = -2, col_bias = |key|^2, largest = 0, add |q|^2 afterwards)
 * State: best_val / best_id [n, k], best first, ties by ascending id (== a stable argsort of the whole row, so the
 * result is independent of the chunking); unfilled slots hold id -1 like faiss.  No [n, N] matrix is ever built.
 * The rules in full (tests/topk_ref.py restates them, tests/test_topk_abi_gpu.py holds both kernels to them bit for bit):
 *   - the value is float32, rounded after each step in this order: scores[r, c] * alpha (alpha 0 is read as 1), then * col_scale[c],
 *     then + col_bias[c]; no fused multiply-add.  Denormals are kept and ordered as numbers;
 *   - the id of column c of row r is ids[r * ld_ids + c] if ids is given, else col_ids[c] if col_ids is given, else col0 + c:
 *     ids overrides col_ids, which overrides col0; the overridden fields are not read;
 *   - a column is absent if its id is < 0 (from any of the three sources; col0 + c < 0 included), if its value is NaN, or if its
 *     value is the worst infinity of the direction (-inf for largest, +inf otherwise: the padding value).  The other infinity is a
 *     value like any other;
 *   - row r has min(ncols, row_ncols[r]) columns: row_ncols[r] <= 0 is an empty row, row_ncols[r] > ncols is clamped; the columns
 *     beyond, and the pad columns of ld / ld_ids, are not read;
 *   - a call folds the state's real entries (id >= 0; slots with id < 0 are unfilled whatever their value) and the chunk's columns:
 *     the k best by (value, ascending id), then id -1 with -inf (largest) / +inf.  Ids are expected to be unique within a row and
 *     across its chunks; a zero is returned with either sign (-0 and +0 compare equal and tie);
 *   - n = 0 is accepted and touches nothing.  ncols = 0 is accepted with scores = NULL: init = 1 writes the padding to all n * k
 *     slots, init = 0 leaves the state's content as it is.  k outside [1, 2048], n < 0, ncols < 0, a NULL state buffer and NULL
 *     scores with ncols > 0 are refused with nothing written.
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnlm_topk {
    const float* scores;  int64_t ld;     /* [n, ncols] chunk, row stride ld elements */
    int64_t n;  int32_t ncols;
    int64_t col0;                         /* id of column c = ids ? ids[r, c] : col_ids ? col_ids[c] : col0 + c (an id < 0: skipped) */
    const int64_t* col_ids;
    const float* col_scale;  const float* col_bias;  float alpha;   /* alpha 0 is read as 1 */
    int32_t k;                            /* <= 2048 */
    int32_t largest;                      /* 1: keep the k largest values, 0: the k smallest */
    int32_t init;                         /* 1: the state is empty (first chunk), buffers need no initialisation */
    float* best_val;  int64_t* best_id;   /* [n, k] */
    const int32_t* row_ncols;             /* optional [n]: row r only has its first row_ncols[r] columns */
    const int64_t* ids;  int64_t ld_ids;  /* optional per-row ids [n, ncols] (candidate lists of an IVF scan); overrides col0 / col_ids */
} gnnlm_topk_t;
int gnnlm_topk_merge(const gnnlm_topk_t* desc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * IVF-PQ scan with asymmetric distance computation (ADC), inner-product metric with residual codes: the
 * search of the reference's kNN index `OPQ64_1024,IVF4096,PQ64`, nprobe 32 (faiss IndexIVFPQ, by_residual;
 * gnnlm_scripts/wiki103/find_knn.sh:8-13, knn/knn_model.py:100) restated for the GPU:
 *     score(q, x) = <q', c_list(x)> + sum_m lut[q][m][code_m(x)],   lut[q][m][c] = <q'_m, pq_centroid[m][c]>
 * with q' the OPQ-rotated query.  The rotation, the coarse scores and the look-up tables are GEMMs
 * (gnnlm_gemm_nt), the probe selection and the final k-selection are gnnlm_topk_merge; this entry point scans the
 * probed lists.  A task = (query, probe slot); tasks come grouped by list so that concurrent workgroups read the
 * same codes.  Dense mode (tau == NULL): every score of the list is written, for the first probes of a query.
 * Filtered mode: only scores above tau[query] (its current k-th best) are appended to the query's candidate rows.
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnlm_ivfpq_scan {
    const uint8_t* codes;  const int64_t* ids;  const int64_t* list_off;   /* lists: codes [N, M], ids [N]; list l = [list_off[l], list_off[l+1]) */
    int32_t M;                            /* 8-bit sub-quantizers, M % 16 == 0, M <= 128 */
    const float* lut;  int64_t ld_lut;    /* [n, M*256] */
    const int64_t* probe_list;  const float* probe_bias;  int32_t ld_probe;   /* [n, ld_probe]: probed lists (-1: none) and <q', centroid> */
    const int32_t* task_q;  const int32_t* task_p;  int64_t n_tasks;
    float* out_val;  int64_t* out_id;  int64_t ld_out;  int32_t p0, seg;      /* dense: column (p - p0) * seg + j, ids -1 beyond the list
                                                                               * (out_val is NOT written there: the -1 marks the column);
                                                                               * out_id NULL (ABI 5): scores only, -inf beyond the list -- the
                                                                               * caller maps the columns it keeps to ids[list_off[list] + j].
                                                                               * Rows of a list beyond seg are dropped */
    const float* tau;  float* cand_val;  int64_t* cand_id;  int32_t* cand_cnt;  int32_t cap;   /* filtered: rows of `cap` slots, cand_cnt[q] counts ALL survivors */
    int32_t packed;                       /* ABI 5: nonzero = `codes` is the image of gnnlm_ivfpq_pack_codes and `lut` the tables of
                                           * gnnlm_ivfpq_pack_lut (M = 32 or 64): the bank-conflict-free scan */
    /* L2 metric (faiss METRIC_L2 with residual codes: `IndexBuilder`'s default, knn/index_builder.py:26,118): the score of key x
     * in list l is  -|q' - c_l - r(x)|^2 = probe_bias - sum_m (list_term[l][m][code_m] - 2 lut[q][m][code_m])  with
     * list_term[l][m][c] = |p_mc|^2 + 2 <c_l,m , p_mc>  ([nlist, M * 256], row stride ld_list_term; faiss's "precomputed table")
     * and probe_bias = -|q' - c_l|^2.  list_term != NULL selects it (row-major codes, packed = 0); larger score = nearer */
    const float* list_term;  int64_t ld_list_term;
    /* Appended within ABI 12 (additive: one member at the end, no existing member moved).  The same L2 score with one term per KEY in
     * place of the per-list table: the 64 list_term entries of a key add up to a constant of the key,
     *     key_term[r] = sum_m list_term[l][m][code_m(r)] = |c_l + r(x)|^2 - |c_l|^2        (gnnlm_ivfpq_key_terms; [N], list order like `ids`)
     * so  -|q' - c_l - r(x)|^2 = probe_bias + 2 sum_m lut[q][m][code_m] - key_term[r]  with the tables of the QUERY alone, as for the
     * inner product: row-major or packed codes, dense and filtered mode, nothing of size nlist.  key_term != NULL selects it;
     * list_term and key_term together are refused */
    const float* key_term;
} gnnlm_ivfpq_scan_t;
int gnnlm_ivfpq_scan(const gnnlm_ivfpq_scan_t* desc, void* stream);
/* Added within ABI 12 (additive: a new entry).  The per-key term of the L2 scan above, once per index (faiss keeps the per-list
 * "precomputed table" instead: IndexIVFPQ::precompute_table behind `IndexBuilder`'s METRIC_L2, knn/index_builder.py:26,118):
 * key_term[r] = sum_m (|p_m,c|^2 + 2 <c_l,m, p_m,c>), c = list_codes[r][m], l the list of row r by list_off (empty lists allowed),
 * coarse [nlist, M * dsub], pq [M, 256, dsub]; accumulated in float64 in ascending (m, element) order and rounded to float32 once.
 * M % 16 == 0, dsub % 4 == 0, 16-byte aligned operands; rows are addressed with 64 bits. */
int gnnlm_ivfpq_key_terms(const uint8_t* list_codes, const int64_t* list_off, int64_t N, int32_t nlist, const float* coarse, const float* pq,
                          int32_t M, int32_t dsub, float* key_term, void* stream);

/* The scan's own device layouts (M = 32 or 64).  Codes: blocks of 64 rows stored [M/16 pieces][64 rows][16 B], and inside a
 * row byte s of half h holds sub-quantizer 32 h + (row + s) mod 32 -- `out` has ceil(N / 64) * 64 * M bytes, rows beyond N
 * zero.  Tables: lut [n, M, 256] (row stride ld_lut) -> out [n, M/32, 256, 32].  With these a lane's look-up s goes to
 * sub-quantizer (lane + s) mod 32 and the 32 lanes of an LDS access group always use 32 different banks. */
int gnnlm_ivfpq_pack_codes(const uint8_t* codes, int64_t N, int32_t M, uint8_t* out, void* stream);
int gnnlm_ivfpq_pack_lut(const float* lut, int64_t ld_lut, int64_t n, int32_t M, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * ABI 6: the filtered scan on the int8 matrix cores, M = 64 (csrc/ivfpq8_scan.hip) -- the thresholded round of the same
 * search (faiss IndexIVFPQ.search behind knn/knn_model.py:100), as a FILTER with a guaranteed bound followed by an exact
 * float32 re-score, so that the candidates and their scores are those of the one-pass float32 scan above:
 *   gnnlm_ivfpq_pack_tiles     codes [N, 64] -> the scan's image: tiles of 16 rows, [tile][g 0..3][i 0..15][p 0..15] =
 *                              code[16 tile + i][16 g + (i + p) % 16], ceil(N / 16) * 1024 bytes, rows beyond N zero
 *   gnnlm_ivfpq_quantize_lut   lut [n, 64, 256] f32 -> qlut [n][2 halves][256 codes][32 slots] u8 and qmeta [n, 4] f32 =
 *                              {delta, sum_m lo_m, max |lut|, 0} with  lut[m][c] < lo_m + (u + 1) delta  for every entry; the
 *                              table byte is the signed u - 128 (what the i8 matrix instruction reads)
 *   gnnlm_ivfpq_scan8          one workgroup per GROUP = up to 8 queries probing one list; a key (row of the list-ordered
 *                              index) is appended to surv[q] = {row, list} iff the integer sum of its 64 table bytes
 *                              reaches the integer image of tau[q] -- a superset of {score > tau[q]}
 *   gnnlm_ivfpq_tau            the threshold itself: a lower bound of the k-th best score from histograms of the integer sums of
 *                              the first D lists (gnnlm_ivfpq_scan8 with out_hist), replacing the float32 dense round + its k-selection
 *   gnnlm_ivfpq_rescore        exact scores of the survivors (summation order of gnnlm_ivfpq_scan's packed kernel),
 *                              score > tau[q] -> (cand_val, cand_id = payload[row]); cand_cnt[q] counts all of them.  With
 *                              `qmeta` the threshold is first refined from the survivors themselves, in the same launch
 * ABI 12: the refinement (ABI 7) has no entry point of its own any more; it runs only inside gnnlm_ivfpq_rescore (ABI 10).
 * ---------------------------------------------------------------------------------------------- */
int gnnlm_ivfpq_pack_tiles(const uint8_t* codes, int64_t N, int32_t M, uint8_t* out, void* stream);
int gnnlm_ivfpq_quantize_lut(const float* lut, int64_t ld_lut, int64_t n, int32_t M, uint8_t* qlut, float* qmeta, void* stream);
/* Added within ABI 11 (additive: a new entry and struct, no existing layout changed).  The ADC tables and their int8 image in
 * one launch: lut [n, 64 * 256] f32 (row stride ld_lut) = <qr_m, pq_mc>, bit for bit what gnnlm_gemm_nt computes from
 * A = qr (lda = ld_qr, sA1 = dsub), W = pq [64][256][dsub] (ldw = dsub, sW1 = 256 dsub), batch1 = 64, K = dsub at the default
 * f32 precision; qlut / qmeta bit for bit what gnnlm_ivfpq_quantize_lut makes of that lut.  M = 64, dsub in {4, 8, 16, 32},
 * every pointer 16-byte aligned; other shapes are refused (use the two calls). */
typedef struct gnnlm_ivfpq_tables {
    const float* qr;  int64_t ld_qr;  int64_t n;
    const float* pq;  int32_t M;  int32_t dsub;
    float* lut;  int64_t ld_lut;
    uint8_t* qlut;  float* qmeta;
} gnnlm_ivfpq_tables_t;
int gnnlm_ivfpq_tables(const gnnlm_ivfpq_tables_t* desc, void* stream);
/* The task table of gnnlm_ivfpq_scan8 from the probe table: (query, probe) pairs of probe_list [n, P] (row stride ld_probe; -1 = none)
 * -> groups of up to 8 queries that probe the same list, in list order: grp_list [G], grp_q [G, 8] (-1 padded), n_groups [1]
 * (device), optionally grp_out [G, 8] = (query * P + probe slot) * seg (the pair's segment of a [n, P, seg] array; NULL: not
 * wanted).  G = n * P / 8 + nlist + 1 entries must be allocated; scratch: 2 * (nlist + 1) int32.  Which queries of a list share a
 * group is not specified (positions come from atomics); the searches' results do not depend on it. */
int gnnlm_ivfpq_build_groups(const int64_t* probe_list, int64_t ld_probe, int64_t n, int32_t P, int32_t nlist, int64_t seg,
                             int32_t* grp_list, int32_t* grp_q, int64_t* grp_out, int32_t* n_groups, int32_t* scratch, void* stream);
typedef struct gnnlm_ivfpq_scan8 {
    const uint8_t* tiles;  const int64_t* list_off;  int32_t M;
    const uint8_t* qlut;  const float* qmeta;
    const float* coarse;  int64_t ld_coarse;          /* [n, nlist] <q', centroid_l>: the bias of list l */
    const float* tau;                                 /* [n] */
    const int32_t* grp_list;  const int32_t* grp_q;   /* [max_groups] list (-1: none), [max_groups, 8] queries (-1: none), sorted by list */
    const int32_t* n_groups;  int32_t max_groups;     /* DEVICE count of groups in use (no host round trip), capacity of the arrays */
    uint32_t* surv;  int32_t* surv_cnt;  int32_t cap; /* [n, cap, 2] {row, list | sum_u << 18}; surv_cnt [n, 16] int32 (one 64-byte line per query: the
                                                       * counters are hammered by atomics), column 0 counts ALL survivors (overflow check) */
    /* threshold pass (out_hist != NULL; tau / surv unused): the integer sums sum_m u (0 .. 255 * 64) of a list's keys are
     * histogrammed per query (1024 bins of 16) and written to out_hist[grp_out[group * 8 + j] .. + 1024) for query j of the group
     * (grp_out < 0: skipped; every (query, list) pair belongs to exactly one group: plain stores) */
    uint32_t* out_hist;  const int64_t* grp_out;
    /* ABI 8, threshold pass only: histogram every sums_stride-th tile of 16 keys of a list (0 / 1: every tile).  A SAMPLE of the
     * keys: the caller asks gnnlm_ivfpq_tau for rank ~k / stride (+ a margin) and must then verify that at least k candidates
     * score above the threshold it got -- gnn-lm_amd/ivfpq.py searches the (rare) queries that fail again with stride 1 */
    int32_t sums_stride;
    /* the workgroups are persistent (one per CU); with work_ctr != NULL ([8, 16] int32, ZEROED by the caller before every call:
     * one counter per XCD, one 64-byte line each) a workgroup fetches its next group from its XCD's counter -- lists of very
     * different lengths stay balanced; NULL: static striding */
    int32_t* work_ctr;
    /* ABI 9: the index's shape, checked -- a survivor record packs the row inside its list into 19 bits and the list into 18, so
     * the filter covers indexes with nlist <= 2^18 lists of fewer than 2^19 keys (max_list = the longest list); longer / more
     * lists are refused here (gnn-lm_amd/ivfpq.py sends such an index to the float32 scan) */
    int32_t nlist;  int64_t max_list;
} gnnlm_ivfpq_scan8_t;
int gnnlm_ivfpq_scan8(const gnnlm_ivfpq_scan8_t* desc, void* stream);
/* tau[q] = a lower bound of query q's k-th best score over its first D probed lists, from the threshold pass's histograms
 * ([n, D, 1024] uint32; list d of query q = probe_list[q, d] with bias probe_bias[q, d]): at least k keys of those lists score
 * above it; -inf if they hold fewer than k keys */
typedef struct gnnlm_ivfpq_tau {
    const uint32_t* hist;  int32_t D;
    const int64_t* probe_list;  const float* probe_bias;  int32_t ld_probe;
    const float* qmeta;
    int64_t n;  int32_t k;
    float* tau;
} gnnlm_ivfpq_tau_t;
int gnnlm_ivfpq_tau(const gnnlm_ivfpq_tau_t* desc, void* stream);
/* ABI 7.  Results of a search over an index that carries labels (payload = id << label_bits | label, -1 = no result): idx [n]
 * -> the ids in place, out_vals [n] (optional) the labels, `val_last` where there is no result (numpy's vals[-1], knn_model.py:198) */
int gnnlm_ivfpq_split_payload(int64_t* idx, int64_t n, int32_t label_bits, int32_t val_last, int32_t* out_vals, void* stream);
/* The two k-selections of the search in kernels of their own (csrc/ivfpq_select.hip).  Each returns bit for bit what
 * gnnlm_topk_merge returns with init = 1 on the same operands (the rules of gnnlm_topk_t: value rounded after each step, an entry
 * is absent if its id is < 0 or its value is NaN or the worst infinity, better value first, then ascending id, -0 == +0, padding
 * id -1 with -inf / +inf); shapes outside the limits are refused with nothing written and the caller uses gnnlm_topk_merge.
 *
 * Probe selection: the k <= 64 best of ncols <= 4096 columns per row, value = scores[r, c] + col_bias[c] (col_bias optional: the
 * L2 route's -|c|^2 / 2), id = c.  One wave per row, the row in registers, no barrier.  ncols = 0 writes the padding (scores may be
 * NULL), n = 0 touches nothing. */
typedef struct gnnlm_ivfpq_select_probes {
    const float* scores;  int64_t ld;     /* [n, ncols], row stride ld elements */
    int64_t n;  int32_t ncols;            /* ncols <= 4096 */
    const float* col_bias;                /* optional [ncols] */
    int32_t k;                            /* <= 64 */
    int32_t largest;                      /* 1: the k largest values, 0: the k smallest */
    float* out_val;  int64_t* out_id;     /* [n, k] */
} gnnlm_ivfpq_select_probes_t;
int gnnlm_ivfpq_select_probes(const gnnlm_ivfpq_select_probes_t* desc, void* stream);
/* Final selection: the k <= 1024 largest of a ragged candidate row -- row r holds min(cap, row_ncols[r]) candidates (row_ncols NULL:
 * cap; <= 0: none), cap <= 16384, value cand_val[r, c], id cand_id[r, c] (a 64-bit payload; payloads need not be unique within a
 * row: equal (value, payload) pairs are interchangeable).  With label_bits > 0 the payload split of gnnlm_ivfpq_split_payload is
 * part of the store: out_id gets payload >> label_bits, out_vals (optional, [n, k]) payload & (2^label_bits - 1), padding slots
 * id -1 and val_last; label_bits = 0 stores the payloads as they are. */
typedef struct gnnlm_ivfpq_select_final {
    const float* cand_val;  int64_t ld_val;   /* [n, cap] */
    const int64_t* cand_id;  int64_t ld_id;   /* [n, cap] */
    const int32_t* row_ncols;                 /* optional [n] */
    int64_t n;  int32_t cap;  int32_t k;
    float* out_val;  int64_t* out_id;         /* [n, k] */
    int32_t label_bits;  int32_t val_last;  int32_t* out_vals;
} gnnlm_ivfpq_select_final_t;
int gnnlm_ivfpq_select_final(const gnnlm_ivfpq_select_final_t* desc, void* stream);
typedef struct gnnlm_ivfpq_rescore {
    const uint8_t* codes;  const int64_t* payload;    /* [N, M] list-ordered codes, [N] what a candidate carries (key id, or id << 24 | label) */
    int32_t M;                                        /* 64 */
    const float* lut;  int64_t ld_lut;                /* [n, M * 256] f32 */
    const float* coarse;  int64_t ld_coarse;
    const float* tau;
    const uint32_t* surv;  const int32_t* surv_cnt;  int32_t cap;
    int64_t n;
    float* cand_val;  int64_t* cand_id;  int32_t* cand_cnt;  int32_t cand_cap;
    /* ABI 10: with `qmeta` (k > 0) a tighter threshold from the survivors themselves, in the same launch ahead of the re-score and
     * under the arrival of the query's table.  A survivor record is {row, list | sum_u << 18} with sum_u the key's integer sum
     * (16383: more than the filter's staging could hold): a lower bound of the key's score over ALL probed lists.
     * tau[q] <- max(tau[q], the k-th largest lower bound of query q's survivors) (at least k keys score above it), the records
     * whose upper bound cannot exceed it are dropped: surv is compacted in place, tau raised in place (both are written through
     * these pointers), out_cnt [n, 16] int32 (column 0; optional) = records left; surv_cnt stays what the filter counted.  The
     * search result does not change.  NULL: the re-score alone. */
    const float* qmeta;  int32_t k;  int32_t* out_cnt;
} gnnlm_ivfpq_rescore_t;
int gnnlm_ivfpq_rescore(const gnnlm_ivfpq_rescore_t* desc, void* stream);
/* Added within ABI 12 (additive: two new entries and structs).  ADDING keys to an index (faiss `add_with_ids` behind
 * knn/index_builder.py:97-109), csrc/ivfpq_add.hip.
 *
 * gnnlm_ivfpq_encode_rows: the residual PQ codes of rows whose list is known.  x [n, d] are the ROTATED rows (row stride ldx),
 * assign [n] the list of each row, coarse [nlist, d] contiguous, pq [M, 256, dsub], norm2 [M, 256] = |p_mc|^2, d = M * dsub:
 *     codes[r][m] = argmin_c ( norm2[m][c] - 2 * dot ),  dot = the fmaf chain from 0 over e = 0 .. dsub - 1 (ascending) of
 *                   (x[r][m dsub + e] - coarse[assign[r]][m dsub + e]) * pq[m][c][e]
 * with the residual rounded to float32 once and ties going to the lowest c (no c below +inf: 0) -- gnnlm_pq_encode's arithmetic
 * on the materialised residual, so the two agree bit for bit.  codes [n, M] u8 with row stride ld_codes.  list_cnt [nlist]
 * (optional) is INCREMENTED by one per encoded row (integer atomics: the result does not depend on order), n_bad (optional) by one
 * per row whose assign lies outside [0, nlist): such a row is skipped, its codes stay as they were, nothing out of range is read.
 * Refused with nothing written: M % 16 != 0, dsub % 4 != 0, d != M * dsub, negative sizes, and with n > 0 null operands or row
 * strides shorter than the rows.  n = 0 touches nothing.  Rows are addressed with 64 bits.  One launch, no allocation, no sync. */
typedef struct gnnlm_ivfpq_encode {
    const float* x;  int64_t ldx;  int64_t n;
    const int64_t* assign;
    const float* coarse;  int32_t nlist;
    const float* pq;  const float* norm2;
    int32_t M;  int32_t dsub;  int32_t d;
    uint8_t* codes;  int64_t ld_codes;
    int64_t* list_cnt;  int32_t* n_bad;
} gnnlm_ivfpq_encode_t;
int gnnlm_ivfpq_encode_rows(const gnnlm_ivfpq_encode_t* desc, void* stream);
/* gnnlm_ivfpq_list_merge: new rows filed behind the old rows of their lists.  Old index: list_off_old [nlist + 1], ids_old [N0],
 * codes_old [N0, M]; new rows: dest [n] (position in the merged arrays), ids_new [n], codes_new [n, M] (row stride ld_new);
 * new_off [nlist + 1] the merged offsets.  Old row j of list l lands at new_off[l] + (j - list_off_old[l]) (a list's old rows move
 * as one run), new row i at dest[i]; ids [N0 + n] and codes [N0 + n, M] are buffers of their own.  A position outside
 * [0, N0 + n) is skipped and counted in n_bad (optional).  M % 16 == 0, codes_old and codes 16-byte aligned; all byte offsets are
 * 64-bit.  One launch, no allocation, no sync; N0 = 0, n = 0 and empty lists are valid. */
typedef struct gnnlm_ivfpq_list_merge {
    const int64_t* list_off_old;  int32_t nlist;  int64_t N0;
    const int64_t* ids_old;  const uint8_t* codes_old;  int32_t M;
    int64_t n;  const int64_t* dest;  const int64_t* ids_new;  const uint8_t* codes_new;  int64_t ld_new;
    const int64_t* new_off;
    int64_t* ids;  uint8_t* codes;
    int32_t* n_bad;
} gnnlm_ivfpq_list_merge_t;
int gnnlm_ivfpq_list_merge(const gnnlm_ivfpq_list_merge_t* desc, void* stream);
/* Added within ABI 12 (additive: one entry and struct).  The COARSE step of an index with many lists without the [n, nlist] score
 * matrix, csrc/ivfpq_coarse.hip: the k <= 64 best lists of every row of x [n, d] (row stride ldx) among coarse [nlist, d]
 * (contiguous, 16-byte aligned), value = <x_r, c_l> (+ col_bias[l], optional), id = l.  The contract is that of
 * gnnlm_ivfpq_select_probes applied to gnnlm_gemm_nt(x, coarse): out_val / out_id [n, k] best first, ties to the lower list, a list
 * whose biased score is NaN or -inf is no entry, rows with fewer than k entries are padded with (-inf, -1).  The dot products are
 * taken on the f32 matrix instruction (v_mfma_f32_16x16x4_f32), accumulated along ascending dimension from 0, the bias added after
 * the sum is complete (one rounding each): on operands whose sums are exact in float32 the result equals the two-step route bit for
 * bit; otherwise values differ from it in the last bits, as two GEMM routes do.
 * The lists are cut into `slabs` >= 1 runs of ceil(nlist / slabs) rounded up to 64; a workgroup holds 64 rows and streams one
 * slab through LDS, every row keeping the k best of its slab on chip.  slabs == 1: the result goes straight to out_val / out_id.
 * slabs > 1: part_val [n, slabs, k] f32 and part_id [n, slabs, k] i64 (the caller's buffers) take the slabs' lists and
 * gnnlm_topk_merge (ids = part_id, slabs * k <= 4096 columns) folds them: two launches.  No allocation, no sync.
 * Refused with nothing written: k outside [1, 64], d <= 0 or d % 4 != 0, negative n / nlist, slabs outside [1, 4096 / k], ldx < d,
 * and with n > 0: a null or host pointer among x, out_val, out_id, (nlist > 0) coarse, (given) col_bias, (slabs > 1) part_val /
 * part_id, or a misaligned coarse.  n = 0 touches nothing; nlist = 0 writes the padding. */
typedef struct gnnlm_ivfpq_coarse {
    const float* x;  int64_t ldx;  int64_t n;
    const float* coarse;  int32_t nlist;  int32_t d;
    const float* col_bias;
    int32_t k;  int32_t slabs;
    float* part_val;  int64_t* part_id;
    float* out_val;  int64_t* out_id;
} gnnlm_ivfpq_coarse_t;
int gnnlm_ivfpq_coarse_probes(const gnnlm_ivfpq_coarse_t* desc, void* stream);
/* Added within ABI 12 (additive: two structs, three entries).  REMOVING keys from an index (faiss `remove_ids`), csrc/ivfpq_remove.hip.
 * Ids are datastore rows, so the ids of the remaining keys and the label table stay as they are: only the three list arrays shrink.
 * Both entries only enqueue (no allocation, no sync), address rows and bytes with 64 bits, and refuse bad shapes with
 * GNNLM_E_INVALID and nothing written.
 *
 * gnnlm_ivfpq_keep_flags: which rows survive.  ids [N] are the index's list_ids, list_off [nlist + 1] its offsets, ranges a DEVICE
 * array [n_ranges][2] of half-open id ranges [lo, hi), sorted by lo, pairwise disjoint, lo < hi (one id: [id, id + 1)).
 * keep[s] = 0 if some range holds ids[s], else 1 (bisection of the ranges); list_keep [nlist] (optional) = survivors per list,
 * WRITTEN, not incremented (zeroed by a launch of its own, then integer atomics: no dependence on launch order).  n_ranges = 0 keeps
 * everything; ids that the index does not hold are no error; ranges that break the precondition give unspecified flags and never an
 * access outside the arrays.  N = 0 writes list_keep = 0 and nothing else; nlist = 0 (with N = 0) touches nothing.  Refused:
 * negative sizes, N > 0 with nlist = 0 or a null ids / list_off / keep, n_ranges > 0 with null ranges. */
typedef struct gnnlm_ivfpq_keep_flags {
    const int64_t* ids;  int64_t N;
    const int64_t* list_off;  int32_t nlist;
    const int64_t* ranges;  int64_t n_ranges;
    uint8_t* keep;  int64_t* list_keep;
} gnnlm_ivfpq_keep_flags_t;
int gnnlm_ivfpq_keep_flags(const gnnlm_ivfpq_keep_flags_t* desc, void* stream);
/* gnnlm_ivfpq_list_compact: the surviving rows (keep[s] != 0) of list_off_old [nlist + 1], ids_old [N0], codes_old [N0, M] into ids
 * and codes, buffers of their own with at least new_off[nlist] rows; new_off [nlist + 1] is the cumulative sum of list_keep, made by
 * the caller.  The survivor of list l with r survivors of that list ahead of it lands at new_off[l] + r: order inside a list and the
 * order of the lists are kept; rows from new_off[nlist] on are not touched.  A list whose survivor count differs from
 * new_off[l + 1] - new_off[l] is counted once in n_bad (optional) and writes nothing outside [new_off[l], new_off[l + 1]).  The
 * result is a pure function of the inputs (no dependence on the grid, on other work or on list lengths): the positions come from a
 * scan in separate launches over chunks of 1024 rows (count, one-workgroup scan of the counts, scatter), never from one workgroup
 * waiting for another.  `workspace`: gnnlm_ivfpq_list_compact_workspace_bytes(N0, nlist) bytes of device memory, 8-byte aligned,
 * contents free.  M % 16 == 0, codes_old and codes 16-byte aligned (rows move as 16-byte pieces, ids as 8 bytes).  N0 = 0 touches
 * nothing.  Refused: M % 16 != 0, negative sizes, N0 > 0 with nlist = 0, and with N0 > 0 a null operand, a misaligned codes pointer,
 * an output that is an input, or a workspace that is null, misaligned or too small. */
typedef struct gnnlm_ivfpq_list_compact {
    const int64_t* list_off_old;  int32_t nlist;  int64_t N0;
    const int64_t* ids_old;  const uint8_t* codes_old;  int32_t M;
    const uint8_t* keep;
    const int64_t* new_off;
    int64_t* ids;  uint8_t* codes;
    int32_t* n_bad;
    void* workspace;  size_t workspace_bytes;
} gnnlm_ivfpq_list_compact_t;
size_t gnnlm_ivfpq_list_compact_workspace_bytes(int64_t N0, int32_t nlist);
int gnnlm_ivfpq_list_compact(const gnnlm_ivfpq_list_compact_t* desc, void* stream);

/* out[0] += sum_i x[i] * (mask ? mask[i] != 0 : 1), accumulated in f64 (score_sum of
 * fairseq_cli/eval_lm.py:273; the reference accumulates in f32 on the CPU) */
int gnnlm_masked_sum_f64(const float* x, const uint8_t* mask, int64_t n, double* out, void* stream);
/* out[g] += sum_i x[g * ld + i], i < n, for the `rows` rows of a matrix (ld >= n), accumulated in f64: the score_sum of every
 * point of a gnnlm_knn_interp_grid result in ONE launch.  Each row is added up in gnnlm_masked_sum_f64's order, so out[g]
 * equals what that call gives for the row, bit for bit. */
int gnnlm_rows_sum_f64(const float* x, int64_t ld, int64_t rows, int64_t n, double* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * HGT forward over the implicit token/neighbour graph
 * (TokenGraphTransformerDecoder.extract_graph_features fairseq/models/transformer.py:1011-1053,
 *  HGT.forward fairseq/models/hgt.py:494-513, HGTLayer.forward :299-420).
 * Weights are PREPARED (folded) tensors, see gnnlm_amd/hgt.py::prepare_hgt_weights and DESIGN.md.
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnlm_hgt_layer {
    /* node type tgt */
    const float *wq_t, *bq_t, *wk_t, *bk_t, *wv_t, *bv_t, *wa_t, *ba_t, *ln_g_t, *ln_b_t;
    /* star edge, absorbed: wku [H, din, dk], wvz_t [H, dk, din], bvz [d] */
    const float *wku, *wvz_t, *bvz;
    int32_t din;
    /* node type ntgt (NULL in the last layer unless ntgt outputs are requested) */
    const float *wq_n, *bq_n, *wk_n, *bk_n, *wv_n, *bv_n, *wa_n, *ba_n, *ln_g_n, *ln_b_n;
    /* ABI 4, layer 0 only, optional (all six or none): the ntgt projections with the OPQ rotation folded in -- [d, M*dsub]
     * weights W' = W . A^T and biases b' = b + W . opq_nba that read the DECODED rows; the rotation (x - b) A itself is then
     * only computed for the rows whose residual the layer needs */
    const float *wq_n0, *bq_n0, *wk_n0, *bk_n0, *wv_n0, *bv_n0;
} gnnlm_hgt_layer_t;

typedef struct gnnlm_hgt {
    int32_t d, n_heads, n_layers, left, right, max_intra_context;
    float ln_eps;
    int32_t M, dsub;
    const float* centroids;    /* [M, 256, dsub] */
    const float* opq_at;       /* [d, M*dsub] = A^T, NULL if the codec has no pre-transform */
    const float* opq_nba;      /* [d] = -(b . A), NULL if no b */
    const uint8_t* codes;  const void* vals;  int32_t vals_itemsize;
    int64_t n_store, row0, n_local;
    const gnnlm_hgt_layer_t* layers;   /* HOST array [n_layers] */
    int32_t gemm_precision;    /* precision of the GEMMs (see gnnlm_gemm_t.precision); 0 = exact f32, 3 = fp16 operands
                                  (`eval_lm --fp16`; attention, LayerNorm and everything that is not a GEMM stay f32) */
    const gnnlm_shards_t* shards;  /* ABI 4 (DEVICE pointer): the code table is this set of mapped shards instead of `codes` */
    /* Appended within ABI 12 (additive: members at the end, zero = off).  `--reinit-nfeat` (language_modeling.py:151-153,
     * transformer.py:1046-1048): the ntgt features are rows of the token-embedding table, x(r) = token_embed[vals[r]], instead of
     * decoded PQ codes.  With token_embed set the codec fields (M, dsub, centroids, opq_*, codes, shards, row0, n_local) are not
     * read, layer 0's `din` is d, `vals` (the whole label table, [n_store]) is required, and fetched codes / the row-keyed K / V
     * of ABI 11 are not available.  Layer 0's star edges read the table through gnnlm_neighbor_labels (no [n_slots, d] buffer
     * for a one-layer model, whose workspace is then no larger than on a code store when k_g <= d, and n_tok * k_g * 4 bytes
     * larger otherwise); the ntgt pipeline starts from gnnlm_token_gather.  Group merge, the centre-state cache and the
     * ragged entry work as for a code store. */
    const float* token_embed;  int64_t ld_token_embed;  int32_t n_vocab;
} gnnlm_hgt_t;

typedef struct gnnlm_hgt_io {
    int32_t n_blocks, T, kg;   /* n_blocks independent blocks of T tokens (causal attention stays inside a block) */
    const float* tgt_feats;    /* [n_blocks*T, d] f32 */
    const int64_t* ids;        /* [n_blocks*T, kg] neighbour rows, -1 = none */
    const uint8_t* fetched_codes;   /* optional [n_blocks*T*kg*(1+l+r), M]: slots already fetched (sharded store) */
    const uint8_t* fetched_valid;   /* with fetched_codes: [n_slots] */
    const int32_t* fetched_index;   /* optional: slot s lives in row fetched_index[s] of fetched_codes (the exchange
                                       returns rows bucketed by owner; the permutation is applied by the consumer) */
    int32_t fetched_centres_only;   /* 1: fetched_* hold only the centre slot of each group ([n_blocks*T*kg, M]);
                                       legal only when no ntgt update is needed (n_layers == 1, out_ntgt == NULL) */
    float* out_tgt;            /* [n_blocks*T, d] */
    float* out_ntgt;           /* optional [n_slots, d]: last layer's ntgt states (API parity / tests) */
    uint8_t* out_valid;        /* optional [n_slots] */
    /* ABI 3.  Layer-0 ntgt states given densely instead of as PQ codes: [n_slots, d] rows (row stride ld_ntgt) with
     * their validity bytes [n_slots] -- what HGT.forward has after its input adapters
     * (`F.gelu(adapt_ws[ntype](feat))` when in_dim != hidden_dim, fairseq/models/hgt.py:476-479,505-507), where the
     * decoded features pass a non-linearity and cannot be folded into the star-edge weights.  The code store is then
     * not read; layer 0's `din` must be d. */
    const float* ntgt_feats;  int64_t ld_ntgt;
    const uint8_t* ntgt_valid;
    /* ABI 6, optional: exact de-duplication of context groups (the reference's own "todo: merge same nodes",
     * fairseq/data/token_block_dataset.py:355).  A group's ntgt states depend on its centre row only (ntgt nodes never
     * receive from tgt nodes), so the ntgt pipeline of every layer runs once per DISTINCT centre row of the batch:
     * group_ids [n_unique] the distinct valid rows, group_index [n_blocks*T*kg] the group of neighbour (i, j) (-1: not a
     * neighbour).  Results are those of the un-merged graph.  Not with ntgt_feats / out_ntgt / out_valid.
     * ABI 9: with fetched_codes (sharded store) the fetched_* arrays describe the slots of the GROUPS -- slot g * (1+l+r) + c
     * of group g -- i.e. only the distinct centre rows of the batch were requested from their owners. */
    const int64_t* group_ids;  int64_t n_unique;  const int32_t* group_index;
    /* ABI 7, optional, with group_ids: a CROSS-BATCH cache of the centre states.  The star edges of layer l >= 1 read the
     * centre slot of a group after l ntgt updates, and that state is a function of the centre row alone (fixed weights and
     * store) -- so it is kept between calls: state_cache [n_layers - 1][cache_cap][d] f32, owned by the caller, who also owns
     * the row -> slot map.  Then group_ids / n_unique name only the groups the cache does NOT hold yet (the ntgt pipeline runs
     * over those and their centre states are written to slots group_slot [n_unique]), and group_index [n_blocks*T*kg] holds
     * the cache SLOT of neighbour (i, j) (-1: not a neighbour), new and old alike.  Same kernels, same per-row arithmetic:
     * the result is that of the un-cached call. */
    float* state_cache;  int64_t cache_cap;  const int32_t* group_slot;
    /* ABI 9, optional, with group_ids: the number of groups lives on the DEVICE (int32, written by gnnlm_group_assign on the
     * same stream) -- `n_unique` is then the CAPACITY of group_ids / group_slot (the worst case: every neighbour its own
     * group), which sizes the workspace and the launches; every kernel of the ntgt pipeline reads the count itself, so the
     * caller never synchronises and the call can be captured into a HIP graph. */
    const int32_t* n_unique_dev;
    /* ABI 9, optional, with state_cache and fetched_codes (sharded store): [cache_cap, M] code rows of the cached centres.
     * Layer 0's star edges read the PQ code of EVERY neighbour; with a sharded store only the groups the cache lacks are
     * fetched, so the code row of a centre is kept beside its states (128 B per slot). */
    uint8_t* code_cache;
    /* ABI 11 (optional): layer 0's K / V projections of the ntgt slots keyed by datastore ROW.  A slot's layer-0 K and V are a
     * function of its code row alone, and neighbouring context groups share rows (a group is the window [o - left, o + right]
     * of its centre, token_block_dataset.py:378-400: centres p and p + 1 share 4 of 5 rows -- what consecutive tokens of real
     * kNN-LM retrieval produce).  With `row_table` (DEVICE int32[n_store], all -1 between calls, owned by the caller; needs
     * group_ids and a local or mapped code store) the distinct slot rows of the batch are found on the device
     * (gnnlm_group_assign's claim pass over the slots' rows), decoded and projected ONCE, and the chain attention reads K / V
     * through the slot -> row map.  Same kernels per row: the output is bit-identical. */
    int32_t* row_table;
} gnnlm_hgt_io_t;

/* ------------------------------------------------------------------------------------------------
 * ABI 9.  Group assignment on the device: which DISTINCT centre rows of a batch have to be computed, and where every
 * neighbour finds its group -- what `torch.unique` + a host round trip did before.  No sort, no synchronisation:
 * `slot_of` is a direct row -> slot table (int32 per datastore row, -1 = none, owned by the caller, persistent) claimed
 * with atomicCAS; new groups are appended to group_ids through a device counter in ARRIVAL order (per-row arithmetic
 * does not depend on the position of a row, so results are bit-identical whatever the order).
 *   merge mode (cache_cap == 0): group_ids = the distinct valid rows of `ids`, group_index[e] = position of neighbour e's
 *       row in group_ids (-1: not a neighbour); slot_of is returned clean (all -1).
 *   cache mode (cache_cap > 0): slots are those of a two-generation cache of capacity cache_cap (halves [0, cap/2) and
 *       [cap/2, cap)); group_ids = the rows the cache lacks, group_slot their new slots, group_index[e] = cache slot of
 *       neighbour e.  When the half being filled has no room for the batch's new rows the OTHER half is emptied and
 *       becomes the one being filled (rows this batch found there are computed again); the caller guarantees
 *       n <= cache_cap / 2 so that a fresh half always has room.  cache_state (DEVICE int32[8], zero-initialised by the
 *       caller once): [0] half being filled, [1] / [2] entries of the halves, [3] generation switches, [4] rows computed so far (low 31 bits).
 * counters (DEVICE int32[4], written): [0] = number of groups (pass it as gnnlm_hgt_io_t.n_unique_dev), [1] = 1 if the
 * generation was switched by this call.  group_ids entries beyond the count are -1.
 * Replaces: nothing in the reference (its graph repeats equal nodes, token_block_dataset.py:355 "todo: merge same nodes").
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnlm_group_assign {
    const int64_t* ids;  int64_t n;      /* neighbour rows of the batch; < 0 or >= n_store: not a neighbour */
    int64_t n_store;
    int32_t* slot_of;                    /* [n_store] */
    int64_t* id_of_slot;                 /* cache mode: [cache_cap] row held by each slot */
    int32_t* cache_state;                /* cache mode: DEVICE int32[8] */
    int64_t cache_cap;
    int64_t* group_ids;                  /* out [n] */
    int32_t* group_slot;                 /* out [n], cache mode */
    int32_t* group_index;                /* out [n] */
    int32_t* counters;                   /* out DEVICE int32[4] */
} gnnlm_group_assign_t;
int gnnlm_group_assign(const gnnlm_group_assign_t* desc, void* stream);

/* x = gelu(x) in place, the exact (erf) form of torch.nn.functional.gelu (input adapters of HGT, hgt.py:507) */
int gnnlm_gelu(float* x, int64_t n, void* stream);
size_t gnnlm_hgt_workspace_bytes(const gnnlm_hgt_t* model, const gnnlm_hgt_io_t* io);
int gnnlm_hgt_forward(const gnnlm_hgt_t* model, const gnnlm_hgt_io_t* io, void* workspace,
                      size_t workspace_bytes, void* stream);
/* The same forward for a RAGGED batch (gnnlm_ragged_t above): `io` describes the packed tokens as ONE run -- io->n_blocks = 1,
 * io->T = blocks->n_tok, every per-token / per-slot array of io sized by that count -- and `blocks` cuts it into the blocks the
 * causal ('tgt','intra','tgt') attention stays inside.  Everything else of the step is per token or per slot and runs as in
 * gnnlm_hgt_forward (group merge, row-keyed layer-0 K / V, centre-state cache, fetched_* included); the causal branch is
 * gnnlm_causal_attn_varlen, so the workspace has no [n_blocks, H, T, T] score and no V^T buffer.  d / n_heads must be one of
 * the d_k that kernel is built for. */
size_t gnnlm_hgt_workspace_bytes_ragged(const gnnlm_hgt_t* model, const gnnlm_hgt_io_t* io, const gnnlm_ragged_t* blocks);
int gnnlm_hgt_forward_ragged(const gnnlm_hgt_t* model, const gnnlm_hgt_io_t* io, const gnnlm_ragged_t* blocks, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Base transformer LM: the decoder whose features the whole pipeline starts from ({split}_dstore/keys.npy, the kNN keys and
 * queries).  Additive to ABI 12: new structs and new entries, no existing member moved.
 * Replaces: TransformerDecoder.extract_features (fairseq/models/transformer.py:700-841) over
 *           TransformerDecoderLayer.forward (fairseq/modules/transformer_layer.py:223-331) for a decoder-only language model
 *           (no encoder attention, decoder_normalize_before = True: transformer_lm.py:225) in eval mode (dropout and
 *           layer-drop are the identity).  Samples are PACKED blocks (gnnlm_ragged_t): no padding, no padding mask.
 * ---------------------------------------------------------------------------------------------- */
/* x[r, :] = fl32(fl32(scale * E[tok[r], :]) + P[pad_idx + 1 + (r - block_off[b]), :]) for packed row r of block b: the token
 * embedding times embed_scale, then the positional embedding of the row's position in its own block, rounded twice as
 * transformer.py:753-759 does (no fused multiply-add).  P is the position table [p_rows, d] -- the sinusoidal one built on the
 * host as SinusoidalPositionalEmbedding.get_embedding does (sinusoidal_positional_embedding.py:36-60), or the learned
 * embed_positions.weight -- or NULL (no_token_positional_embeddings: x = fl32(scale * E[tok])).  One wave per row, 16-byte
 * loads and stores: d % 4 == 0, ld_e, ld_p, ldo multiples of 4, E / P / out 16-byte aligned.
 * A token id outside [0, n_vocab) is never followed: its row is written as zeros and counted in *n_bad (optional DEVICE int32,
 * added to; the caller zeroes it), and so is a row whose position lies beyond the table (memory safety only, see max_len).
 * `max_len` is HOST data, the longest block of the call (the lengths are host-known, as for gnnlm_ragged_tiles): with P,
 * pad_idx + 1 + max_len > p_rows is refused with GNNLM_E_INVALID before anything is launched.  blocks->tiles is not read. */
typedef struct gnnlm_lm_embed {
    const int64_t* tokens;     /* [n_tok] */
    const float* E;  int64_t ld_e;  int32_t n_vocab, d;   /* [n_vocab, d] (gnnlm_amd.token_embed) */
    const float* P;  int64_t ld_p, p_rows;                /* optional [p_rows, d] */
    int32_t pad_idx;
    float scale;               /* sqrt(d), or 1 with no_scale_embedding; used as given (0 is 0) */
    int64_t max_len;           /* HOST: the longest block */
    float* out;  int64_t ldo;  /* [n_tok, d] */
    int32_t* n_bad;            /* optional DEVICE int32 */
} gnnlm_lm_embed_t;
int gnnlm_lm_embed(const gnnlm_lm_embed_t* desc, const gnnlm_ragged_t* blocks, void* stream);

/* x = max(x, 0) in place (activation_fn relu of the feed-forward block, transformer_layer.py:311; a NaN stays a NaN, as
 * torch.relu).  gnnlm_gemm_nt's store epilogue has no activation: at 4 * ffn bytes per token and layer beside 4 * d * ffn
 * flops of GEMM an in-place pass is the right size. */
int gnnlm_relu(float* x, int64_t n, void* stream);

typedef struct gnnlm_tlm_layer {
    const float *ln1_g, *ln1_b;            /* self_attn_layer_norm [d] */
    const float *wqkv, *bqkv;              /* [3d, d], [3d]: q | k | v rows (in_proj_weight, or q_proj / k_proj / v_proj concatenated) */
    const float *wo, *bo;                  /* self_attn.out_proj [d, d], [d] */
    const float *ln2_g, *ln2_b;            /* final_layer_norm [d] */
    const float *w1, *b1, *w2, *b2;        /* fc1 [ffn, d], [ffn]; fc2 [d, ffn], [d] */
} gnnlm_tlm_layer_t;

/* The d_k^-0.5 of `q *= self.scaling` (multihead_attention.py) is FOLDED into the q rows of wqkv and bqkv by whoever
 * prepares the weights (gnnlm_amd.transformer_lm): the orchestrator applies no scaling.  The fold is exact when d_k is a power of
 * 4 (16, 64: a power of two) and one extra float32 rounding of the q weights otherwise (32, 128) -- inside the 5e-5 feature bar. */
typedef struct gnnlm_tlm {
    int32_t L, d, H, ffn;
    int32_t act, precision;    /* act: 0 relu, 1 gelu (the exact erf form).  precision: of every GEMM, as gnnlm_gemm_t.precision (0 f32,
                                  1 / 2 split-bf16, 3 fp16 operands with f32 accumulation); attention, LayerNorm and the embed stay f32 */
    float ln_eps;              /* 0 is read as 1e-5 */
    float scale;               /* embed_scale */
    const float* E;  int64_t ld_e;  int32_t n_vocab, pad_idx;
    const float* P;  int64_t ld_p, p_rows;                /* optional position table (gnnlm_lm_embed_t) */
    const float *ln_emb_g, *ln_emb_b;      /* optional layernorm_embedding (both or none) */
    const float *ln_out_g, *ln_out_b;      /* optional final layer_norm (both or none) */
    const gnnlm_tlm_layer_t* layers;       /* HOST array [L] */
} gnnlm_tlm_t;

typedef struct gnnlm_tlm_io {
    const int64_t* tokens;     /* [n_tok] source tokens of the packed blocks */
    gnnlm_ragged_t blocks;     /* block_off and tiles (gnnlm_ragged_tiles) */
    int64_t max_len;           /* HOST: the longest block (checked against the position table) */
    float* out;                /* [n_tok, d]: the features, after the final layer_norm when there is one */
    float* last_inner;         /* optional [n_tok, d]: inner_states[-1], before the final layer_norm */
    float* last_ffn_input;     /* optional [n_tok, d]: the last layer's final_layer_norm output (transformer_layer.py:309-310) */
    int32_t* n_bad;            /* optional DEVICE int32: token ids outside [0, n_vocab), added to (gnnlm_lm_embed_t) */
} gnnlm_tlm_io_t;
/* Per layer: LayerNorm, ONE q|k|v GEMM [n_tok, 3d], gnnlm_causal_attn_varlen, out-projection GEMM with bias and the residual as R
 * (in place), LayerNorm, fc1 GEMM + bias, the activation in place, fc2 GEMM + bias + residual.  Only enqueues on `stream`: no
 * allocation, no synchronisation.  GNNLM_E_INVALID before anything is launched or written: L < 1, d / H outside {16, 32, 64, 128},
 * H * d_k != d, d or ffn not a positive multiple of 4, act outside 0..1, precision outside 0..3, a NULL tokens / out / E / layers or
 * layer member, half a LayerNorm pair, n_tok >= 2^31, what gnnlm_lm_embed refuses, a NULL or too small workspace.  n_tok = 0 is
 * accepted and touches nothing.  gnnlm_transformer_lm_workspace_bytes: n_tok * (3 d + max(3 d, ffn)) floats plus alignment. */
size_t gnnlm_transformer_lm_workspace_bytes(const gnnlm_tlm_t* model, const gnnlm_tlm_io_t* io);
int gnnlm_transformer_lm_forward(const gnnlm_tlm_t* model, const gnnlm_tlm_io_t* io, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Incremental decoding of the base transformer LM: a K/V cache, the attention of ONE new row per sequence against it, the
 * prefill and the step that use them, and the pick of the next token.  Additive to ABI 12: new structs and new entries.
 * Replaces: the incremental_state branches of MultiheadAttention.forward (fairseq/modules/multihead_attention.py: saved
 *           prev_key / prev_value, concatenated with the new row) under TransformerDecoder.extract_features(...,
 *           incremental_state=) (fairseq/models/transformer.py:739-750, which keeps the last token only), and the sampling step
 *           of fairseq/search.py:231-265.
 * ---------------------------------------------------------------------------------------------- */
/* The cache is a DESCRIPTOR over caller-owned memory: nothing here allocates.  k and v are f32 [L][B][cap][d]: row u of sequence
 * b in layer l starts at l * ld_layer + b * ld_seq + u * ld_row, holds K' (V') of the H heads side by side (head h at columns
 * h * d_k ..), and is valid for u < len[b].  ld_row >= d, ld_seq >= cap * ld_row, ld_layer >= B * ld_seq, all multiples of 4; k
 * and v 16-byte aligned.  len / done / n_bad live on the DEVICE: a kernel reads them when it runs, so a captured graph follows
 * them from replay to replay.  A len[b] outside [0, cap) cannot be verified against the memory: the row is counted in *n_bad
 * (added to; the caller zeroes it) and never followed -- nothing of sequence b is read or written. */
#define GNNLM_DECODE_CHUNK 128            /* keys of one (b, h) that one wave takes: the unit of the split, fixed */
typedef struct gnnlm_kv_cache {
    float *k, *v;                         /* [L][B][cap][d] */
    int64_t ld_row, ld_seq, ld_layer;     /* in floats */
    int32_t L, B, cap, d;
    int32_t* len;                         /* DEVICE [B]: keys held per sequence */
    int32_t* done;                        /* optional DEVICE [B]: != 0 = the sequence has ended */
    int32_t* n_bad;                       /* optional DEVICE int32: rows whose len is outside [0, cap), added to */
} gnnlm_kv_cache_t;

/* One layer, one new row per sequence.  For every row b with done[b] == 0 and 0 <= len[b] < cap:
 *   cache row len[b] of layer `layer` := k_new[b], v_new[b]   (bit for bit; no other cache byte is written)
 *   out[b, h*dk:(h+1)*dk] = sum_{u <= len[b]} softmax_u(q_bh . K_bhu) V_bhu
 * q is used as given (the d_k^-0.5 is folded into wqkv: gnnlm_tlm_t).  All maths in f32.  A done row appends nothing and gets a
 * zero out row; a row with len[b] outside [0, cap) appends nothing, gets zeros and is counted in *cache.n_bad (a done row is
 * not counted).  len is NOT changed: the caller advances it once all layers have run (gnnlm_transformer_lm_step does).
 * Split: the keys of one (b, h) are cut into chunks of GNNLM_DECODE_CHUNK; one wave takes one chunk -- K and V rows straight
 * into registers with 16-byte loads, every cached byte once, a running (maximum, sum, accumulator) per lane group, merged
 * inside the wave in a fixed order -- and stores its (maximum, sum, accumulator) in the workspace.  A second small launch
 * combines the chunks of a (b, h) in ascending chunk order and writes out.  No float atomics: out[b] depends only on len[b],
 * q[b], k_new[b], v_new[b] and the cache rows [0, len[b]) of b -- not on B, the other rows, cap or max_len -- and is the same bits
 * on every run.  Cache rows above len[b] are never read.
 * `max_len` is HOST data: an upper bound on len[b] + 1 over the rows that take part (it sizes the grid and the workspace; 0 is
 * read as cap).  A row with len[b] + 1 > max_len is treated as out of range (zeros, counted).
 * GNNLM_E_INVALID before anything is launched: dk outside {16, 32, 64, 128}, H < 1, H * dk != cache.d, layer outside [0, L),
 * B < 0, cap < 1, max_len outside [0, cap], a stride that is too small or no multiple of 4, a pointer that is NULL or not
 * 16-byte aligned, a workspace smaller than gnnlm_decode_attn_workspace_bytes.  B = 0 is accepted and touches nothing. */
typedef struct gnnlm_decode_attn {
    const float *q, *k_new, *v_new;  int64_t ld;     /* [B, H*dk] each, one row stride ld >= H*dk (the q | k | v GEMM output) */
    float* out;  int64_t ldo;                        /* [B, H*dk] */
    gnnlm_kv_cache_t cache;
    int32_t layer, H, dk;
    int32_t max_len;                                 /* HOST: len[b] + 1 <= max_len; 0 = cap */
    void* workspace;  size_t workspace_bytes;
} gnnlm_decode_attn_t;
/* B * H * ceil(max_len / GNNLM_DECODE_CHUNK) * (dk + 4) floats; for a descriptor with max_len = 0 pass cap */
size_t gnnlm_decode_attn_workspace_bytes(int32_t B, int32_t H, int32_t dk, int32_t max_len);
int gnnlm_decode_attn(const gnnlm_decode_attn_t* desc, void* stream);

/* gnnlm_transformer_lm_forward over packed prompts that also fills the cache: block b is sequence b.  After each layer's q|k|v
 * GEMM one copy kernel writes the K' and V' rows of block b to cache rows [0, len_b) of sequence b of that layer; a last tiny
 * launch sets len[b] = len_b.  done is not touched.  The forward itself enqueues exactly what gnnlm_transformer_lm_forward
 * enqueues, so `io`'s outputs are the same bits.  Workspace: gnnlm_transformer_lm_workspace_bytes.  Refused before anything is
 * launched, beyond what the forward refuses: io->blocks.n_blocks != cache->B, io->max_len > cache->cap (a block longer than
 * the cache; max_len is host-known), cache->d != model->d, cache->L != model->L, a cache that gnnlm_decode_attn would refuse.  A
 * block that turns out longer than io->max_len on the device is cut at io->max_len rows (memory safety only). */
int gnnlm_transformer_lm_prefill(const gnnlm_tlm_t* model, const gnnlm_tlm_io_t* io, const gnnlm_kv_cache_t* cache,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* One decoding step: token b is appended to sequence b.  x[b] = fl32(fl32(scale * E[tok[b]]) + P[pad_idx + 1 + len[b]]) (the two
 * roundings of gnnlm_lm_embed, the position read on the device; an id outside [0, n_vocab) or a len[b] outside [0, cap) gives a
 * zero row and is counted in *n_bad), then per layer LayerNorm, the q|k|v GEMM with M = B, gnnlm_decode_attn, the out-projection
 * with bias and residual, LayerNorm, fc1, the activation, fc2 with bias and residual; the optional final LayerNorm; and one last
 * tiny launch does len[b] += 1 for the rows that are not done and in range.  The rows of a done sequence are computed from
 * a zero attention output and mean nothing.
 * `max_len` is HOST data: an upper bound on len[b] + 1 over EVERY execution of the enqueued work -- for a captured graph, over
 * every replay.  max_len < 1, max_len > cache->cap and pad_idx + 1 + max_len > p_rows (with a position table) are refused before
 * anything is launched, as is everything gnnlm_transformer_lm_forward and gnnlm_decode_attn refuse.  The call only enqueues: no
 * allocation, no host read, no synchronisation -- it can be captured in a HIP graph. */
typedef struct gnnlm_tlm_step_io {
    const int64_t* tokens;     /* DEVICE [B] */
    int64_t max_len;           /* HOST */
    float* out;                /* [B, d] */
    float* last_inner;         /* optional [B, d] */
    float* last_ffn_input;     /* optional [B, d] */
    int32_t* n_bad;            /* optional DEVICE int32: token ids outside the vocabulary, added to */
} gnnlm_tlm_step_io_t;
size_t gnnlm_transformer_lm_step_workspace_bytes(const gnnlm_tlm_t* model, const gnnlm_kv_cache_t* cache, const gnnlm_tlm_step_io_t* io);
int gnnlm_transformer_lm_step(const gnnlm_tlm_t* model, const gnnlm_kv_cache_t* cache, const gnnlm_tlm_step_io_t* io,
                              void* workspace, size_t workspace_bytes, void* stream);

/* The next token of every row from its SORTED top-N (what gnnlm_topk_merge leaves: logp [B, N] best first, ids [B, N], N <= 2048).
 *   u == NULL: greedy, column 0.
 *   u given (DEVICE f32 [B], in [0, 1)): the smallest j with c_j > u[b] * c_{N-1}, c the inclusive prefix sum of
 *   exp(logp_j - logp_0) in float32 (association order unspecified).  A -inf (or NaN) entry contributes 0 and is never picked.
 *   This is probs = lprobs.topk(k).exp_(); torch.multinomial(probs, 1) of search.py:231-247 with the caller's random numbers.
 * next[b] = ids[b, j]; next_logp[b] (optional) = logp[b, j], the column's own value, not renormalised (search.py:258-265).
 * done (optional DEVICE int32 [B]): a done row gets next = pad and is otherwise untouched; a pick equal to eos sets done[b] = 1.
 * A row whose logp[b, 0] is not finite has nothing to pick from: next = pad, done = 1 (if given), counted in *n_bad (optional
 * DEVICE int32, added to); its next_logp is left alone.  One wave per row.
 * GNNLM_E_INVALID before anything is launched: N outside [1, 2048], B < 0, ld_logp / ld_ids < N, a NULL logp / ids / next.
 * B = 0 is accepted and touches nothing. */
typedef struct gnnlm_sample_topk {
    const float* logp;  int64_t ld_logp;  /* [B, N] */
    const int64_t* ids;  int64_t ld_ids;  /* [B, N] */
    int32_t B, N;
    const float* u;                       /* optional [B] */
    int64_t pad, eos;
    int64_t* next;                        /* [B] */
    float* next_logp;                     /* optional [B] */
    int32_t* done;                        /* optional [B] */
    int32_t* n_bad;                       /* optional */
} gnnlm_sample_topk_t;
int gnnlm_sample_topk(const gnnlm_sample_topk_t* desc, void* stream);

/* Nucleus (top-p) sampling over DENSE rows: the next token of every row from logp [B, V] float32 as gnnlm_adaptive_log_probs /
 * gnnlm_dense_log_probs / gnnlm_knn_mix_dense leave it -- search.Sampling._sample_topp and the draw of Sampling.step
 * (fairseq/search.py:174-217, 228-265) with the caller's random numbers.  Additive to ABI 12: a new struct and a new entry.
 * For a row lp[0 .. V) that is not done:
 *   mass     m_j = exp(lp_j) for a finite lp_j, 0 for -inf.  Nothing is renormalised and no maximum is subtracted: the reference
 *            compares cumsum(exp(lprobs)) with p in absolute terms (search.py:191-198), and a row need not sum to 1.
 *   bad      a row with a NaN, a +inf or no positive mass (no finite entry, or none whose exp is a positive float32) is bad:
 *            next = pad, done = 1 (if given), counted in *n_bad; next_logp, n_keep and keep_mass are left alone; the other rows
 *            of the call are unaffected.
 *   order    larger value first, then smaller id (gnnlm_topk_merge's and gnnlm_row_rank's rule; -0 equals +0).
 *   nucleus  c_i the inclusive prefix sums of the masses in that order, n_pos the number of finite entries:
 *            n = min(n_pos, 1 + #{i : c_i < topp}), the nucleus the first n entries of the order (mask = cumsum.lt(p) plus "one
 *            more word", search.py:198-205); of the entries equal to the n-th value those with the smallest ids are in.  topp is any
 *            value > 0, +inf included; at or above the row's mass, n = n_pos: sampling from the whole vocabulary.
 *   draw     in ascending id: the smallest id whose inclusive prefix sum of nucleus masses exceeds u[b] * S, S the nucleus mass;
 *            should u * S round up to S, the last member with mass.
 * next[b] = the id; next_logp[b] (optional) = lp[id], bit for bit, not renormalised (search.py:258-265); n_keep[b] (optional) = n;
 * keep_mass[b] (optional) = S.  done / eos / pad as in gnnlm_sample_topk: a done row gets next = pad and is otherwise untouched; a
 * pick equal to eos sets done[b] = 1.
 * One workgroup per row, one launch, no workspace, nothing read back: capturable.  A row's outputs are a function of its own lp, V,
 * topp and u alone -- not of B, ld, the pointer's alignment or what else runs: every sum is an integer sum of the masses in a
 * per-row fixed point, trunc(expf(lp_j) * 2^s) with 2^s chosen from the row's maximum so that V of them fit 63 bits.  Every sum that
 * is compared with topp or with u * S is within a relative E(V) = 2^-21 + 2^(2 ceil(log2 V) - 62) of its exact value (the prefix
 * sums of the draw: relative to S; 7.2e-7 at V = 2^20; csrc/sample_topp.hip derives it): where topp and u * S are further than
 * that from every prefix sum, n, the set and the id are those of the float64 restatement (tests/topp_ref.py).
 * Rows need 4-byte alignment only and ld >= V need not be a multiple of 4; nothing at or beyond column V is read.
 * GNNLM_E_INVALID before anything is launched: topp not > 0 (NaN), V outside [1, 2^24] (the bound above is 6.2e-5 there), B < 0,
 * ld < V, a NULL logp / u / next, a misaligned pointer.  B = 0 is accepted and touches nothing. */
typedef struct gnnlm_sample_topp {
    const float* logp;  int64_t ld;       /* [B, V], row stride ld */
    int32_t B, V;
    double topp;
    const float* u;                       /* DEVICE [B], in [0, 1) */
    int64_t pad, eos;
    int64_t* next;                        /* [B] */
    float* next_logp;                     /* optional [B] */
    int32_t* done;                        /* optional [B] */
    int32_t* n_bad;                       /* optional */
    int32_t* n_keep;                      /* optional [B] */
    float* keep_mass;                     /* optional [B] */
} gnnlm_sample_topp_t;
int gnnlm_sample_topp(const gnnlm_sample_topp_t* desc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Beam search on the K/V cache: the decode attention through a per-hypothesis table of cache slots, the step that uses it, and
 * the selection of the next hypotheses.  Additive to ABI 12: new structs and new entries; nothing above launches anything else.
 * Replaces: search.BeamSearch.step (fairseq/search.py:49-85), the selection half of SequenceGenerator._generate
 *           (fairseq/sequence_generator.py:359-497) and reorder_incremental_state (:266-271), which index-selects every layer's
 *           saved K and V by parent after every step.  Here a hypothesis is a cache sequence ("slot") s; its key row u lives in
 *           slot src[s][u], so a reorder copies 4 bytes per key and the keys of a shared prompt are held once.
 * ---------------------------------------------------------------------------------------------- */
/* gnnlm_decode_attn with the table: `a` exactly as gnnlm_decode_attn takes it (B = a.cache.B hypotheses), src DEVICE int32
 * [a.cache.B][ld_src], ld_src >= cache.cap.  For u < len[s] key row u of hypothesis s is row u of slot src[s][u]; the new row
 * len[s] is read from k_new / v_new and written to row len[s] of slot s ITSELF, exactly as gnnlm_decode_attn writes it.  Chunks,
 * lane groups, unroll, butterfly, the combine launch, the workspace size and the done / n_bad / max_len rules are those of
 * gnnlm_decode_attn: given the same q, len and the same key and value rows in the same u order, out[s] is the same bits as on a
 * contiguous cache.  A table entry outside [0, cache.B) at u < len[s] is never followed: the row gets zeros and is counted in
 * *n_bad (its new row is still appended).  Entries at u >= len[s] are never read.  Refused like gnnlm_decode_attn, and: src NULL
 * or not 4-byte aligned (with B > 0), ld_src < cache.cap. */
typedef struct gnnlm_beam_attn {
    gnnlm_decode_attn_t a;
    const int32_t* src;  int64_t ld_src;
} gnnlm_beam_attn_t;
int gnnlm_beam_attn(const gnnlm_beam_attn_t* desc, void* stream);

/* gnnlm_transformer_lm_step with gnnlm_beam_attn in place of gnnlm_decode_attn in every layer; everything else -- arguments,
 * workspace (gnnlm_transformer_lm_step_workspace_bytes), refusals, the launches around the attention -- is that entry's.  Only
 * enqueues. */
int gnnlm_transformer_lm_step_beam(const gnnlm_tlm_t* model, const gnnlm_kv_cache_t* cache, const gnnlm_tlm_step_io_t* io,
                                   const int32_t* src, int64_t ld_src, void* workspace, size_t workspace_bytes, void* stream);

/* One beam-search step of every sentence: one launch, one workgroup per sentence b; hypothesis j of b is slot b * beam + j.
 * Nothing is read back; every count lives on the device, so a captured step replays with fixed pointers.
 * A sentence with finished[b] != 0 (or t[b] outside [0, max_new]) is left untouched.  Otherwise, with t = t[b]:
 *   candidates  (j, c), j < beam_in, c < N: value fl32(score_in[b * beam + j] + cand_val[b * beam_in + j, c]) -- one float32 add,
 *               lprobs.add_(scores) -- token cand_id[b * beam_in + j, c].  Absent: cand_val not finite, or a sum that is not finite.
 *   order       value descending, then j ascending, then token ascending (the flat index order j * V + token; torch.topk leaves
 *               ties unspecified).  The first C = min(2 * beam, present) candidates are the step's.
 *   finalize    scanning the first min(beam, C) in order, a candidate whose token is eos is finalized while fin_n[b] < beam, into
 *               slot f = fin_n[b]++: fin_tok[b, f, 0 .. t] = its parent's tokens of steps 0 .. t - 1, then eos; fin_cum[b, f, 0 .. t]
 *               = the parent's cumulative scores, then the value; fin_len[b, f] = t + 1; fin_score[b, f] = the value (raw: the
 *               length normalisation is the host's).
 *   survive     the first beam candidates among the C whose token is not eos become hypotheses 0 .. beam - 1: next = token,
 *               parent = b * beam + j (the slot), score_out = value; the step is recorded as hist_tok / hist_par (j) / hist_score
 *               [b, t, .] (backpointers: a finalized hypothesis is read back along them).  Hypotheses beyond the survivors are
 *               dead: next = pad, score_out = -inf, parent = the slot itself -- all their later candidates are absent.
 *   table       (src_out given) with len = len[b * beam], for u < min(len, cap): src_out[b * beam + j][u] = src_in[parent][u]
 *               (beam_in == 1: src_in is not read, the entry is b * beam, the slot of the prompt); and if len < cap,
 *               src_out[b * beam + j][len] = b * beam + j.  src_in == src_out is allowed (a column is read whole before it is
 *               written), as is score_in == score_out.
 *   finish      if fin_n[b] == beam or t == max_new (where the host has left only eos): finished[b] = 1 and done[b * beam + j] = 1
 *               for every j.  Last, t[b] = t + 1.
 * GNNLM_E_INVALID before anything is launched: beam outside [1, 32], N < 2 * beam, beam_in not 1 or beam, beam_in * N > 8192
 * (the candidates of a sentence are held in 32 KB of LDS), B < 0, max_new < 0, ld_val / ld_id < N, a NULL cand_val / cand_id /
 * score_in / score_out / t / finished / len / done / next / parent / hist_* / fin_*, src_out with ld_src < cap or cap < 0 or
 * (beam_in == beam) without src_in, a misaligned pointer.  B = 0 is accepted and touches nothing. */
typedef struct gnnlm_beam_select {
    const float* cand_val;  int64_t ld_val;     /* [B * beam_in, N] sorted, as gnnlm_topk_merge leaves it */
    const int64_t* cand_id;  int64_t ld_id;     /* [B * beam_in, N] */
    int32_t B, beam, beam_in, N;
    int64_t eos, pad;
    int32_t max_new;                            /* steps are 0 .. max_new */
    int32_t cap;                                /* table columns: u < cap <= ld_src */
    const float* score_in;  float* score_out;   /* [B, beam]; beam_in == 1 reads column 0 only */
    int32_t* t;                                 /* DEVICE [B]: the step counter */
    int32_t* finished;                          /* DEVICE [B] */
    const int32_t* len;                         /* DEVICE [B * beam]: the cache's len (slot b * beam is read) */
    int32_t* done;                              /* DEVICE [B * beam]: the cache's done */
    int64_t* next;  int32_t* parent;            /* [B * beam] */
    const int32_t* src_in;  int32_t* src_out;  int64_t ld_src;   /* optional [B * beam][ld_src] */
    int64_t* hist_tok;  int32_t* hist_par;  float* hist_score;   /* [B][max_new + 1][beam] */
    int32_t* fin_n;                             /* DEVICE [B]: finalized hypotheses held */
    int64_t* fin_tok;  float* fin_cum;          /* [B][beam][max_new + 1] */
    int32_t* fin_len;  float* fin_score;        /* [B][beam] */
} gnnlm_beam_select_t;
int gnnlm_beam_select(const gnnlm_beam_select_t* desc, void* stream);

/* gnnlm_beam_select with the reference's two diverse strategies: search.DiverseBeamSearch (fairseq/search.py:105-164: groups,
 * strength) and search.DiverseSiblingsSearch (:291-353: rate).  Only how the step's candidate list is drawn differs; finalize,
 * survive, table and finish are gnnlm_beam_select's own, run on that list.  One launch, one workgroup per sentence, nothing read back.
 * Additive to ABI 12: a new struct and a new entry; gnnlm_beam_select_t and gnnlm_beam_select are as they were.
 *   groups   G = groups, beam_g = beam / G.  Group g owns the hypotheses j = g, g + G, ..; with beam_in == 1 every group takes the
 *            sentence's one row.  The groups run in order.  The value of group g's candidate (j, c) with token k is
 *            fl32(score_in[j] + fl32(cand_val + fl32(-strength * n[k]))), n[k] = how many candidates the groups before g chose for
 *            token k at this step -- all of their chosen candidates, survivors or not; with n[k] == 0 the value is
 *            gnnlm_beam_select's fl32(score_in[j] + cand_val).  Absent: cand_val or the value not finite.  Inside a group the order
 *            is gnnlm_beam_select's (value descending, j ascending, token ascending); its first C_g = min(2 * beam_g, present) are
 *            chosen.  The step's list has 2 * beam places: place c * G + g holds candidate c of group g, a place without one (c >=
 *            C_g) is empty; the list is NOT sorted again.  The penalty stays in the value, hence in score_out and the histories.
 *   siblings (groups == 1, rate != 0, beam_in == beam; with beam_in == 1 the rate is not applied) the candidate that is the c-th of
 *            hypothesis j, c = 1 .. min(2 * beam, present of j) in j's own order (fl32(score_in[j] + cand_val) descending, token
 *            ascending, column ascending), has the value fl32(fl32(score_in[j] + cand_val) - fl32(c * rate)); j's later
 *            candidates are absent.  The list is the first min(2 * beam, present) of those under gnnlm_beam_select's order.
 *   the list finalize scans the places below beam, survive every place, both in place order; an empty place is skipped.  When an eos
 *            is finalized the survivors behind it move up, so a hypothesis of one group may continue another group's (the reference's
 *            behaviour).  groups == 1 with rate == 0 gives gnnlm_beam_select's results bit for bit.
 * Both penalties only lower a value and fewer than 2 * beam tokens can carry one, so the best 2 * beam_g penalised candidates of a
 * hypothesis lie among its 2 * beam best unpenalised ones: N >= 2 * beam columns are enough, and negative penalties are refused.
 * GNNLM_E_INVALID before anything is launched: whatever gnnlm_beam_select refuses in `sel`, groups < 1, beam % groups != 0, strength
 * or rate negative or not finite, groups > 1 together with rate != 0. */
typedef struct gnnlm_beam_select_diverse {
    gnnlm_beam_select_t sel;
    int32_t groups;                             /* G >= 1, beam % G == 0 */
    float strength;                             /* >= 0; read with groups > 1 */
    float rate;                                 /* >= 0; != 0 only with groups == 1 */
    int32_t reserved;                           /* leave 0 */
} gnnlm_beam_select_diverse_t;
int gnnlm_beam_select_diverse(const gnnlm_beam_select_diverse_t* desc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * kNN-LM on the base LM: the SCORED rows of packed samples (each sample = context rows, then scored rows: --context-window) as
 * one contiguous [n_out, d] query matrix, and / or the same rows scaled to unit length for a cosine index -- one launch instead of
 * one slice per sample + torch.cat + the four-op normalisation.  Additive to ABI 12: a new struct and a new entry.
 * Replaces: the slice of sequence_scorer.py:115-118 (which searches every row, context included; here only the scored rows are
 *           searched) and `queries / torch.sqrt(torch.sum(queries ** 2, dim=-1, keepdims=True))` of knn/knn_model.py:181-184.
 * Output row r, r in [out_off[b], out_off[b + 1]), is source row (block_off[b] - block_off[0]) + skip[b] + (r - out_off[b]).
 *   dst      the row as it is, bit for bit.
 *   dst_unit fl32(x / fl32(sqrt(s))), s = the float32 sum of the row's d squares (order unspecified; products may be fused into the
 *            sum): a correctly rounded square root, then a correctly rounded DIVISION per element -- the reference's expression, not
 *            a multiplication by the reciprocal.  A zero row gives what the division gives (0 / 0 = NaN); it is not special-cased.
 * One wave per output row, the row's block found by bisection of out_off (as gnnlm_lm_embed finds its block).  16-byte loads and
 * stores when d, every stride in use and every pointer in use allow (multiples of 4 floats / 16 bytes); a scalar path otherwise.
 * GNNLM_E_INVALID before anything is launched: d <= 0, a stride < d, both outputs NULL, a negative count, n_out >= 2^31, a missing
 * table, a pointer that is not 4-byte aligned.
 * The TABLES are checked on the device, by a one-block kernel that counts violations into *n_bad (DEVICE int32, zeroed by the
 * caller, added to): skip[b] < 0, skip[b] > the block's length, a block of negative length, out_off[0] != 0,
 * out_off[b + 1] - out_off[b] != length - skip, out_off[n_blocks] != n_out.  With wait != 0 the call waits for that count (4 bytes;
 * the stream is synchronised) and refuses a violation with GNNLM_E_INVALID before the pack kernel is launched -- no output is
 * touched.  With wait == 0 nothing is read back (the hot path: the caller looks at *n_bad when it looks at its results).  n_bad
 * NULL: the tables are not checked.  In every mode the pack kernel itself follows no table entry it cannot verify: a row whose
 * block is described outside [0, n_tok), whose skip is outside [0, length] or that lies beyond what its block yields is skipped,
 * never read and never written. */
typedef struct gnnlm_pack_rows {
    const float* src;  int64_t ld_src;      /* [n_tok, ld_src], ld_src >= d */
    const int32_t* block_off;               /* DEVICE [n_blocks + 1], as gnnlm_ragged_t: only differences from block_off[0] are read */
    const int32_t* skip;                    /* DEVICE [n_blocks]: rows at the front of each block that are NOT taken; NULL = 0 */
    const int32_t* out_off;                 /* DEVICE [n_blocks + 1]: prefix sums of (length - skip), out_off[0] = 0 */
    float* dst;  int64_t ld_dst;            /* [n_out, d] the rows as they are; may be NULL */
    float* dst_unit;  int64_t ld_unit;      /* [n_out, d] the rows scaled to unit length; may be NULL */
    int32_t n_blocks, d;
    int64_t n_tok, n_out;
    int32_t* n_bad;                         /* optional DEVICE int32: table violations, added to */
    int32_t wait;                           /* != 0 (needs n_bad): read the count back and refuse a violation before the pack kernel */
} gnnlm_pack_rows_t;
int gnnlm_pack_rows(const gnnlm_pack_rows_t* desc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sharded store, requester side: bucket the requested global rows by owning rank
 * (owner = row / rows_per_rank, out-of-range rows stay on `self_rank`).
 *   counts[world]   rows per owner (device, int64)
 *   send_rows[n]    the rows grouped by owner (order inside a bucket is unspecified)
 *   inv[n]          position of request s inside send_rows (so payload[inv[s]] answers request s)
 * counts must be zeroed by the caller; `cursor` is an int64[world] scratch.
 * ---------------------------------------------------------------------------------------------- */
int gnnlm_bucket_rows(const int64_t* rows, int64_t n, int64_t n_store, int64_t rows_per_rank, int32_t world,
                      int32_t self_rank, int64_t* counts, int64_t* cursor, int64_t* send_rows, int32_t* inv,
                      void* stream);

/* Fixed-capacity variant (no host round trip anywhere in the exchange): owner o's requests are written to
 * send_rows[o*cap, (o+1)*cap), unused slots hold -1 (the call prefills), inv[s] = slot of request s, or world*cap
 * for a request that is not a row of the store or did not fit its bucket (the latter are counted in *overflow,
 * which the call ADDS to).  `cursor` is an int64[world] scratch.  Equal-split all-to-alls can then be used. */
int gnnlm_bucket_rows_padded(const int64_t* rows, int64_t n, int64_t n_store, int64_t rows_per_rank, int32_t world,
                             int64_t cap, int64_t* cursor, int64_t* send_rows, int32_t* inv, int64_t* overflow, void* stream);

/* Peer-mapped alternative to the exchange: every rank maps the shards of its peers into its own address
 * space (hipIpcOpenMemHandle; over xGMI the loads of this kernel then go to the owner's HBM directly) and gathers the
 * requested rows itself -- one kernel, no collective, no bucketing, payload in request order.  shard[g] is the base of the
 * rows [shard_row0[g], shard_row0[g] + shard_rows[g]) rank g HOLDS (its range plus halo, if any); the owner of a row is
 * row / rows_per_rank as in gnnlm_bucket_rows.  Rows outside [0, n_store) (the -1 of invalid slots) give zero rows and
 * out_valid 0.  row_bytes: 1..16 or a multiple of 16 (128-B code rows, 4-B / 2-B labels). */
typedef struct gnnlm_peer_gather {
    const void* shard[16];
    int64_t shard_row0[16], shard_rows[16];
    int32_t world, row_bytes;
    int64_t rows_per_rank, n_store;
    const int64_t* rows;  int64_t n;
    void* out;                 /* [n, row_bytes] */
    uint8_t* out_valid;        /* optional [n] */
} gnnlm_peer_gather_t;
int gnnlm_gather_rows_peer(const gnnlm_peer_gather_t* desc, void* stream);
/* hipDeviceEnablePeerAccess(peer) for the current device (no error if already enabled); the Python side calls it once per
 * peer before the first gather when the shards live on other devices */
int gnnlm_enable_peer_access(int32_t peer_device);

/* ------------------------------------------------------------------------------------------------
 * Opt-in live timing (bench.py's roofline): while a profile is open every launch of the selected
 * kernels is bracketed by HIP events on its own stream.  One profile at a time; launches from several host threads
 * may be recorded into it (records and pools are mutex-guarded).
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnlm_profile_entry {
    int32_t kernel_id;
    int64_t launches;
    double total_ms;           /* sum of event-measured launch durations */
    double flops, bytes;       /* algorithmic work of those launches */
} gnnlm_profile_entry_t;
const char* gnnlm_kernel_name(int32_t kernel_id);
int gnnlm_profile_begin(uint32_t kernel_mask);      /* bit i selects kernel id i */
int gnnlm_profile_end(gnnlm_profile_entry_t* out, int32_t n_max, int32_t* n_out);   /* synchronises the events */

/* ------------------------------------------------------------------------------------------------
 * Owning HBM store for non-torch callers (DataStore / PlasmaArray residency,
 * knn/data_store.py:29-64, fairseq/tasks/language_modeling.py:274-276).  These DO allocate and the
 * uploads synchronise the given stream before returning.
 * ---------------------------------------------------------------------------------------------- */
typedef struct gnnlm_store gnnlm_store_t;
int gnnlm_store_create(int64_t n_store, int64_t row0, int64_t n_local, int32_t M, int32_t vals_itemsize,
                       int32_t device, gnnlm_store_t** out);
int gnnlm_store_upload_codes(gnnlm_store_t* s, const uint8_t* host_codes, int64_t first_local_row, int64_t n_rows, void* stream);
int gnnlm_store_upload_vals(gnnlm_store_t* s, const void* host_vals, int64_t first_local_row, int64_t n_rows, void* stream);
const uint8_t* gnnlm_store_codes(const gnnlm_store_t* s);
const void* gnnlm_store_vals(const gnnlm_store_t* s);
int gnnlm_store_destroy(gnnlm_store_t* s);

/* ------------------------------------------------------------------------------------------------
 * Incremental decoding through the HGT: generation from the GNN-LM itself.  Additive to ABI 12: new entries over the structs
 * above, no new struct, no member moved.
 * Replaces: HGTLayer.infer (fairseq/models/hgt.py:81-297), which the reference never reaches (extract_graph_features asserts
 *           incremental_state is None, transformer.py:1028; infer hard-codes max_len = 512 and no growing graph is built).
 * The step is EXACT.  In the implicit graph ntgt nodes never receive from tgt nodes, a token's star edges read only its own
 * neighbours' context groups, and the ('tgt','intra','tgt') edges are u -> w for u <= w inside a block: the output row of
 * token w in every layer is a function of its own input row, its own neighbour ids and the layer's folded K' / V' rows of
 * the tokens before it.  Those rows are what the cache holds.
 *
 * The cache is a gnnlm_kv_cache_t of its own with L = model->n_layers and d = model->d: row u of sequence b in layer l holds
 * the K' (V') row of token u of block b that layer l's tgt projections produce -- relation_att * relation_pri / sqrt(d_k)
 * folded into K', relation_msg into V' (gnnlm_hgt_layer_t.wk_t / wv_t), heads side by side.  len is its own; done may point
 * at the base LM cache's array.
 * ---------------------------------------------------------------------------------------------- */
/* gnnlm_hgt_forward_ragged over packed prompts that also fills the cache: block b is sequence b.  After every layer's tgt
 * projections one copy kernel writes the K' and V' rows of block b to cache rows [0, len_b) of sequence b of that layer; a last
 * tiny launch sets len[b] = len_b.  done is not touched.  The forward itself enqueues exactly what gnnlm_hgt_forward_ragged
 * enqueues, so io->out_tgt is the same bits.  Workspace: gnnlm_hgt_workspace_bytes_ragged.  Refused before anything is
 * launched, beyond what the forward refuses: blocks->n_blocks != cache->B, a longest block that the host knows to exceed
 * cache->cap (it holds at least ceil(n_tok / n_blocks) rows), cache->d != model->d, cache->L != model->n_layers, a cache that
 * gnnlm_decode_attn would refuse.  A block that turns out longer than cache->cap on the device is cut at cap rows (memory
 * safety only). */
int gnnlm_hgt_prefill(const gnnlm_hgt_t* model, const gnnlm_hgt_io_t* io, const gnnlm_ragged_t* blocks,
                      const gnnlm_kv_cache_t* cache, void* workspace, size_t workspace_bytes, void* stream);
/* One decoding step: `io` holds ONE new token per sequence (io->n_blocks = cache->B, io->T = 1; tgt_feats, ids and out_tgt
 * have B rows).  Per layer it runs gnnlm_hgt_forward's loop with one substitution: the causal branch is gnnlm_decode_attn of
 * the new q row against the layer's cache rows -- which appends the new K' / V' rows -- and enters the message sum through
 * the residual operand of the star branch's output GEMM.  The star branch, the ntgt updates, the group merge (group_ids /
 * n_unique_dev), state_cache and row_table are those of the forward.  One last tiny launch does len[b] += 1 for the rows that
 * are not done and in range.
 * A row with done[b] != 0, or len[b] outside [0, min(cap, max_len)), follows gnnlm_decode_attn's contract: nothing is
 * appended, an out-of-range row is counted once in *cache->n_bad, and its out_tgt row means nothing.
 * `max_len` is HOST data, the rule of gnnlm_tlm_step_io_t.max_len: an upper bound on len[b] + 1 over every execution of the
 * enqueued work.  The call only enqueues: no allocation, no host read, no synchronisation -- it can be captured in a HIP graph.
 * GNNLM_E_INVALID before anything is launched, gnnlm_last_error() naming the field: io->T != 1, io->n_blocks != cache->B,
 * model->max_intra_context > 0 (the decode kernel has no window), io->ntgt_feats (input adapters), io->fetched_codes /
 * model->shards (sharded and peer stores), model->token_embed (--reinit-nfeat), io->out_ntgt / out_valid, d / n_heads outside
 * {16, 32, 64, 128}, max_len outside [1, cache->cap], cache->d != model->d, cache->L != model->n_layers, and everything
 * gnnlm_hgt_forward and gnnlm_decode_attn refuse. */
size_t gnnlm_hgt_step_workspace_bytes(const gnnlm_hgt_t* model, const gnnlm_hgt_io_t* io, const gnnlm_kv_cache_t* cache,
                                      int32_t max_len);
int gnnlm_hgt_step(const gnnlm_hgt_t* model, const gnnlm_hgt_io_t* io, const gnnlm_kv_cache_t* cache, int32_t max_len,
                   void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNLM_H */
