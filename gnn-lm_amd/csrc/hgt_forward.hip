// The HGT forward over the implicit token / neighbour graph (include/gnnlm.h: gnnlm_hgt_forward, gnnlm_hgt_forward_ragged and their
// workspace sizes).  The orchestrator only enqueues kernels on the given stream (no allocation, no synchronisation), so a caller may
// capture it into a hipGraph.  hgt_forward_impl at the end of the file is the table of contents: plan, carve, validate, the layer-0
// ntgt states, then per layer the tgt update and the ntgt update.  gnnlm_hgt_prefill and gnnlm_hgt_step are the same loop with a
// K' / V' cache: the prefill copies every layer's rows into it, the step runs its causal branch against it (decode_attn.hip).
#include "host.h"

namespace gnnlm {
namespace {

constexpr int MAX_WINDOWS = 128;

// layer 0's ntgt projections with the OPQ rotation folded into their weights: they then take the decoded rows
bool folded_layer0(const gnnlm_hgt_t& m) {
    if (!m.opq_at || !m.layers) return false;
    const gnnlm_hgt_layer_t& w0 = m.layers[0];
    return w0.wq_n0 && w0.bq_n0 && w0.wk_n0 && w0.bk_n0 && w0.wv_n0 && w0.bv_n0;
}
// layer 0's K / V projections once per distinct datastore ROW of the batch's slots (ABI 11): merged groups on a local or mapped
// store, rotation-folded layer-0 weights, and a model whose layer 0 computes a subset of the slots (the un-elided forward with
// out_ntgt keeps the slot-keyed path)
bool row_keyed_kv(const gnnlm_hgt_t& m, const gnnlm_hgt_io_t& io) {
    if (m.token_embed) return false;               // tied to the OPQ fold: a token store has none
    if (!io.row_table || !io.group_ids || io.fetched_codes || io.ntgt_feats || io.out_ntgt || m.n_layers < 2) return false;
    return folded_layer0(m) && m.n_layers - 2 < std::max(m.left, m.right);
}

// Everything the forward derives from (m, io, rg), each quantity beside its rule: HgtPlan{m, io, rg} evaluates them once, in order,
// and the carve, the checks and the stages read them.  Plain arithmetic on whatever the descriptors hold -- the size functions run
// it on descriptors that nobody has checked.
struct HgtPlan {
    const gnnlm_hgt_t& m;  const gnnlm_hgt_io_t& io;  const gnnlm_ragged_t* rg;
    // the incremental entries: the K' / V' cache that gnnlm_hgt_prefill (with rg) fills and gnnlm_hgt_step (without) decodes
    // against, and the step's host bound on len[b] + 1
    const gnnlm_kv_cache_t* kv = nullptr;  const int step_len = 0;
    const int d = m.d, H = m.n_heads, dk = H > 0 ? d / H : 0, T = io.T, kg = io.kg, nb = io.n_blocks, n_g = 1 + m.left + m.right, L = m.n_layers;
    const bool dense0 = io.ntgt_feats != nullptr;       // layer-0 ntgt states given (input adapters): no code store
    // `--reinit-nfeat`: ntgt features = rows of the token-embedding table (transformer.py:1046-1048); explicit layer-0 states win
    const bool token = m.token_embed != nullptr && !dense0;
    const bool ntgt = m.n_layers > 1 || io.out_ntgt != nullptr;      // some layer's ntgt update is consumed: by a later layer, or by the caller
    // ABI 6: the ntgt pipeline over the DISTINCT centre rows of the batch (io.group_ids); the star edges reach a group through io.group_index
    const bool dedup = io.group_ids != nullptr;
    // ABI 7: centre states kept across calls (io.state_cache): group_ids are the groups the cache lacks, group_index holds slots
    const bool cached = io.state_cache != nullptr;
    const int32_t* gdev = io.n_unique_dev;      // ABI 9: the number of groups lives on the device; n_unique is then the capacity of the group arrays
    const bool ragged = rg != nullptr;          // gnnlm_hgt_forward_ragged: the packed tokens are one run of io.T rows, cut into blocks by rg
    const bool step = kv != nullptr && !ragged; // gnnlm_hgt_step: one new row per block, the causal branch is decode_attn -> HgtBufs.mc
    // the causal branch in one kernel that adds itself into the message sum: the recipe shape's, or the varlen one
    const bool fusedc = !step && (ragged || causal_attn_fused_ok(T, dk));
    const bool rowv = fusedc || step;           // V' row-major beside q and K' (the GEMM path wants V'^T instead)
    const size_t attn_bytes = step ? decode_attn_workspace_bytes(nb, H, dk, step_len) : 0;
    const int dpq = (dense0 || token) ? d : m.M * m.dsub;       // width of layer 0's neighbour rows
    // the carve's own rule for that width: it does not look at ntgt_feats, so with dense layer-0 states on a model with M * dsub > d
    // it over-allocates U, Z and the slot buffers.  Kept: workspace sizes are something callers see
    const int64_t carve_dpq = token ? d : (int64_t)m.M * m.dsub;
    const int64_t Tt = (int64_t)io.n_blocks * io.T, Tp = (io.T + 3) & ~3;       // tokens; T padded to 4
    const int64_t G = dedup ? io.n_unique : Tt * io.kg, S = G * n_g;            // context groups; slot rows
    const int64_t ld_hn0 = dense0 ? io.ld_ntgt : d;                             // row stride of the layer-0 ntgt states
    const bool fold0 = ntgt && !dense0 && !token && S != 0 && folded_layer0(m);        // layer 0 projects the decoded rows (hn[1])
    const bool by_row = ntgt && row_keyed_kv(m, io);            // carved for; used where fold0 holds too (S != 0)
    const bool nb_row = dedup && io.fetched_codes && !cached;   // merged groups on fetched codes, no cache: layer 0's star edges read HgtBufs.nb_row
    int validate(const void* ws, const Carver& c) const;
};

// Scratch of one call.  Two buffers are used twice, and the order of the launches is what makes that sound:
//   (1) aout holds the neighbours' labels (nb_label) until layer 0's a_linear: layer 0's star_attn is their only reader and that
//       GEMM is aout's first writer;
//   (2) chain attention runs in place over nq: a (group, head) task loads before it stores.
struct HgtBufs {
    // tgt side
    float *q, *k, *vt, *scores, *mc, *U, *Z, *ms, *aout, *has_nb;
    char* attn_ws;                   // gnnlm_hgt_step: the chunk partials of decode_attn (HgtPlan.attn_bytes)
    // ntgt side
    float *nq, *nk, *nv;
    uint8_t* valid;
    int32_t *rows_out, *rows_kv;     // slot subsets of the elided ntgt updates
    int32_t *win_counts;             // device-side group count (ABI 9): rows per GEMM window x multiplier
    int32_t *nb_row;                 // merged groups on fetched codes: code row of every neighbour's centre
    int32_t *nb_label;               // token store: label of every neighbour (-1: none), layer 0's index into the embedding table
    // ABI 11, layer 0's K / V keyed by datastore row: the slots' rows, the distinct ones, slot -> position, their count, validity, decoded rows
    int64_t *slot_row, *urows;
    int32_t *slot_u, *row_cnt, *win_counts_u;
    uint8_t* uvalid;
    float* xu;
};

// What one layer hands to the next, and the ping-pong buffers it moves between.
struct HgtState {
    float *ht[2] = {}, *hn[2] = {};
    const float* ht_in = nullptr;       // tgt states entering the layer
    const float* hn_cur = nullptr;      // ntgt states entering the layer
    int64_t ld_hn = 0;                  // row stride of hn_cur (the caller's buffer in the dense0 case)
    const uint8_t* valid = nullptr;     // validity of the slot rows
};

void carve_hgt(const HgtPlan& p, Carver& c, HgtBufs& b, HgtState& st) {
    const int64_t Tt = p.Tt, d = p.d, H = p.H, S = p.S, dpq = p.carve_dpq, dmax = std::max<int64_t>(dpq, d);
    b = HgtBufs{};
    st.ht[0] = c.take<float>(Tt * d);
    st.ht[1] = c.take<float>(Tt * d);
    if (p.ragged || p.step) {
        // packed blocks of unequal length: q | k' | v' row-major back to back (one 3d-wide GEMM writes them whatever the token
        // count), no V^T and no [n_blocks, H, T, T] score buffer -- the varlen kernel keeps one tile of scores in registers
        // (the step: the new rows' q | k' | v' the same way, for decode_attn)
        b.q = c.take<float>(3 * Tt * d);
        b.k = b.q + Tt * d;
        b.vt = b.k + Tt * d;
    } else {
        b.q = c.take<float>(Tt * d);
        b.k = c.take<float>(Tt * d);
        b.vt = c.take<float>((int64_t)p.nb * d * p.Tp);
        b.scores = c.take<float>((int64_t)p.nb * H * p.T * p.Tp);
    }
    b.mc = c.take<float>(Tt * d);
    b.U = c.take<float>(Tt * H * dmax);
    b.Z = c.take<float>(Tt * H * dmax);
    b.ms = c.take<float>(Tt * d);
    b.aout = c.take<float>(Tt * d);
    b.has_nb = c.take<float>(Tt);
    if (p.step) b.attn_ws = c.take<char>((int64_t)p.attn_bytes);
    b.win_counts = p.gdev ? c.take<int32_t>(MAX_WINDOWS * 8) : nullptr;
    b.nb_row = p.nb_row ? c.take<int32_t>(Tt * p.kg) : nullptr;
    // token store: the labels live in aout when they fit (k_g <= d: every recipe; invariant (1) of HgtBufs), so that a one-layer
    // step then needs no more workspace than on a code store; with k_g > d they get n_tok * k_g * 4 bytes of their own
    b.nb_label = !p.token ? nullptr : (p.kg <= d ? reinterpret_cast<int32_t*>(b.aout) : c.take<int32_t>(Tt * p.kg));
    if (!p.ntgt) return;
    st.hn[0] = c.take<float>(S * dmax);
    st.hn[1] = c.take<float>(S * dmax);
    b.nq = c.take<float>(S * dmax);
    b.nk = c.take<float>(S * dmax);
    b.nv = c.take<float>(S * dmax);
    b.valid = c.take<uint8_t>(S);
    b.rows_out = c.take<int32_t>(S);
    b.rows_kv = c.take<int32_t>(S);
    if (!p.by_row) return;
    b.slot_row = c.take<int64_t>(S);
    b.urows = c.take<int64_t>(S);
    b.slot_u = c.take<int32_t>(S);
    b.row_cnt = c.take<int32_t>(4);
    b.win_counts_u = c.take<int32_t>(MAX_WINDOWS * 8);
    b.uvalid = c.take<uint8_t>(S);
    b.xu = c.take<float>(S * dpq);
}

size_t hgt_workspace_bytes(const gnnlm_hgt_t& m, const gnnlm_hgt_io_t& io, const gnnlm_ragged_t* rg, const gnnlm_kv_cache_t* kv = nullptr,
                           int step_len = 0) {
    Carver c(nullptr);
    HgtBufs b;
    HgtState st;
    carve_hgt(HgtPlan{m, io, rg, kv, step_len}, c, b, st);
    return c.off + 256;
}

// The ntgt projections of a multi-layer step run over [groups x slots] rows of a few KB each: from ~1 M rows on, the operand
// spans more than 2^32 bytes and the GEMM kernel with 32-bit row offsets (gemm_f32_sched.hip, the fastest one for these
// shapes: 133-136 against 123-128 TFLOP/s, tools/gemm_bigm_bench.py) is no longer eligible.  Rows are independent, so the
// launches walk the groups in WINDOWS whose rows fit 32-bit byte offsets: same kernels per row as a 4-block step, same bits.
struct GroupWindows {
    int64_t G, per;       // groups, groups per window (a multiple of 128)
    int n_g;
    const int32_t* counts = nullptr;      // device-side group count: counts[w * 8 + mult - 1] = rows of window w x mult (window_counts)
    GroupWindows(int64_t G_, int n_g_, int64_t row_bytes) : G(G_), n_g(n_g_) {
        const int64_t max_rows = ((1ll << 32) - 1) / std::max<int64_t>(row_bytes, 1);
        const int64_t max_groups = std::max<int64_t>(128, max_rows / n_g / 128 * 128);
        const int64_t n_win = std::max<int64_t>(1, cdiv(G, max_groups));
        per = std::min<int64_t>(max_groups, cdiv(cdiv(G, n_win), (int64_t)128) * 128);
    }
    int64_t n_windows() const { return std::max<int64_t>(1, cdiv(G, per)); }
    const int32_t* m_dev(int64_t g0, int mult) const { return counts ? counts + (g0 / per) * 8 + (mult - 1) : nullptr; }
};
// the windows of a layer's slot rows; f0: layer 0 projecting the decoded rows (HgtPlan.fold0); ld_hn: row stride of the layer's ntgt states
GroupWindows slot_windows(const HgtPlan& p, bool f0, int64_t ld_hn) {
    const int64_t ld_pin = f0 ? p.dpq : ld_hn;
    return GroupWindows(p.G, p.n_g, 4 * (int64_t)std::max<int64_t>(std::max<int64_t>(ld_pin, ld_hn), std::max(p.d, p.dpq)));
}
// the windows of the distinct datastore rows (ABI 11)
GroupWindows row_windows(const HgtPlan& p) { return GroupWindows(p.S, 1, 4 * (int64_t)std::max(p.d, p.dpq)); }

// The slots of every group that a launch works on: `n` of the group's n_g, listed in `rows` = group_rows(n slots of G groups), or
// (rows == nullptr) all of them.  The list is group-major with indices g * n_g + slot, so its PREFIX is the row map of any window
// once the operands are based at the window's first row.
struct SlotSel { const int32_t* rows; int n; };
// C = A W^T + bias on the selected slot rows of every group, window by window (C's row stride is N)
int linear_windows(const GroupWindows& w, const SlotSel& sel, const float* A, int64_t lda, const float* W, const float* bias, float* C,
                   int N, int K, hipStream_t s) {
    for (int64_t g0 = 0; g0 < w.G; g0 += w.per) {
        const int64_t g1 = std::min(w.G, g0 + w.per), r0 = g0 * w.n_g, n = (g1 - g0) * sel.n;
        const int32_t* m_dev = w.m_dev(g0, sel.n);
        if (sel.rows) GNNLM_TRY(linear_rows(A + r0 * lda, lda, W, bias, C + r0 * N, N, sel.rows, n, N, K, 1.f, s, (g1 - g0) * w.n_g, m_dev));
        else GNNLM_TRY(linear(A + r0 * lda, lda, W, bias, C + r0 * N, n, N, K, nullptr, 1.f, s, m_dev));
    }
    return OK;
}

// which part of layer l's ntgt update runs.  Only what a later layer reads is computed (outputs identical to the full update): the
// last layer's star edges read the CENTRE slot of each group, and a slot's update depends on its path neighbours at distance 1
// (build_ntgt_edges(context=1)) -- so layer l has to deliver the slots within r = n_layers - 2 - l positions of the centre, from
// K / V of the slots within r + 1.  L = 3, l = r = 2: layer 0 writes 3 of 5 slots (Q, a_linear, LayerNorm on 3/5 of the rows),
// layer 1 the centre only (Q, a_linear on 1/5, K and V on 3/5): 3.2 of the 8 655360 x 1024 x 1024 GEMMs of the two updates go
// away.  With out_ntgt (API parity, tests) everything is computed.
struct NtgtStep {
    bool run;           // a later layer -- or the caller -- consumes the update
    int rad;            // the slots within rad positions of the centre are written
    bool all_slots;     // ... which is every slot
    bool f0;            // layer 0 with folded weights: the projections read the decoded rows
};
NtgtStep ntgt_step(const HgtPlan& p, int l) {
    const gnnlm_hgt_t& m = p.m;
    NtgtStep t;
    t.run = p.ntgt && (l != p.L - 1 || p.io.out_ntgt) && p.S > 0;
    t.rad = p.io.out_ntgt ? p.n_g : m.n_layers - 2 - l;
    t.all_slots = t.rad >= std::max(m.left, m.right);
    t.f0 = l == 0 && p.fold0;
    return t;
}

// Every refusal of the forward, in front of the first launch, worded in the plan's own names.  (Tt == 0 after the first four
// checks: an empty batch is accepted whatever else the descriptors hold.)
int HgtPlan::validate(const void* ws, const Carver& c) const {
    GNNLM_REQUIRE(m.layers && m.n_layers >= 1, "hgt: no layers");
    GNNLM_REQUIRE(m.gemm_precision >= 0 && m.gemm_precision <= 3, "hgt: gemm_precision must be 0, 1, 2 or 3");
    GNNLM_REQUIRE(m.d > 0 && m.n_heads > 0 && m.d % m.n_heads == 0, "hgt: d must be divisible by n_heads");
    GNNLM_REQUIRE(io.n_blocks >= 0 && io.T >= 0 && io.kg > 0, "hgt: bad io shape");
    if (Tt == 0) return OK;
    GNNLM_REQUIRE(io.tgt_feats && io.ids && io.out_tgt, "hgt: null io");
    GNNLM_REQUIRE(dense0 || token || (m.centroids && m.M > 0 && m.dsub > 0), "hgt: codec missing");
    GNNLM_REQUIRE(dense0 || token || io.fetched_codes || m.codes || m.shards, "hgt: no code store");
    GNNLM_REQUIRE(!token || (m.vals && (m.vals_itemsize == 2 || m.vals_itemsize == 4) && m.n_vocab > 0 && m.n_store > 0),
                  "hgt: token_embed needs vals (int16 / int32, the whole label table), n_vocab and n_store");
    GNNLM_REQUIRE(!token || (m.ld_token_embed >= m.d && m.ld_token_embed % 4 == 0 && (uintptr_t)m.token_embed % 16 == 0),
                  "hgt: token_embed needs ld_token_embed >= d (a multiple of 4) and 16-byte alignment");
    GNNLM_REQUIRE(!token || (!io.fetched_codes && !io.code_cache), "hgt: token_embed excludes fetched codes");
    GNNLM_REQUIRE(!dense0 || (io.ntgt_valid && io.ld_ntgt >= m.d && io.ld_ntgt % 4 == 0 && !io.fetched_codes),
                  "hgt: ntgt_feats needs ntgt_valid, ld_ntgt >= d (a multiple of 4) and no fetched_codes");
    GNNLM_REQUIRE(!(io.fetched_centres_only && ntgt), "hgt: fetched_centres_only needs n_layers == 1 and no out_ntgt");
    // the ntgt update keeps a context group in registers / on the stack (chain attention, the row-subset selections) and
    // addresses slot rows with 32-bit indices
    GNNLM_REQUIRE(!ntgt || (m.left >= 0 && m.right >= 0 && 1 + m.left + m.right <= 8), "hgt: ntgt update needs 1 + left + right <= 8");
    GNNLM_REQUIRE(!ntgt || (int64_t)io.n_blocks * io.T * io.kg * (1 + m.left + m.right) < (1ll << 31),
                  "hgt: ntgt update needs n_blocks * T * k_g * (1 + left + right) < 2^31 slot rows per call");
    GNNLM_REQUIRE(!io.fetched_codes || io.fetched_valid || io.fetched_centres_only, "hgt: fetched_codes needs fetched_valid");
    GNNLM_REQUIRE(!dedup || (ntgt && !dense0 && io.group_index && io.n_unique >= 0 && !io.out_ntgt && !io.out_valid),
                  "hgt: group_ids needs group_index, a multi-layer model on a code store and no ntgt outputs");
    GNNLM_REQUIRE(!gdev || dedup, "hgt: n_unique_dev needs group_ids");
    GNNLM_REQUIRE(!cached || (dedup && io.cache_cap > 0 && (io.group_slot || io.n_unique == 0) && m.n_layers > 1),
                  "hgt: state_cache needs group_ids / group_index / group_slot, cache_cap > 0 and a multi-layer model");
    // ABI 9: merged groups on a sharded store -- the fetched slots are those of the groups; with the cache, the code rows of the
    // cached centres live in io.code_cache (layer 0's star edges read the code of every neighbour, fetched now or not)
    GNNLM_REQUIRE(!(cached && io.fetched_codes) || (io.code_cache && m.M % 16 == 0), "hgt: state_cache on fetched codes needs code_cache and M % 16 == 0");
    GNNLM_REQUIRE(dk % 4 == 0 && d % 4 == 0 && dpq % 4 == 0, "hgt: d_k and the PQ dimension must be multiples of 4");
    GNNLM_REQUIRE(dense0 || token || m.opq_at || dpq == d, "hgt: without OPQ the PQ dimension must equal d");
    GNNLM_REQUIRE(!rg || (nb == 1 && rg->n_tok == Tt && rg->n_blocks >= 1 && rg->block_off && rg->tiles),
                  "hgt: a ragged batch needs io.n_blocks == 1, io.T == blocks.n_tok and the block / tile tables");
    GNNLM_REQUIRE(!rg || causal_attn_varlen_ok(dk), "hgt: ragged batches need d / n_heads in {16, 32, 64, 128}");
    if (kv) {
        // everything decode_attn would refuse in the middle of the layer loop is refused here, in front of the first launch
        GNNLM_TRY(check_kv_cache(*kv));
        GNNLM_REQUIRE(decode_attn_ok(dk), "hgt: a K/V cache needs d / n_heads in {16, 32, 64, 128}");
        GNNLM_REQUIRE(kv->d == d, "hgt: cache->d != model->d");
        GNNLM_REQUIRE(kv->L == m.n_layers, "hgt: cache->L != model->n_layers");
    }
    if (kv && rg) {
        GNNLM_REQUIRE(rg->n_blocks == kv->B, "hgt_prefill: blocks->n_blocks != cache->B");
        // the longest block holds at least ceil(n_tok / n_blocks) rows: what the host knows of max_len without reading the table
        GNNLM_REQUIRE(cdiv(rg->n_tok, (int64_t)rg->n_blocks) <= kv->cap, "hgt_prefill: a block is longer than the cache (max_len > cache->cap)");
    }
    if (step) {
        GNNLM_REQUIRE(io.T == 1, "hgt_step: io->T must be 1 (one new row per block)");
        GNNLM_REQUIRE(io.n_blocks == kv->B, "hgt_step: io->n_blocks != cache->B");
        GNNLM_REQUIRE(m.max_intra_context <= 0, "hgt_step: model->max_intra_context > 0 is not built (the decode kernel has no window)");
        GNNLM_REQUIRE(!io.ntgt_feats, "hgt_step: io->ntgt_feats (input adapters) is not built");
        GNNLM_REQUIRE(!io.fetched_codes && !m.shards, "hgt_step: io->fetched_codes / model->shards (sharded and peer stores) are not built");
        GNNLM_REQUIRE(!m.token_embed, "hgt_step: model->token_embed (--reinit-nfeat) is not built");
        GNNLM_REQUIRE(!io.out_ntgt && !io.out_valid, "hgt_step: io->out_ntgt / io->out_valid are not built");
        GNNLM_REQUIRE(step_len >= 1 && step_len <= kv->cap, "hgt_step: max_len outside [1, cache->cap] (the cache is full)");
    }
    GNNLM_REQUIRE(ws && c.fits(), "hgt: workspace too small (see gnnlm_hgt_workspace_bytes)");
    for (int l = 0; l < m.n_layers; ++l) {
        const gnnlm_hgt_layer_t& w = m.layers[l];
        const int din = w.din;
        GNNLM_REQUIRE(w.wq_t && w.wk_t && w.wv_t && w.wa_t && w.ln_g_t && w.ln_b_t && w.wku && w.wvz_t,
                      "hgt: layer has null tgt weights");
        GNNLM_REQUIRE(din == (l == 0 ? dpq : d), "hgt: layer.din must be M*dsub for layer 0 and d afterwards");
        const NtgtStep t = ntgt_step(*this, l);
        if (!t.run) continue;
        GNNLM_REQUIRE(w.wq_n && w.wk_n && w.wv_n && w.wa_n && w.ln_g_n && w.ln_b_n, "hgt: layer has null ntgt weights");
        if (gdev) {
            const GroupWindows win = slot_windows(*this, t.f0, l == 0 ? ld_hn0 : d);
            GNNLM_REQUIRE(win.n_windows() <= MAX_WINDOWS, "hgt: too many GEMM windows for a device-side group count");
        }
        if (t.f0 && by_row) {
            const GroupWindows winu = row_windows(*this);
            GNNLM_REQUIRE(winu.n_windows() <= MAX_WINDOWS, "hgt: too many GEMM windows for the row-keyed projections");
        }
    }
    return OK;
}

// q, k', v' of the batch: [Tt, ld] with the three at column offsets 0 / d / 2d when they come out of one GEMM
struct TgtQkv { const float *q, *k, *v; int64_t ld; };

// One call: the descriptors, what was derived from them, the scratch and the stream.  The stages are its members, in the order
// in which hgt_forward_impl runs them; what crosses layers is in the HgtState they are handed.
struct HgtForward {
    const HgtPlan& p;  const HgtBufs& b;  hipStream_t s;
    const gnnlm_hgt_t& m = p.m;  const gnnlm_hgt_io_t& io = p.io;  const gnnlm_ragged_t* rg = p.rg;

    // (ABI 11) the distinct ROWS among the slots (a claim pass over the slots' rows against the caller's second row table, handed
    // back clean), decoded once; their count stays on the device (row_cnt[0]).  The slots' own decode (g) stays: layer 0's Q and the
    // LayerNorm residual are per slot
    int decode_distinct_rows(const GatherParams& g) const {
        GNNLM_TRY(slot_rows(io.group_ids, p.G, p.gdev, m.left, m.right, m.n_layers - 1, m.n_store, b.slot_row, s));   // (layer 0's K / V reach: n_layers - 2 + 1 positions)
        gnnlm_group_assign_t ra{};
        ra.ids = b.slot_row; ra.n = p.S; ra.n_store = m.n_store; ra.slot_of = io.row_table;
        ra.group_ids = b.urows; ra.group_index = b.slot_u; ra.counters = b.row_cnt;
        GNNLM_TRY(group_assign(ra, s));
        GatherParams gu = g;
        gu.ids = b.urows; gu.n_groups = p.S; gu.left = 0; gu.right = 0; gu.n_groups_dev = b.row_cnt;
        gu.out_valid = b.uvalid; gu.out_x = b.xu; gu.ld_x = p.dpq;
        return gather_decode(gu, s);
    }

    // (a) the ntgt states that enter layer 0 and their validity: the caller's, none, token-embedding rows or decoded codes
    int layer0_ntgt_states(HgtState& st) const {
        st.ld_hn = p.ld_hn0;
        if (p.dense0) {
            st.hn_cur = io.ntgt_feats;
            st.valid = io.ntgt_valid;
            if (io.out_valid) GNNLM_HIP(hipMemcpyAsync(io.out_valid, st.valid, (size_t)p.S, hipMemcpyDeviceToDevice, s));
            return OK;
        }
        if (!p.ntgt) return OK;
        st.hn_cur = st.hn[0];
        st.valid = b.valid;
        if (p.S == 0) return OK;                        // a de-duplicated batch without a single valid neighbour
        GatherParams g{};
        if (p.token) {
            // the embedding row of every slot's label (the no-OPQ shape of the branch below)
            gnnlm_token_gather_t tg{};
            tg.ids = p.dedup ? io.group_ids : io.ids; tg.n_groups = p.G; tg.left = m.left; tg.right = m.right;
            tg.n_store = m.n_store; tg.vals = m.vals; tg.vals_itemsize = m.vals_itemsize;
            tg.n_vocab = m.n_vocab; tg.d = p.d; tg.embed = m.token_embed; tg.ld_embed = m.ld_token_embed;
            tg.out_x = st.hn[0]; tg.ld_x = p.d; tg.out_valid = b.valid;
            tg.n_groups_dev = p.gdev;
            GNNLM_TRY(token_gather(tg, s));
        } else {
            // PQ lookup of every slot, then the OPQ rotation (pq_wrapper.py:189-202)
            g.codes = io.fetched_codes ? io.fetched_codes : m.codes;
            if (!io.fetched_codes) g.shards = m.shards;
            g.direct = io.fetched_codes ? 1 : 0;
            g.in_valid = io.fetched_valid;
            g.in_index = io.fetched_index;
            g.vals = nullptr; g.vals_itemsize = 4;
            g.n_store = m.n_store; g.row0 = m.row0; g.n_local = m.n_local;
            g.M = m.M; g.dsub = m.dsub; g.centroids = m.centroids;
            g.ids = p.dedup ? io.group_ids : io.ids; g.n_groups = p.G; g.left = m.left; g.right = m.right;
            g.n_groups_dev = p.gdev;
            g.out_valid = b.valid;
            // fold0: layer 0's ntgt projections take the decoded rows (rotation folded into their weights); the rotation itself is
            // computed inside the layer, for the rows whose residual is needed only.  Else the rotation runs here, if there is one
            g.out_x = p.fold0 ? st.hn[1] : (m.opq_at ? b.nq : st.hn[0]);
            g.ld_x = m.opq_at ? p.dpq : p.d;
            GNNLM_TRY(gather_decode(g, s));
            if (m.opq_at && !p.fold0) GNNLM_TRY(linear(b.nq, p.dpq, m.opq_at, m.opq_nba, st.hn[0], p.S, p.d, p.dpq, nullptr, 1.f, s));
        }
        if (io.out_valid) GNNLM_HIP(hipMemcpyAsync(io.out_valid, b.valid, (size_t)p.S, hipMemcpyDeviceToDevice, s));
        if (p.fold0 && p.by_row) GNNLM_TRY(decode_distinct_rows(g));
        return OK;
    }

    // (b) tgt projections (hgt.py:315-322 with the 'intra' relation folded into K and V); V' row-major only for the one-kernel
    // causal branch
    int tgt_projections(const HgtState& st, const gnnlm_hgt_layer_t& w, TgtQkv& o) const {
        const int d = p.d;
        const int64_t Tt = p.Tt;
        o = TgtQkv{b.q, b.k, b.vt, d};
        const bool qkv_one = p.rowv && w.bq_t && w.wk_t == w.wq_t + (int64_t)d * d &&
                             w.wv_t == w.wk_t + (int64_t)d * d && w.bk_t == w.bq_t + d && w.bv_t == w.bk_t + d &&
                             b.k == b.q + Tt * d && b.vt == b.k + Tt * d;
        if (qkv_one) {
            // weights stored back to back (hgt.py does): ONE 3d-wide GEMM instead of three d-wide ones (same input; 1536
            // tiles on the 512 workgroup slots instead of 3 x 512 with a prologue and an epilogue each)
            o.k = b.q + d; o.v = b.q + 2 * d; o.ld = 3 * (int64_t)d;
            return linear(st.ht_in, d, w.wq_t, w.bq_t, b.q, Tt, 3 * d, d, nullptr, 1.f, s);
        }
        GNNLM_TRY(linear(st.ht_in, d, w.wq_t, w.bq_t, b.q, Tt, d, d, nullptr, 1.f, s));
        GNNLM_TRY(linear(st.ht_in, d, w.wk_t, w.bk_t, b.k, Tt, d, d, nullptr, 1.f, s));
        // recipe shape: V' row-major, then scores + masked softmax + P.V in one kernel (causal_attn.hip)
        // (the kernel itself runs after the star branch and adds its result into the message sum, see tgt_output)
        if (p.rowv) GNNLM_TRY(linear(st.ht_in, d, w.wv_t, w.bv_t, b.vt, Tt, d, d, nullptr, 1.f, s));
        return OK;
    }

    // (c') gnnlm_hgt_step's causal branch: the new row of every block against the layer's cached K' / V' rows -> b.mc.  q is used
    // as given -- the scale is folded into K' -- and the new K' / V' rows are appended to the cache by the same kernel
    int causal_step(const TgtQkv& qkv, int l) const {
        gnnlm_decode_attn_t a{};
        a.q = qkv.q; a.k_new = qkv.k; a.v_new = qkv.v; a.ld = qkv.ld;
        a.out = b.mc; a.ldo = p.d;
        a.cache = *p.kv; a.layer = l; a.H = p.H; a.dk = p.dk; a.max_len = p.step_len;
        a.workspace = b.attn_ws; a.workspace_bytes = p.attn_bytes;
        if (l > 0) a.cache.n_bad = nullptr;                 // a row out of range is counted once per step, not once per layer
        return decode_attn(a, nullptr, s);
    }

    // (c) the causal branch as GEMMs: V'^T, scores, masked softmax, P.V -> b.mc
    int causal_unfused(const HgtState& st, const gnnlm_hgt_layer_t& w) const {
        const int d = p.d, H = p.H, dk = p.dk, T = p.T, nb = p.nb;
        const int64_t Tp = p.Tp;
        {   // V'^T[blk][n][t] = sum_k Wv'[n,k] h[blk*T + t, k] + bv'[n]
            GemmParams g{};
            g.A = w.wv_t; g.lda = d; g.W = st.ht_in; g.ldw = d; g.C = b.vt; g.ldc = Tp;
            g.bias = w.bv_t; g.bias_mode = 2;
            g.M = d; g.N = T; g.K = d; g.batch1 = nb;
            g.sW1 = (int64_t)T * d; g.sC1 = (int64_t)d * Tp;
            GNNLM_TRY(gemm_nt(g, s));
        }
        {   // causal scores S[blk,h] = Q_h K'_h^T   (scale folded into K')
            GemmParams g{};
            g.A = b.q; g.lda = d; g.W = b.k; g.ldw = d; g.C = b.scores; g.ldc = Tp;
            g.M = T; g.N = T; g.K = dk; g.batch1 = nb; g.batch2 = H;
            g.sA1 = (int64_t)T * d; g.sA2 = dk; g.sW1 = (int64_t)T * d; g.sW2 = dk;
            g.sC1 = (int64_t)H * T * Tp; g.sC2 = (int64_t)T * Tp;
            GNNLM_TRY(gemm_nt(g, s));
        }
        GNNLM_TRY(causal_softmax(b.scores, (int64_t)nb * H, T, Tp, m.max_intra_context, s));
        GemmParams g{};     // m_causal[blk, :, h] = P[blk,h] V'_h
        g.A = b.scores; g.lda = Tp; g.W = b.vt; g.ldw = Tp; g.C = b.mc; g.ldc = d;
        g.M = T; g.N = dk; g.K = (int)Tp; g.batch1 = nb; g.batch2 = H;
        g.sA1 = (int64_t)H * T * Tp; g.sA2 = (int64_t)T * Tp;
        g.sW1 = (int64_t)d * Tp; g.sW2 = (int64_t)dk * Tp;
        g.sC1 = (int64_t)T * d; g.sC2 = dk;
        return gemm_nt(g, s);
    }

    // (d) where layer l's star edges find their neighbours: validity, then X / codes / indices
    int star_source(const HgtState& st, int l, StarAttnParams& a) const {
        const int n_g = p.n_g, d = p.d;
        if (p.cached) { }                                      // a cached group is a valid one: x_index >= 0 says it all
        else if (p.ntgt || p.dense0) { a.nb_valid = st.valid; a.nb_valid_stride = n_g; }        // centre slot of each group
        else if (io.fetched_valid) { a.nb_valid = io.fetched_valid; a.nb_valid_stride = io.fetched_centres_only ? 1 : n_g; }
        if (p.dedup) a.x_index = io.group_index;
        if (p.token && l == 0) {
            // X = E, one row per vocabulary entry; (i, j) is a neighbour iff its id is a row of the store and its label an entry
            // (the only reader of nb_label: invariant (1) of HgtBufs)
            a.nb_valid = nullptr; a.x_index = b.nb_label;
            a.X = m.token_embed; a.ldx = m.ld_token_embed; a.x_group_stride = 1;
        } else if (p.cached && l > 0) {
            a.X = io.state_cache + (int64_t)(l - 1) * io.cache_cap * d; a.ldx = d; a.x_group_stride = 1;
        } else if (l == 0 && !p.dense0 && p.dedup && io.fetched_codes) {
            // merged groups on a sharded store: neighbour e's code row is the centre slot of its group
            if (p.cached) {
                GNNLM_TRY(scatter_code_rows(io.fetched_codes, io.fetched_index, n_g, io.fetched_valid, io.code_cache, io.group_slot, p.gdev, p.G, m.M, s));
                a.codes = io.code_cache; a.codes_index = io.group_index;
            } else {
                GNNLM_TRY(nb_code_rows(io.group_index, io.fetched_index, n_g, p.Tt * p.kg, b.nb_row, s));
                a.codes = io.fetched_codes; a.codes_index = b.nb_row;
            }
            a.codes_direct = 1;
            a.row0 = 0; a.n_local = 0; a.M = m.M; a.dsub = m.dsub; a.centroids = m.centroids;
        } else if (l == 0 && !p.dense0) {
            a.codes = io.fetched_codes ? io.fetched_codes : m.codes;
            if (!io.fetched_codes) a.shards = m.shards;
            a.codes_direct = io.fetched_codes ? (io.fetched_centres_only ? 1 : n_g) : 0;
            a.codes_index = io.fetched_codes ? io.fetched_index : nullptr;
            a.row0 = m.row0; a.n_local = m.n_local; a.M = m.M; a.dsub = m.dsub; a.centroids = m.centroids;
        } else {
            a.X = st.hn_cur; a.ldx = st.ld_hn; a.x_group_stride = n_g;
        }
        return OK;
    }

    // the star branch: absorbed queries U[i,h,:] = Wku_h q[i,h,:], then the attention over each token's neighbours -> b.Z, b.has_nb
    int star_branch(const HgtState& st, int l, const TgtQkv& qkv) const {
        const gnnlm_hgt_layer_t& w = m.layers[l];
        const int H = p.H, dk = p.dk, din = w.din;
        GemmParams g{};
        g.A = qkv.q; g.lda = qkv.ld; g.W = w.wku; g.ldw = dk; g.C = b.U; g.ldc = (int64_t)H * din;
        g.M = (int)p.Tt; g.N = din; g.K = dk; g.batch1 = H;
        g.sA1 = dk; g.sW1 = (int64_t)din * dk; g.sC1 = din;
        GNNLM_TRY(gemm_nt(g, s));
        StarAttnParams a{};
        a.U = b.U; a.ids = io.ids; a.T = (int)p.Tt; a.H = H; a.D = din; a.kg = p.kg;
        a.Z = b.Z; a.has_nb = b.has_nb;
        a.n_store = m.n_store;
        GNNLM_TRY(star_source(st, l, a));
        return star_attn(a, s);
    }

    // (e) 2*agg = Z Wvz + has_nb * bvz + m_causal, then a_linear on the cross-type mean (0.5 folded into alpha) + residual, then
    // LayerNorm (hgt.py:397-405) -> ht_out
    int tgt_output(const HgtState& st, const gnnlm_hgt_layer_t& w, const TgtQkv& qkv, float* ht_out) const {
        const int d = p.d, H = p.H, dk = p.dk, din = w.din;
        GemmParams g{};
        g.A = b.Z; g.lda = (int64_t)H * din; g.W = w.wvz_t; g.ldw = din; g.C = b.ms; g.ldc = d;
        g.bias = w.bvz; g.bias_mode = 1; g.gate = b.has_nb;
        if (!p.fusedc) { g.R = b.mc; g.ldr = d; }
        g.M = (int)p.Tt; g.N = dk; g.K = din; g.batch1 = H;
        g.sA1 = din; g.sW1 = (int64_t)dk * din; g.sC1 = dk; g.sB1 = dk; g.sR1 = dk;
        GNNLM_TRY(gemm_nt(g, s));
        // recipe shape: the causal branch adds itself into the sum with coalesced row accesses -- cheaper than
        // the residual loads of the GEMM epilogue (same value: star + causal, fp32 addition commutes)
        if (rg) GNNLM_TRY(causal_attn_varlen(qkv.q, qkv.k, qkv.v, qkv.ld, b.ms, d, *rg, H, dk, m.max_intra_context, s, true));
        else if (p.fusedc) GNNLM_TRY(causal_attn_fused(qkv.q, qkv.k, qkv.v, qkv.ld, b.ms, d, p.nb, p.T, H, dk, m.max_intra_context, s, true));
        GNNLM_TRY(linear(b.ms, d, w.wa_t, w.ba_t, b.aout, p.Tt, d, d, nullptr, 0.5f, s));       // b.aout's first writer: invariant (1) of HgtBufs
        return layernorm(b.aout, d, w.ln_g_t, w.ln_b_t, ht_out, d, p.Tt, d, m.ln_eps, nullptr, s, st.ht_in, d);    // + h (hgt.py:403)
    }

    // (f) layer l's ntgt update (ntgt_step(l).run): residual rows -> Q -> K, V -> chain attention -> a_linear -> LayerNorm, on
    // every slot or on the slots a later layer reads
    int ntgt_update(HgtState& st, int l, const NtgtStep& t) const {
        const gnnlm_hgt_layer_t& w = m.layers[l];
        const int d = p.d, dpq = p.dpq, n_g = p.n_g;
        const bool last = l == p.L - 1, f0 = t.f0;
        float* hn_out = (last && io.out_ntgt) ? io.out_ntgt : (st.hn_cur == st.hn[0] ? st.hn[1] : st.hn[0]);
        // projection inputs: the layer's ntgt states, or (layer 0 with folded weights) the decoded rows
        const float* pin = f0 ? st.hn[1] : st.hn_cur;
        const int64_t ld_pin = f0 ? dpq : st.ld_hn;
        const int kin = f0 ? dpq : d;
        const float *Wq = f0 ? w.wq_n0 : w.wq_n, *Bq = f0 ? w.bq_n0 : w.bq_n, *Wk = f0 ? w.wk_n0 : w.wk_n,
                    *Bk = f0 ? w.bk_n0 : w.bk_n, *Wv = f0 ? w.wv_n0 : w.wv_n, *Bv = f0 ? w.bv_n0 : w.bv_n;
        GroupWindows win = slot_windows(p, f0, st.ld_hn);
        if (p.gdev) {
            GNNLM_TRY(window_counts(p.gdev, p.G, win.per, (int)win.n_windows(), b.win_counts, s));
            win.counts = b.win_counts;
        }
        SlotSel out{nullptr, n_g}, kv{nullptr, n_g};      // the slots written, and the slots whose K and V they read
        if (!t.all_slots) {
            // slot of the position `o` relative to the centre: centre first, then o - left .. o - 1, then o + 1 .. o + right
            auto slot = [&](int o) { return o == 0 ? 0 : (o < 0 ? m.left + 1 + o : m.left + o); };
            int sel_out[8], sel_kv[8];
            out = SlotSel{b.rows_out, 0};
            kv = SlotSel{b.rows_kv, 0};
            for (int o = -std::min(t.rad, m.left); o <= std::min(t.rad, m.right); ++o) sel_out[out.n++] = slot(o);
            for (int o = -std::min(t.rad + 1, m.left); o <= std::min(t.rad + 1, m.right); ++o) sel_kv[kv.n++] = slot(o);
            GNNLM_TRY(group_rows(b.rows_out, p.G, n_g, sel_out, out.n, s));
            GNNLM_TRY(group_rows(b.rows_kv, p.G, n_g, sel_kv, kv.n, s));
        }
        if (f0) GNNLM_TRY(linear_windows(win, out, st.hn[1], dpq, m.opq_at, m.opq_nba, st.hn[0], d, dpq, s));      // residual of the rows written
        GNNLM_TRY(linear_windows(win, out, pin, ld_pin, Wq, Bq, b.nq, d, kin, s));
        const bool by_row = f0 && p.by_row;     // (ABI 11) K / V of layer 0 once per distinct datastore row (row_keyed_kv: never all_slots)
        if (by_row) {
            GroupWindows winu = row_windows(p);
            GNNLM_TRY(window_counts(b.row_cnt, p.S, winu.per, (int)winu.n_windows(), b.win_counts_u, s));
            winu.counts = b.win_counts_u;
            GNNLM_TRY(linear_windows(winu, SlotSel{nullptr, 1}, b.xu, dpq, Wk, Bk, b.nk, d, kin, s));
            GNNLM_TRY(linear_windows(winu, SlotSel{nullptr, 1}, b.xu, dpq, Wv, Bv, b.nv, d, kin, s));
        } else {
            GNNLM_TRY(linear_windows(win, kv, pin, ld_pin, Wk, Bk, b.nk, d, kin, s));
            GNNLM_TRY(linear_windows(win, kv, pin, ld_pin, Wv, Bv, b.nv, d, kin, s));
        }
        ChainAttnParams ca{};
        ca.Q = b.nq; ca.K = b.nk; ca.V = b.nv; ca.ld = d; ca.valid = st.valid;
        ca.n_groups = p.G; ca.left = m.left; ca.right = m.right; ca.H = p.H; ca.dk = p.dk;
        ca.n_groups_dev = p.gdev;
        ca.out = b.nq; ca.ldo = d;      // in place over Q: invariant (2) of HgtBufs
        if (!t.all_slots) ca.radius_p1 = t.rad + 1;
        if (by_row) ca.kv_index = b.slot_u;
        GNNLM_TRY(chain_attn(ca, s));
        GNNLM_TRY(linear_windows(win, out, b.nq, d, w.wa_n, w.ba_n, b.nk, d, d, s));
        GNNLM_TRY(layernorm(b.nk, d, w.ln_g_n, w.ln_b_n, hn_out, d, p.G * out.n, d, m.ln_eps, st.valid, s, st.hn_cur, st.ld_hn, out.rows, p.gdev, out.n));
        st.hn_cur = hn_out;
        st.ld_hn = d;
        // the centre slot (row g * n_g) of every computed group -> its cache slot, for layer l + 1's star edges now and later
        if (p.cached && !last) GNNLM_TRY(scatter_rows(hn_out, (int64_t)n_g * d, io.state_cache + (int64_t)l * io.cache_cap * d, d, io.group_slot, p.G, d, s, p.gdev));
        return OK;
    }
};

// kv with rg: gnnlm_hgt_prefill, the ragged forward whose K' / V' rows also go to the cache.  kv without rg: gnnlm_hgt_step, one new
// row per block whose causal branch reads the cache (step_len: the host's bound on len[b] + 1).
int hgt_forward_impl(const gnnlm_hgt_t& m, const gnnlm_hgt_io_t& io, void* ws, size_t ws_bytes, hipStream_t s, const gnnlm_ragged_t* rg = nullptr,
                     const gnnlm_kv_cache_t* kv = nullptr, int step_len = 0) {
    // plan and carve are arithmetic only: nothing is read through a pointer or enqueued before the checks have passed
    const HgtPlan p{m, io, rg, kv, step_len};
    HgtBufs b;
    HgtState st;
    Carver c(ws, ws_bytes);
    carve_hgt(p, c, b, st);
    GNNLM_TRY(p.validate(ws, c));
    if (p.Tt == 0) return OK;                           // empty batch: nothing to do
    GemmPrecisionScope prec_scope(m.gemm_precision);
    const HgtForward f{p, b, s};

    GNNLM_TRY(f.layer0_ntgt_states(st));
    // token store: layer 0's star edges read the embedding table itself through the neighbours' labels, whatever the depth
    // (cached groups have no slot rows in this call, a one-layer model has none at all)
    if (p.token) GNNLM_TRY(neighbor_labels(io.ids, p.Tt * p.kg, m.n_store, m.vals, m.vals_itemsize, m.n_vocab, b.nb_label, s));
    // V^T buffer of the GEMM path: its padding columns (t >= T) are read by the P.V GEMM against zero probabilities
    if (!p.rowv) GNNLM_HIP(hipMemsetAsync(b.vt, 0, sizeof(float) * (size_t)p.nb * p.d * p.Tp, s));

    st.ht_in = io.tgt_feats;
    for (int l = 0; l < m.n_layers; ++l) {
        const gnnlm_hgt_layer_t& w = m.layers[l];
        float* ht_out = l == m.n_layers - 1 ? io.out_tgt : st.ht[l & 1];
        TgtQkv qkv;
        GNNLM_TRY(f.tgt_projections(st, w, qkv));
        // prefill: the block's K' / V' rows are rows [0, len_b) of its sequence in this layer of the cache
        if (kv && rg) GNNLM_TRY(kv_cache_fill(qkv.k, qkv.v, qkv.ld, *kv, l, *rg, kv->cap, s));
        if (p.step) GNNLM_TRY(f.causal_step(qkv, l));
        else if (!p.fusedc) GNNLM_TRY(f.causal_unfused(st, w));
        GNNLM_TRY(f.star_branch(st, l, qkv));
        GNNLM_TRY(f.tgt_output(st, w, qkv, ht_out));
        const NtgtStep t = ntgt_step(p, l);
        if (t.run) GNNLM_TRY(f.ntgt_update(st, l, t));
        st.ht_in = ht_out;
    }
    if (kv && rg) GNNLM_TRY(kv_len_set(*kv, rg->block_off, kv->cap, s));
    if (p.step) GNNLM_TRY(kv_len_advance(*kv, step_len, s));
    return OK;
}

}  // namespace
}  // namespace gnnlm

using namespace gnnlm;

extern "C" {

size_t gnnlm_hgt_workspace_bytes(const gnnlm_hgt_t* m, const gnnlm_hgt_io_t* io) {
    return !m || !io ? 0 : hgt_workspace_bytes(*m, *io, nullptr);
}
int gnnlm_hgt_forward(const gnnlm_hgt_t* m, const gnnlm_hgt_io_t* io, void* workspace, size_t workspace_bytes,
                      void* stream) {
    GNNLM_DESC(m);
    GNNLM_DESC(io);
    return hgt_forward_impl(*m, *io, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t gnnlm_hgt_workspace_bytes_ragged(const gnnlm_hgt_t* m, const gnnlm_hgt_io_t* io, const gnnlm_ragged_t* blocks) {
    return !m || !io || !blocks ? 0 : hgt_workspace_bytes(*m, *io, blocks);
}
int gnnlm_hgt_forward_ragged(const gnnlm_hgt_t* m, const gnnlm_hgt_io_t* io, const gnnlm_ragged_t* blocks, void* workspace,
                             size_t workspace_bytes, void* stream) {
    GNNLM_DESC(m);
    GNNLM_DESC(io);
    GNNLM_DESC(blocks);
    return hgt_forward_impl(*m, *io, workspace, workspace_bytes, (hipStream_t)stream, blocks);
}
int gnnlm_hgt_prefill(const gnnlm_hgt_t* m, const gnnlm_hgt_io_t* io, const gnnlm_ragged_t* blocks, const gnnlm_kv_cache_t* cache,
                      void* workspace, size_t workspace_bytes, void* stream) {
    GNNLM_DESC(m);
    GNNLM_DESC(io);
    GNNLM_DESC(blocks);
    GNNLM_DESC(cache);
    return hgt_forward_impl(*m, *io, workspace, workspace_bytes, (hipStream_t)stream, blocks, cache);
}
size_t gnnlm_hgt_step_workspace_bytes(const gnnlm_hgt_t* m, const gnnlm_hgt_io_t* io, const gnnlm_kv_cache_t* cache, int32_t max_len) {
    return !m || !io || !cache ? 0 : hgt_workspace_bytes(*m, *io, nullptr, cache, max_len);
}
int gnnlm_hgt_step(const gnnlm_hgt_t* m, const gnnlm_hgt_io_t* io, const gnnlm_kv_cache_t* cache, int32_t max_len, void* workspace,
                   size_t workspace_bytes, void* stream) {
    GNNLM_DESC(m);
    GNNLM_DESC(io);
    GNNLM_DESC(cache);
    return hgt_forward_impl(*m, *io, workspace, workspace_bytes, (hipStream_t)stream, nullptr, cache, max_len);
}

}  // extern "C"
