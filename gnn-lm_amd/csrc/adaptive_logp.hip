// The target-only tied adaptive softmax (include/gnnlm.h: gnnlm_adaptive_target_logp): log-probability of every row's target from
// the head and, for the rows of each tail band only, that band.  The orchestrator only enqueues kernels on the given stream (no
// allocation, no synchronisation), so a caller may capture it into a hipGraph.
#include "host.h"

namespace gnnlm {
namespace {

struct AsmBufs {
    float *head_part, *head_lse, *head_picked, *xi, *tail_part, *tail_lse, *tail_picked;
    int32_t *head_pick, *band_rows, *band_pick, *band_count;
};

void carve_asm(const gnnlm_adaptive_softmax_t& w, int64_t n, Carver& c, AsmBufs& b) {
    const int nt = w.n_bands - 1;
    const int64_t head_n = w.cutoff[0] + nt;
    int64_t max_size = 0, max_dim = 0;
    for (int i = 1; i < w.n_bands; ++i) {
        max_size = std::max<int64_t>(max_size, w.cutoff[i] - w.cutoff[i - 1]);
        max_dim = std::max<int64_t>(max_dim, w.dim[i]);
    }
    b.head_part = c.take<float>(n * 4 * cdiv(head_n, 128));
    b.head_lse = c.take<float>(n);
    b.head_picked = c.take<float>(n);
    b.head_pick = c.take<int32_t>(n);
    b.band_rows = c.take<int32_t>(std::max(nt, 1) * n);
    b.band_pick = c.take<int32_t>(std::max(nt, 1) * n);
    b.band_count = c.take<int32_t>(8);
    b.xi = c.take<float>(n * max_dim);
    b.tail_part = c.take<float>(n * 4 * cdiv(std::max<int64_t>(max_size, 1), 128));
    b.tail_lse = c.take<float>(n);
    b.tail_picked = c.take<float>(n);
}

int adaptive_impl(const gnnlm_adaptive_softmax_t& w, const float* x, int64_t ldx, const int64_t* target, int64_t n,
                  float* lm_logp, void* ws, size_t ws_bytes, hipStream_t s) {
    // everything is checked here, in front of the first launch: what gemm_nt() would refuse half-way through the call included
    GNNLM_REQUIRE(w.n_bands >= 1 && w.n_bands <= 8 && w.head_w && w.d > 0 && w.d % 4 == 0, "adaptive: bad weights");
    GNNLM_REQUIRE(w.gemm_precision >= 0 && w.gemm_precision <= 3, "adaptive: gemm_precision must be 0, 1, 2 or 3");
    GNNLM_REQUIRE(w.cutoff[0] >= 1, "adaptive: cutoffs must be positive and strictly ascending");
    GNNLM_REQUIRE((uintptr_t)w.head_w % 16 == 0, "adaptive: weights must be 16-byte aligned");
    for (int i = 1; i < w.n_bands; ++i) {
        GNNLM_REQUIRE(w.cutoff[i] > w.cutoff[i - 1], "adaptive: cutoffs must be positive and strictly ascending");
        GNNLM_REQUIRE(w.proj_t[i] && w.emb[i] && w.dim[i] > 0 && w.dim[i] % 4 == 0, "adaptive: bad tail band");
        GNNLM_REQUIRE((uintptr_t)w.proj_t[i] % 16 == 0 && (uintptr_t)w.emb[i] % 16 == 0, "adaptive: weights must be 16-byte aligned");
    }
    GNNLM_REQUIRE(n >= 0 && n < (1ll << 31), "adaptive: bad row count");
    GNNLM_REQUIRE(x && target && lm_logp, "adaptive: null io");
    GNNLM_REQUIRE(ldx >= w.d && ldx % 4 == 0 && (uintptr_t)x % 16 == 0, "adaptive: x must be 16-byte aligned with ldx >= d, ldx % 4 == 0");
    if (n == 0) return OK;
    Carver c(ws, ws_bytes);
    AsmBufs b;
    carve_asm(w, n, c, b);
    GNNLM_REQUIRE(ws && c.fits(), "adaptive: workspace too small (see gnnlm_adaptive_workspace_bytes)");
    GNNLM_REQUIRE((uintptr_t)ws % 16 == 0, "adaptive: the workspace must be 16-byte aligned");
    GemmPrecisionScope prec_scope(w.gemm_precision);
    const int nt = w.n_bands - 1;
    const int head_n = w.cutoff[0] + nt;

    BandSplitParams bs;
    bs.target = target; bs.n = n; bs.n_bands = w.n_bands;
    for (int i = 0; i < w.n_bands; ++i) bs.cutoff[i] = w.cutoff[i];
    bs.head_pick = b.head_pick; bs.band_rows = b.band_rows; bs.band_pick = b.band_pick; bs.band_count = b.band_count;
    GNNLM_TRY(band_split(bs, s));

    {   // head: [E_0 ; class_proj] (adaptive_softmax.py:24-47,184-188)
        GemmParams g{};
        g.A = x; g.lda = ldx; g.W = w.head_w; g.ldw = w.d;
        g.lse_part = b.head_part; g.lse_pick = b.head_pick; g.lse_picked = b.head_picked;
        g.M = (int)n; g.N = head_n; g.K = w.d;
        // tile walk: bands of 4 m-tiles, n slow inside a band.  An XCD's 32 concurrently running 256 x 256 tiles then form a 4 x 8
        // block (4 A panels + 8 W panels in flight through its L2) instead of a 32 x 1 column (32 + 1): PMC FETCH_SIZE x 2 of the
        // 8192 x 20004 x 1024 head 2.74 GB -> 0.97 GB per launch (tools/pmc_head_order.sh; GM = 8: 1.02, GM = 16: 1.53).  That is
        // the floor of this tile size -- tiles x (1 MiB / 8 + 1 MiB / 4) = 0.95 GB: a panel is 1 MiB and the L2 4 MiB, nothing
        // survives from one block of tiles to the next -- and the time does not move (2.457 ms either way: MFMA-bound)
        if (n >= 1024) g.tile_order = 2 + 4;
        GNNLM_TRY(gemm_nt(g, s));     // logits are reduced in the epilogue, never written
    }
    GNNLM_TRY(lse_reduce(b.head_part, 2 * (int)cdiv(head_n, 128), n, nullptr, b.head_lse, s));
    GNNLM_TRY(head_logp(b.head_picked, b.head_lse, b.head_pick, lm_logp, n, s));

    for (int i = 1; i < w.n_bands; ++i) {   // tails (adaptive_softmax.py:91-115,199-203), target rows only
        const int size = w.cutoff[i] - w.cutoff[i - 1];
        const int32_t* rows = b.band_rows + (int64_t)(i - 1) * n;
        const int32_t* pick = b.band_pick + (int64_t)(i - 1) * n;
        const int32_t* cnt = b.band_count + (i - 1);
        GemmParams g{};
        g.A = x; g.lda = ldx; g.a_rows = rows; g.W = w.proj_t[i]; g.ldw = w.d; g.C = b.xi; g.ldc = w.dim[i];
        g.M = (int)n; g.N = w.dim[i]; g.K = w.d; g.m_dev = cnt;
        GNNLM_TRY(gemm_nt(g, s));
        GemmParams t{};
        t.A = b.xi; t.lda = w.dim[i]; t.W = w.emb[i]; t.ldw = w.dim[i];
        t.lse_part = b.tail_part; t.lse_pick = pick; t.lse_picked = b.tail_picked;
        t.M = (int)n; t.N = size; t.K = w.dim[i]; t.m_dev = cnt;
        GNNLM_TRY(gemm_nt(t, s));
        GNNLM_TRY(lse_reduce(b.tail_part, 2 * (int)cdiv(size, 128), n, cnt, b.tail_lse, s));
        GNNLM_TRY(tail_combine(b.tail_picked, b.tail_lse, rows, cnt, n, lm_logp, s));
    }
    return OK;
}

}  // namespace
}  // namespace gnnlm

using namespace gnnlm;

extern "C" {

size_t gnnlm_adaptive_workspace_bytes(const gnnlm_adaptive_softmax_t* w, int64_t n) {
    if (!w) return 0;
    Carver c(nullptr);
    AsmBufs b;
    carve_asm(*w, n, c, b);
    return c.off + 256;
}
int gnnlm_adaptive_target_logp(const gnnlm_adaptive_softmax_t* w, const float* x, int64_t ldx, const int64_t* target,
                               int64_t n, float* lm_logp, void* workspace, size_t workspace_bytes, void* stream) {
    GNNLM_DESC(w);
    return adaptive_impl(*w, x, ldx, target, n, lm_logp, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
