// gnnlm_gemm_nt on the host: normalise the descriptor, refuse what the contract refuses, ask gemm_route.h which kernel, tile
// and grid the problem takes, and launch it.  The kernels and their launchers live in gemm_f32.hip (register-staged),
// gemm_f32_sched.hip (hand-placed main loop), gemm_f32_dma.hip (LDS-DMA staging, A-stationary), gemm_f32_skinny.hip (narrow
// outputs) and gemm_split.hip (pre-split bf16 / fp16 planes); which shapes go where is written in gemm_route.h and nowhere else.
#include "gemm_route.h"
#include "kernels.h"

namespace gnnlm {

thread_local int g_default_gemm_precision = 0;

int gemm_nt(const GemmParams& desc, hipStream_t stream) {
    GemmParams p = desc;
    if (p.precision == 0) p.precision = g_default_gemm_precision;
    if (p.alpha == 0.f) p.alpha = 1.f;
    if (p.batch1 == 0) p.batch1 = 1;
    if (p.batch2 == 0) p.batch2 = 1;
    GNNLM_REQUIRE(p.A && p.W && (p.C || p.lse_part), "gemm: null operand");
    GNNLM_REQUIRE(p.M >= 0 && p.N > 0 && p.K > 0, "gemm: bad shape");
    GNNLM_REQUIRE(p.K % 4 == 0 && p.lda % 4 == 0 && p.ldw % 4 == 0, "gemm: K, lda, ldw must be multiples of 4");
    GNNLM_REQUIRE(((uintptr_t)p.A % 16 == 0) && ((uintptr_t)p.W % 16 == 0), "gemm: operands must be 16-byte aligned");
    GNNLM_REQUIRE(p.sA1 % 4 == 0 && p.sA2 % 4 == 0 && p.sW1 % 4 == 0 && p.sW2 % 4 == 0, "gemm: batch strides must be multiples of 4");
    GNNLM_REQUIRE(p.batch1 >= 1 && p.batch2 >= 1, "gemm: bad batch");
    GNNLM_REQUIRE(p.precision >= 0 && p.precision <= 3, "gemm: precision must be 0 (f32 MFMA), 1 (bf16x3), 2 (bf16x6) or 3 (fp16)");
    GNNLM_REQUIRE(!p.lse_part || p.batch1 * p.batch2 == 1, "gemm: the LSE epilogue does not support batches");
    GNNLM_REQUIRE(!p.lse_part || p.alpha > 0.f, "gemm: the LSE epilogue needs alpha > 0");
    // the LSE epilogue reduces alpha * A.W^T and nothing else (gemm_epilogue.inc): operands it would drop are refused, not ignored
    GNNLM_REQUIRE(!p.lse_part || (!p.bias && !p.gate && !p.R && !p.c_rows), "gemm: the LSE epilogue takes no bias, gate, R or c_rows");
    GNNLM_REQUIRE(p.tile_order >= 0 && p.tile_order <= MAX_TILE_ORDER, "gemm: tile_order must be 0 (auto), 1 (n fastest), 2 (m fastest) or 2+GM (bands of GM m-tiles)");
    if (p.M == 0) return OK;
    p.tile_order = gemm_tile_order(p);

    const GemmRoute route = gemm_route(p, gemm_switches());
    const int64_t tiles = gemm_tiles(route, p);
    GNNLM_REQUIRE(tiles < (1ll << 31), "gemm: grid too large");
    const dim3 grid((unsigned)gemm_grid(route, p, tiles));
    const bool split = route == GemmRoute::SPLIT128 || route == GemmRoute::SPLIT256;
    GemmPlanes planes;
    if (split) {        // the plane pass is profiled as K_SPLIT, ahead of the GEMM's own scope
        const int rc = gemm_split_planes(route, p, stream, &planes);
        if (rc != OK) return rc;
    }

    const double nb = (double)p.batch1 * p.batch2;
    ProfScope prof(K_GEMM, stream, 2.0 * p.M * (double)p.N * p.K * nb,
                   4.0 * ((double)p.M * p.K + (double)p.N * p.K + (double)p.M * p.N) * nb, p.m_dev, (double)p.M, true);
    if (prof.slot) p.m_out = prof.slot;
    int rc = OK;
    switch (route) {
        case GemmRoute::REG64:
        case GemmRoute::REG128: gemm_launch_reg(route, p, grid, stream); break;
        case GemmRoute::SCHED128: rc = gemm_launch_sched(p, grid, stream); break;
        case GemmRoute::DMA128:
        case GemmRoute::DMA256:
        case GemmRoute::ASTAT128: rc = gemm_launch_dma(route, p, grid, stream); break;
        case GemmRoute::SKINNY32: gemm_launch_skinny(p, grid, stream); break;
        case GemmRoute::SPLIT128:
        case GemmRoute::SPLIT256: gemm_launch_split(route, p, planes, grid, stream); break;
        case GemmRoute::NONE: break;
    }
    if (rc != OK) return rc;
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
