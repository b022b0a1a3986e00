// Which kernel gnnlm_gemm_nt launches for a problem, on what tile and grid, and the order a kernel visits its tiles in: the
// one place where the nine routes of the f32 "NT" GEMM are chosen.  Plain C++17, no HIP: gemm.hip asks gemm_route() before
// its switch, the kernels share gemm_tile_walk(), and tests/gemm_route_main.cpp builds this header alone with a host compiler.
//
//   route      kernel (file)                                    tile      threads  grid
//   reg64      gemm_nt_f32_kernel<64, 64>    (gemm_f32.hip)      64 x 64   256      min(tiles, 1024)
//   reg128     gemm_nt_f32_kernel<128, 128>  (gemm_f32.hip)      128 x 128 256      min(tiles, 768; bf16x6: 512)
//   sched128   gemm_nt_f32_sched_kernel      (gemm_f32_sched.hip) 128 x 128 256     min(tiles, 512)
//   dma128     gemm_nt_f32_dma_kernel<.,128> (gemm_f32_dma.hip)  128 x 128 256      min(tiles, 512)
//   dma256     gemm_nt_f32_dma_kernel<.,256> (gemm_f32_dma.hip)  256 x 256 512      min(tiles, 256)
//   astat128   gemm_lse_astationary_kernel   (gemm_f32_dma.hip)  128 x 128 256      768
//   skinny32   gemm_nt_f32_skinny_kernel     (gemm_f32_skinny.hip) 32 x 32 256      tiles
//   split128   gemm_planes_kernel<128>       (gemm_split.hip)    128 x 128 256      tiles (m_dev: min(tiles, 512))
//   split256   gemm_planes_kernel<256>       (gemm_split.hip)    256 x 256 512      tiles (m_dev: min(tiles, 512))
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include "../../include/gnnlm.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GNNLM_HD __host__ __device__
#else
#define GNNLM_HD
#endif

namespace gnnlm {

enum class GemmRoute : int { NONE, REG64, REG128, SCHED128, DMA128, DMA256, ASTAT128, SKINNY32, SPLIT128, SPLIT256 };
constexpr int N_GEMM_ROUTES = 10;

// tile edge and threads per workgroup of every route, with its name
struct GemmGeometry { const char* name; int tile, threads; };
constexpr GemmGeometry GEMM_GEOMETRY[N_GEMM_ROUTES] = {
    {"none", 0, 0},          {"reg64", 64, 256},      {"reg128", 128, 256},   {"sched128", 128, 256}, {"dma128", 128, 256},
    {"dma256", 256, 512},    {"astat128", 128, 256},  {"skinny32", 32, 256},  {"split128", 128, 256}, {"split256", 256, 512}};
inline const GemmGeometry& gemm_geometry(GemmRoute r) { return GEMM_GEOMETRY[(int)r]; }

// ---------------------------------------------------------------------------------------------- the thresholds
constexpr int MAX_TILE_ORDER = 66;         // tile_order 2 + GM, GM in 1..64
// register-staged kernel (gemm_f32.hip): 128x128 tiles unless they would leave CUs without a workgroup (256 CUs); the log-sum-exp
// epilogue exists for 128-wide tiles only, so such a problem is never `small`
constexpr int SMALL_TILES = 256;
// big-tile split-bf16 / fp16 path (gemm_split.hip): precision != 0 when the problem fills the chip
constexpr int SPLIT_MIN_K = 256;
constexpr int SPLIT_MIN_TILES = 256;       // 128x128 tiles
// 256x256 tiles when they still give every CU >= 2 workgroups over the launch.  A device-side M is a small fraction of its bound
// where the bound is a token count (the softmax tails: 128-tiles), and of the order of the bound where it counts the slot rows
// of a batch's context groups (ABI 9: the ntgt projections of a multi-layer step, M >= 2^17 -- merged groups are a good
// third of all groups or more): those keep the big tiles (22.2 k -> 25 k tokens/s on the 3-layer recipe under bf16x3)
constexpr int SPLIT_BIG_TILES = 512;       // 256x256 tiles
constexpr int SPLIT_MDEV_BIG_M = 1 << 17;
// narrow outputs (gemm_f32_skinny.hip): decided from N, K and the batch only -- never from the row count, because the k split over
// the waves changes the summation order and a row's bits may not depend on how many rows its launch carries
constexpr int SKINNY_MAX_N = 256;
constexpr int SKINNY_K_MULT = 32;
constexpr int SKINNY_MIN_K = 512;
// hand-placed main loop (gemm_f32_sched.hip): exact f32, K a multiple of 64 (the loop runs stage pairs), 128x128 tiles filling
// the chip, rows addressed with 32-bit byte offsets inside the panel.  K = 128 (absorbed queries): 191 us on the register-staged
// kernel, 206 there, hence the smallest K (GNNLM_GEMM_SCHED_MINK moves it)
constexpr int SCHED_MIN_K = 256;
constexpr int SCHED_K_MULT = 64;
// the softmax head (>= 2048 tiles of 256x256) runs in the same time there as on the 256x256 LDS-DMA kernel (2.47 ms), but with
// 128-wide W panels it pulls the A panel through the fabric twice as often (PMC FETCH_SIZE 2.9 vs 1.4 GB): stays on dma256
constexpr int SCHED_HEAD_TILES = 2048;
// LDS-DMA staged main loop (gemm_f32_dma.hip).  Where it pays, measured per launch inside the step (rocprofv3 trace, us;
// register-staged -> LDS-DMA): LSE head 8192x20002x1024 2689 -> 2571, tail band 1 147 -> 147; store epilogue: projections
// 146 -> 145, absorbed queries (K = 128) 191 -> 209, 163840x1024x1024 of the 3-layer path 127.7 -> 123.4 TFLOP/s.  So the LSE
// problems take it and the store-epilogue problems stay on the register-staged kernel ...
// ... except the head-sized ones, which get the 256x256 tiles: 655360x1024x1024 (3-layer path) 123 -> 128 TFLOP/s
// ... and (tools/gemm_bench.py step8k, us: register-staged -> LDS-DMA, 128x128 tiles) the step's K = 1024 problems
// 8192x1024x1024 169 -> 157, 8192x3072x1024 (Q, K, V in one) 464 -> 436, Z Wvz (batch 8, N = 128) 150 -> 142; K = 128
// (absorbed queries) stays where it is (200 -> 218).  A store problem with a device-side row count never takes it.
// Sending every store problem there and switching the route off were build-time A/B switches once; the figures above are their verdict.
constexpr int DMA_BK = 32;                 // k per stage: BK = 16 (4 WG/CU) measured 126.8 against 136.3 TFLOP/s at 4096^3
constexpr int DMA_BIG_TILES = 2048;        // 256x256 tiles from this many of them on (8 per CU)
constexpr int DMA_MIN_K = 128;
constexpr int DMA_STORE_MIN_K = 512;       // store problems below it only with the big tiles
// A-stationary kernel for short-K log-sum-exp problems (the 207,744-word tail band: K = 64, ~1000 live rows); its grid is 768
// workgroups, at least one per m-tile
constexpr int ASTAT_K = 64;
constexpr int ASTAT_GRID = 768;
constexpr int ASTAT_MAX_M = 128 * ASTAT_GRID;

// ---------------------------------------------------------------------------------------------- the runtime switches
// GNNLM_GEMM_SCHED (A/B runs): 0 = never the hand-placed loop, 1 = store-epilogue problems only, 3 (default) = log-sum-exp
// problems too, 7 = the softmax head as well.  GNNLM_GEMM_SCHED_MINK: smallest K of that kernel.  GNNLM_GEMM_SKINNY=0: narrow
// outputs stay on the 64x64 tiles.
struct GemmSwitches { int sched = 3, sched_min_k = SCHED_MIN_K, skinny = 1; };
inline GemmSwitches gemm_switches_from_env() {
    GemmSwitches s;
    if (const char* e = getenv("GNNLM_GEMM_SCHED")) s.sched = atoi(e);
    if (const char* e = getenv("GNNLM_GEMM_SCHED_MINK")) s.sched_min_k = atoi(e);
    if (const char* e = getenv("GNNLM_GEMM_SKINNY")) s.skinny = atoi(e);
    return s;
}
// read once per process
inline const GemmSwitches& gemm_switches() {
    static const GemmSwitches s = gemm_switches_from_env();
    return s;
}

inline int64_t gemm_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------------------------- the dispatcher
// p is normalised (precision resolved, alpha and the batch counts non-zero) and accepted by gemm_nt's refusals.  No side effects.
inline GemmRoute gemm_route(const gnnlm_gemm_t& p, const GemmSwitches& sw) {
    if (p.M == 0) return GemmRoute::NONE;
    const int64_t nb = (int64_t)p.batch1 * p.batch2;
    const bool lse = p.lse_part != nullptr, m_dev = p.m_dev != nullptr;
    const int64_t tiles128 = gemm_cdiv(p.M, 128) * gemm_cdiv(p.N, 128), tiles256 = gemm_cdiv(p.M, 256) * gemm_cdiv(p.N, 256);

    // pre-split planes + LDS-DMA
    if (p.precision != 0 && nb == 1 && p.K >= SPLIT_MIN_K && tiles128 >= SPLIT_MIN_TILES)
        return (!m_dev || p.M >= SPLIT_MDEV_BIG_M) && tiles256 >= SPLIT_BIG_TILES ? GemmRoute::SPLIT256 : GemmRoute::SPLIT128;
    // narrow outputs: 32x32 tiles, k split over the waves
    if (sw.skinny && p.precision == 0 && !lse && nb == 1 && p.N <= SKINNY_MAX_N && p.K % SKINNY_K_MULT == 0 && p.K >= SKINNY_MIN_K)
        return GemmRoute::SKINNY32;
    if (!lse && tiles128 * nb < SMALL_TILES) return GemmRoute::REG64;

    // hand-placed main loop; rows are addressed by 32-bit byte offsets from the panel base of the tile's batch, and gathered rows
    // index [0, a_rows_bound)
    const int64_t a_rows = p.a_rows ? p.a_rows_bound : (int64_t)p.M;
    if (sw.sched && p.precision == 0 && !(lse && !(sw.sched & 2)) &&
        !(lse && !m_dev && !(sw.sched & 4) && tiles256 >= SCHED_HEAD_TILES) &&
        p.K % SCHED_K_MULT == 0 && p.K >= sw.sched_min_k && tiles128 * nb >= SMALL_TILES &&
        (int64_t)p.N * p.ldw * 4 < (1ll << 32) && a_rows > 0 && a_rows * p.lda * 4 < (1ll << 32))
        return GemmRoute::SCHED128;

    // LDS-DMA staged main loop
    if (lse || !(m_dev || (p.K < DMA_STORE_MIN_K && tiles256 * nb < DMA_BIG_TILES))) {
        if (p.precision == 0 && p.K == ASTAT_K && lse && nb == 1 && p.M <= ASTAT_MAX_M) return GemmRoute::ASTAT128;
        if (p.precision == 0 && p.K % DMA_BK == 0 && p.K >= DMA_MIN_K)
            return !m_dev && tiles256 * nb >= DMA_BIG_TILES ? GemmRoute::DMA256 : GemmRoute::DMA128;
    }
    return GemmRoute::REG128;
}

// (batch, tile) pairs of the launch
inline int64_t gemm_tiles(GemmRoute r, const gnnlm_gemm_t& p) {
    const int t = gemm_geometry(r).tile;
    return t ? gemm_cdiv(p.M, t) * gemm_cdiv(p.N, t) * ((int64_t)p.batch1 * p.batch2) : 0;
}

// Workgroups of the launch.  The kernels that walk a tile list run a pool of resident workgroups: 256 CUs x the kernel variant's
// workgroups per CU (a multiple of 8 = XCDs).
inline int64_t gemm_grid(GemmRoute r, const gnnlm_gemm_t& p, int64_t tiles) {
    const auto pool = [&](int64_t n) { return tiles < n ? tiles : n; };
    switch (r) {
        case GemmRoute::REG64: return pool(256 * 4);
        case GemmRoute::REG128: return pool(256 * (p.precision == 2 ? 2 : 3));
        case GemmRoute::SCHED128: return pool(512);
        case GemmRoute::DMA128: return pool(256 * 2);
        case GemmRoute::DMA256: return pool(256 * 1);
        case GemmRoute::ASTAT128: return ASTAT_GRID;
        case GemmRoute::SKINNY32: return tiles;
        case GemmRoute::SPLIT128:
        case GemmRoute::SPLIT256: return p.m_dev ? pool(512) : tiles;
        case GemmRoute::NONE: break;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- the tile walk
// tile_order 0 (auto): consecutive tiles share the panel of the larger operand.  Resolved before the dispatch, never part of it.
inline int gemm_tile_order(const gnnlm_gemm_t& p) {
    return p.tile_order ? p.tile_order : (!p.m_dev && (double)p.M > (double)p.N) ? 1 : 2;
}

// List position t -> tile (tm, tn) of a tiles_m x tiles_n problem, tile_order resolved (1: n fastest, 2: m fastest, 2 + GM: bands of
// GM m-tiles; inside a band n is the slow index, the last band may be short).  One text for the kernels and the host test.
// The text is a macro so that the register-staged kernel (gemm_f32.hip) can expand it in place: called as a function there, the
// same arithmetic comes out of the compiler with another register allocation.  Everything else calls gemm_tile_walk().
#define GNNLM_TILE_WALK(order_, t_, tiles_m_, tiles_n_, tm_, tn_)                            \
    if ((order_) == 1) { tm_ = (t_) / (tiles_n_); tn_ = (t_) % (tiles_n_); }                 \
    else if ((order_) == 2) { tn_ = (t_) / (tiles_m_); tm_ = (t_) % (tiles_m_); }            \
    else {                                                                                   \
        const int GM_ = (order_) - 2;                                                        \
        const int band_ = (t_) / (GM_ * (tiles_n_));                                         \
        const int rest_ = (tiles_m_) - band_ * GM_;                                          \
        const int m_in_ = GM_ < rest_ ? GM_ : rest_;                                         \
        const int r_ = (t_) - band_ * GM_ * (tiles_n_);                                      \
        tn_ = r_ / m_in_;                                                                    \
        tm_ = band_ * GM_ + r_ % m_in_;                                                      \
    }
GNNLM_HD inline void gemm_tile_walk(int tile_order, unsigned t, int tiles_m, int tiles_n, int& tm, int& tn) {
    GNNLM_TILE_WALK(tile_order, t, tiles_m, tiles_n, tm, tn)
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------- pieces the kernels share
// Taken by a kernel file only where its machine code stays what the pasted copy gave (checked per file on the device assembly): the
// MFMA step passes that everywhere; a shared work-list prologue and a shared clamped A-row index changed the register allocation of
// the register-staged, LDS-DMA, skinny and split kernels, so those few lines stay written out in each kernel.

// Four k of one 32x32 accumulator on the f32 matrix cores; SWAP (the log-sum-exp epilogue) exchanges the operands, which leaves the
// transposed tile in the accumulator (gemm_epilogue.inc).
template <bool SWAP, typename Acc>
__device__ __forceinline__ void gemm_mfma4(Acc& acc, const float4& a, const float4& b) {
    if constexpr (SWAP) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.x, a.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.y, a.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.z, a.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b.w, a.w, acc, 0, 0, 0);
    } else {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
}
#endif

}  // namespace gnnlm
