// Asks csrc/gemm_route.h from the command line (tests/test_gemm_ref_cpu.py builds this with a host compiler):
//   route      stdin, one normalised descriptor per line: M N K precision lse m_dev batch1 batch2 lda ldw a_rows a_rows_bound tile_order
//              (lse, m_dev, a_rows: 0 / 1 = pointer absent / present) -> "<route name> <resolved tile_order>"; the switches come
//              from the environment as in the library
//   walk O TM TN   the tile walk of order O over TM x TN tiles: "tm tn" per list position
//   constants  "NAME value" per dispatch constant
#include <stdio.h>
#include <string.h>

#include "../gnn-lm_amd/csrc/gemm_route.h"

using namespace gnnlm;

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!strcmp(mode, "constants")) {
#define C(name) printf(#name " %d\n", (int)name);
        C(DMA_BK) C(DMA_BIG_TILES) C(DMA_MIN_K) C(DMA_STORE_MIN_K) C(ASTAT_K) C(ASTAT_MAX_M) C(SCHED_MIN_K) C(SCHED_K_MULT)
        C(SCHED_HEAD_TILES) C(SKINNY_MAX_N) C(SKINNY_K_MULT) C(SKINNY_MIN_K) C(SPLIT_MIN_K) C(SPLIT_MIN_TILES) C(SPLIT_BIG_TILES)
        C(SPLIT_MDEV_BIG_M) C(SMALL_TILES) C(MAX_TILE_ORDER)
        return 0;
    }
    if (!strcmp(mode, "walk") && argc == 5) {
        const int order = atoi(argv[2]), tiles_m = atoi(argv[3]), tiles_n = atoi(argv[4]);
        for (unsigned t = 0; t < (unsigned)(tiles_m * tiles_n); ++t) {
            int tm = -1, tn = -1;
            gemm_tile_walk(order, t, tiles_m, tiles_n, tm, tn);
            printf("%d %d\n", tm, tn);
        }
        return 0;
    }
    if (strcmp(mode, "route")) return 2;
    static float part;
    static int32_t count, rows;
    long long M, N, K, prec, lse, m_dev, b1, b2, lda, ldw, a_rows, bound, order;
    while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &M, &N, &K, &prec, &lse, &m_dev, &b1, &b2, &lda, &ldw,
                 &a_rows, &bound, &order) == 13) {
        gnnlm_gemm_t p = {};
        p.M = (int32_t)M; p.N = (int32_t)N; p.K = (int32_t)K; p.precision = (int32_t)prec; p.batch1 = (int32_t)b1; p.batch2 = (int32_t)b2;
        p.lda = lda; p.ldw = ldw; p.a_rows_bound = bound; p.tile_order = (int32_t)order; p.alpha = 1.f;
        p.lse_part = lse ? &part : nullptr; p.m_dev = m_dev ? &count : nullptr; p.a_rows = a_rows ? &rows : nullptr;
        printf("%s %d\n", gemm_geometry(gemm_route(p, gemm_switches())).name, gemm_tile_order(p));
    }
    return 0;
}
