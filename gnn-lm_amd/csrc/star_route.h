// Which kernel gnnlm_star_attn launches for a shape, with how much LDS and how many threads: the one place where the routes
// of the star attention are chosen.  Plain C++17, no HIP: star_attn() (star_attn.hip) asks star_route() before its switch, the
// three kernel files take their constants and LDS layouts from here, and tests/star_route_main.cpp builds this header alone
// with a host compiler.
//
//   route         kernel (file)                             source  shape                                        tokens / workgroup
//   tab<8,128>    star_attn_tab_kernel<8, 128> (star_tab.hip)   PQ   k_g <= 128, dsub 8, M = 128                   4
//   tab<8,0>      star_attn_tab_kernel<8, 0>   (star_tab.hip)   PQ   k_g <= 128, dsub 8, M % 16 == 0               4
//   tab<4,0>      star_attn_tab_kernel<4, 0>   (star_tab.hip)   PQ   k_g <= 128, dsub 4, M % 16 == 0, LDS <= 160 KiB  4
//   dense<n>      star_dense_kernel<n>         (star_dense.hip) X    D = 256 n, n in {1, 2, 4}, H <= 8, LDS <= 64 KiB  1
//   generic<n>    star_attn_kernel<n>          (star_attn.hip)  any  everything else; n float4 of the row per lane  1
// star_attn() has already refused what no kernel reads safely (16-byte alignment of U, Z, X, the centroids and the code rows
// the kernels load 16 bytes at a time), so the route is a function of the shape and the source alone.
#pragma once
#include <stddef.h>
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

enum class StarRoute : int { NONE, TAB8M, TAB8, TAB4, DENSE1, DENSE2, DENSE4, GENERIC1, GENERIC2, GENERIC4 };
constexpr int N_STAR_ROUTES = 10;
constexpr const char* STAR_ROUTE_NAME[N_STAR_ROUTES] = {"none",     "tab<8,128>", "tab<8,0>",   "tab<4,0>",   "dense<1>",
                                                        "dense<2>", "dense<4>",   "generic<1>", "generic<2>", "generic<4>"};
inline const char* star_route_name(StarRoute r) { return STAR_ROUTE_NAME[(int)r]; }
inline bool star_route_is_tab(StarRoute r) { return r == StarRoute::TAB8M || r == StarRoute::TAB8 || r == StarRoute::TAB4; }

// ---------------------------------------------------------------------------------------------- the constants
constexpr int HB = 8;                   // heads per pass (generic, dense) / per launch (tab)
constexpr int KGM = 128;                // tab: neighbours per token (padded)
constexpr int CD = 32;                  // tab: feature dims per chunk
constexpr int TPW = 4;                  // tab: tokens per workgroup
constexpr int TABF = CD * 256;          // tab: floats per table chunk (32 KiB)
constexpr int SCS = KGM + 4;            // tab: score row stride -- the heads of a token land on different banks
constexpr int STAR_THREADS = 256;       // generic, dense: 4 waves per token
constexpr int STAR_TAB_THREADS = 768;   // tab: 8 compute waves (two per token) + 4 loader waves (table and U in, Z out)
constexpr int STAR_LDS_MAX = 160 * 1024;        // what a workgroup can have
constexpr int STAR_LDS_TWO_WG = 64 * 1024;      // generic, dense: keep >= 2 workgroups per CU

// ---------------------------------------------------------------------------------------------- LDS layouts
// tab: byte offsets of the table-resident kernel's buffers
struct Carve {
    int tab, sc, ubuf, okf, lcodes, total;      // byte offsets
};
GNNLM_HD inline Carve carve(int M) {
    Carve c;
    c.tab = 0;
    c.sc = c.tab + 2 * TABF * 4;
    c.ubuf = c.sc + TPW * HB * SCS * 4;
    c.okf = c.ubuf + 2 * TPW * 1024;
    c.lcodes = c.okf + TPW * KGM;
    c.total = c.lcodes + TPW * KGM * M;
    return c;
}
// dense: [HB][D] query rows, [4 waves][HB][2] softmax states, [kg] int64 rows
inline size_t star_dense_lds_bytes(int D, int kg) { return (size_t)(HB * D + 4 * HB * 2) * sizeof(float) + (size_t)kg * sizeof(int64_t); }
// generic: [HB][kg] scores, [HB][D] cross-wave sums, [kg] validity; then the token's code rows (PQ source, when staged)
inline size_t star_generic_base_lds(int D, int kg) { return (size_t)(HB * kg + HB * D + ((kg + 3) & ~3)) * sizeof(float); }
inline size_t star_generic_code_lds(int M, int kg) { return ((size_t)kg * M + 15) & ~size_t(15); }

// ---------------------------------------------------------------------------------------------- the runtime switch
// GNNLM_STAR_GENERIC (A/B runs, any value): the generic kernel instead of the table-resident and the dense one.  Mapped shards
// have no other kernel than the table-resident one and keep it.
struct StarSwitches { bool generic = false; };
inline StarSwitches star_switches_from_env() {
    StarSwitches s;
    s.generic = getenv("GNNLM_STAR_GENERIC") != nullptr;
    return s;
}
// read once per process
inline const StarSwitches& star_switches() {
    static const StarSwitches s = star_switches_from_env();
    return s;
}

// ---------------------------------------------------------------------------------------------- the dispatcher
struct StarPlan {
    StarRoute route = StarRoute::NONE;
    bool staged = false;            // generic, PQ source: the token's code rows are staged in LDS (else read from the store)
    size_t lds_bytes = 0;           // dynamic LDS of the launch
    int threads = 0;                // workgroup size
    int heads_per_pass = HB;        // tab: heads per launch; generic: per pass inside the kernel; dense: all of them (H <= HB)
};

// p is accepted by star_attn's refusals (one source, M * dsub == D, dsub % 4 == 0, the alignments).  No side effects.  A plan
// whose lds_bytes exceed STAR_LDS_MAX (a generic launch with a very large k_g) is for star_attn to refuse.
inline StarPlan star_route(const gnnlm_star_attn_t& p, const StarSwitches& sw) {
    StarPlan plan;
    if (p.T == 0) return plan;
    const bool pq = p.codes || p.shards;
    // table-resident formulation: the default for the PQ source with k_g <= 128
    if (pq && (p.shards || !sw.generic) && p.kg <= KGM && (p.dsub == 4 || p.dsub == 8) && p.M % 16 == 0 && p.D % CD == 0 &&
        carve(p.M).total <= STAR_LDS_MAX) {
        plan.route = p.dsub == 4 ? StarRoute::TAB4 : p.M == 128 ? StarRoute::TAB8M : StarRoute::TAB8;
        plan.lds_bytes = (size_t)carve(p.M).total;
        plan.threads = STAR_TAB_THREADS;
        return plan;
    }
    plan.threads = STAR_THREADS;
    // dense rows at the recipe's widths: one pass over the rows.  The LDS bound is part of the choice: a shape with a very large
    // k_g keeps the generic two-pass kernel
    if (!pq && !sw.generic && p.H <= HB && (p.D == 256 || p.D == 512 || p.D == 1024) &&
        star_dense_lds_bytes(p.D, p.kg) <= (size_t)STAR_LDS_TWO_WG) {
        plan.route = p.D == 1024 ? StarRoute::DENSE4 : p.D == 512 ? StarRoute::DENSE2 : StarRoute::DENSE1;
        plan.lds_bytes = star_dense_lds_bytes(p.D, p.kg);
        return plan;
    }
    const int nq = p.D / 4;
    plan.route = nq <= 64 ? StarRoute::GENERIC1 : nq <= 128 ? StarRoute::GENERIC2 : StarRoute::GENERIC4;
    const size_t base = star_generic_base_lds(p.D, p.kg), code = p.codes ? star_generic_code_lds(p.M, p.kg) : 0;
    plan.staged = p.codes && base + code <= (size_t)STAR_LDS_TWO_WG;
    plan.lds_bytes = base + (plan.staged ? code : 0);
    return plan;
}

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------- pieces the kernels share
// Sum 8 per-lane partials over the 64 lanes with a transposing butterfly: 10 shuffles instead of 48.
// On return lane 8*h holds the total of v[h].  (generic and dense kernel)
__device__ __forceinline__ float reduce8(const float (&v)[HB], int lane) {
    const bool b5 = lane & 32, b4 = lane & 16, b3 = lane & 8;
    float w[4], y[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const float send = b5 ? v[t] : v[t + 4];
        const float keep = b5 ? v[t + 4] : v[t];
        w[t] = keep + __shfl_xor(send, 32, 64);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float send = b4 ? w[t] : w[t + 2];
        const float keep = b4 ? w[t + 2] : w[t];
        y[t] = keep + __shfl_xor(send, 16, 64);
    }
    float r;
    {
        const float send = b3 ? y[0] : y[1];
        const float keep = b3 ? y[1] : y[0];
        r = keep + __shfl_xor(send, 8, 64);
    }
    r += __shfl_xor(r, 4, 64);
    r += __shfl_xor(r, 2, 64);
    r += __shfl_xor(r, 1, 64);
    return r;
}
#endif

}  // namespace gnnlm
