// What the stages of the int8 IVF-PQ search (ivfpq8_prep.hip, ivfpq8_scan.hip, ivfpq8_rescore.hip) and the host that allocates
// their buffers (IVFPQIndex in ivfpq.py) have to agree on: buffer sizes, the survivor record, the launch arithmetic of the entry
// points.  Plain C++17, no HIP: tests/ivfpq8_layout_main.cpp builds this header alone with a host compiler, and
// tests/test_ivfpq8_layout_cpu.py holds IVFPQIndex's constants against it.
//   buffer                     shape (host)                 written by                       read by
//   qlut u8, qmeta f32         [n, 2, 256, 32], [n, 4]      quantize_lut / ivfpq_tables      scan8; qmeta: tau, refine too
//   grp_list / grp_q / grp_out [G], [G, QG], [G, QG]        build_groups (G: groups_cap)     scan8
//   hist u32                   [n, D, HIST_BINS]            scan8<SUMS>                      tau
//   surv u32                   [n, cap, 2]  (SurvRec)       scan8 (filter)                   refine, rescore
//   surv_cnt / out_cnt i32     [n, SURV_CNT_STRIDE]         scan8 (filter) / refine          refine, rescore, host
//   work_ctr i32               [8 XCDs, 16]                 host (zeros)                     scan8: the persistent workgroups' group counters
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GNNLM_HD __host__ __device__
#else
#define GNNLM_HD
#endif

namespace gnnlm {

constexpr int QG = 8;                                   // queries per workgroup of the scan = per group of the task table
constexpr int TQ = 32;                                  // queries per workgroup of the tables kernel (= the MFMA's rows)
constexpr int QLUT_BYTES = 64 * 256;                    // one query's quantised table: [half][code][32 slots] bytes
constexpr int TAB_BYTES = 2 * 256 * 32 * QG;            // the scan's LDS tables, [half][code][slot][query]: 128 KiB
#ifndef GNNLM_IVF8_WAVE_CAP
#define GNNLM_IVF8_WAVE_CAP 240                         // (a tuning macro of the filter; here because the filter's LDS size follows from it)
#endif
constexpr int WAVE_CAP = GNNLM_IVF8_WAVE_CAP;           // KEY entries (8 bytes: a key of the tile with its four queries' excesses) a wave stages per task
constexpr int SCAN_CTL = 768;                           // behind the tables: [16 waves][8] flush counters, then {counters, thresholds, queries}[8] of the group, twice (groups alternate)
constexpr int SCAN_LDS = TAB_BYTES + SCAN_CTL + 16 * WAVE_CAP * 8;
constexpr int HIST_BINS = 1024, HIST_SHIFT = 4;         // threshold pass: sum_u (0 .. 16320) >> 4
constexpr int SUMS_LDS = TAB_BYTES + QG * HIST_BINS * 4;  // = 160 KiB: the whole LDS of a CU
constexpr int SURV_CNT_STRIDE = 16;                     // survivor counters one per 64-byte line: they are hammered by atomics
static_assert(TAB_BYTES == QG * QLUT_BYTES, "a group's LDS tables are its queries' byte tables, interleaved");
static_assert(SCAN_LDS <= 160 * 1024 && SUMS_LDS <= 160 * 1024, "the scan's tables + staging regions / histograms exceed a CU's LDS");

// a survivor record is {row, list | sum_u << 18}: the key's integer sum (14 bits; SURV_SUM_BIG = "at least threshold + 254": the
// wave's LDS staging entry has one byte per query for the distance to the threshold) above an 18-bit list
constexpr int SURV_ROW_BITS = 19, SURV_LIST_BITS = 18, SURV_EXCESS_MAX = 254, SURV_SUM_BIG = 16383;
static_assert(SURV_SUM_BIG == (1 << (32 - SURV_LIST_BITS)) - 1 && SURV_SUM_BIG > 16320, "list and sum share the record's second word");
struct SurvRec { uint32_t row, word; };
GNNLM_HD constexpr SurvRec surv_pack(uint32_t row, uint32_t list, uint32_t sum) { return SurvRec{row, list | sum << SURV_LIST_BITS}; }
GNNLM_HD constexpr uint32_t surv_list(uint32_t word) { return word & ((1u << SURV_LIST_BITS) - 1u); }
GNNLM_HD constexpr uint32_t surv_sum(uint32_t word) { return word >> SURV_LIST_BITS; }

constexpr int64_t ivf8_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
// build_groups: rows of the task table for n queries with P probes each (every list's last group may be partly filled), and the
// threads of its fill launch (the table's slots, or the two [nlist + 1] scratch arrays)
constexpr int64_t groups_cap(int64_t n, int64_t P, int64_t nlist) { return n * P / QG + nlist + 1; }
constexpr int64_t groups_fill(int64_t G, int64_t nlist) { return G * QG > 2 * (nlist + 1) ? G * QG : 2 * (nlist + 1); }
// scan8: persistent workgroups, one per CU, a multiple of 8 (workgroup b runs on XCD b % 8 and walks that XCD's range of groups)
constexpr int64_t scan8_grid(int64_t max_groups, int64_t cus) {
    const int64_t by_groups = 8 * ivf8_cdiv(max_groups, 8), by_cus = 8 * ivf8_cdiv(cus > 8 ? cus : 8, 8);
    return by_groups < by_cus ? by_groups : by_cus;
}
constexpr size_t scan8_lds(bool sums) { return sums ? SUMS_LDS : SCAN_LDS; }
// rescore: the query's f32 table [M][256], then one code row per thread
constexpr size_t rescore_lds(int M, int threads) { return (size_t)M * 256 * 4 + (size_t)threads * M; }
constexpr int64_t tables_grid(int64_t n) { return ivf8_cdiv(n, TQ); }

#if defined(__HIPCC__)
// (shared by the filter and the refinement) The integer image of a query's threshold for one list: a key can score above tau only if the MFMA's sum (sum_u - 128 * 64: the
// table bytes are u - 128) reaches it.  eps: rounding of the f32 score chain (65 adds), of sum_lo and of this formula's
// subtractions: (M + 2) 2^-22 sum |terms|.  survive iff sum_u + 64 > thr' with thr' in (thr - 1, thr + 1)
__device__ __forceinline__ int filter_threshold(const float* __restrict__ qmeta, int64_t q, float bias, float tau) {
    const float delta = qmeta[q * 4], sum_lo = qmeta[q * 4 + 1], amax = qmeta[q * 4 + 2];
    const float eps = 66.f * 2.3841858e-7f * (64.f * amax + fabsf(bias) + (fabsf(tau) < INFINITY ? fabsf(tau) : 0.f));
    const float thr = ((tau - bias) - sum_lo - eps) / delta - 64.f;
    return !(thr == thr) || thr <= -1.0e9f ? -(1 << 30) : (thr >= 1.0e9f ? 0x7fffffff : (int)floorf(thr) - 128 * 64);
}
#endif

}  // namespace gnnlm
