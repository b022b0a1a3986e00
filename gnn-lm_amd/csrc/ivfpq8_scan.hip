// IVF-PQ list scan on the int8 matrix cores, M = 64 (the reference's kNN index `OPQ64_1024,IVF4096,PQ64`, nprobe 32:
// gnnlm_scripts/wiki103/find_knn.sh:8-13, searched by faiss on the CPU at knn/knn_model.py:100).
//
// The f32 scan of ivfpq.hip does one 8-byte LDS read per (two queries, key, sub-quantizer) and one packed add: it runs at
// the LDS read rate with 4 bytes per (query, key, sub-quantizer).  Here the scan is a FILTER followed by an exact
// re-score of what passes, and the filter needs one BYTE per (query, key, sub-quantizer):
//
//   * a query's ADC table is quantised to 8 bits with a guaranteed one-sided bound (quantize_lut_kernel, ivfpq8_prep.hip):
//         u[m][c] = min(255, floor((L[m][c] - lo_m) * inv)),   lo_m = min_c L[m][c],   L[m][c] < lo_m + (u + 1) delta
//     (stored as the signed byte u - 128: v_mfma_i32_*_i8 reads signed operands, the threshold absorbs the 128 * 64)
//     so that   score(q, x) = bias + sum_m L[m][code_m(x)]  <  bias + sum_lo + (sum_m u + M) delta + eps  =: UB(x);
//   * EIGHT queries that probe the same list share a workgroup; the LDS table entry of (sub-quantizer, code) is the 8
//     queries' bytes, so one ds_read_b64 serves 8 (query, key) pairs (LDS: 128 KiB of tables);
//   * the sums over the 64 sub-quantizers are taken by the matrix core: a lane's four look-ups ARE the 32-byte dense operand
//     of v_smfmac_i32_16x16x128_i8 (column = key, k = (look-up, query)), the other operand is the constant selector
//     S[query m][(look-up, query')] = [query' == m] -- two non-zeros in every four along k at most, i.e. exactly what the
//     2:4-SPARSE operand format holds: one instruction adds 16 keys x 16 sub-quantizers x 8 queries in the 16 busy cycles
//     the dense v_mfma_i32_16x16x64_i8 of round 3 took for half of that (PMC: SQ_VALU_MFMA_BUSY_CYCLES / SQ_INSTS_MFMA = 16.0
//     for both).  The integer sums are exact, the matrix core is the adder;
//   * a key survives for query j iff its integer sum reaches T_j = the integer image of the query's threshold tau (its
//     k-th best exact score after the dense round): UB(x) <= tau  =>  score(x) <= tau, so no key of the exact
//     one-pass scan (score > tau) is lost; survivors (row, list) are staged in LDS and appended to the query's list;
//   * ivfpq_rescore_kernel (ivfpq8_rescore.hip) then recomputes the survivors' scores in float32 IN THE SUMMATION ORDER OF THE
//     f32 SCAN (ivfpq.hip, scan_rot), keeps score > tau and emits (score, payload[row]): the candidate set and every candidate's
//     bits are those of the one-pass f32 scan -- the search result is identical, by construction and by test.
//
// Look-ups are bank-conflict free by the same rotation idea as ivfpq.hip: a tile is 16 keys; lane (g = lane / 16,
// i = lane % 16) owns sub-quantizers 16 g .. 16 g + 15 of key i and reads them in the order 16 g + (i + p) % 16, the table
// is stored [half][code][32 slots] x 8 B, so the 32 lanes of an LDS access group hit 32 different slots; the key bytes are
// stored in that rotated order (gnnlm_ivfpq_pack_tiles), and the LDS address of a look-up is one v_perm_b32.
// Here: the filter and the threshold pass (one kernel, two variants) and the kernel that turns the pass's histograms into tau.
// Before them: ivfpq8_prep.hip; after them: ivfpq8_rescore.hip; what the three share: ivfpq8_layout.h.
#include "kernels.h"
#include "ivfpq8_layout.h"

namespace gnnlm {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

#define GNNLM_PERM(hi_, lo_, sel_) __builtin_amdgcn_perm((hi_), (lo_), (sel_))
#ifndef GNNLM_IVF8_NW
#define GNNLM_IVF8_NW 16         // waves per workgroup of the scan (A/B: 8)
#endif
constexpr int NW = GNNLM_IVF8_NW, NTH = 64 * NW;
#ifndef GNNLM_IVF8_PF
#define GNNLM_IVF8_PF 3         // tiles of code bytes in flight per wave of the filter = steps per block of the loop (every register name is static).
                                // A/B with exact waits, medians of 7 searches: 3: 8.17 ms, 4: 9.06, 6: 8.82, 8: 9.21 -- depth buys nothing, the steps past
                                // the end of a list (up to PF - 1 per wave and group) cost
#endif
#ifndef GNNLM_IVF8_PF_SUMS
#define GNNLM_IVF8_PF_SUMS 3    // ... of the threshold pass
#endif
// (the ablation and phase-clock builds this kernel once carried, what they measured and how to re-create one: HISTORY.md, "The filter
// on the sparse matrix instruction, and what bounds it now")
// SUMS = false: the filter (survivors of the integer threshold).  SUMS = true: the threshold pass -- the integer sums sum_u of a
// list's keys are HISTOGRAMMED per query in LDS (bins of 16, atomics without return) and the (query, list) histogram is written
// to the segment grp_out names; nothing is compared, no per-key output.
// One `====` header per phase of a group.  It stays ONE function: the kernel sits at 128 VGPRs with a hand-pinned schedule, and the
// table fill and the selector as __device__ __forceinline__ functions (arguments by reference, by value or a returned struct alike)
// gave other register assignments in both variants and one more instruction in the threshold pass.
template <bool SUMS>
__global__ __launch_bounds__(NTH) void ivfpq_scan8_kernel(gnnlm_ivfpq_scan8_t p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];       // tables at LDS address 0 (look-up addresses are absolute)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // consecutive workgroups go to consecutive XCDs: give each XCD a contiguous range of the list-sorted groups
    // The workgroups are PERSISTENT (one per CU: the tables take the CU's LDS): workgroup b of XCD b % 8 walks the groups b / 8,
    // b / 8 + gridDim / 8, ... of its XCD's range -- the groups of one list are neighbours in that order, so they run side by
    // side on one XCD and share the list's bytes in its L2; no workgroup launch (and LDS allocation) between two groups.
    const int n_groups = min(*p.n_groups, p.max_groups);
    const int per_xcd = (n_groups + 7) >> 3;
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)smem != 0u) __builtin_trap();
    // The first group of a workgroup is b / 8; the next ones come from the XCD's counter (work_ctr: lists of different lengths
    // stay balanced) or, without one, by striding
    bool first = true;
    int gi = (int)(blockIdx.x >> 3);
    int* next_s = reinterpret_cast<int*>(smem + TAB_BYTES);                   // (free between two groups)
    int nxt = 0;                                                             // (thread 0) the counter's value for the group after this one
    int gi_next = 0, par = 0;
    // the index of the next group: thread 0's to everybody (three barriers; the filter's groups do this inside the two barriers their end has anyway)
    auto next_index = [&]() -> int { return p.work_ctr ? (int)(gridDim.x >> 3) + nxt : gi + (int)(gridDim.x >> 3); };
    auto advance_slow = [&]() {
        __syncthreads();                                                     // the group's tables and histograms are done with
        if (tid == 0) *next_s = next_index();
        __syncthreads();
        gi_next = *next_s;
        __syncthreads();
    };
    for (;;) {
    // ================================================================================ the group, and the one after it
    if (!first) gi = gi_next;
    first = false;
    if (gi >= per_xcd) break;
    const int grp = (int)(blockIdx.x & 7) * per_xcd + gi;
    if (grp >= n_groups) break;
    // the NEXT group's index is asked for now and read at the end of this group: the atomic's round trip (and nothing but it) used to
    // stand between two groups, 135 times per workgroup
    if (tid == 0 && p.work_ctr) nxt = atomicAdd(&p.work_ctr[(blockIdx.x & 7) * 16], 1);
    const int list = p.grp_list[grp];
    if (list < 0) { advance_slow(); continue; }
    const int64_t lo = p.list_off[list], hi = p.list_off[list + 1];
    if (hi <= lo) {
        // an empty list: the threshold pass still owes ivfpq_tau_kernel a (zero) histogram for every (query, list) pair of the group
        if (SUMS) {
            for (int u = 0; u < QG; ++u) {
                const int64_t ob = p.grp_out[(int64_t)grp * QG + u];
                if (p.grp_q[(int64_t)grp * QG + u] < 0 || ob < 0) continue;
                for (int e = tid; e < HIST_BINS; e += NTH) p.out_hist[ob + e] = 0u;
            }
        }
        advance_slow();
        continue;
    }
    // this wave's staged KEY entries: {(row - lo) << 3 | 4 (g & 1), the four queries' bytes min(255, excess + 1) (0: no survivor)}
    uint2* wbuf = reinterpret_cast<uint2*>(smem + TAB_BYTES + SCAN_CTL) + __builtin_amdgcn_readfirstlane(wave) * WAVE_CAP;   // (a wave-uniform base: scalar)
    int* wc = reinterpret_cast<int*>(smem + TAB_BYTES) + wave * QG;          // this wave's per-slot counters / first positions (a flush in the middle of a group)
    // the group's [0..8) counters / first positions, [8..16) thresholds, [16..24) queries; two copies in turn: a wave that is done with a group
    // sets the next one up while others still write the records of this one
    par ^= 1;
    int* wgc = reinterpret_cast<int*>(smem + TAB_BYTES + 512) + 32 * par;
    const int* gq = p.grp_q + (int64_t)grp * QG;
    uint2* surv = reinterpret_cast<uint2*>(p.surv);                           // survivor records (SurvRec, ivfpq8_layout.h)
    int qs[QG];
#pragma unroll
    for (int j = 0; j < QG; ++j) qs[j] = gq[j];
    // ======================== the 8 queries' byte tables -> LDS [half][code][slot] x 8 B: a 4 x 8 byte transpose per thread and step
    {
        constexpr int FILL = QLUT_BYTES / 4 / NTH;       // dwords of each query's table per thread
        constexpr int FB = SUMS ? 1 : FILL;              // of which in flight at once (the threshold pass has no registers to spare)
#pragma unroll
        for (int i0 = 0; i0 < FILL; i0 += FB) {
            uint32_t w[FB][QG];
#pragma unroll
            for (int it = 0; it < FB; ++it)
#pragma unroll
                for (int j = 0; j < QG; ++j)
                    w[it][j] = qs[j] >= 0 ? reinterpret_cast<const uint32_t*>(p.qlut + (int64_t)qs[j] * QLUT_BYTES)[tid + (i0 + it) * NTH] : 0u;
#pragma unroll
            for (int it = 0; it < FB; ++it) {
                uint32_t o[8];
#pragma unroll
                for (int hq = 0; hq < 2; ++hq) {         // queries 4 hq .. 4 hq + 3 -> dword hq of the four entries
                    const uint32_t a = w[it][4 * hq], b = w[it][4 * hq + 1], c = w[it][4 * hq + 2], d = w[it][4 * hq + 3];
                    const uint32_t t0 = GNNLM_PERM(b, a, 0x05010400u), t1 = GNNLM_PERM(b, a, 0x07030602u);
                    const uint32_t t2 = GNNLM_PERM(d, c, 0x05010400u), t3 = GNNLM_PERM(d, c, 0x07030602u);
                    o[0 + hq] = GNNLM_PERM(t2, t0, 0x05040100u);
                    o[2 + hq] = GNNLM_PERM(t2, t0, 0x07060302u);
                    o[4 + hq] = GNNLM_PERM(t3, t1, 0x05040100u);
                    o[6 + hq] = GNNLM_PERM(t3, t1, 0x07060302u);
                }
                uint4* dst = reinterpret_cast<uint4*>(smem) + 2 * (tid + (i0 + it) * NTH);
                dst[0] = uint4{o[0], o[1], o[2], o[3]};
                dst[1] = uint4{o[4], o[5], o[6], o[7]};
            }
        }
    }
    // ================================================================================ thresholds (filter) / histograms (threshold pass)
    const int j = lane & 15, g = lane >> 4;
    const int qs_lane = lane < QG ? gq[lane] : -1;                           // lanes 0..7: the query of slot `lane` (flush of the survivors)
    uint32_t* hist = reinterpret_cast<uint32_t*>(smem + TAB_BYTES);          // SUMS: [8 queries][HIST_BINS] counters
    if (SUMS) for (int e = tid; e < QG * HIST_BINS; e += NTH) hist[e] = 0u;
    // ---- the D layout of the sparse instruction: D[query 4 g + r][key j] in register r of lane (g, j) -- lanes 0..31 hold the 8 queries
    // of the group for the 16 keys of a tile, lanes 32..63 the unused rows 8..15 of the selector.  Integer thresholds per register
    // (clamped to +-16384: a sum lies in [-8192, 8128], so the test is the same and sum - T cannot overflow)
    constexpr int T_NEVER = 16384;
    int T4[4] = {T_NEVER, T_NEVER, T_NEVER, T_NEVER};
    // SUMS: lane (g, j) counts two queries of key j: g < 2 its own registers 0, 1 (queries 4 g, 4 g + 1), g >= 2 the registers 2, 3 of
    // lane (g - 2, j), which arrive by v_permlane32_swap (queries 4 (g - 2) + 2, + 3): two atomics per lane on all 64 lanes
    // (odd keys count their two queries in the other order: every atomic instruction then spreads over all 8 histograms, 8 lanes each --
    // counters of one address serialise)
    uint32_t *hist_a = nullptr, *hist_b = nullptr;
    if (SUMS) {
        const int q0 = 4 * (g & 1) + (g >= 2 ? 2 : 0) + (j & 1), q1 = q0 ^ 1;
        if (gq[q0] >= 0 && p.grp_out[(int64_t)grp * QG + q0] >= 0) hist_a = hist + q0 * HIST_BINS;
        if (gq[q1] >= 0 && p.grp_out[(int64_t)grp * QG + q1] >= 0) hist_b = hist + q1 * HIST_BINS;
    } else if (g < 2) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qr = gq[4 * g + r];
            if (qr >= 0) T4[r] = max(-T_NEVER, min(T_NEVER, filter_threshold(p.qmeta, qr, p.coarse[(int64_t)qr * p.ld_coarse + list], p.tau[qr])));
        }
    }
    if (!SUMS && wave == 0) {
        int Tl = 0;                                                          // lane s < 8: the threshold of slot s
#pragma unroll
        for (int sl = 0; sl < QG; ++sl) {
            const int t = __builtin_amdgcn_readlane(T4[sl & 3], 16 * (sl >> 2));
            if (lane == sl) Tl = t;
        }
        if (lane < QG) { wgc[lane] = 0; wgc[8 + lane] = Tl; wgc[16 + lane] = qs_lane; }
    }
    // the accumulators start at 1 - T: register r then holds the key's EXCESS over query 4 g + r's threshold PLUS ONE, a survivor is a
    // positive one -- and v_sat_pk_u8_i16 turns the four registers into the entry's four bytes (0: not a survivor)
    const v4i negT = SUMS ? v4i{0, 0, 0, 0} : v4i{1 - T4[0], 1 - T4[1], 1 - T4[2], 1 - T4[3]};
    __syncthreads();                                                       // the tables are in place
    // ======================== the lane's constants of the tile loop: slot byte offsets of look-ups 2 s / 2 s + 1 and the table half in byte 2
    uint32_t tc[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const uint32_t s0 = (uint32_t)(16 * (g & 1) + ((j + 2 * s) & 15)) << 3, s1 = (uint32_t)(16 * (g & 1) + ((j + 2 * s + 1) & 15)) << 3;
        tc[s] = s0 | s1 << 8 | (uint32_t)(g >> 1) << 16;
    }
    // The selector S[query m][(look-up, query')] = [query' == m] as the SPARSE operand of v_smfmac_i32_16x16x128_i8 (2 kept values out of every
    // 4 along k; layout measured with tools/probes/smfmac_layout.hip): lane (kb, m) holds 16 kept bytes -- bytes 8 h .. 8 h + 7 meet a 16-byte
    // stretch of the dense operand (two look-ups of 8 query bytes), kept byte s its group of four bytes 4 (s / 2) .. + 3 at the position the
    // index register names (2 bits per kept byte).  Row m < 8 keeps a 1 at query byte m of both look-ups of each stretch, rows 8 .. 15 nothing.
    uint32_t sel[4] = {0u, 0u, 0u, 0u}, sidx = 0xccccccccu;                  // pairs default to positions (0, 3)
    if (j < QG) {
        const int pos = j & 3;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int lk = 0; lk < 2; ++lk) {
                const int s0 = 8 * h + 2 * (2 * lk + (j >> 2));               // the kept pair of the group that holds byte m of look-up lk
                const int sb = pos < 3 ? s0 : s0 + 1;                        // (position 3 goes to the pair's second byte, whose index is 3 already)
                sel[sb >> 2] |= 1u << (8 * (sb & 3));
                if (pos < 3) sidx = (sidx & ~(3u << (2 * s0))) | (uint32_t)pos << (2 * s0);
            }
    }
    const v4i Asel = {(int)sel[0], (int)sel[1], (int)sel[2], (int)sel[3]};

    // ---- the list's tiles: wave w takes tiles w, w + 16, ... two per step.  Everything that steers the loop is scalar (the wave
    // index through readfirstlane), the code bytes come by buffer loads off one resource over the list's tile range (lane
    // offset in a VGPR, tile offset in an SGPR, out-of-range tiles read as zeros): no vector instruction is spent on addresses
    const int64_t t_lo = lo >> 4;
    const int nt = (int)(((hi - 1) >> 4) - t_lo) + 1;                        // tiles that hold rows of the list
    const int len = (int)(hi - lo), row_shift = (int)(lo & 15);               // local row of (tile u, key i) = 16 u + i - row_shift
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p.tiles) + t_lo * 1024, 0, nt * 1024, 0x00020000);
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int voff = lane * 16;
    const uint32_t rs_lane = (uint32_t)((j - row_shift) * 8) + (uint32_t)(4 * (g & 1));   // the lane's part of an entry's row word: (row << 3 | slot base) - 128 u
    auto load_tile = [&](int u) -> v4u {
        return __builtin_amdgcn_raw_buffer_load_b128(rs, voff, __builtin_amdgcn_readfirstlane(u * 1024), 0);   // (u is wave-uniform: tell the compiler)
    };
    // look-ups 4 q .. 4 q + 3 of one tile (= the 32-byte dense operand of one matrix instruction): address = {0, half, code byte, slot
    // offset} by one v_perm_b32 each
    auto lookups4 = [&](const v4u& cw, int q, v8i& X) __attribute__((always_inline)) {
        const uint32_t w[4] = {cw.x, cw.y, cw.z, cw.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int pp = 4 * q + e;                                        // look-up pp: byte pp of the lane's 16 code bytes
            const uint32_t ad = GNNLM_PERM(w[pp >> 2], tc[pp >> 1], 0x0c020000u | (uint32_t)(4 + (pp & 3)) << 8 | (uint32_t)(pp & 1));
            const u32x2 x = *reinterpret_cast<const __attribute__((address_space(3))) u32x2*>(ad);
            X[2 * e] = (int)x.x;
            X[2 * e + 1] = (int)x.y;
        }
    };
    // ================================================================================ survivors: staging and flushes (filter)
    // Survivors of one tile.  A wave stages KEY entries in its OWN LDS region: a lane whose key survives for at least one of its
    // four queries writes {local row, slot base; one byte per query: min(255, excess + 1), 0 = no survivor} at a position the wave
    // computes itself: a scalar count of what it has staged so far + the lane's rank inside the tile's ONE compare mask (v_mbcnt).
    // Straight-line code for every tile (round 5 appended per query register, each behind its own scalar test and branch: the
    // compare / append phase of a tile took as long as its look-ups, by the phase clocks of HISTORY.md); no LDS atomic, nothing to
    // wait for.  A full region is flushed by the wave alone, the regions left at the end of the group by the workgroup together: one
    // global atomic per query slot for the first positions (below).
    int wcnt = 0;                                                            // (scalar) entries staged by this wave
    // A staged region -> the queries' lists, in two passes over the region (it stays in LDS; nothing is carried in registers between
    // them -- round 5 kept every entry and its rank in registers across the end-of-group barriers, 10 of the kernel's 128):
    // (1) every (entry, query) survivor adds one to its query slot's counter, an LDS atomic WITHOUT return on one of 8 counters (the
    // wave's own for a flush in the middle of a group, the workgroup's at its end); lanes 0..7 turn the totals into first positions
    // with ONE global atomic per slot and leave them in the counters; (2) every survivor takes its position from its slot's counter
    // (LDS atomic with return) and goes there.
    auto count_entries = [&](int* ctr) __attribute__((always_inline)) {
        for (int c = lane; c < wcnt; c += 64) {
            const uint2 e = wbuf[c];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (e.y >> (8 * r) & 255u) atomicAdd(&ctr[(e.x & 4u) + r], 1);
        }
    };
    auto write_entries = [&](int* pos) __attribute__((always_inline)) {
        for (int c = lane; c < wcnt; c += 64) {
            const uint2 e = wbuf[c];
            const uint32_t row = (uint32_t)(lo + ((e.x >> 3) & ((1u << SURV_ROW_BITS) - 1u)));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b8 = (int)(e.y >> (8 * r) & 255u);
                if (b8 == 0) continue;
                const int sl = (int)(e.x & 4u) + r;
                const int64_t at = atomicAdd(&pos[sl], 1);
                const int Tsl = wgc[8 + sl], qsl = wgc[16 + sl];
                if (at < p.cap && qsl >= 0) {
                    // the key's integer sum sum_u = excess + T + 128 * 64 (0 .. 16320); SURV_SUM_BIG: more than the entry's byte could hold
                    const int ex = b8 - 1;
                    const int su = ex >= SURV_EXCESS_MAX ? SURV_SUM_BIG : min(SURV_SUM_BIG - 1, max(0, ex + Tsl + 128 * 64));
                    const SurvRec rec = surv_pack(row, (uint32_t)list, (uint32_t)su);
                    surv[(int64_t)qsl * p.cap + at] = uint2{rec.row, rec.word};
                }
            }
        }
        wcnt = 0;
    };
    // a full region in the middle of a group (the best lists of a query hold thousands of its survivors): the wave flushes alone
    auto flush_wave = [&]() __attribute__((always_inline)) {
        if (wcnt == 0) return;
        if (lane < QG) wc[lane] = 0;
        count_entries(wc);
        if (lane < QG) {
            const int tot = wc[lane];
            wc[lane] = (tot > 0 && qs_lane >= 0) ? atomicAdd(&p.surv_cnt[(int64_t)qs_lane * SURV_CNT_STRIDE], tot) : 0;
        }
        write_entries(wc);
    };
    // ================================================================================ one tile
    // Software pipeline at the grain of ONE matrix instruction: the four look-ups behind instruction q of tile i + 1 are issued right after
    // instruction q of tile i has read the same registers (one set of 32 look-up registers per lane; a second set, the next tile's look-ups
    // all issued ahead of this tile's instructions, measured the same: 8.35 against 8.17 ms).  The code bytes of tile i + PF are requested at
    // the top of step i into the registers tile i's bytes leave; the loop is unrolled PF times so that every name is static.
    constexpr int PF = SUMS ? GNNLM_IVF8_PF_SUMS : GNNLM_IVF8_PF;
    v8i X[4];
    // (the threshold pass may histogram a SAMPLE of the list: every TS-th tile, starting at a tile that differs from list to list)
    const int TS = SUMS ? max(1, p.sums_stride) : 1;
    auto step = [&](const v4u& cn, v4u& cl, int u) __attribute__((always_inline)) {
        cl = load_tile(u + PF * NW * TS);
        v4i acc = negT;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = __builtin_amdgcn_smfmac_i32_16x16x128_i8(Asel, X[q], acc, (int)sidx, 0, 0);
            lookups4(cn, q, X[q]);
            // nothing crosses: left alone, the scheduler deals the 16 reads out look-up-major (by address register), every quarter is then
            // complete only when nearly all 16 reads are, and the first matrix instruction of the next step waits for a drained queue
            __builtin_amdgcn_sched_barrier(0);
        }
        const int row = 16 * u + j - row_shift;                              // the lane's key (local row of the list)
        const bool edge = u == 0 || u >= nt - 1;                             // the two edge tiles share rows with the neighbouring lists (and beyond: nothing)
        if (SUMS) {
            // (LDS atomics without return: nothing waits for them)
            const gnnlm_u32x2 w2 = __builtin_amdgcn_permlane32_swap((uint32_t)acc[2], (uint32_t)acc[2], false, false);
            const gnnlm_u32x2 w3 = __builtin_amdgcn_permlane32_swap((uint32_t)acc[3], (uint32_t)acc[3], false, false);
            const int e0 = g >= 2 ? (int)w2.x : acc[0], e1 = g >= 2 ? (int)w3.x : acc[1];
            const int s0 = (j & 1) ? e1 : e0, s1 = (j & 1) ? e0 : e1;
            if (!edge || (unsigned)row < (unsigned)len) {
                if (hist_a) atomicAdd(&hist_a[(s0 + 128 * 64) >> HIST_SHIFT], 1u);
                if (hist_b) atomicAdd(&hist_b[(s1 + 128 * 64) >> HIST_SHIFT], 1u);
            }
        } else {
            // the entry's four bytes: registers 0, 1 and 2, 3 packed as int16 pairs (one v_perm_b32 each; |value| < 2^15), saturated to
            // unsigned bytes (v_sat_pk_u8_i16: <= 0 -> 0, > 255 -> 255), one compare for the whole lane, one LDS write
            if (wcnt + 32 > WAVE_CAP) flush_wave();                          // a tile adds at most 32 entries (lanes 0 .. 31: 2 x 16 keys' query halves)
            uint32_t lo8, hi8;
            const uint32_t p01 = GNNLM_PERM((uint32_t)acc[1], (uint32_t)acc[0], 0x05040100u), p23 = GNNLM_PERM((uint32_t)acc[3], (uint32_t)acc[2], 0x05040100u);
            asm("v_sat_pk_u8_i16 %0, %1" : "=v"(lo8) : "v"(p01));
            asm("v_sat_pk_u8_i16 %0, %1" : "=v"(hi8) : "v"(p23));
            const uint32_t ex4 = GNNLM_PERM(hi8, lo8, 0x05040100u);             // (the low halves of both: whatever the instruction leaves in the upper ones)
            // rows outside the list (the edge tiles, steps past the list's end) fail ONE unsigned compare of the entry's row word against a
            // scalar limit: (row << 3 | slot) < lim, lim = len << 3 on an edge tile, everything elsewhere (a negative row is a huge word)
            const uint32_t rowslot = ((uint32_t)(16 * u) << 3) + rs_lane;
            const uint32_t lim = edge ? (uint32_t)len << 3 : 0xffffffffu;
            uint32_t ex4r = rowslot < lim ? ex4 : 0u;
            asm("" : "+v"(ex4r));                                            // (opaque: left alone, the compiler turns the select back into an AND of two compares and
            const bool keep = ex4r != 0u;                                    //  re-materialises the mask through a VGPR for the ballot)
            const uint64_t m = __builtin_amdgcn_ballot_w64(keep);
            const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if (keep) wbuf[wcnt + rank] = uint2{rowslot, ex4r};
            wcnt = __builtin_amdgcn_readfirstlane(wcnt + __builtin_popcountll(m));   // (scalar: the compiler's divergence analysis gives up on it)
        }
    };
    // ================================================================================ the list's tiles
    {
        int u = SUMS ? wv * TS + list % TS : wv;                                  // (by list, not by group: which queries share a group is not specified)
        v4u C[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) C[i] = load_tile(u + i * NW * TS);        // (loads beyond the list's tiles return zeros)
#pragma unroll
        for (int q = 0; q < 4; ++q) lookups4(C[0], q, X[q]);
        // The loop is left only between two blocks of PF steps and every step of a block RUNS -- a step beyond the list's tiles reads zeros (the
        // buffer's range check) and takes the edge tiles' path, where its rows fail the range test.  With an exit or a skipped step inside the
        // block the compiler's s_waitcnt insertion merges paths with different loads in flight and falls back to waiting for (nearly) all of
        // them: `vmcnt(1)` with seven tiles in flight, once per block -- the waves stood at the code loads 17 % of their time (PMC).
#define GNNLM_IVF8_STEP(t) if constexpr (PF > (t)) { step(C[((t) + 1) % PF], C[(t)], u); u += NW * TS; }
        while (u < nt) {
            GNNLM_IVF8_STEP(0) GNNLM_IVF8_STEP(1) GNNLM_IVF8_STEP(2) GNNLM_IVF8_STEP(3)
            GNNLM_IVF8_STEP(4) GNNLM_IVF8_STEP(5) GNNLM_IVF8_STEP(6) GNNLM_IVF8_STEP(7)
        }
#undef GNNLM_IVF8_STEP
        static_assert(PF >= 3 && PF <= 8, "GNNLM_IVF8_PF");
    }
    // ================================================================================ end of the group
    if (SUMS) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < QG; ++u) {
            const int64_t ob = p.grp_out[(int64_t)grp * QG + u];
            if (qs[u] < 0 || ob < 0) continue;
            for (int e = tid; e < HIST_BINS; e += NTH) p.out_hist[ob + e] = hist[u * HIST_BINS + e];
        }
        advance_slow();
        continue;
    }
    // the 16 waves' regions -> the queries' lists with ONE global atomic per query slot for the whole
    // workgroup (the counters are contended: 30 lists x their groups add to every query's): the entries take their ranks on the
    // workgroup's 8 LDS counters (zeroed when the group was set up)
    count_entries(wgc);
    if (tid == 0) *next_s = next_index();                                    // (the next group's index rides on the same two barriers)
    __syncthreads();
    if (tid < QG) {
        const int tot = wgc[tid];
        wgc[tid] = (tot > 0 && qs_lane >= 0) ? atomicAdd(&p.surv_cnt[(int64_t)qs_lane * SURV_CNT_STRIDE], tot) : 0;
    }
    __syncthreads();
    gi_next = *next_s;
    write_entries(wgc);
    // no barrier here: the tables are free (every wave has left its tile loop), the staging regions are the waves' own, the next group's
    // counters are the other copy, and nobody flushes (the wave-0 counters hold *next_s) before the next "tables in place" barrier
    }
}

// Threshold from the histograms of a query's D dense lists (written by the SUMS pass): a LOWER bound of its k-th best exact
// score.  score(x) >= bias_l + sum_lo + sum_u(x) delta' (delta' a hair below delta), so with v(x) = sum_u(x) + off_l,
// off_l <= (bias_l - bias_min) / delta, the k-th largest v gives tau = bias_min + sum_lo + v_k delta' - eps: at least k keys score
// >= tau.  Bins of 16: a key of bin b of list l counts in the combined bin b + (off_l >> 4) -- its lower edge bounds v from below.
__global__ __launch_bounds__(1024) void ivfpq_tau_kernel(gnnlm_ivfpq_tau_t p) {
    constexpr int CB = 2 * HIST_BINS;                                        // combined bins (list offsets up to HIST_BINS bins)
    __shared__ int comb[CB];
    __shared__ int part[1024];
    __shared__ int bstar_s;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const float delta = p.qmeta[q * 4], sum_lo = p.qmeta[q * 4 + 1], amax = p.qmeta[q * 4 + 2];
    float bmin = INFINITY, bmax = -INFINITY;
    for (int d = 0; d < p.D; ++d) {
        if (p.probe_list[q * p.ld_probe + d] < 0) continue;
        const float b = p.probe_bias[q * p.ld_probe + d];
        bmin = fminf(bmin, b);
        bmax = fmaxf(bmax, b);
    }
    int c0 = 0, c1 = 0;                                                      // combined bins tid and tid + 1024
    for (int d = 0; d < p.D; ++d) {
        if (p.probe_list[q * p.ld_probe + d] < 0) continue;
        // floor of the bias difference in units of delta, a little low on purpose (a smaller offset only lowers the bound)
        const float offf = (p.probe_bias[q * p.ld_probe + d] - bmin) / delta * 0.9999f - 1.f;
        const int sh = (int)fminf(fmaxf(offf, 0.f), (float)(HIST_BINS << HIST_SHIFT)) >> HIST_SHIFT;
        const uint32_t* h = p.hist + (q * p.D + d) * HIST_BINS;
        const int b0 = tid - sh, b1 = tid + 1024 - sh;
        if (b0 >= 0 && b0 < HIST_BINS) c0 += (int)h[b0];
        if (b1 >= 0 && b1 < HIST_BINS) c1 += (int)h[b1];
    }
    comb[tid] = c0;
    comb[tid + 1024] = c1;
    if (tid == 0) bstar_s = -1;
    __syncthreads();
    // b*: the highest combined bin whose suffix count reaches k.  Thread t owns bins [2 t, 2 t + 2); suffix sums over the threads
    // by a doubling scan in LDS, then the one thread whose pair holds the crossing picks the bin
    const int h0 = comb[2 * tid], h1 = comb[2 * tid + 1], mine = h0 + h1;
    part[tid] = mine;
    __syncthreads();
    int suf = mine;                                                          // sum of part[t .. 1023]
    for (int step = 1; step < 1024; step <<= 1) {
        const int other = tid + step < 1024 ? part[tid + step] : 0;
        __syncthreads();
        suf += other;
        part[tid] = suf;
        __syncthreads();
    }
    if (suf >= p.k && suf - mine < p.k) bstar_s = (suf - mine + h1 >= p.k) ? 2 * tid + 1 : 2 * tid;   // exactly one thread
    __syncthreads();
    if (tid == 0) {
        float tau = -INFINITY;
        if (bstar_s >= 0) {
            const float eps = 66.f * 2.3841858e-7f * (64.f * amax + fmaxf(fabsf(bmin), fabsf(bmax)));
            tau = (bmin + sum_lo) + (float)(bstar_s << HIST_SHIFT) * delta * (1.f - 6.1035156e-5f) - eps;   // delta (1 - 2^-14) < 1 / inv
            tau -= fabsf(tau) * 2.3841858e-7f + 1e-30f;                       // strictly below the k keys' scores: candidates are score > tau
        }
        p.tau[q] = tau;
    }
}

}  // namespace

int ivfpq_scan8(const gnnlm_ivfpq_scan8_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.max_groups >= 0, "ivfpq_scan8: bad group count");
    if (d.max_groups == 0) return OK;
    GNNLM_REQUIRE(d.tiles && d.list_off && d.qlut && d.qmeta && d.coarse && d.grp_list && d.grp_q && d.n_groups &&
                      (d.out_hist || (d.tau && d.surv && d.surv_cnt && d.cap > 0)),
                  "ivfpq_scan8: null operand");
    GNNLM_REQUIRE(d.M == 64 && (uintptr_t)d.tiles % 16 == 0 && (uintptr_t)d.qlut % 4 == 0, "ivfpq_scan8: need M = 64, aligned images");
    GNNLM_REQUIRE(!d.out_hist || d.grp_out, "ivfpq_scan8: out_hist needs grp_out");
    GNNLM_REQUIRE(d.nlist > 0 && d.nlist <= (1 << SURV_LIST_BITS) && d.max_list >= 0 && d.max_list < (1ll << SURV_ROW_BITS),
                  "ivfpq_scan8: the survivor records hold 18 bits of list and 19 bits of row: need 0 < nlist <= 2^18 and max_list < 2^19");
    GNNLM_LDS_OPT_IN(&ivfpq_scan8_kernel<false>, scan8_lds(false));
    GNNLM_LDS_OPT_IN(&ivfpq_scan8_kernel<true>, scan8_lds(true));
    ProfScope prof(d.out_hist ? K_IVF8S : K_IVF8, stream, 0.0, 0.0);   // work figures are device-side (list lengths): bench.py computes them
    int dev = 0, cus = 0;
    GNNLM_HIP(hipGetDevice(&dev));
    GNNLM_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const dim3 grid((unsigned)scan8_grid(d.max_groups, cus));           // persistent: one per CU
    if (d.out_hist) hipLaunchKernelGGL(ivfpq_scan8_kernel<true>, grid, dim3(NTH), scan8_lds(true), stream, d);
    else hipLaunchKernelGGL(ivfpq_scan8_kernel<false>, grid, dim3(NTH), scan8_lds(false), stream, d);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int ivfpq_tau(const gnnlm_ivfpq_tau_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.n >= 0 && d.n < (1ll << 31) && d.D >= 1 && d.k > 0, "ivfpq_tau: bad shape");
    if (d.n == 0) return OK;
    GNNLM_REQUIRE(d.hist && d.probe_list && d.probe_bias && d.qmeta && d.tau && d.ld_probe >= d.D, "ivfpq_tau: null operand");
    ProfScope prof(K_TAU, stream, 0.0, 4.0 * (double)d.n * d.D * HIST_BINS);
    hipLaunchKernelGGL(ivfpq_tau_kernel, dim3((unsigned)d.n), dim3(1024), 0, stream, d);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
