// The int8 IVF-PQ search (scheme: ivfpq8_scan.hip; record and buffer shapes: ivfpq8_layout.h), what follows the filter: a tighter threshold
// from the survivors' own integer sums, the exact float32 scores of those that can still beat it, the split of the result's payloads.
#include "kernels.h"
#include "ivfpq8_layout.h"

namespace gnnlm {
namespace {

typedef unsigned v4u __attribute__((ext_vector_type(4)));
// A TIGHTER threshold from the survivors themselves, then the survivors that can still beat it (round 4).  The threshold pass's
// tau is a lower bound of the k-th best score from the first D lists, histogrammed in bins of 16: the filter lets ~6 x k keys
// through and ~4 x k of them score above tau.  Every survivor carries its integer sum (as the excess over its query's integer
// threshold), i.e. a lower bound LB(x) = bias_l + sum_lo + sum_u(x) delta' - eps <= score(x) over ALL probed lists, un-binned:
// the k-th largest LB is a valid and much tighter threshold tau1 (at least k keys score >= it), and only the survivors whose
// UPPER bound exceeds tau1 (the filter's own integer test, with tau1) need an exact score.  One workgroup per query:
// (1) the k-th largest LB to the resolution of a 2048-bin histogram over [tau, max LB] (one pass: a lower edge is a valid threshold too),
// (2) compaction of the records in place, count in `out_cnt` (surv_cnt keeps the filter's count: the overflow check reads it),
// tau[q] = max(tau, tau1).  The search result is unchanged: candidates stay a superset of the true k best.
#ifndef GNNLM_REFINE_NT
#define GNNLM_REFINE_NT 1024     // threads per query (A/B: 512 was slower, 0.46 against 0.40 ms)
#endif
// (a workgroup's refinement as a function: the prologue of the fused refine + re-score launch.  Of the descriptor it WRITES the
// survivor records [n, cap, 2] (compacted in place), tau [n] (raised in place) and out_cnt [n, 16] (column 0: the records left);
// `hist`: 2048 ints of LDS the caller lends.  Returns the records left and the threshold to every thread.)
template <int EPT>
__device__ __forceinline__ void refine_wg(const gnnlm_ivfpq_rescore_t& p, const int64_t q, int* hist, int& n_left, float& tau_left) {
    constexpr int NT = GNNLM_REFINE_NT, NB = 2048, NWV = NT / 64;
    __shared__ int wtot[NWV];
    __shared__ int dig_s, base_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(p.surv_cnt[q * SURV_CNT_STRIDE], p.cap);
    uint2* surv = reinterpret_cast<uint2*>(const_cast<uint32_t*>(p.surv)) + q * p.cap;
    const float tau0 = p.tau[q];
    n_left = n;
    tau_left = tau0;
    if (n < p.k || !(tau0 > -INFINITY)) {                                    // fewer survivors than k, or no threshold at all (the sums say nothing)
        if (tid == 0 && p.out_cnt) p.out_cnt[q * SURV_CNT_STRIDE] = n;
        return;
    }
    const float delta = p.qmeta[q * 4], sum_lo = p.qmeta[q * 4 + 1], amax = p.qmeta[q * 4 + 2];
    const float dlo = delta * (1.f - 6.1035156e-5f);                         // delta (1 - 2^-14) < 1 / inv (ivfpq_tau_kernel)
    const float* coarse = p.coarse + q * p.ld_coarse;
    // LB of a record: bias_l + sum_lo + sum_u delta' - eps (eps: the float32 rounding of the score chain), strictly below the score
    auto lower_bound = [&](const uint2& rec) -> float {
        const int list = (int)surv_list(rec.y);
        int su = (int)surv_sum(rec.y);
        const float bias = coarse[list];
        if (su >= SURV_SUM_BIG) su = min(16320, max(0, filter_threshold(p.qmeta, q, bias, tau0) + SURV_EXCESS_MAX + 128 * 64));   // (rare: the very best keys)
        const float eps = 66.f * 2.3841858e-7f * (64.f * amax + fabsf(bias));
        const float lb = (bias + sum_lo) + (float)su * dlo - eps;
        return lb - (fabsf(lb) * 2.3841858e-7f + 1e-30f);                    // candidates are score > tau
    };
    // the first EPT * NT records live in registers (one memory round trip); longer lists (a doubled capacity) re-read the rest
    constexpr int C0 = EPT * NT;
    uint2 rrec[EPT];
    float rlb[EPT];
#pragma unroll
    for (int e = 0; e < EPT; ++e) rrec[e] = surv[min(tid + e * NT, n - 1)];
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        rlb[e] = tid + e * NT < n ? lower_bound(rrec[e]) : -INFINITY;
        mx = fmaxf(mx, rlb[e]);
    }
    for (int c = C0 + tid; c < n; c += NT) mx = fmaxf(mx, lower_bound(surv[c]));
    // ---- (1) the k-th largest LB, to the resolution of 2048 bins over [tau0, max LB] (far finer than the 64-delta slack of the
    // bounds; a float radix select of the exact value serialises on LDS atomics: the bounds of a query share their leading bits)
    __shared__ float wmax[NWV];
    mx = wave_max(mx);
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    mx = wmax[0];
    for (int w = 1; w < NWV; ++w) mx = fmaxf(mx, wmax[w]);
    const float span = mx - tau0;
    float tau1 = tau0;
    if (span > 0.f) {                                                        // (else no bound above the old threshold: nothing to gain)
        const float inv_w = (float)NB / span * (1.f - 1e-6f);
        for (int e = tid; e < NB; e += NT) hist[e] = 0;
        __syncthreads();
        auto bin_of = [&](float lb) -> int { return lb >= tau0 ? min(NB - 1, (int)((lb - tau0) * inv_w)) : -1; };
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int bn = bin_of(rlb[e]);
            if (bn >= 0) atomicAdd(&hist[bn], 1);
        }
        for (int c = C0 + tid; c < n; c += NT) {
            const int bn = bin_of(lower_bound(surv[c]));
            if (bn >= 0) atomicAdd(&hist[bn], 1);
        }
        __syncthreads();
        // the highest bin whose suffix count reaches k (thread t owns bins 2 t, 2 t + 1; suffix sums by shuffles, then over the waves)
        constexpr int BPT = NB / NT;
        int own[BPT], mine = 0;
#pragma unroll
        for (int bb = 0; bb < BPT; ++bb) { own[bb] = hist[BPT * tid + bb]; mine += own[bb]; }
        int suf = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_down(suf, d, 64);
            if (lane + d < 64) suf += o;
        }
        if (lane == 0) wtot[wave] = suf;
        if (tid == 0) dig_s = -1;
        __syncthreads();
        for (int w = wave + 1; w < NWV; ++w) suf += wtot[w];
        if (suf >= p.k && suf - mine < p.k) {
            int acc_ = suf - mine;
#pragma unroll
            for (int bb = BPT - 1; bb >= 0; --bb) {
                if (acc_ + own[bb] >= p.k) { dig_s = BPT * tid + bb; break; }
                acc_ += own[bb];
            }
        }
        __syncthreads();
        if (dig_s > 0) {
            // every bound of bins >= dig_s is >= tau0 + dig_s / inv_w: at least k keys score above it (two roundings of slack)
            const float t = tau0 + (float)dig_s / inv_w * (1.f - 2e-6f);
            tau1 = fmaxf(tau0, t - fabsf(t) * 4.7683716e-7f);
        }
    }
    // ---- (2) keep the records whose upper bound exceeds tau1.  A record is dropped only if its UPPER bound (bias + sum_lo +
    // (sum_u + 64) delta + eps, the filter's) lies below tau1 with a margin of 0.1 % of the sum term + 2 delta for this formula's
    // own rounding: a slightly weaker test than the filter's integer one
    auto keep_rec = [&](const uint2& rec) -> bool {
        const int list = (int)surv_list(rec.y), su = (int)surv_sum(rec.y);
        if (su >= SURV_SUM_BIG) return true;
        const float bias = coarse[list];
        const float eps = 66.f * 2.3841858e-7f * (64.f * amax + fabsf(bias) + fabsf(tau1));
        const float ub = (bias + sum_lo) + (float)(su + 66) * delta * 1.001f + eps;
        return !(ub < tau1);
    };
    // the register-resident records: every thread counts what it keeps, one exclusive scan over the threads, then the writes
    // (all reads happened long ago: in place is safe)
    int kept = 0;
    uint32_t kmask = 0u;
#pragma unroll
    for (int e = 0; e < EPT; ++e)
        if (tid + e * NT < n && keep_rec(rrec[e])) { kmask |= 1u << e; ++kept; }
    int incl = kept;                                                         // inclusive prefix over the lanes of the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    __syncthreads();                                                         // (wtot is free again)
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int at = incl - kept;
    for (int w = 0; w < wave; ++w) at += wtot[w];
    int total = 0;
    for (int w = 0; w < NWV; ++w) total += wtot[w];
#pragma unroll
    for (int e = 0; e < EPT; ++e)
        if (kmask >> e & 1u) surv[at++] = rrec[e];
    // the rest of a longer list, chunk by chunk behind what has been written (write index <= read index)
    if (n > C0) {
        if (tid == 0) base_s = total;
        __syncthreads();
        for (int c0 = C0; c0 < n; c0 += NT) {
            const int c = c0 + tid;
            uint2 rec = uint2{0u, 0u};
            bool keep = false;
            if (c < n) { rec = surv[c]; keep = keep_rec(rec); }
            const uint64_t m = __builtin_amdgcn_ballot_w64(keep);
            const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            __syncthreads();
            if (lane == 0) wtot[wave] = __builtin_popcountll(m);
            __syncthreads();                                                 // (every read of the chunk is done: the writes stay behind them)
            int before = base_s;
            for (int w = 0; w < wave; ++w) before += wtot[w];
            if (keep) surv[before + rank] = rec;
            __syncthreads();
            if (tid == 0) { int tot = 0; for (int w = 0; w < NWV; ++w) tot += wtot[w]; base_s += tot; }
            __syncthreads();
        }
        total = base_s;
    }
    if (tid == 0) {
        if (p.out_cnt) p.out_cnt[q * SURV_CNT_STRIDE] = total;
        const_cast<float*>(p.tau)[q] = tau1;
    }
    n_left = total;
    tau_left = tau1;
}

// Exact float32 scores of the survivors, in the summation order of the f32 scan (ivfpq.hip scan_rot: look-up s of half h
// goes to sub-quantizer 32 h + (row + s) % 32, even look-ups into one chain, odd ones into the other, halves in order,
// score = bias + (chain0 + chain1)).  One workgroup per query, its table in LDS.
#ifndef GNNLM_RESCORE_NT
#define GNNLM_RESCORE_NT 1024   // threads per query (A/B, medians of 7: 1024: 1.14 ms, 512: 1.13, 256 with two workgroups per CU: 1.34)
#endif
// (a workgroup's re-score as a function: `n` records of query q against the threshold `tau`; TAB_READY: the query's table is already
// on its way into rtab by LDS-DMA -- the fused launch below -- and the caller has waited for it)
template <int M, bool TAB_READY>
__device__ __forceinline__ void rescore_wg(const gnnlm_ivfpq_rescore_t& p, const int64_t q, const int n, const float tau, float* rtab) {
    __shared__ int ccnt;
    constexpr int NT = GNNLM_RESCORE_NT;                                    // 16 waves: the survivors' code rows are random 64-B reads
    uint32_t* cdw = reinterpret_cast<uint32_t*>(rtab + M * 256);            // dword k of thread t at [k][t]: bank = t mod 32 for stores and byte reads alike
    const int tid = threadIdx.x;
    if (tid == 0) ccnt = 0;
    const uint2* surv = reinterpret_cast<const uint2*>(p.surv) + q * p.cap;
    // Three loads deep, in an order that never drains the queue (s_waitcnt vmcnt counts in issue order): survivor i's code row and
    // bias are consumed while row i + 1 and the RECORD {row, list} of survivor i + 2 are in flight; a step issues record i + 3 first,
    // then bias and row i + 2 (their addresses come from a record that is one step old: waiting for it leaves the younger loads in
    // flight).  Over a loop's back edge the compiler's wait insertion loses the issue order and drains the queue at the loop head
    // (vmcnt(0)); the first 16 steps (16384 survivors: every capacity the search uses by default) are therefore unrolled -- straight-
    // line code, exact waits, no copies between the register sets.  Indices beyond n are clamped (unconditional loads).
    const int last = max(n - 1, 0);
    auto record = [&](int e, uint2& rec) __attribute__((always_inline)) { rec = surv[min(e, last)]; };
    auto rowload = [&](const uint2& rec, v4u (&cr)[M / 16], float& bias) __attribute__((always_inline)) {
        bias = p.coarse[q * p.ld_coarse + surv_list(rec.y)];                // (first: the youngest loads of a step are the row's)
        const v4u* crow = reinterpret_cast<const v4u*>(p.codes + (int64_t)rec.x * M);
#pragma unroll
        for (int c16 = 0; c16 < M / 16; ++c16) cr[c16] = crow[c16];
    };
    uint2 recC = uint2{0u, 0u}, recD = recC;                                // records in flight (alternating)
    v4u cr0[M / 16], cr1[M / 16];                                           // code rows: two register sets, alternating -- no copies
    float bias0 = 0.f, bias1 = 0.f;
    uint32_t rid0 = 0u, rid1 = 0u;
    if (n > 0) {
        if (!TAB_READY) {
            const float4* src = reinterpret_cast<const float4*>(p.lut + q * p.ld_lut);
            float4* dst = reinterpret_cast<float4*>(rtab);
            for (int e = tid; e < M * 64; e += NT) dst[e] = src[e];
        }
        uint2 r0, r1;
        record(tid, r0);
        record(tid + NT, r1);
        record(tid + 2 * NT, recC);
        rowload(r0, cr0, bias0);
        rid0 = r0.x;
        rowload(r1, cr1, bias1);
        rid1 = r1.x;
    }
    __syncthreads();
    const uint8_t* cb = reinterpret_cast<const uint8_t*>(cdw + tid);        // byte m of the row: cb[(m >> 2) * 4 * NT + (m & 3)]
    // one survivor: its row (set `cr`) -> LDS, the next loads issued (record i + 3 into rec_new, then row i + 2 -- named by rec_old,
    // which arrived a step ago -- into the set just freed), then the 64 look-ups
    auto one = [&](int e, v4u (&cr)[M / 16], float& bset, uint32_t& rset, const uint2& rec_old, uint2& rec_new) __attribute__((always_inline)) {
        const int64_t row = rset;
        const float bias = bset;
#pragma unroll
        for (int c16 = 0; c16 < M / 16; ++c16) {
            cdw[(4 * c16 + 0) * NT + tid] = cr[c16].x;
            cdw[(4 * c16 + 1) * NT + tid] = cr[c16].y;
            cdw[(4 * c16 + 2) * NT + tid] = cr[c16].z;
            cdw[(4 * c16 + 3) * NT + tid] = cr[c16].w;
        }
        record(e + 3 * NT, rec_new);
        rowload(rec_old, cr, bset);
        rset = rec_old.x;
        const int rot = (int)(row & 31);
        float a0 = 0.f, a1 = 0.f;
#pragma unroll
        for (int h = 0; h < M / 32; ++h) {
#pragma unroll 8
            for (int s = 0; s < 32; s += 2) {
                const int m0 = 32 * h + ((rot + s) & 31), m1 = 32 * h + ((rot + s + 1) & 31);
                a0 = a0 + rtab[m0 * 256 + cb[(m0 >> 2) * (4 * NT) + (m0 & 3)]];
                a1 = a1 + rtab[m1 * 256 + cb[(m1 >> 2) * (4 * NT) + (m1 & 3)]];
            }
        }
        const float score = bias + (a0 + a1);
        if (score > tau) {
            const int pos = atomicAdd(&ccnt, 1);
            if (pos < p.cand_cap) {
                p.cand_val[q * p.cand_cap + pos] = score;
                p.cand_id[q * p.cand_cap + pos] = row;                       // the payload follows below: a load here would make the loop
            }                                                                // wait for it AND for the code rows requested before it
        }
    };
    int e = tid;
#pragma unroll
    for (int it = 0; it < 8; ++it) {                                         // 16 steps, straight-line
        if (e >= n) break;
        one(e, cr0, bias0, rid0, recC, recD);
        e += NT;
        if (e >= n) break;
        one(e, cr1, bias1, rid1, recD, recC);
        e += NT;
    }
    for (; e < n; e += 2 * NT) {                                             // beyond 16384 survivors (a doubled capacity): the rolled loop
        one(e, cr0, bias0, rid0, recC, recD);
        if (e + NT >= n) break;
        one(e + NT, cr1, bias1, rid1, recD, recC);
    }
    __syncthreads();
    if (tid == 0) p.cand_cnt[q] = ccnt;
    // rows -> payloads (ids, labels): every thread's loads independent of each other, nothing else in flight
    const int nc = min(ccnt, p.cand_cap);
    // (loading the payload with every row instead, and the first records without waiting for the count, moved the time into the first
    // phase and added requests: 1.22 against 1.14 ms -- the kernel runs at ~0.7 of the memory system's request rate, ~3 per record)
    for (int e = tid; e < nc; e += NT) p.cand_id[q * p.cand_cap + e] = p.payload[p.cand_id[q * p.cand_cap + e]];
}

template <int M>
__global__ __launch_bounds__(GNNLM_RESCORE_NT) void ivfpq_rescore_kernel(gnnlm_ivfpq_rescore_t p) {
    extern __shared__ __attribute__((aligned(16))) float rtab[];            // [M][256] f32, then the threads' code rows [M / 4 dwords][NT]
    const int64_t q = blockIdx.x;
    rescore_wg<M, false>(p, q, min(p.surv_cnt[q * SURV_CNT_STRIDE], p.cap), p.tau[q], rtab);
}

// Refinement + re-score of a query in ONE launch (round 6; gnnlm_ivfpq_rescore with `qmeta`).  As two kernels they were one workgroup
// per query each, both waiting on memory most of their time (the re-score 40 % of its 35 us for its 64-KiB table to arrive: copied
// through registers behind a barrier -- the phase clocks of HISTORY.md, "What FETCH_SIZE counts").  Here the table is requested FIRST,
// by LDS-DMA (no registers, nothing waits for it), the refinement runs while it arrives (its histogram in the code rows' staging area),
// and the re-score starts on the records the refinement has just compacted (in place, in the query's survivor list: this workgroup's
// own writes, ordered by the barrier).  Same arithmetic, same order: the candidates are those the two launches gave.
static_assert(GNNLM_REFINE_NT == GNNLM_RESCORE_NT, "the fused refine + re-score launch runs both on one workgroup shape");
template <int EPT>
__global__ __launch_bounds__(GNNLM_RESCORE_NT) void ivfpq_refine_rescore_kernel(gnnlm_ivfpq_rescore_t p) {
    constexpr int M = 64;
    extern __shared__ __attribute__((aligned(16))) float rtab[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int n0 = min(p.surv_cnt[q * SURV_CNT_STRIDE], p.cap);
    if (n0 > 0) {
        // [64][256] f32 = 64 pieces of 1 KiB: wave w brings pieces 4 w .. 4 w + 3 (global_load_lds_dwordx4: 16 B per lane, lane order;
        // M0 = the piece's LDS byte address).  From inline asm: the compiler's counters do not see them -- its own waits only ever
        // get more conservative by that -- and would otherwise guard every LDS read of the refinement with vmcnt(0)
        const float* src = p.lut + q * p.ld_lut + (4 * wave) * 256 + 4 * lane;
        const unsigned dst = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)rtab + (unsigned)(4 * __builtin_amdgcn_readfirstlane(wave)) * 1024u;
        unsigned keep_;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %1, off\n\tglobal_load_lds_dwordx4 %1, off offset:1024\n\t"
                     "global_load_lds_dwordx4 %1, off offset:2048\n\tglobal_load_lds_dwordx4 %1, off offset:3072\n\t"
                     "s_mov_b32 m0, %0"
                     : "=&s"(keep_) : "v"(src), "s"(dst) : "memory");
    }
    int n_left;
    float tau_left;
    refine_wg<EPT>(p, q, reinterpret_cast<int*>(rtab + M * 256), n_left, tau_left);   // (histogram: where the code rows are staged afterwards)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                         // this wave's table pieces have landed (and its compacted records have left)
    __syncthreads();                                                         // ... everybody's
    rescore_wg<M, true>(p, q, n_left, tau_left, rtab);
}

// the search's results: payload (id << label_bits | label, -1 = none) -> id in place, label to out_vals (none: `val_last`, what
// numpy's vals[-1] reads for the reference, knn/knn_model.py:198)
__global__ __launch_bounds__(256) void split_payload_kernel(int64_t* __restrict__ idx, int64_t n, int label_bits, int32_t val_last, int32_t* __restrict__ out_vals) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int64_t v = idx[e];
    idx[e] = v < 0 ? v : v >> label_bits;
    if (out_vals) out_vals[e] = v < 0 ? val_last : (int32_t)(v & ((1ll << label_bits) - 1));
}

}  // namespace

int ivfpq_rescore(const gnnlm_ivfpq_rescore_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.n >= 0 && d.n < (1ll << 31), "ivfpq_rescore: bad query count");
    if (d.n == 0) return OK;
    GNNLM_REQUIRE(d.codes && d.payload && d.lut && d.coarse && d.tau && d.surv && d.surv_cnt && d.cand_val && d.cand_id && d.cand_cnt &&
                      d.cap > 0 && d.cand_cap > 0,
                  "ivfpq_rescore: null operand");
    GNNLM_REQUIRE(d.M == 64 && d.ld_lut >= (int64_t)d.M * 256 && d.ld_lut % 4 == 0 && (uintptr_t)d.lut % 16 == 0 &&
                      (uintptr_t)d.codes % 16 == 0,
                  "ivfpq_rescore: need M = 64, 16-byte aligned tables");
    ProfScope prof(K_RESCORE, stream, 0.0, 0.0);
    const size_t lds = rescore_lds(d.M, GNNLM_RESCORE_NT);
    if (d.qmeta) {                                                          // refinement + re-score in one launch (ABI 10)
        GNNLM_REQUIRE(d.k > 0, "ivfpq_rescore: the refinement needs k > 0");
        GNNLM_LDS_OPT_IN(&ivfpq_refine_rescore_kernel<8>, lds);
        hipLaunchKernelGGL(ivfpq_refine_rescore_kernel<8>, dim3((unsigned)d.n), dim3(GNNLM_RESCORE_NT), lds, stream, d);
    } else {
        GNNLM_LDS_OPT_IN(&ivfpq_rescore_kernel<64>, lds);
        hipLaunchKernelGGL(ivfpq_rescore_kernel<64>, dim3((unsigned)d.n), dim3(GNNLM_RESCORE_NT), lds, stream, d);
    }
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int ivfpq_split_payload(int64_t* idx, int64_t n, int label_bits, int32_t val_last, int32_t* out_vals, hipStream_t stream) {
    GNNLM_REQUIRE(idx && n >= 0 && label_bits > 0 && label_bits < 32, "ivfpq_split_payload: bad arguments");
    if (n == 0) return OK;
    hipLaunchKernelGGL(split_payload_kernel, dim3((unsigned)cdiv(n, (int64_t)256)), dim3(256), 0, stream, idx, n, label_bits, val_last, out_vals);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
