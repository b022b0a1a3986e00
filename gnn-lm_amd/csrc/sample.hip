// The next token of every row from its sorted top-N (include/gnnlm.h: gnnlm_sample_topk): greedy, or top-k sampling with the
// caller's uniform numbers -- probs = lprobs.topk(k).exp_(); torch.multinomial(probs, 1) of fairseq/search.py:231-247.
//
// One wave per row.  Lane l owns the run of `per` = ceil(N / 64) consecutive columns [l * per, (l + 1) * per); the prefix sum is
// c_j = (the wave scan of the runs of the lanes below l) + (the run's columns up to j, summed in ascending order), and c_{N-1} the
// scan's last value.  Should u * c_{N-1} round up to c_{N-1} itself, the last column with mass is taken.
#include "host.h"

namespace gnnlm {
namespace {

constexpr int MAX_N = 2048, NONE = 0x7fffffff;

__device__ __forceinline__ float mass(float lp, float lp0) { return lp > -INFINITY ? expf(lp - lp0) : 0.f; }   // NaN: 0 too

__global__ __launch_bounds__(256) void sample_topk_kernel(gnnlm_sample_topk_t p) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= p.B) return;
    if (p.done && p.done[b] != 0) {
        if (lane == 0) p.next[b] = p.pad;
        return;
    }
    const float* lp = p.logp + b * p.ld_logp;
    const float lp0 = lp[0];
    if (!(fabsf(lp0) < INFINITY)) {                         // nothing to pick from (an empty top-N, or NaN)
        if (lane == 0) {
            p.next[b] = p.pad;
            if (p.done) p.done[b] = 1;
            if (p.n_bad) atomicAdd(p.n_bad, 1);
        }
        return;
    }
    int pick = 0;
    if (p.u) {
        const int per = (p.N + 63) / 64;
        const int j0 = lane * per, j1 = min(p.N, j0 + per);
        float run = 0.f;
        for (int j = j0; j < j1; ++j) run += mass(lp[j], lp0);
        float incl = run;                                   // inclusive scan over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        const float total = __shfl(incl, 63, 64);
        const float thr = p.u[b] * total;
        float before = __shfl_up(incl, 1, 64);
        if (lane == 0) before = 0.f;
        int found = NONE, last = -1;                     // the first column of this run over the threshold; its last column with mass
        float in_run = 0.f;
        for (int j = j0; j < j1; ++j) {
            const float e = mass(lp[j], lp0);
            in_run += e;
            if (e > 0.f) {
                last = j;
                if (found == NONE && before + in_run > thr) found = j;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            found = min(found, __shfl_xor(found, o, 64));
            last = max(last, __shfl_xor(last, o, 64));
        }
        pick = found != NONE ? found : last;             // (u * total rounded up to total: the last column with mass)
    }
    if (lane == 0) {
        const int64_t id = p.ids[b * p.ld_ids + pick];
        p.next[b] = id;
        if (p.next_logp) p.next_logp[b] = lp[pick];
        if (p.done && id == p.eos) p.done[b] = 1;
    }
}

}  // namespace

int sample_topk(const gnnlm_sample_topk_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.N >= 1 && d.N <= MAX_N, "sample_topk: N outside [1, 2048]");
    GNNLM_REQUIRE(d.B >= 0, "sample_topk: B < 0");
    GNNLM_REQUIRE(d.ld_logp >= d.N && d.ld_ids >= d.N, "sample_topk: ld_logp / ld_ids < N");
    if (d.B == 0) return OK;
    GNNLM_REQUIRE(d.logp && d.ids && d.next, "sample_topk: logp / ids / next missing");
    GNNLM_REQUIRE((uintptr_t)d.logp % 4 == 0 && (uintptr_t)d.u % 4 == 0 && (uintptr_t)d.ids % 8 == 0 && (uintptr_t)d.next % 8 == 0 &&
                  (uintptr_t)d.next_logp % 4 == 0 && (uintptr_t)d.done % 4 == 0 && (uintptr_t)d.n_bad % 4 == 0, "sample_topk: a misaligned pointer");
    ProfScope prof(K_MISC, stream, 2.0 * d.B * d.N, 8.0 * d.B * d.N + 24.0 * d.B);
    hipLaunchKernelGGL(sample_topk_kernel, dim3((unsigned)cdiv(d.B, 4)), dim3(256), 0, stream, d);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm

using namespace gnnlm;

extern "C" int gnnlm_sample_topk(const gnnlm_sample_topk_t* d, void* stream) {
    GNNLM_DESC(d);
    return sample_topk(*d, (hipStream_t)stream);
}
