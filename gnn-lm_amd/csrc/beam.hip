// One beam-search step of every sentence (include/gnnlm.h: gnnlm_beam_select): search.BeamSearch.step (fairseq/search.py:49-85)
// and the selection half of SequenceGenerator._generate (fairseq/sequence_generator.py:359-497) in one launch.
//
// One workgroup per sentence.  The beam_in * N candidate values fl32(score + lprob) are staged in LDS; the step's up to 2 * beam
// candidates are then drawn one per round, each round an arg-max under the total order (value descending, hypothesis ascending,
// token ascending) -- a lane's own candidates, a butterfly over the wave, the four waves through LDS.  Every candidate takes part,
// not only a row's first 2 * beam columns: the float32 add can round two columns of a row to one value, and the tie then goes to
// the smaller token wherever it stood.  Lane 0 scans the drawn list (at most 64 entries) for the finalized and the surviving
// hypotheses; the histories are backpointers, walked only when a hypothesis is finalized; the table of cache slots is permuted
// column by column, a column read whole (LDS, the staging area again) before it is written, so it may be updated in place.
#include "host.h"

namespace gnnlm {
namespace {

constexpr int MAX_BEAM = 32, MAX_CAND = 8192, NT = 256;

// does candidate (va, ia) come before (vb, ib)?  i = j * N + column; i < 0 is "none" and carries -inf, which no real candidate has
__device__ __forceinline__ bool before(float va, int ia, float vb, int ib, int N, const int64_t* ids, int64_t ld_id) {
    if (va != vb) return va > vb;
    if (ia < 0 || ib < 0 || ia == ib) return false;
    const int ja = ia / N, jb = ib / N;
    if (ja != jb) return ja < jb;
    const int64_t ta = ids[ja * ld_id + (ia - ja * N)], tb = ids[jb * ld_id + (ib - jb * N)];
    if (ta != tb) return ta < tb;
    return ia < ib;
}

__global__ __launch_bounds__(NT) void beam_select_kernel(gnnlm_beam_select_t p) {
    __shared__ float val[MAX_CAND];                          // the candidates' values; later the table's columns [beam][NT]
    __shared__ float w_v[NT / 64];
    __shared__ int w_i[NT / 64];
    __shared__ float sel_v[2 * MAX_BEAM];
    __shared__ int sel_j[2 * MAX_BEAM];
    __shared__ long long sel_t[2 * MAX_BEAM];
    __shared__ int act[MAX_BEAM], fin[MAX_BEAM], par[MAX_BEAM];
    __shared__ int n_act, n_new, fin0;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (p.finished[b] != 0) return;
    const int t = p.t[b];
    if (t < 0 || t > p.max_new) return;
    const int beam = p.beam, bin = p.beam_in, N = p.N, n = bin * N;
    const int64_t s0 = (int64_t)b * beam;
    const float* cv = p.cand_val + (int64_t)b * bin * p.ld_val;
    const int64_t* ci = p.cand_id + (int64_t)b * bin * p.ld_id;
    for (int i = tid; i < n; i += NT) {
        const int j = i / N, c = i - j * N;
        const float v = cv[j * p.ld_val + c];
        const float s = p.score_in[s0 + j] + v;
        val[i] = fabsf(v) < INFINITY && fabsf(s) < INFINITY ? s : -INFINITY;
    }
    __syncthreads();
    int C = 0;
    for (int r = 0; r < 2 * beam; ++r) {
        float bv = -INFINITY;
        int bi = -1;
        for (int i = tid; i < n; i += NT) {
            const float v = val[i];
            if (v > -INFINITY && before(v, i, bv, bi, N, ci, p.ld_id)) {
                bv = v;
                bi = i;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (before(ov, oi, bv, bi, N, ci, p.ld_id)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            w_v[wave] = bv;
            w_i[wave] = bi;
        }
        __syncthreads();
        bv = w_v[0];
        bi = w_i[0];
        for (int w = 1; w < NT / 64; ++w)
            if (before(w_v[w], w_i[w], bv, bi, N, ci, p.ld_id)) {
                bv = w_v[w];
                bi = w_i[w];
            }
        if (bi < 0) break;                                   // (the same for every thread) nothing present is left
        if (tid == 0) {
            const int j = bi / N;
            sel_v[r] = bv;
            sel_j[r] = j;
            sel_t[r] = ci[j * p.ld_id + (bi - j * N)];
            val[bi] = -INFINITY;
        }
        C = r + 1;
        __syncthreads();
    }
    if (tid == 0) {
        int nf = min(max(p.fin_n[b], 0), beam), k = 0, na = 0;
        fin0 = nf;
        for (int r = 0; r < min(beam, C); ++r)
            if (sel_t[r] == p.eos && nf < beam) {
                fin[k++] = r;
                ++nf;
            }
        for (int r = 0; r < C && na < beam; ++r)
            if (sel_t[r] != p.eos) act[na++] = r;
        n_act = na;
        n_new = k;
        p.fin_n[b] = nf;
    }
    __syncthreads();
    const int T1 = p.max_new + 1;
    if (tid < beam) {                                        // hypothesis tid of the next step
        const int j = tid;
        const bool live = j < n_act;
        const int r = live ? act[j] : 0;
        const int jp = live ? sel_j[r] : j;
        const float sc = live ? sel_v[r] : -INFINITY;
        const int64_t tok = live ? (int64_t)sel_t[r] : p.pad;
        par[j] = jp;
        p.next[s0 + j] = tok;
        p.parent[s0 + j] = (int32_t)(s0 + jp);
        p.score_out[s0 + j] = sc;
        const int64_t h = ((int64_t)b * T1 + t) * beam + j;
        p.hist_tok[h] = tok;
        p.hist_par[h] = jp;
        p.hist_score[h] = sc;
    }
    if (tid < n_new) {                                       // a finalized hypothesis: its parent's history along the backpointers
        const int r = fin[tid], slot = fin0 + tid;
        int64_t* ft = p.fin_tok + (s0 + slot) * T1;
        float* fc = p.fin_cum + (s0 + slot) * T1;
        int cur = sel_j[r];
        for (int s = t - 1; s >= 0; --s) {                   // (steps below t: written by earlier launches)
            const int64_t h = ((int64_t)b * T1 + s) * beam + cur;
            ft[s] = p.hist_tok[h];
            fc[s] = p.hist_score[h];
            cur = min(max(p.hist_par[h], 0), beam - 1);
        }
        ft[t] = p.eos;
        fc[t] = sel_v[r];
        p.fin_len[s0 + slot] = t + 1;
        p.fin_score[s0 + slot] = sel_v[r];
    }
    if (fin0 + n_new >= beam || t == p.max_new) {
        if (tid < beam) p.done[s0 + tid] = 1;
        if (tid == 0) p.finished[b] = 1;
    }
    __syncthreads();                                         // par[]; and nobody reads val[] as values any more
    if (p.src_out) {
        const int len = p.len[s0];
        const int rows = min(max(len, 0), p.cap);
        int* cols = reinterpret_cast<int*>(val);             // [beam][NT]: this thread's column, every hypothesis
        for (int u = tid; u < rows; u += NT) {
            if (bin == 1) {
                for (int j = 0; j < beam; ++j) p.src_out[(s0 + j) * p.ld_src + u] = (int32_t)s0;
            } else {
                for (int j = 0; j < beam; ++j) cols[j * NT + tid] = p.src_in[(s0 + j) * p.ld_src + u];
                for (int j = 0; j < beam; ++j) p.src_out[(s0 + j) * p.ld_src + u] = cols[par[j] * NT + tid];
            }
        }
        if (len >= 0 && len < p.cap && tid < beam) p.src_out[(s0 + tid) * p.ld_src + len] = (int32_t)(s0 + tid);
    }
    if (tid == 0) p.t[b] = t + 1;
}

}  // namespace

int beam_select(const gnnlm_beam_select_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.beam >= 1 && d.beam <= MAX_BEAM, "beam_select: beam outside [1, 32]");
    GNNLM_REQUIRE(d.N >= 2 * d.beam, "beam_select: N < 2 * beam");
    GNNLM_REQUIRE(d.beam_in == 1 || d.beam_in == d.beam, "beam_select: beam_in must be 1 or beam");
    GNNLM_REQUIRE((int64_t)d.beam_in * d.N <= MAX_CAND, "beam_select: beam_in * N > 8192");
    GNNLM_REQUIRE(d.B >= 0 && d.max_new >= 0, "beam_select: B < 0 or max_new < 0");
    GNNLM_REQUIRE(d.ld_val >= d.N && d.ld_id >= d.N, "beam_select: ld_val / ld_id < N");
    GNNLM_REQUIRE(!d.src_out || (d.cap >= 0 && d.ld_src >= d.cap), "beam_select: cap < 0 or ld_src < cap");
    if (d.B == 0) return OK;
    GNNLM_REQUIRE(d.cand_val && d.cand_id && d.score_in && d.score_out && d.t && d.finished && d.len && d.done && d.next && d.parent,
                  "beam_select: cand_val / cand_id / score_in / score_out / t / finished / len / done / next / parent missing");
    GNNLM_REQUIRE(d.hist_tok && d.hist_par && d.hist_score && d.fin_n && d.fin_tok && d.fin_cum && d.fin_len && d.fin_score,
                  "beam_select: hist_* / fin_* missing");
    GNNLM_REQUIRE(!d.src_out || d.beam_in == 1 || d.src_in, "beam_select: src_out without src_in (beam_in == beam)");
    GNNLM_REQUIRE(((uintptr_t)d.cand_val | (uintptr_t)d.score_in | (uintptr_t)d.score_out | (uintptr_t)d.t | (uintptr_t)d.finished |
                   (uintptr_t)d.len | (uintptr_t)d.done | (uintptr_t)d.parent | (uintptr_t)d.src_in | (uintptr_t)d.src_out |
                   (uintptr_t)d.hist_par | (uintptr_t)d.hist_score | (uintptr_t)d.fin_n | (uintptr_t)d.fin_cum | (uintptr_t)d.fin_len |
                   (uintptr_t)d.fin_score) % 4 == 0 &&
                  ((uintptr_t)d.cand_id | (uintptr_t)d.next | (uintptr_t)d.hist_tok | (uintptr_t)d.fin_tok) % 8 == 0,
                  "beam_select: a misaligned pointer");
    const double cand = (double)d.B * d.beam_in * d.N, tab = d.src_out ? 8.0 * d.B * d.beam * d.cap : 0.0;
    ProfScope prof(K_MISC, stream, cand, 12.0 * cand + tab + 64.0 * d.B * d.beam);
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)d.B), dim3(NT), 0, stream, d);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm

using namespace gnnlm;

extern "C" int gnnlm_beam_select(const gnnlm_beam_select_t* d, void* stream) {
    GNNLM_DESC(d);
    return beam_select(*d, (hipStream_t)stream);
}
