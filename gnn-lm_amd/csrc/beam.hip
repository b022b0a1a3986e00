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
//
// gnnlm_beam_select_diverse (search.DiverseBeamSearch, search.py:105-164; search.DiverseSiblingsSearch, :291-353) differs in how
// the list is drawn and shares everything behind it (finish_step).  Groups: the groups run one after the other; a group stages the
// values of its own hypotheses' candidates, each lowered by strength times the number of times its token stands among the
// candidates the earlier groups chose (those tokens, at most 2 * beam, are a list in LDS that a candidate scans), draws its
// 2 * beam / G candidates by the same rounds and writes candidate c to place c * G + g of the list.  Siblings: a candidate's rank
// among its hypothesis's own candidates is counted against the row's staged values, rank * rate is taken off, and the rounds run
// as in the plain kernel.
#include "host.h"

namespace gnnlm {
namespace {

constexpr int MAX_BEAM = 32, MAX_CAND = 8192, NT = 256;

struct SelectLds {
    float val[MAX_CAND];                                     // the candidates' values; later the table's columns [beam][NT]
    float w_v[NT / 64];
    int w_i[NT / 64];
    float sel_v[2 * MAX_BEAM];                               // the step's list: value, hypothesis (< 0: an empty place), token
    int sel_j[2 * MAX_BEAM];
    long long sel_t[2 * MAX_BEAM];
    int act[MAX_BEAM], fin[MAX_BEAM], par[MAX_BEAM];
    int n_act, n_new, fin0;
};

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

// candidate q of group g: row q / N of the group's hypotheses g, g + G, .. (one_row: the sentence's only row), column q % N
__device__ __forceinline__ int group_cand(int q, int N, int G, int g, bool one_row) {
    const int row = q / N;
    return (one_row ? 0 : g + row * G) * N + (q - row * N);
}

// One round: the first of the n candidates still present in s.val under the order -> its index i (-1: none is left) and value, the
// same in every thread.  GROUPS: the n candidates are group g's (group_cand); otherwise i = 0 .. n - 1.  Ends behind a barrier that
// every thread has passed; the caller's barrier after its own writes closes the round.
template <bool GROUPS>
__device__ __forceinline__ int draw(SelectLds& s, int n, int N, int G, int g, bool one_row, const int64_t* ci, int64_t ld_id, float& v_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float bv = -INFINITY;
    int bi = -1;
    for (int q = tid; q < n; q += NT) {
        const int i = GROUPS ? group_cand(q, N, G, g, one_row) : q;
        const float v = s.val[i];
        if (v > -INFINITY && before(v, i, bv, bi, N, ci, ld_id)) {
            bv = v;
            bi = i;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (before(ov, oi, bv, bi, N, ci, ld_id)) {
            bv = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        s.w_v[wave] = bv;
        s.w_i[wave] = bi;
    }
    __syncthreads();
    bv = s.w_v[0];
    bi = s.w_i[0];
    for (int w = 1; w < NT / 64; ++w)
        if (before(s.w_v[w], s.w_i[w], bv, bi, N, ci, ld_id)) {
            bv = s.w_v[w];
            bi = s.w_i[w];
        }
    v_out = bv;
    return bi;
}

// Everything behind the step's list s.sel_*[0 .. L): finalize, survive, table, finish (include/gnnlm.h).  Called by every thread
// behind a barrier after the list's last write.
__device__ __forceinline__ void finish_step(const gnnlm_beam_select_t& p, SelectLds& s, int b, int t, int L) {
    const int tid = threadIdx.x;
    const int beam = p.beam, bin = p.beam_in;
    const int64_t s0 = (int64_t)b * beam;
    if (tid == 0) {
        int nf = min(max(p.fin_n[b], 0), beam), k = 0, na = 0;
        s.fin0 = nf;
        for (int r = 0; r < min(beam, L); ++r)
            if (s.sel_j[r] >= 0 && s.sel_t[r] == p.eos && nf < beam) {
                s.fin[k++] = r;
                ++nf;
            }
        for (int r = 0; r < L && na < beam; ++r)
            if (s.sel_j[r] >= 0 && s.sel_t[r] != p.eos) s.act[na++] = r;
        s.n_act = na;
        s.n_new = k;
        p.fin_n[b] = nf;
    }
    __syncthreads();
    const int T1 = p.max_new + 1;
    if (tid < beam) {                                        // hypothesis tid of the next step
        const int j = tid;
        const bool live = j < s.n_act;
        const int r = live ? s.act[j] : 0;
        const int jp = live ? s.sel_j[r] : j;
        const float sc = live ? s.sel_v[r] : -INFINITY;
        const int64_t tok = live ? (int64_t)s.sel_t[r] : p.pad;
        s.par[j] = jp;
        p.next[s0 + j] = tok;
        p.parent[s0 + j] = (int32_t)(s0 + jp);
        p.score_out[s0 + j] = sc;
        const int64_t h = ((int64_t)b * T1 + t) * beam + j;
        p.hist_tok[h] = tok;
        p.hist_par[h] = jp;
        p.hist_score[h] = sc;
    }
    if (tid < s.n_new) {                                     // a finalized hypothesis: its parent's history along the backpointers
        const int r = s.fin[tid], slot = s.fin0 + tid;
        int64_t* ft = p.fin_tok + (s0 + slot) * T1;
        float* fc = p.fin_cum + (s0 + slot) * T1;
        int cur = s.sel_j[r];
        for (int u = t - 1; u >= 0; --u) {                   // (steps below t: written by earlier launches)
            const int64_t h = ((int64_t)b * T1 + u) * beam + cur;
            ft[u] = p.hist_tok[h];
            fc[u] = p.hist_score[h];
            cur = min(max(p.hist_par[h], 0), beam - 1);
        }
        ft[t] = p.eos;
        fc[t] = s.sel_v[r];
        p.fin_len[s0 + slot] = t + 1;
        p.fin_score[s0 + slot] = s.sel_v[r];
    }
    if (s.fin0 + s.n_new >= beam || t == p.max_new) {
        if (tid < beam) p.done[s0 + tid] = 1;
        if (tid == 0) p.finished[b] = 1;
    }
    __syncthreads();                                         // par[]; and nobody reads val[] as values any more
    if (p.src_out) {
        const int len = p.len[s0];
        const int rows = min(max(len, 0), p.cap);
        int* cols = reinterpret_cast<int*>(s.val);           // [beam][NT]: this thread's column, every hypothesis
        for (int u = tid; u < rows; u += NT) {
            if (bin == 1) {
                for (int j = 0; j < beam; ++j) p.src_out[(s0 + j) * p.ld_src + u] = (int32_t)s0;
            } else {
                for (int j = 0; j < beam; ++j) cols[j * NT + tid] = p.src_in[(s0 + j) * p.ld_src + u];
                for (int j = 0; j < beam; ++j) p.src_out[(s0 + j) * p.ld_src + u] = cols[s.par[j] * NT + tid];
            }
        }
        if (len >= 0 && len < p.cap && tid < beam) p.src_out[(s0 + tid) * p.ld_src + len] = (int32_t)(s0 + tid);
    }
    if (tid == 0) p.t[b] = t + 1;
}

__global__ __launch_bounds__(NT) void beam_select_kernel(gnnlm_beam_select_t p) {
    __shared__ SelectLds s;
    const int b = blockIdx.x, tid = threadIdx.x;
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
        const float sc = p.score_in[s0 + j] + v;
        s.val[i] = fabsf(v) < INFINITY && fabsf(sc) < INFINITY ? sc : -INFINITY;
    }
    __syncthreads();
    int C = 0;
    for (int r = 0; r < 2 * beam; ++r) {
        float bv;
        const int bi = draw<false>(s, n, N, 1, 0, false, ci, p.ld_id, bv);
        if (bi < 0) break;                                   // (the same for every thread) nothing present is left
        if (tid == 0) {
            const int j = bi / N;
            s.sel_v[r] = bv;
            s.sel_j[r] = j;
            s.sel_t[r] = ci[j * p.ld_id + (bi - j * N)];
            s.val[bi] = -INFINITY;
        }
        C = r + 1;
        __syncthreads();
    }
    finish_step(p, s, b, t, C);
}

__global__ __launch_bounds__(NT) void beam_select_diverse_kernel(gnnlm_beam_select_t p, int G, float strength, float rate) {
    __shared__ SelectLds s;
    __shared__ float raw[MAX_CAND];                          // siblings: the unpenalised values, to rank a row's candidates against
    __shared__ long long chosen[2 * MAX_BEAM];               // groups: the tokens of the candidates chosen so far at this step
    __shared__ int n_chosen;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (p.finished[b] != 0) return;
    const int t = p.t[b];
    if (t < 0 || t > p.max_new) return;
    const int beam = p.beam, bin = p.beam_in, N = p.N;
    const bool one_row = bin == 1, siblings = G == 1 && rate != 0.0f && !one_row;
    const int rows_g = one_row ? 1 : beam / G, ng = rows_g * N, per_group = 2 * (beam / G);
    const int64_t s0 = (int64_t)b * beam;
    const float* cv = p.cand_val + (int64_t)b * bin * p.ld_val;
    const int64_t* ci = p.cand_id + (int64_t)b * bin * p.ld_id;
    if (tid < 2 * beam) s.sel_j[tid] = -1;
    if (tid == 0) n_chosen = 0;
    if (siblings) {
        for (int i = tid; i < ng; i += NT) {
            const int j = i / N, c = i - j * N;
            const float v = cv[j * p.ld_val + c];
            const float sc = __fadd_rn(p.score_in[s0 + j], v);
            raw[i] = fabsf(v) < INFINITY && fabsf(sc) < INFINITY ? sc : -INFINITY;
        }
    }
    __syncthreads();
    int L = 0;
    for (int g = 0; g < G; ++g) {
        const int nc = n_chosen;
        for (int q = tid; q < ng; q += NT) {                 // the group's values
            const int i = group_cand(q, N, G, g, one_row), j = i / N, c = i - j * N;
            float out = -INFINITY;
            if (siblings) {
                const float x = raw[i];
                if (x > -INFINITY) {
                    int rank = 1;                            // 1 + the row's present candidates that come before this one
                    for (int c2 = 0; c2 < N; ++c2) {
                        const float y = raw[j * N + c2];
                        if (y > x) {
                            ++rank;
                        } else if (y == x && c2 != c) {
                            const int64_t ta = ci[j * p.ld_id + c2], tb = ci[j * p.ld_id + c];
                            rank += ta < tb || (ta == tb && c2 < c);
                        }
                    }
                    const float sc = __fsub_rn(x, __fmul_rn((float)rank, rate));
                    if (rank <= 2 * beam && fabsf(sc) < INFINITY) out = sc;
                }
            } else {
                const float v = cv[j * p.ld_val + c];
                float x = v;
                if (nc > 0 && fabsf(v) < INFINITY) {
                    const long long tok = ci[j * p.ld_id + c];
                    int cnt = 0;
                    for (int k = 0; k < nc; ++k) cnt += chosen[k] == tok;
                    if (cnt) x = __fadd_rn(v, __fmul_rn(-strength, (float)cnt));
                }
                const float sc = __fadd_rn(p.score_in[s0 + j], x);
                if (fabsf(v) < INFINITY && fabsf(sc) < INFINITY) out = sc;
            }
            s.val[i] = out;
        }
        __syncthreads();
        for (int r = 0; r < per_group; ++r) {
            float bv;
            const int bi = draw<true>(s, ng, N, G, g, one_row, ci, p.ld_id, bv);
            if (bi < 0) break;                               // (the same for every thread) the group has nothing present left
            if (tid == 0) {
                const int j = bi / N, at = r * G + g;
                const long long tok = ci[j * p.ld_id + (bi - j * N)];
                s.sel_v[at] = bv;
                s.sel_j[at] = j;
                s.sel_t[at] = tok;
                s.val[bi] = -INFINITY;
                chosen[nc + r] = tok;
                n_chosen = nc + r + 1;
            }
            L = max(L, r * G + g + 1);
            __syncthreads();
        }
        __syncthreads();                                     // (a group that ended early: its last reads of w_* before the next stage)
    }
    finish_step(p, s, b, t, L);
}

int check_select(const gnnlm_beam_select_t& d) {
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
    return OK;
}

}  // namespace

int beam_select(const gnnlm_beam_select_t& d, hipStream_t stream) {
    if (const int rc = check_select(d)) return rc;
    if (d.B == 0) return OK;
    const double cand = (double)d.B * d.beam_in * d.N, tab = d.src_out ? 8.0 * d.B * d.beam * d.cap : 0.0;
    ProfScope prof(K_MISC, stream, cand, 12.0 * cand + tab + 64.0 * d.B * d.beam);
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)d.B), dim3(NT), 0, stream, d);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int beam_select_diverse(const gnnlm_beam_select_diverse_t& dd, hipStream_t stream) {
    const gnnlm_beam_select_t& d = dd.sel;
    GNNLM_REQUIRE(dd.groups >= 1, "beam_select_diverse: groups < 1");
    GNNLM_REQUIRE(dd.strength >= 0.0f && dd.strength < INFINITY, "beam_select_diverse: strength negative or not finite");
    GNNLM_REQUIRE(dd.rate >= 0.0f && dd.rate < INFINITY, "beam_select_diverse: rate negative or not finite");
    GNNLM_REQUIRE(dd.groups == 1 || dd.rate == 0.0f, "beam_select_diverse: groups > 1 together with rate != 0");
    if (const int rc = check_select(d)) return rc;
    GNNLM_REQUIRE(d.beam % dd.groups == 0, "beam_select_diverse: beam % groups != 0");
    if (d.B == 0) return OK;
    const double cand = (double)d.B * d.beam_in * d.N, tab = d.src_out ? 8.0 * d.B * d.beam * d.cap : 0.0;
    ProfScope prof(K_MISC, stream, cand, 12.0 * cand + tab + 64.0 * d.B * d.beam);
    hipLaunchKernelGGL(beam_select_diverse_kernel, dim3((unsigned)d.B), dim3(NT), 0, stream, d, (int)dd.groups, dd.strength, dd.rate);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm

using namespace gnnlm;

extern "C" int gnnlm_beam_select(const gnnlm_beam_select_t* d, void* stream) {
    GNNLM_DESC(d);
    return beam_select(*d, (hipStream_t)stream);
}

extern "C" int gnnlm_beam_select_diverse(const gnnlm_beam_select_diverse_t* d, void* stream) {
    GNNLM_DESC(d);
    return beam_select_diverse(*d, (hipStream_t)stream);
}
