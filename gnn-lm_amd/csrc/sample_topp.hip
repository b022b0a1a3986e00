// Nucleus (top-p) sampling over dense log-prob rows (include/gnnlm.h: gnnlm_sample_topp): the nucleus of search.Sampling._sample_topp
// (fairseq/search.py:174-217) found without a sort, and one draw from it with the caller's uniform number.
//
// One workgroup of 1024 threads per row, six sweeps of the row at the most, separated by __syncthreads(); no workspace, no host read.
//
//   sweep 0    the row's maximum M, the count of finite entries n_pos, NaN / +inf.
//   masses     every sum is an INTEGER sum.  With 2^(e-1) <= expf(M) < 2^e and H = ceil(log2 V), the mass of an entry is
//              fix(x) = trunc(expf(x) * 2^s), s = 63 - H - e, a uint64 below 2^(63 - H): V of them cannot overflow, and integer
//              addition is associative, so no sum depends on the order the atomics, the waves or the chunks happen to take -- a
//              row's bits follow from its own values alone, whatever B, ld and the pointer's alignment are.
//   sweeps 1-3 a radix select on the order-preserving key of the value, 11 / 11 / 10 bits: an LDS table of per-bin masses (two copies,
//              by lane parity, to halve same-address collisions; ds_add_u64), a block scan over the bins from the top, the bin in
//              which the prefix mass reaches p.  After sweep 3 the threshold key T, the mass above it and the mass of the entries
//              equal to it are known; their number and how many of them are admitted follow by division, all of them having the one
//              mass fix(T).  A row whose total mass is <= p keeps its n_pos finite entries and skips sweeps 2 and 3.
//   sweep 4    chunks of consecutive ids (256 * k entries, at most 2048 chunks), one wave per chunk: the mass above T and the count of
//              entries equal to T; a block scan over the chunks admits the ties with the smallest ids, gives S and the chunk that
//              holds trunc(u * S).
//   sweep 5    one wave walks that chunk in ascending id.
//
// Error bound E on every sum that is compared with p (relative to the sum) or with u * S (relative to S):
//     E(V) = 2^-21 + 2^(2 H - 62),   H = ceil(log2 V):    7.2e-7 at V = 2^20, 6.2e-5 at V = 2^24 (the largest V taken).
//   2^-21: expf within 4 ulp of exp (the device library documents 1).  2^(2H - 62): each truncation loses less than one unit, a sum
//   of at most V = 2^H terms less than 2^H units; every prefix sum of the order, and S, holds the row's largest entry, at least
//   2^(e-1) * 2^s = 2^(62 - H) units.  The sums themselves are exact.  (Entries below the float32 range, x < -87.3, carry an absolute error
//   of 2^-149 each instead: nothing next to any p or S a caller can mean.)
#include "host.h"

namespace gnnlm {
namespace {

using u64 = unsigned long long;
constexpr int NT = 1024, NW = NT / 64, BINS = 2048, MAX_CHUNKS = 2048, MAX_V = 1 << 24;
constexpr unsigned KEY_NEG_INF = 0x007fffffu;

// larger value <=> larger key; -0 and +0 share one
__device__ __forceinline__ unsigned key_of(float x) {
    unsigned b = __float_as_uint(x);
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ u64 mass_of(float x, double scale) { return x > -INFINITY ? __double2ull_rz((double)expf(x) * scale) : 0ull; }

// The row as groups of four from the 16-byte aligned address at or below its start: group q holds columns 4 q - off .. 4 q - off + 3.
// The groups [q_lo, q_hi) lie inside the row, one wide load each; the first and the last group, where the row's ends cut them, are read
// column by column, and a place outside [0, V) is never read: it counts as -inf.
struct Row {
    const float* ap;
    int off, V, G, q_lo, q_hi;
};
__device__ __forceinline__ void load_wide(const Row& r, int q, float (&x)[4]) {
    const float4 v = *reinterpret_cast<const float4*>(r.ap + 4 * (int64_t)q);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
}
__device__ __forceinline__ void load4(const Row& r, int q, float (&x)[4]) {
    if (q >= r.q_lo && q < r.q_hi) {
        load_wide(r, q, x);
    } else {
        const int j0 = 4 * q - r.off;
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = (j0 + i >= 0 && j0 + i < r.V) ? r.ap[4 * (int64_t)q + i] : -INFINITY;
    }
}

// One sweep of the row by the whole workgroup, in no particular order: f(x) for every entry (and for some -inf that stand for places
// outside the row).  A thread issues four wide loads, a workgroup's stride apart, with no branch between them, before it uses any:
// one workgroup reads a row at the rate its loads in flight allow, and a branch per load makes the compiler wait for each.
constexpr int AHEAD = 4;
template <class F>
__device__ __forceinline__ void sweep(const Row& r, int tid, F&& f) {
    int q = r.q_lo + tid;
    for (; q + (AHEAD - 1) * NT < r.q_hi; q += AHEAD * NT) {
        float x[AHEAD][4];
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) load_wide(r, q + k * NT, x[k]);
#pragma unroll
        for (int k = 0; k < AHEAD; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) f(x[k][i]);
    }
    for (; q < r.q_hi; q += NT) {
        float x[4];
        load_wide(r, q, x);
#pragma unroll
        for (int i = 0; i < 4; ++i) f(x[i]);
    }
    // the cut groups: group 0 when the row starts inside it, group G - 1 when the row ends inside it (one group when G = 1)
    if ((tid == 0 && r.q_lo == 1) || (tid == 1 && r.q_hi < r.G && !(r.G == 1 && r.q_lo == 1))) {
        float x[4];
        load4(r, tid == 0 ? 0 : r.G - 1, x);
#pragma unroll
        for (int i = 0; i < 4; ++i) f(x[i]);
    }
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ u64 wave_scan(u64 v) {            // inclusive
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
// s_w [NW]: free on entry for every thread that has passed the last barrier
__device__ __forceinline__ u64 block_sum(u64 v, u64* s_w) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) t += s_w[w];
    return t;
}
__device__ __forceinline__ u64 block_scan(u64 v, u64* s_w, u64& total) {   // inclusive over threadIdx.x
    const u64 incl = wave_scan(v);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 63) s_w[wave] = incl;
    __syncthreads();
    u64 base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (w < wave) base += s_w[w];
        total += s_w[w];
    }
    return incl + base;
}

__global__ __launch_bounds__(NT) void sample_topp_kernel(gnnlm_sample_topp_t p) {
    __shared__ u64 s_hist[2 * BINS];             // sweeps 1-3: two copies of the bins; sweep 4: the chunks' masses and tie counts
    __shared__ u64 s_w[NW];
    __shared__ u64 s_sel[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    if (p.done && p.done[b] != 0) {
        if (tid == 0) p.next[b] = p.pad;
        return;
    }
    const float* lp = p.logp + b * p.ld;
    Row r;
    r.off = (int)(((uintptr_t)lp & 15) >> 2);
    r.ap = lp - r.off;                                       // 16-byte aligned; nothing in front of lp is read through it
    r.V = p.V;
    r.G = (p.V + r.off + 3) >> 2;
    r.q_lo = r.off ? 1 : 0;
    r.q_hi = (p.V + r.off) >> 2;

    // ---- sweep 0: the maximum, the finite entries, NaN and +inf
    unsigned kmax = 0, npos = 0, nbad = 0;
    sweep(r, tid, [&](float x) {
        nbad += (x != x) | (x == INFINITY);
        npos += fabsf(x) < INFINITY;
        kmax = max(kmax, key_of(x));                         // (a NaN's key means nothing: the row is bad anyway)
    });
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, o, 64));
    if (lane == 0) s_w[wave] = kmax;
    __syncthreads();
    kmax = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) kmax = max(kmax, (unsigned)s_w[w]);
    const u64 counts = block_sum(((u64)nbad << 32) | npos, s_w);
    const float m_max = expf(value_of(kmax));
    int pick = -1;
    int n_keep = 0;
    float keep_mass = 0.f;
    if ((counts >> 32) == 0 && (unsigned)counts != 0 && m_max > 0.f && m_max < INFINITY) {
        int e;
        frexp((double)m_max, &e);
        const int H = p.V > 1 ? 32 - __clz(p.V - 1) : 0;
        const double scale = ldexp(1.0, 63 - H - e);
        const double pd = p.topp * scale;
        const u64 p_fix = pd < 9.0e18 ? max(__double2ull_ru(pd), 1ull) : ~0ull;      // every sum is below 2^63

        // ---- sweeps 1-3: the bin in which the prefix mass reaches p, digit by digit
        unsigned T = KEY_NEG_INF;        // members: key > T, and the `adm` smallest ids with key == T
        u64 adm = 0, mT = 0;
        unsigned prefix = 0;
        u64 need = p_fix;
        bool all = false;
        for (int pass = 0; pass < 3; ++pass) {
            const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, nb = pass == 2 ? 1024 : 2048;
            const unsigned himask = pass == 0 ? 0u : pass == 1 ? 0xffe00000u : 0xfffffc00u;
            __syncthreads();
            for (int i = tid; i < 2 * BINS; i += NT) s_hist[i] = 0;
            __syncthreads();
            u64* mine = s_hist + (lane & 1) * BINS;
            sweep(r, tid, [&](float x) {
                const unsigned k = key_of(x);
                if ((k & himask) == prefix) {
                    const u64 m = mass_of(x, scale);
                    if (m) atomicAdd(&mine[(k >> shift) & (nb - 1)], m);
                }
            });
            __syncthreads();
            const int b0 = nb - 1 - 2 * tid;                 // thread t owns bins b0 and b0 - 1: the walk is from the top
            const u64 h0 = b0 >= 0 ? s_hist[b0] + s_hist[BINS + b0] : 0;
            const u64 h1 = b0 >= 1 ? s_hist[b0 - 1] + s_hist[BINS + b0 - 1] : 0;
            u64 total;
            const u64 incl = block_scan(h0 + h1, s_w, total);
            if (pass == 0 && total <= need) {                // p at or above the row's mass: every finite entry
                all = true;
                break;
            }
            const u64 excl = incl - (h0 + h1);
            if (excl < need && incl >= need) {
                const bool first = excl + h0 >= need;
                s_sel[0] = (u64)(first ? b0 : b0 - 1);
                s_sel[1] = first ? excl : excl + h0;
            }
            __syncthreads();
            prefix |= (unsigned)s_sel[0] << shift;
            need -= s_sel[1];
        }
        if (!all) {
            T = prefix;
            mT = mass_of(value_of(T), scale);
            adm = mT ? (need + mT - 1) / mT : 1;                     // the smallest a with (mass above T) + a * mT >= p
        }

        // ---- sweep 4: per chunk of consecutive ids, the mass above T and the entries equal to T
        u64* s_cm = s_hist;
        unsigned* s_ct = reinterpret_cast<unsigned*>(s_hist + BINS);
        const int sub = (r.G + 64 * MAX_CHUNKS - 1) / (64 * MAX_CHUNKS);
        const int NC = (r.G + 64 * sub - 1) / (64 * sub);
        unsigned n_above = 0;
        __syncthreads();
        for (int c0 = AHEAD * wave; c0 < NC; c0 += AHEAD * NW) {         // a wave takes four chunks a turn: four loads in flight
            u64 m[AHEAD] = {};
            unsigned ties[AHEAD] = {};
            for (int i = 0; i < sub; ++i) {
                float x[AHEAD][4];
                const int q0 = (c0 * sub + i) * 64, q3 = ((c0 + AHEAD - 1) * sub + i) * 64 + 63;      // the turn's first and last group
                if (q0 >= r.q_lo && q3 < r.q_hi) {           // (wave-uniform) all inside the row: four loads, no branch between them
#pragma unroll
                    for (int k = 0; k < AHEAD; ++k) load_wide(r, ((c0 + k) * sub + i) * 64 + lane, x[k]);
                } else {
#pragma unroll
                    for (int k = 0; k < AHEAD; ++k) {
                        const int q = ((c0 + k) * sub + i) * 64 + lane;
                        if (c0 + k < NC && q < r.G) load4(r, q, x[k]);
                        else x[k][0] = x[k][1] = x[k][2] = x[k][3] = -INFINITY;
                    }
                }
#pragma unroll
                for (int k = 0; k < AHEAD; ++k)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const unsigned key = key_of(x[k][j]);
                        if (key > T) {
                            m[k] += mass_of(x[k][j], scale);
                            ++n_above;
                        } else if (key == T) {
                            ++ties[k];
                        }
                    }
            }
#pragma unroll
            for (int k = 0; k < AHEAD; ++k)
                if (c0 + k < NC) {
                    const u64 ms = wave_sum(m[k]), ts = wave_sum(ties[k]);
                    if (lane == 0) s_cm[c0 + k] = ms, s_ct[c0 + k] = (unsigned)ts;
                }
        }
        __syncthreads();
        const int c0 = 2 * tid;                              // thread t owns chunks 2 t and 2 t + 1
        const u64 t0 = c0 < NC ? s_ct[c0] : 0, t1 = c0 + 1 < NC ? s_ct[c0 + 1] : 0;
        const u64 a0 = c0 < NC ? s_cm[c0] : 0, a1 = c0 + 1 < NC ? s_cm[c0 + 1] : 0;
        u64 unused;
        const u64 tb0 = block_scan(t0 + t1, s_w, unused) - (t0 + t1), tb1 = tb0 + t0;      // ties in front of the chunk
        const u64 g0 = min(t0, adm > tb0 ? adm - tb0 : 0ull), g1 = min(t1, adm > tb1 ? adm - tb1 : 0ull);
        const u64 mm0 = a0 + g0 * mT, mm1 = a1 + g1 * mT;
        u64 S;
        const u64 incl = block_scan(mm0 + mm1, s_w, S);
        n_keep = (int)(block_sum(n_above, s_w) + adm);
        keep_mass = (float)((double)S / scale);
        const u64 target = min(__double2ull_rz((double)p.u[b] * (double)S), S - 1);        // u * S rounded up to S: the last member
        const u64 excl = incl - (mm0 + mm1);
        if (excl <= target && target < incl) {
            const bool first = target < excl + mm0;
            s_sel[0] = (u64)(first ? c0 : c0 + 1);
            s_sel[1] = first ? excl : excl + mm0;
            s_sel[2] = first ? tb0 : tb1;
        }
        __syncthreads();

        // ---- sweep 5: the chunk that holds the target, in ascending id
        if (wave == 0) {
            const int c = (int)s_sel[0];
            u64 base = s_sel[1], tbase = s_sel[2];
            for (int i = 0; i < sub && pick < 0; ++i) {
                const int q = (c * sub + i) * 64 + lane;
                float x[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (q < r.G) load4(r, q, x);
                unsigned k[4];
                u64 lt = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) k[j] = key_of(x[j]), lt += k[j] == T;
                const u64 lt_incl = wave_scan(lt);
                u64 rank = tbase + lt_incl - lt;             // of this lane's first tie
                u64 m[4], lm = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    m[j] = k[j] > T ? mass_of(x[j], scale) : (k[j] == T && rank++ < adm) ? mT : 0ull;
                    lm += m[j];
                }
                const u64 w_incl = wave_scan(lm);
                const u64 lo = base + w_incl - lm;
                const unsigned long long hit = __ballot(lo <= target && target < lo + lm);
                if (hit) {
                    const int src = __ffsll(hit) - 1;
                    int mine = -1;
                    u64 run = lo;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        run += m[j];
                        if (mine < 0 && run > target) mine = 4 * q - r.off + j;
                    }
                    pick = __shfl(mine, src, 64);
                } else {
                    base += __shfl(w_incl, 63, 64);
                    tbase += __shfl(lt_incl, 63, 64);
                }
            }
        }
    }
    if (tid == 0) {
        if (pick < 0 || pick >= p.V) {                       // a bad row: NaN, +inf, or no positive mass
            p.next[b] = p.pad;
            if (p.done) p.done[b] = 1;
            if (p.n_bad) atomicAdd(p.n_bad, 1);
            return;
        }
        p.next[b] = pick;
        if (p.next_logp) p.next_logp[b] = lp[pick];
        if (p.done && pick == p.eos) p.done[b] = 1;
        if (p.n_keep) p.n_keep[b] = n_keep;
        if (p.keep_mass) p.keep_mass[b] = keep_mass;
    }
}

}  // namespace

int sample_topp(const gnnlm_sample_topp_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.topp > 0, "sample_topp: topp must be greater than 0");
    GNNLM_REQUIRE(d.V >= 1 && d.V <= MAX_V, "sample_topp: V outside [1, 2^24]");
    GNNLM_REQUIRE(d.B >= 0, "sample_topp: B < 0");
    GNNLM_REQUIRE(d.ld >= d.V, "sample_topp: ld < V");
    if (d.B == 0) return OK;
    GNNLM_REQUIRE(d.logp && d.u && d.next, "sample_topp: logp / u / next missing");
    GNNLM_REQUIRE((uintptr_t)d.logp % 4 == 0 && (uintptr_t)d.u % 4 == 0 && (uintptr_t)d.next % 8 == 0 && (uintptr_t)d.next_logp % 4 == 0 &&
                  (uintptr_t)d.done % 4 == 0 && (uintptr_t)d.n_bad % 4 == 0 && (uintptr_t)d.n_keep % 4 == 0 && (uintptr_t)d.keep_mass % 4 == 0,
                  "sample_topp: a misaligned pointer");
    // sweeps 0, 1 and 4 always; 2, 3 and a chunk more when the row's mass exceeds p, which only the device knows: booked when p is finite
    const double sweeps = d.topp < INFINITY ? 5.0 : 3.0;
    ProfScope prof(K_MISC, stream, 8.0 * d.B * d.V, sweeps * 4.0 * d.B * d.V + 32.0 * d.B);
    hipLaunchKernelGGL(sample_topp_kernel, dim3((unsigned)d.B), dim3(NT), 0, stream, d);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm

using namespace gnnlm;

extern "C" int gnnlm_sample_topp(const gnnlm_sample_topp_t* d, void* stream) {
    GNNLM_DESC(d);
    return sample_topp(*d, (hipStream_t)stream);
}
