// Decode-step attention against a K/V cache (include/gnnlm.h: gnnlm_kv_cache_t, gnnlm_decode_attn) and the three small cache
// kernels of the prefill and the step: the incremental_state branch of fairseq's MultiheadAttention for ONE new row per sequence.
//
// The work is memory-bound (2 * len * d * 4 bytes per sequence and layer against 4 * len * d flops), and a single query gives
// the matrix cores nothing to do, so K and V rows go straight into registers with 16-byte loads and the dot products run on
// the VALU.  The keys of one (b, h) are cut into chunks of GNNLM_DECODE_CHUNK; one wave takes one chunk, so B * H * chunks waves
// are in flight whatever B * H is.  A wave's lanes form G = 256 / d_k groups of d_k / 4 lanes: a group holds one key row per load
// (each lane 4 columns) and keeps its own running (maximum, sum, accumulator) over the keys g, g + G, ... of the chunk; the groups
// are merged once at the end of the chunk in a fixed butterfly.  The chunk's triple goes to the workspace and a second launch
// combines the chunks of a (b, h) in ascending order -- no float atomics, so a row's bits depend on that row alone.
#include "host.h"

namespace gnnlm {
namespace {

constexpr int CHUNK = GNNLM_DECODE_CHUNK;
constexpr int UNR = 4;                     // keys per group in flight: 2 * UNR 16-byte loads per lane

struct DecParams {
    const float *q, *k_new, *v_new; int64_t ld;
    float *kc, *vc;                        // the layer's planes [B][cap][ld_row]
    int64_t ld_row, ld_seq;
    int cap;                               // the rows a len may name: min(cache.cap, max_len)
    const int32_t* len; const int32_t* done; int32_t* n_bad;
    float* part;                           // [B * H * n_chunk][DK + 4]: (max, sum, 0, 0), accumulator
    float* out; int64_t ldo;
    int B, H, n_chunk;
    int32_t* keys_out;                     // profiling only (else nullptr): the keys the launch really attends, summed over b
    SlotTable tab;                         // IND only (gnnlm_beam_attn): key row u < len of b is row u of cache sequence src[b][u]
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// IND (gnnlm_beam_attn): the cached rows are found through p.src; the loads, the arithmetic and their order are the same, so a row's
// bits are those of the contiguous cache.  A table entry outside [0, B) is not followed and flags the chunk's partial (third float).
template <int DK, bool IND = false>
__global__ __launch_bounds__(256) void decode_attn_chunk_kernel(DecParams p) {
    constexpr int LPK = DK / 4;            // lanes per key row
    constexpr int G = 64 / LPK;            // key rows per wave-wide load
    static_assert(CHUNK % (G * UNR) == 0, "a chunk is a whole number of unrolled passes");
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (int64_t)p.B * p.H * p.n_chunk) return;
    const int c = (int)(item % p.n_chunk);
    const int bh = (int)(item / p.n_chunk);
    const int h = bh % p.H, b = bh / p.H;
    if (p.done && p.done[b] != 0) return;
    const int len = p.len[b];
    if (len < 0 || len >= p.cap) return;   // never followed; the combine kernel counts it
    const int u0 = c * CHUNK;
    if (u0 > len) return;
    const int g = lane / LPK, sub = lane % LPK;
    const int64_t col = (int64_t)h * DK + sub * 4;
    const float* qp = p.q + b * p.ld + col;
    const float* knp = p.k_new + b * p.ld + col;
    const float* vnp = p.v_new + b * p.ld + col;
    float* kb = p.kc + b * p.ld_seq + col;
    float* vb = p.vc + b * p.ld_seq + col;
    if (len - u0 < CHUNK && g == 0) {      // this wave's chunk holds the new row: append it (its own columns; H waves cover the row)
        st4(kb + (int64_t)len * p.ld_row, ld4(knp));
        st4(vb + (int64_t)len * p.ld_row, ld4(vnp));
    }
    const float4 q4 = ld4(qp);
    [[maybe_unused]] const int32_t* tab = IND ? p.tab.src + b * p.tab.ld : nullptr;
    [[maybe_unused]] bool bad = false;
    float m = -INFINITY, s = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int it = 0; it < CHUNK / G; it += UNR) {
        if (u0 + it * G > len) break;      // (wave-uniform) nothing valid from here on
        float sc[UNR];
        float4 v4[UNR];
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const int u = u0 + (it + j) * G + g;
            bool valid = u <= len;
            // the new row is read from k_new / v_new, not back from the cache; an invalid key reads nothing of the cache either
            const float* kp = u < len ? kb + (int64_t)u * p.ld_row : knp;
            const float* vp = u < len ? vb + (int64_t)u * p.ld_row : vnp;
            if constexpr (IND) {
                if (u < len) {
                    const int slot = tab[u];
                    if (slot >= 0 && slot < p.B) {
                        const int64_t off = slot * p.ld_seq + col + (int64_t)u * p.ld_row;
                        kp = p.kc + off;
                        vp = p.vc + off;
                    } else {                                   // never followed: nothing of the cache is read for this key
                        kp = knp;
                        vp = vnp;
                        valid = false;
                        bad = true;
                    }
                }
            }
            const float4 k4 = ld4(kp);
            const float4 vv = ld4(vp);
            float dot = q4.x * k4.x;
            dot = fmaf(q4.y, k4.y, dot);
            dot = fmaf(q4.z, k4.z, dot);
            dot = fmaf(q4.w, k4.w, dot);
#pragma unroll
            for (int o = 1; o < LPK; o <<= 1) dot += __shfl_xor(dot, o, 64);
            sc[j] = valid ? dot : -INFINITY;
            v4[j] = valid ? vv : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float mx = m;
#pragma unroll
        for (int j = 0; j < UNR; ++j) mx = fmaxf(mx, sc[j]);
        if (mx == -INFINITY) continue;     // (this group has no valid key yet)
        const float corr = m == -INFINITY ? 0.f : expf(m - mx);
        s *= corr;
        acc.x *= corr; acc.y *= corr; acc.z *= corr; acc.w *= corr;
#pragma unroll
        for (int j = 0; j < UNR; ++j) {
            const float e = sc[j] == -INFINITY ? 0.f : expf(sc[j] - mx);
            s += e;
            acc.x = fmaf(e, v4[j].x, acc.x);
            acc.y = fmaf(e, v4[j].y, acc.y);
            acc.z = fmaf(e, v4[j].z, acc.z);
            acc.w = fmaf(e, v4[j].w, acc.w);
        }
        m = mx;
    }
    // merge the G groups: the chunk's maximum, then the rescaled sums in a fixed butterfly
    float M = m;
#pragma unroll
    for (int o = LPK; o < 64; o <<= 1) M = fmaxf(M, __shfl_xor(M, o, 64));
    const float sc_g = m == -INFINITY ? 0.f : expf(m - M);
    s *= sc_g;
    acc.x *= sc_g; acc.y *= sc_g; acc.z *= sc_g; acc.w *= sc_g;
#pragma unroll
    for (int o = LPK; o < 64; o <<= 1) {
        s += __shfl_xor(s, o, 64);
        acc.x += __shfl_xor(acc.x, o, 64);
        acc.y += __shfl_xor(acc.y, o, 64);
        acc.z += __shfl_xor(acc.z, o, 64);
        acc.w += __shfl_xor(acc.w, o, 64);
    }
    float* dst = p.part + item * (DK + 4);
    float flag = 0.f;
    if constexpr (IND) flag = __any(bad) ? 1.f : 0.f;
    if (lane == 0) st4(dst, make_float4(M, s, flag, 0.f));
    if (g == 0) st4(dst + 4 + sub * 4, acc);
}

// The chunks of a (b, h) in ascending order; a wave takes G (b, h) pairs, each lane 4 output columns.
template <int DK, bool IND = false>
__global__ __launch_bounds__(64) void decode_attn_combine_kernel(DecParams p) {
    constexpr int LPK = DK / 4;
    constexpr int G = 64 / LPK;
    const int lane = threadIdx.x;
    const int g = lane / LPK, sub = lane % LPK;
    if (p.keys_out && blockIdx.x == 0 && lane == 0) {         // the profiler's work count: len[b] + 1 keys of every row that takes part
        int64_t keys = 0;
        for (int i = 0; i < p.B; ++i) {
            const int l = p.len[i];
            if (!(p.done && p.done[i] != 0) && l >= 0 && l < p.cap) keys += l + 1;
        }
        *p.keys_out = (int32_t)min(keys, (int64_t)0x7fffffff);
    }
    const int64_t bh = (int64_t)blockIdx.x * G + g;
    if (bh >= (int64_t)p.B * p.H) return;
    const int h = (int)(bh % p.H), b = (int)(bh / p.H);
    float* o = p.out + b * p.ldo + (int64_t)h * DK + sub * 4;
    const bool dn = p.done && p.done[b] != 0;
    const int len = p.len[b];
    bool bad = len < 0 || len >= p.cap;
    if constexpr (IND) {                                      // a chunk that met a table entry outside [0, B): the row is out of range
        if (!dn && !bad) {
            const float* f = p.part + bh * p.n_chunk * (DK + 4);
            for (int c = 0; c < len / CHUNK + 1; ++c, f += DK + 4) bad |= f[2] != 0.f;
        }
    }
    if (dn || bad) {
        st4(o, make_float4(0.f, 0.f, 0.f, 0.f));
        if (!dn && h == 0 && sub == 0 && p.n_bad) atomicAdd(p.n_bad, 1);
        return;
    }
    const int nc = len / CHUNK + 1;
    const float* src = p.part + bh * p.n_chunk * (DK + 4);
    float M = -INFINITY, S = 0.f;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int c = 0; c < nc; ++c, src += DK + 4) {
        const float4 ms = ld4(src);
        const float4 a = ld4(src + 4 + sub * 4);
        const float mn = fmaxf(M, ms.x);
        if (mn == -INFINITY) continue;
        const float fa = M == -INFINITY ? 0.f : expf(M - mn);
        const float fb = ms.x == -INFINITY ? 0.f : expf(ms.x - mn);
        S = S * fa + ms.y * fb;
        A.x = A.x * fa + a.x * fb;
        A.y = A.y * fa + a.y * fb;
        A.z = A.z * fa + a.z * fb;
        A.w = A.w * fa + a.w * fb;
        M = mn;
    }
    st4(o, make_float4(A.x / S, A.y / S, A.z / S, A.w / S));
}

struct FillParams {
    const float *k, *v; int64_t ld_src;    // the K' and V' rows [n_tok, ld_src] of the packed tokens
    float *kc, *vc; int64_t ld_row, ld_seq;
    const int32_t* block_off; int n_blocks; int64_t n_tok;
    int d4, max_rows;
};
// One wave per packed row: its block by bisection (as lm_embed_kernel), its position in the block is its cache row.
__global__ __launch_bounds__(256) void kv_cache_fill_kernel(FillParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.n_tok) return;
    const int64_t base = p.block_off[0];
    const int lo = last_block(p.block_off, p.n_blocks, r, base);
    const int64_t t = r - ((int64_t)p.block_off[lo] - base);
    if (t < 0 || t >= p.max_rows) return;                  // (the host refused a block longer than the cache: memory safety only)
    const float4* ks = reinterpret_cast<const float4*>(p.k + r * p.ld_src);
    const float4* vs = reinterpret_cast<const float4*>(p.v + r * p.ld_src);
    float4* kd = reinterpret_cast<float4*>(p.kc + lo * p.ld_seq + t * p.ld_row);
    float4* vd = reinterpret_cast<float4*>(p.vc + lo * p.ld_seq + t * p.ld_row);
    for (int e = lane; e < p.d4; e += 64) {
        kd[e] = ks[e];
        vd[e] = vs[e];
    }
}

__global__ __launch_bounds__(256) void kv_len_set_kernel(int32_t* len, const int32_t* block_off, int B, int max_rows) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) len[b] = max(0, min(block_off[b + 1] - block_off[b], max_rows));
}
__global__ __launch_bounds__(256) void kv_len_advance_kernel(int32_t* len, const int32_t* done, int B, int cap) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B || (done && done[b] != 0)) return;
    const int l = len[b];
    if (l >= 0 && l < cap) len[b] = l + 1;
}

}  // namespace

bool decode_attn_ok(int dk) { return dk == 16 || dk == 32 || dk == 64 || dk == 128; }

int check_kv_cache(const gnnlm_kv_cache_t& c) {
    GNNLM_REQUIRE(c.L >= 1 && c.B >= 0 && c.cap >= 1 && c.d >= 4 && c.d % 4 == 0, "kv_cache: needs L >= 1, B >= 0, cap >= 1, d % 4 == 0");
    GNNLM_REQUIRE(c.ld_row >= c.d && c.ld_row % 4 == 0, "kv_cache: ld_row must be a multiple of 4 and >= d");
    GNNLM_REQUIRE(c.ld_seq >= (int64_t)c.cap * c.ld_row && c.ld_seq % 4 == 0, "kv_cache: ld_seq must be a multiple of 4 and >= cap * ld_row");
    GNNLM_REQUIRE(c.ld_layer >= (int64_t)c.B * c.ld_seq && c.ld_layer % 4 == 0, "kv_cache: ld_layer must be a multiple of 4 and >= B * ld_seq");
    if (c.B == 0) return OK;
    GNNLM_REQUIRE(c.k && c.v && (uintptr_t)c.k % 16 == 0 && (uintptr_t)c.v % 16 == 0, "kv_cache: k / v missing or not 16-byte aligned");
    GNNLM_REQUIRE(c.len && (uintptr_t)c.len % 4 == 0 && (uintptr_t)c.done % 4 == 0 && (uintptr_t)c.n_bad % 4 == 0, "kv_cache: len missing, or len / done / n_bad misaligned");
    return OK;
}

size_t decode_attn_workspace_bytes(int B, int H, int dk, int max_len) {
    if (B <= 0 || H <= 0 || dk <= 0 || max_len <= 0) return 0;
    return (size_t)B * H * cdiv(max_len, CHUNK) * (dk + 4) * sizeof(float);
}

namespace {
template <bool IND>
void launch_dec(int dk, dim3 g1, dim3 g2, hipStream_t stream, const DecParams& p) {
#define GNNLM_DEC(DK)                                                                                  \
    case DK:                                                                                           \
        hipLaunchKernelGGL((decode_attn_chunk_kernel<DK, IND>), g1, dim3(256), 0, stream, p);          \
        hipLaunchKernelGGL((decode_attn_combine_kernel<DK, IND>), g2, dim3(64), 0, stream, p);         \
        break;
    switch (dk) { GNNLM_DEC(16) GNNLM_DEC(32) GNNLM_DEC(64) GNNLM_DEC(128) }
#undef GNNLM_DEC
}
}  // namespace

// tab == nullptr: gnnlm_decode_attn, its two launches as they always were; else gnnlm_beam_attn
int decode_attn(const gnnlm_decode_attn_t& d, const SlotTable* tab, hipStream_t stream) {
    const gnnlm_kv_cache_t& c = d.cache;
    GNNLM_REQUIRE(decode_attn_ok(d.dk), "decode_attn: d_k must be 16, 32, 64 or 128");
    int rc = check_kv_cache(c);
    if (rc != OK) return rc;
    GNNLM_REQUIRE(d.H >= 1 && (int64_t)d.H * d.dk == c.d, "decode_attn: H * d_k != cache.d");
    GNNLM_REQUIRE(d.layer >= 0 && d.layer < c.L, "decode_attn: layer outside [0, L)");
    GNNLM_REQUIRE(d.max_len >= 0 && d.max_len <= c.cap, "decode_attn: max_len outside [0, cap]");
    GNNLM_REQUIRE(d.ld >= c.d && d.ld % 4 == 0 && d.ldo >= c.d && d.ldo % 4 == 0, "decode_attn: ld / ldo must be multiples of 4 and >= H * d_k");
    if (tab) GNNLM_REQUIRE(tab->ld >= c.cap, "beam_attn: ld_src < cache.cap");
    if (c.B == 0) return OK;
    if (tab) GNNLM_REQUIRE(tab->src && (uintptr_t)tab->src % 4 == 0, "beam_attn: src missing or misaligned");
    GNNLM_REQUIRE(d.q && d.k_new && d.v_new && d.out, "decode_attn: q / k_new / v_new / out missing");
    GNNLM_REQUIRE(((uintptr_t)d.q | (uintptr_t)d.k_new | (uintptr_t)d.v_new | (uintptr_t)d.out) % 16 == 0, "decode_attn: q / k_new / v_new / out must be 16-byte aligned");
    const int bound = d.max_len ? d.max_len : c.cap;
    const size_t need = decode_attn_workspace_bytes(c.B, d.H, d.dk, bound);
    GNNLM_REQUIRE(d.workspace && (uintptr_t)d.workspace % 16 == 0 && d.workspace_bytes >= need, "decode_attn: workspace missing, misaligned or too small");
    DecParams p{d.q, d.k_new, d.v_new, d.ld, c.k + d.layer * c.ld_layer, c.v + d.layer * c.ld_layer, c.ld_row, c.ld_seq, bound,
                c.len, c.done, c.n_bad, reinterpret_cast<float*>(d.workspace), d.out, d.ldo, c.B, d.H, (int)cdiv(bound, CHUNK), nullptr,
                tab ? *tab : SlotTable{}};
    const int64_t items = (int64_t)c.B * d.H * p.n_chunk;
    GNNLM_REQUIRE(cdiv(items, 4) < (1ll << 31), "decode_attn: too many chunks for one launch");
    // work: K and V read once, the partials written and read once -- stated for B * bound keys, which is all the host knows, and
    // scaled by the keys the rows really hold (sum of len[b] + 1), which the combine kernel reports when a profile is open
    ProfScope prof(K_CAUSAL, stream, 4.0 * c.B * bound * c.d,
                   8.0 * c.B * bound * c.d + 8.0 * items * (d.dk + 4) + 16.0 * c.B * c.d + (tab ? 4.0 * d.H * c.B * bound : 0.0),
                   c.len, (double)c.B * bound, true);
    if (!prof.slot) prof.sd = nullptr;                        // (no slot to be had: the bound stands, unscaled)
    p.keys_out = prof.slot;
    const dim3 g1((unsigned)cdiv(items, 4)), g2((unsigned)cdiv((int64_t)c.B * d.H, 256 / d.dk));
    if (tab) launch_dec<true>(d.dk, g1, g2, stream, p);
    else launch_dec<false>(d.dk, g1, g2, stream, p);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int kv_cache_fill(const float* k, const float* v, int64_t ld_src, const gnnlm_kv_cache_t& c, int layer, const gnnlm_ragged_t& rg,
                  int max_rows, hipStream_t stream) {
    if (rg.n_tok == 0) return OK;
    FillParams p{k, v, ld_src, c.k + layer * c.ld_layer, c.v + layer * c.ld_layer, c.ld_row, c.ld_seq, rg.block_off, rg.n_blocks, rg.n_tok,
                 c.d / 4, max_rows};
    ProfScope prof(K_MISC, stream, 0.0, 16.0 * rg.n_tok * c.d);
    hipLaunchKernelGGL(kv_cache_fill_kernel, dim3((unsigned)cdiv(rg.n_tok, 4)), dim3(256), 0, stream, p);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int kv_len_set(const gnnlm_kv_cache_t& c, const int32_t* block_off, int max_rows, hipStream_t stream) {
    if (c.B == 0) return OK;
    hipLaunchKernelGGL(kv_len_set_kernel, dim3((unsigned)cdiv(c.B, 256)), dim3(256), 0, stream, c.len, block_off, c.B, max_rows);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int kv_len_advance(const gnnlm_kv_cache_t& c, int bound, hipStream_t stream) {
    if (c.B == 0) return OK;
    hipLaunchKernelGGL(kv_len_advance_kernel, dim3((unsigned)cdiv(c.B, 256)), dim3(256), 0, stream, c.len, c.done, c.B, bound);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm

using namespace gnnlm;

extern "C" {

size_t gnnlm_decode_attn_workspace_bytes(int32_t B, int32_t H, int32_t dk, int32_t max_len) {
    return decode_attn_workspace_bytes(B, H, dk, max_len);
}
int gnnlm_decode_attn(const gnnlm_decode_attn_t* d, void* stream) {
    GNNLM_DESC(d);
    return decode_attn(*d, nullptr, (hipStream_t)stream);
}
int gnnlm_beam_attn(const gnnlm_beam_attn_t* d, void* stream) {
    GNNLM_DESC(d);
    const SlotTable tab{d->src, d->ld_src};
    return decode_attn(d->a, &tab, (hipStream_t)stream);
}

}  // extern "C"
