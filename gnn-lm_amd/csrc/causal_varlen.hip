// Causal ('tgt','intra','tgt') attention over PACKED blocks of unequal length (--sample-break-mode eos / complete /
// complete_doc: a batch is a run of sentences, not n_blocks x T).  Replaces fn.v_dot_u + edge_softmax + u_mul_e/sum of
// hgt.py:354-356,383-385 on the disjoint union dgl.batch makes of the samples' graphs (monolingual_dataset.py:261).
//
// A work item is (block, head, tile of 32 queries), looked up in a tile table the host derives from the block lengths
// (ragged_tiles: heaviest tiles first, so one long block beside a thousand short ones does not become the tail of the launch);
// one wave per item, four independent items per workgroup.  Layout as in the 256 x 128 kernel (causal_attn.hip): scores as
// S^T = K' Q^T with v_mfma_f32_32x32x2_f32, so accumulator rows are KEYS and lane & 31 is the query -- a query's 32 scores of a
// key tile sit in two lanes, the mask and the softmax are in-lane plus one v_permlane32_swap.  What is new is the running
// maximum / sum over key tiles (a block of 3000 tokens has 94 of them; nothing but one tile of scores is ever live) and the
// product: out^T = V'^T P^T, whose B operand is the probability register as it lies (k pair = the two halves' keys) and whose
// accumulator columns are again the QUERIES -- so the rescale by exp(m_old - m_new) is in-lane too, and a lane ends up with
// runs of 4 consecutive output columns of its own query (float4 stores).  K' and V' rows are read from global memory in the
// operand layout (a K' row by its own lane in 16-byte pieces, a V' row by 32 lanes side by side): a tile's 32 rows are shared
// by nobody but the heads' sibling waves, so there is nothing for LDS to share.
//
// Rows outside a block are never read for a result: key / query rows past the block's end are clamped to its last row and
// masked, and a table entry that does not describe rows of [0, n_tok) is skipped.
#include "common.h"
#include "kernels.h"

#include <algorithm>
#include <vector>

namespace gnnlm {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct VarlenParams {
    const float* Q; const float* K; const float* V; float* out;
    int64_t ld, ldo, n_tok;
    const int32_t* block_off; const int32_t* tiles;
    int n_blocks, n_tiles, H, max_ctx, accumulate;
};

template <int DK>
__global__ __launch_bounds__(256) void causal_attn_varlen_kernel(VarlenParams p) {
    constexpr int NS = DK / 8;                    // 16-byte steps of a lane through its K' / Q row (k = 8 s + 4 half + e)
    constexpr int NC = (DK + 31) / 32;            // 32-column chunks of V' / out
    const int lane = threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= (int64_t)p.n_tiles * p.H) return;
    const int tile = (int)(item / p.H), h = (int)(item % p.H);
    const int blk = p.tiles[2 * tile], qt = p.tiles[2 * tile + 1];
    if (blk < 0 || blk >= p.n_blocks || qt < 0) return;
    const int64_t base = p.block_off[0];
    const int64_t r0 = p.block_off[blk] - base, r1 = p.block_off[blk + 1] - base;
    if (r0 < 0 || r1 > p.n_tok || r1 <= r0) return;
    const int len = (int)(r1 - r0), q0 = 32 * qt;
    if (q0 >= len) return;
    const int q = q0 + l32, last = len - 1;
    const float* Qb = p.Q + r0 * p.ld + h * DK;
    const float* Kb = p.K + r0 * p.ld + h * DK;
    const float* Vb = p.V + r0 * p.ld + h * DK;

    float4 qreg[NS];
    {
        const float* qr = Qb + (int64_t)min(q, last) * p.ld + 4 * half;
#pragma unroll
        for (int s_ = 0; s_ < NS; ++s_) qreg[s_] = *reinterpret_cast<const float4*>(qr + 8 * s_);
    }
    f32x16 oc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) oc[c][r] = 0.f;
    float m = -INFINITY, lsum = 0.f;              // running maximum (both lanes of a query agree) and this lane's share of the sum
    const bool vcol = DK >= 32 || l32 < DK;

    const int kt_lo = p.max_ctx > 0 ? max(0, q0 - p.max_ctx + 1) / 32 : 0;
    for (int kt = kt_lo; kt <= qt; ++kt) {
        const int k0 = 32 * kt;
        f32x16 sc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[r] = 0.f;
        {
            const float* kr = Kb + (int64_t)min(k0 + l32, last) * p.ld + 4 * half;
#pragma unroll
            for (int s_ = 0; s_ < NS; ++s_) {
                const float4 a = *reinterpret_cast<const float4*>(kr + 8 * s_);
                sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qreg[s_].x, sc, 0, 0, 0);
                sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qreg[s_].y, sc, 0, 0, 0);
                sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qreg[s_].z, sc, 0, 0, 0);
                sc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qreg[s_].w, sc, 0, 0, 0);
            }
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            const bool ok = key <= q && key < len && (p.max_ctx <= 0 || q - key < p.max_ctx);
            sc[r] = ok ? sc[r] : -INFINITY;
            tmax = fmaxf(tmax, sc[r]);
        }
        {
            const gnnlm_u32x2 x = __builtin_amdgcn_permlane32_swap(__float_as_uint(tmax), __float_as_uint(tmax), false, false);
            tmax = fmaxf(__uint_as_float(x.x), __uint_as_float(x.y));
        }
        const float m_new = fmaxf(m, tmax);
        const float alpha = m == -INFINITY ? 0.f : expf(m - m_new);     // (nothing seen so far: sum and accumulators are zero)
        float tsum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = sc[r] == -INFINITY ? 0.f : expf(sc[r] - m_new);
            sc[r] = e;
            tsum += e;
        }
        lsum = lsum * alpha + tsum;
        m = m_new;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int r = 0; r < 16; ++r) oc[c][r] *= alpha;
        // out^T[col][query] += V'^T[col][key] P^T[key][query]: A = V'[key(r, half)][32 c + l32], B = the probability register
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* vr = Vb + (int64_t)min(k0 + (r & 3) + 8 * (r >> 2) + 4 * half, last) * p.ld + l32;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const float v = vcol ? vr[32 * c] : 0.f;
                oc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(v, sc[r], oc[c], 0, 0, 0);
            }
        }
    }
    {
        const gnnlm_u32x2 x = __builtin_amdgcn_permlane32_swap(__float_as_uint(lsum), __float_as_uint(lsum), false, false);
        lsum = __uint_as_float(x.x) + __uint_as_float(x.y);
    }
    if (q >= len) return;
    const float inv = 1.f / lsum;                 // the diagonal key is always valid: the sum is positive
    float* ob = p.out + (r0 + q) * p.ldo + h * DK + 4 * half;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int col = 32 * c + 8 * g;       // + 4 half + 0..3: accumulator registers 4 g .. 4 g + 3
            if (col + 4 * half >= DK) continue;
            float4 o = make_float4(oc[c][4 * g] * inv, oc[c][4 * g + 1] * inv, oc[c][4 * g + 2] * inv, oc[c][4 * g + 3] * inv);
            float4* dst = reinterpret_cast<float4*>(ob + col);
            if (p.accumulate) {
                const float4 t = *dst;
                o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
            }
            *dst = o;
        }
}

}  // namespace

int64_t ragged_tiles(const int32_t* block_off, int n_blocks, int32_t* tiles) {
    if (!block_off || n_blocks < 0) return -1;
    int64_t n = 0;
    for (int b = 0; b < n_blocks; ++b) {
        const int64_t len = (int64_t)block_off[b + 1] - block_off[b];
        if (len < 1) return -1;
        n += (len + 31) / 32;
    }
    if (!tiles) return n;
    std::vector<std::pair<int32_t, int32_t>> t;
    t.reserve((size_t)n);
    for (int b = 0; b < n_blocks; ++b)
        for (int32_t qt = 0; qt < (block_off[b + 1] - block_off[b] + 31) / 32; ++qt) t.emplace_back(b, qt);
    // a tile's work is its number of key tiles, qt + 1: heaviest first, blocks in order among equals
    std::stable_sort(t.begin(), t.end(), [](const std::pair<int32_t, int32_t>& a, const std::pair<int32_t, int32_t>& b) { return a.second > b.second; });
    for (int64_t i = 0; i < n; ++i) { tiles[2 * i] = t[(size_t)i].first; tiles[2 * i + 1] = t[(size_t)i].second; }
    return n;
}

bool causal_attn_varlen_ok(int dk) { return dk == 16 || dk == 32 || dk == 64 || dk == 128; }

int causal_attn_varlen(const float* Q, const float* K, const float* V, int64_t ld, float* out, int64_t ldo, const gnnlm_ragged_t& rg,
                       int H, int dk, int max_ctx, hipStream_t stream, bool accumulate) {
    GNNLM_REQUIRE(Q && K && V && out, "causal_attn_varlen: null operand");
    GNNLM_REQUIRE(causal_attn_varlen_ok(dk), "causal_attn_varlen: d_k must be 16, 32, 64 or 128");
    GNNLM_REQUIRE(H > 0 && rg.n_blocks >= 0 && rg.n_tiles >= 0 && rg.n_tok >= 0 && rg.n_tok < (1ll << 31), "causal_attn_varlen: bad shape");
    GNNLM_REQUIRE(ld % 4 == 0 && ldo % 4 == 0 && ld >= (int64_t)H * dk && ldo >= (int64_t)H * dk, "causal_attn_varlen: row strides must be multiples of 4 and >= H * d_k");
    GNNLM_REQUIRE(((uintptr_t)Q % 16 == 0) && ((uintptr_t)K % 16 == 0) && ((uintptr_t)V % 16 == 0) && ((uintptr_t)out % 16 == 0),
                  "causal_attn_varlen: operands must be 16-byte aligned");
    if (rg.n_blocks == 0 || rg.n_tok == 0) return OK;
    GNNLM_REQUIRE(rg.block_off && rg.tiles, "causal_attn_varlen: block_off / tiles missing (see gnnlm_ragged_tiles)");
    // every block has at least one token and at most 31 rows of its last tile are empty
    GNNLM_REQUIRE(rg.n_blocks <= rg.n_tok && rg.n_tiles >= rg.n_blocks && (int64_t)rg.n_tiles <= rg.n_tok / 32 + rg.n_blocks,
                  "causal_attn_varlen: the tile count does not fit n_blocks blocks of n_tok tokens");
    VarlenParams p{Q, K, V, out, ld, ldo, rg.n_tok, rg.block_off, rg.tiles, rg.n_blocks, rg.n_tiles, H, max_ctx, accumulate ? 1 : 0};
    const int64_t items = (int64_t)rg.n_tiles * H;
    // algorithmic upper estimate: every tile against its key tiles as if all blocks were one (the lengths live on the device)
    ProfScope prof(K_CAUSAL, stream, 4.0 * 32 * 32 * dk * items, 16.0 * rg.n_tok * H * dk);
    const dim3 grid((unsigned)cdiv(items, 4)), block(256);
    switch (dk) {
        case 16: hipLaunchKernelGGL(causal_attn_varlen_kernel<16>, grid, block, 0, stream, p); break;
        case 32: hipLaunchKernelGGL(causal_attn_varlen_kernel<32>, grid, block, 0, stream, p); break;
        case 64: hipLaunchKernelGGL(causal_attn_varlen_kernel<64>, grid, block, 0, stream, p); break;
        default: hipLaunchKernelGGL(causal_attn_varlen_kernel<128>, grid, block, 0, stream, p); break;
    }
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
