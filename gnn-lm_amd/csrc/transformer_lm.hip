// Base transformer LM (include/gnnlm.h: gnnlm_lm_embed, gnnlm_relu, gnnlm_transformer_lm_forward): the decoder-only, pre-norm
// language model of fairseq's transformer_lm in eval mode -- TransformerDecoder.extract_features (fairseq/models/transformer.py:
// 700-841) over TransformerDecoderLayer.forward (fairseq/modules/transformer_layer.py:223-331) -- on PACKED blocks.
//
// New device code: two row kernels.  Everything heavy is an entry point the library already has (gemm_nt with bias / residual,
// causal_attn_varlen, layernorm, gelu); the orchestrator only enqueues them on the caller's stream.
#include "host.h"

namespace gnnlm {
namespace {

struct EmbedParams {
    const int64_t* tokens;
    const float* E; int64_t ld_e; int n_vocab, d4;
    const float* P; int64_t ld_p, p_rows; int pad_idx;
    float scale;
    float* out; int64_t ldo;
    const int32_t* block_off; int n_blocks; int64_t n_tok;
    int32_t* n_bad;
};

// One wave per packed row.  The row's block is found by bisection of the (wave-uniform) offset table; only differences of
// block_off are read, as everywhere (gnnlm_ragged_t).  Two roundings per element: __fmul_rn / __fadd_rn are never contracted.
__global__ __launch_bounds__(256) void lm_embed_kernel(EmbedParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.n_tok) return;
    float4* o = reinterpret_cast<float4*>(p.out + r * p.ldo);
    const int64_t tok = p.tokens[r];
    bool ok = tok >= 0 && tok < p.n_vocab;
    const float4* pr = nullptr;
    if (p.P) {
        const int64_t base = p.block_off[0];
        int lo = 0, hi = p.n_blocks;                       // the last b with block_off[b] - base <= r
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)p.block_off[mid] - base <= r) lo = mid; else hi = mid;
        }
        const int64_t pos = (int64_t)p.pad_idx + 1 + (r - ((int64_t)p.block_off[lo] - base));
        ok = ok && pos >= 0 && pos < p.p_rows;             // (the host refused a block longer than the table: memory safety only)
        pr = reinterpret_cast<const float4*>(p.P + (ok ? pos : 0) * p.ld_p);
    }
    if (!ok) {
        for (int e = lane; e < p.d4; e += 64) o[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane == 0 && p.n_bad) atomicAdd(p.n_bad, 1);
        return;
    }
    const float4* er = reinterpret_cast<const float4*>(p.E + tok * p.ld_e);
    const float s = p.scale;
    for (int e = lane; e < p.d4; e += 64) {
        const float4 v = er[e];
        float4 x = make_float4(__fmul_rn(s, v.x), __fmul_rn(s, v.y), __fmul_rn(s, v.z), __fmul_rn(s, v.w));
        if (pr) {
            const float4 q = pr[e];
            x = make_float4(__fadd_rn(x.x, q.x), __fadd_rn(x.y, q.y), __fadd_rn(x.z, q.z), __fadd_rn(x.w, q.w));
        }
        o[e] = x;
    }
}

struct StepEmbedParams {
    const int64_t* tokens;
    const float* E; int64_t ld_e; int n_vocab, d4;
    const float* P; int64_t ld_p, p_rows; int pad_idx;
    float scale;
    float* out; int64_t ldo;
    const int32_t* len; int B, cap;
    int32_t* n_bad;
};

// lm_embed_kernel for a decoding step: one wave per sequence, the position is pad_idx + 1 + len[b], read here.  The same two
// roundings, the same zero row and count for an id outside the vocabulary -- and for a len[b] the cache cannot hold.
__global__ __launch_bounds__(256) void lm_embed_step_kernel(StepEmbedParams p) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= p.B) return;
    float4* o = reinterpret_cast<float4*>(p.out + b * p.ldo);
    const int64_t tok = p.tokens[b];
    const int len = p.len[b];
    bool ok = tok >= 0 && tok < p.n_vocab && len >= 0 && len < p.cap;
    const float4* pr = nullptr;
    if (p.P) {
        const int64_t pos = (int64_t)p.pad_idx + 1 + len;
        ok = ok && pos < p.p_rows;                          // (the host refused a max_len beyond the table: memory safety only)
        pr = reinterpret_cast<const float4*>(p.P + (ok ? pos : 0) * p.ld_p);
    }
    if (!ok) {
        for (int e = lane; e < p.d4; e += 64) o[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane == 0 && p.n_bad) atomicAdd(p.n_bad, 1);
        return;
    }
    const float4* er = reinterpret_cast<const float4*>(p.E + tok * p.ld_e);
    const float s = p.scale;
    for (int e = lane; e < p.d4; e += 64) {
        const float4 v = er[e];
        float4 x = make_float4(__fmul_rn(s, v.x), __fmul_rn(s, v.y), __fmul_rn(s, v.z), __fmul_rn(s, v.w));
        if (pr) {
            const float4 q = pr[e];
            x = make_float4(__fadd_rn(x.x, q.x), __fadd_rn(x.y, q.y), __fadd_rn(x.z, q.z), __fadd_rn(x.w, q.w));
        }
        o[e] = x;
    }
}

// v < 0 ? 0 : v keeps a NaN (both comparisons false), as torch.relu; fmaxf would drop it
__device__ __forceinline__ float relu1(float v) { return v < 0.f ? 0.f : v; }
__global__ __launch_bounds__(256) void relu4_kernel(float4* x, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) {
        const float4 v = x[i];
        x[i] = make_float4(relu1(v.x), relu1(v.y), relu1(v.z), relu1(v.w));
    }
}
__global__ __launch_bounds__(256) void relu1_kernel(float* x, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = relu1(x[i]);
}

int check_embed(const gnnlm_lm_embed_t& e, const gnnlm_ragged_t& rg) {
    GNNLM_REQUIRE(rg.n_tok >= 0 && rg.n_tok < (1ll << 31) && rg.n_blocks >= 0, "lm_embed: bad block table");
    GNNLM_REQUIRE(e.d > 0 && e.d % 4 == 0, "lm_embed: d % 4 != 0");
    GNNLM_REQUIRE(e.n_vocab > 0, "lm_embed: empty vocabulary");
    GNNLM_REQUIRE(e.E && e.ld_e >= e.d && e.ld_e % 4 == 0 && (uintptr_t)e.E % 16 == 0, "lm_embed: E must be [n_vocab, d], 16-byte aligned, ld_e % 4 == 0");
    GNNLM_REQUIRE(e.ldo >= e.d && e.ldo % 4 == 0, "lm_embed: ldo must be a multiple of 4 and >= d");
    if (e.P) {
        GNNLM_REQUIRE(e.ld_p >= e.d && e.ld_p % 4 == 0 && (uintptr_t)e.P % 16 == 0, "lm_embed: P must be [p_rows, d], 16-byte aligned, ld_p % 4 == 0");
        GNNLM_REQUIRE(e.pad_idx >= 0 && e.max_len >= 0, "lm_embed: bad pad_idx / max_len");
        GNNLM_REQUIRE((int64_t)e.pad_idx + 1 + e.max_len <= e.p_rows,
                      "lm_embed: a block is longer than the position table holds (pad_idx + 1 + max_len > p_rows)");
    }
    if (rg.n_tok == 0) return OK;
    GNNLM_REQUIRE(e.tokens && e.out && (uintptr_t)e.out % 16 == 0, "lm_embed: tokens / out missing or out not 16-byte aligned");
    GNNLM_REQUIRE(!e.P || (rg.block_off && rg.n_blocks >= 1 && rg.n_blocks <= rg.n_tok), "lm_embed: positions need block_off with 1 .. n_tok blocks");
    return OK;
}

int launch_embed(const gnnlm_lm_embed_t& e, const gnnlm_ragged_t& rg, hipStream_t stream) {
    if (rg.n_tok == 0) return OK;
    EmbedParams p{e.tokens, e.E, e.ld_e, e.n_vocab, e.d / 4, e.P, e.ld_p, e.p_rows, e.pad_idx, e.scale, e.out, e.ldo,
                  rg.block_off, rg.n_blocks, rg.n_tok, e.n_bad};
    ProfScope prof(K_MISC, stream, (e.P ? 2.0 : 1.0) * rg.n_tok * e.d, (e.P ? 12.0 : 8.0) * rg.n_tok * e.d + 8.0 * rg.n_tok);
    hipLaunchKernelGGL(lm_embed_kernel, dim3((unsigned)cdiv(rg.n_tok, 4)), dim3(256), 0, stream, p);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

struct TlmBufs { float *x, *h, *a, *wide; };
void take_tlm(const gnnlm_tlm_t& m, int64_t n, Carver& c, TlmBufs& b) {
    b.x = c.take<float>(n * m.d);
    b.h = c.take<float>(n * m.d);
    b.a = c.take<float>(n * m.d);
    b.wide = c.take<float>(n * std::max<int64_t>(3 * (int64_t)m.d, m.ffn));      // q | k | v of the attention block, then the fc1 output
}
size_t carve_tlm(const gnnlm_tlm_t& m, int64_t n, char* base, TlmBufs& b) {
    Carver c(base);
    take_tlm(m, n, c, b);
    return c.off + 256;
}

int check_tlm(const gnnlm_tlm_t& m) {
    GNNLM_REQUIRE(m.L >= 1 && m.layers, "transformer_lm: needs L >= 1 layers");
    GNNLM_REQUIRE(m.d > 0 && m.d % 4 == 0, "transformer_lm: d % 4 != 0");
    GNNLM_REQUIRE(m.ffn > 0 && m.ffn % 4 == 0, "transformer_lm: ffn % 4 != 0");
    GNNLM_REQUIRE(m.H > 0 && m.d % m.H == 0 && causal_attn_varlen_ok(m.d / m.H), "transformer_lm: d_k = d / H must be 16, 32, 64 or 128 with H * d_k == d");
    GNNLM_REQUIRE(m.act == 0 || m.act == 1, "transformer_lm: act must be 0 (relu) or 1 (gelu)");
    GNNLM_REQUIRE(m.precision >= 0 && m.precision <= 3, "transformer_lm: precision must be 0 .. 3");
    GNNLM_REQUIRE(m.ln_eps >= 0.f, "transformer_lm: ln_eps < 0");
    GNNLM_REQUIRE(!m.ln_emb_g == !m.ln_emb_b && !m.ln_out_g == !m.ln_out_b, "transformer_lm: a LayerNorm needs both its weight and its bias");
    for (int l = 0; l < m.L; ++l) {
        const gnnlm_tlm_layer_t& w = m.layers[l];
        GNNLM_REQUIRE(w.ln1_g && w.ln1_b && w.wqkv && w.bqkv && w.wo && w.bo && w.ln2_g && w.ln2_b && w.w1 && w.b1 && w.w2 && w.b2,
                      "transformer_lm: a layer member is NULL");
    }
    return OK;
}

gnnlm_lm_embed_t embed_of(const gnnlm_tlm_t& m, const gnnlm_tlm_io_t& io, float* out) {
    gnnlm_lm_embed_t e{};
    e.tokens = io.tokens;
    e.E = m.E; e.ld_e = m.ld_e; e.n_vocab = m.n_vocab; e.d = m.d;
    e.P = m.P; e.ld_p = m.ld_p; e.p_rows = m.p_rows; e.pad_idx = m.pad_idx;
    e.scale = m.scale; e.max_len = io.max_len;
    e.out = out; e.ldo = m.d; e.n_bad = io.n_bad;
    return e;
}

int check_tlm_cache(const gnnlm_tlm_t& m, const gnnlm_kv_cache_t& c) {
    GNNLM_TRY(check_kv_cache(c));
    GNNLM_REQUIRE(c.d == m.d && c.L == m.L, "transformer_lm: the cache's d / L differ from the model's");
    return OK;
}

// cache != nullptr (gnnlm_transformer_lm_prefill): block b is sequence b, its K' / V' rows are copied into the cache after each
// layer's q|k|v GEMM and len is set at the end; the launches of the forward itself are the same either way
int tlm_forward(const gnnlm_tlm_t& m, const gnnlm_tlm_io_t& io, void* ws, size_t ws_bytes, hipStream_t s, const gnnlm_kv_cache_t* cache = nullptr) {
    GNNLM_TRY(check_tlm(m));
    const gnnlm_ragged_t& rg = io.blocks;
    if (cache) {
        GNNLM_TRY(check_tlm_cache(m, *cache));
        GNNLM_REQUIRE(rg.n_blocks == cache->B, "transformer_lm_prefill: n_blocks != the cache's B");
        GNNLM_REQUIRE(io.max_len >= 0 && io.max_len <= cache->cap, "transformer_lm_prefill: a block is longer than the cache (max_len > cap)");
    }
    const int64_t n = rg.n_tok;
    const int d = m.d, dk = m.d / m.H;
    const float eps = m.ln_eps == 0.f ? 1e-5f : m.ln_eps;
    {
        const gnnlm_lm_embed_t probe = embed_of(m, io, reinterpret_cast<float*>(ws));
        GNNLM_TRY(check_embed(probe, rg));
    }
    if (n == 0) return OK;
    GNNLM_REQUIRE(io.tokens && io.out, "transformer_lm: tokens / out missing");
    GNNLM_REQUIRE(((uintptr_t)io.out | (uintptr_t)io.last_inner | (uintptr_t)io.last_ffn_input) % 16 == 0, "transformer_lm: outputs must be 16-byte aligned");
    GNNLM_REQUIRE(rg.block_off && rg.tiles && rg.n_blocks >= 1 && rg.n_blocks <= n && rg.n_tiles >= rg.n_blocks &&
                  (int64_t)rg.n_tiles <= n / 32 + rg.n_blocks, "transformer_lm: block_off / tiles missing or inconsistent (see gnnlm_ragged_tiles)");
    TlmBufs b;
    GNNLM_REQUIRE(ws && (uintptr_t)ws % 16 == 0 && carve_tlm(m, n, nullptr, b) <= ws_bytes, "transformer_lm: workspace missing, misaligned or too small");
    carve_tlm(m, n, reinterpret_cast<char*>(ws), b);
    GemmPrecisionScope prec_scope(m.precision);

    GNNLM_TRY(launch_embed(embed_of(m, io, b.x), rg, s));
    if (m.ln_emb_g) GNNLM_TRY(layernorm(b.x, d, m.ln_emb_g, m.ln_emb_b, b.x, d, n, d, eps, nullptr, s));
    for (int l = 0; l < m.L; ++l) {
        const gnnlm_tlm_layer_t& w = m.layers[l];
        const bool last = l == m.L - 1;
        // self-attention block: x += out_proj(attn(LN(x)))
        GNNLM_TRY(layernorm(b.x, d, w.ln1_g, w.ln1_b, b.h, d, n, d, eps, nullptr, s));
        GNNLM_TRY(linear(b.h, d, w.wqkv, w.bqkv, b.wide, n, 3 * d, d, nullptr, ALPHA_UNSET, s));
        if (cache) GNNLM_TRY(kv_cache_fill(b.wide, 3 * (int64_t)d, *cache, l, rg, (int)io.max_len, s));
        GNNLM_TRY(causal_attn_varlen(b.wide, b.wide + d, b.wide + 2 * d, 3 * (int64_t)d, b.a, d, rg, m.H, dk, 0, s));
        GNNLM_TRY(linear(b.a, d, w.wo, w.bo, b.x, n, d, d, b.x, ALPHA_UNSET, s));
        // feed-forward block: x += fc2(act(fc1(LN(x))))
        float* h2 = last && io.last_ffn_input ? io.last_ffn_input : b.h;
        GNNLM_TRY(layernorm(b.x, d, w.ln2_g, w.ln2_b, h2, d, n, d, eps, nullptr, s));
        GNNLM_TRY(linear(h2, d, w.w1, w.b1, b.wide, n, m.ffn, d, nullptr, ALPHA_UNSET, s));
        GNNLM_TRY(m.act == 0 ? relu(b.wide, n * m.ffn, s) : gelu(b.wide, n * m.ffn, s));
        // the last layer's residual sum is inner_states[-1]: it lands where it is wanted
        float* dst = !last ? b.x : (io.last_inner ? io.last_inner : (m.ln_out_g ? b.x : io.out));
        GNNLM_TRY(linear(b.wide, m.ffn, w.w2, w.b2, dst, n, d, m.ffn, b.x, ALPHA_UNSET, s));
        if (last) {
            if (m.ln_out_g) GNNLM_TRY(layernorm(dst, d, m.ln_out_g, m.ln_out_b, io.out, d, n, d, eps, nullptr, s));
            else if (dst != io.out) GNNLM_HIP(hipMemcpyAsync(io.out, dst, (size_t)n * d * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    if (cache) GNNLM_TRY(kv_len_set(*cache, rg.block_off, (int)io.max_len, s));
    return OK;
}

size_t carve_step(const gnnlm_tlm_t& m, int B, int max_len, char* base, TlmBufs& b, float** attn_ws, size_t* attn_bytes) {
    Carver c(base);
    take_tlm(m, B, c, b);
    const size_t n = decode_attn_workspace_bytes(B, m.H, m.H > 0 ? m.d / m.H : 0, max_len);
    float* a = reinterpret_cast<float*>(c.take<char>((int64_t)n));
    if (attn_ws) *attn_ws = a;
    if (attn_bytes) *attn_bytes = n;
    return c.off + 256;
}

// beam (gnnlm_transformer_lm_step_beam): every layer's attention reads its cached rows through the table src
int tlm_step(const gnnlm_tlm_t& m, const gnnlm_kv_cache_t& c, const gnnlm_tlm_step_io_t& io, void* ws, size_t ws_bytes, hipStream_t s,
             bool beam = false, const int32_t* src = nullptr, int64_t ld_src = 0) {
    GNNLM_TRY(check_tlm(m));
    GNNLM_TRY(check_tlm_cache(m, c));
    const int B = c.B, d = m.d, dk = m.d / m.H;
    const float eps = m.ln_eps == 0.f ? 1e-5f : m.ln_eps;
    GNNLM_REQUIRE(io.max_len >= 1 && io.max_len <= c.cap, "transformer_lm_step: max_len outside [1, cap] (the cache is full)");
    GNNLM_REQUIRE(m.E && m.ld_e >= d && m.ld_e % 4 == 0 && (uintptr_t)m.E % 16 == 0 && m.n_vocab > 0, "transformer_lm_step: E must be [n_vocab, d], 16-byte aligned, ld_e % 4 == 0");
    if (m.P) {
        GNNLM_REQUIRE(m.ld_p >= d && m.ld_p % 4 == 0 && (uintptr_t)m.P % 16 == 0 && m.pad_idx >= 0, "transformer_lm_step: P must be [p_rows, d], 16-byte aligned, ld_p % 4 == 0");
        GNNLM_REQUIRE((int64_t)m.pad_idx + 1 + io.max_len <= m.p_rows,
                      "transformer_lm_step: the position table does not hold the next position (pad_idx + 1 + max_len > p_rows)");
    }
    if (B == 0) return OK;
    GNNLM_REQUIRE(io.tokens && io.out, "transformer_lm_step: tokens / out missing");
    GNNLM_REQUIRE(((uintptr_t)io.out | (uintptr_t)io.last_inner | (uintptr_t)io.last_ffn_input) % 16 == 0, "transformer_lm_step: outputs must be 16-byte aligned");
    TlmBufs b;
    float* attn_ws = nullptr;
    size_t attn_bytes = 0;
    GNNLM_REQUIRE(ws && (uintptr_t)ws % 16 == 0 && carve_step(m, B, (int)io.max_len, nullptr, b, nullptr, nullptr) <= ws_bytes,
                  "transformer_lm_step: workspace missing, misaligned or too small");
    carve_step(m, B, (int)io.max_len, reinterpret_cast<char*>(ws), b, &attn_ws, &attn_bytes);
    GemmPrecisionScope prec_scope(m.precision);

    {
        StepEmbedParams p{io.tokens, m.E, m.ld_e, m.n_vocab, d / 4, m.P, m.ld_p, m.p_rows, m.pad_idx, m.scale, b.x, d, c.len, B, (int)io.max_len, io.n_bad};
        ProfScope prof(K_MISC, s, (m.P ? 2.0 : 1.0) * B * d, (m.P ? 12.0 : 8.0) * B * d + 12.0 * B);
        hipLaunchKernelGGL(lm_embed_step_kernel, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, s, p);
        GNNLM_LAUNCH_CHECK();
    }
    if (m.ln_emb_g) GNNLM_TRY(layernorm(b.x, d, m.ln_emb_g, m.ln_emb_b, b.x, d, B, d, eps, nullptr, s));
    gnnlm_decode_attn_t a{};
    a.q = b.wide; a.k_new = b.wide + d; a.v_new = b.wide + 2 * d; a.ld = 3 * (int64_t)d;
    a.out = b.a; a.ldo = d;
    a.cache = c; a.H = m.H; a.dk = dk; a.max_len = (int32_t)io.max_len;
    a.workspace = attn_ws; a.workspace_bytes = attn_bytes;
    for (int l = 0; l < m.L; ++l) {
        const gnnlm_tlm_layer_t& w = m.layers[l];
        const bool last = l == m.L - 1;
        GNNLM_TRY(layernorm(b.x, d, w.ln1_g, w.ln1_b, b.h, d, B, d, eps, nullptr, s));
        GNNLM_TRY(linear(b.h, d, w.wqkv, w.bqkv, b.wide, B, 3 * d, d, nullptr, ALPHA_UNSET, s));
        a.layer = l;
        if (l > 0) a.cache.n_bad = nullptr;                 // a row out of range is counted once per step, not once per layer
        GNNLM_TRY(beam ? beam_attn(a, src, ld_src, s) : decode_attn(a, s));
        GNNLM_TRY(linear(b.a, d, w.wo, w.bo, b.x, B, d, d, b.x, ALPHA_UNSET, s));
        float* h2 = last && io.last_ffn_input ? io.last_ffn_input : b.h;
        GNNLM_TRY(layernorm(b.x, d, w.ln2_g, w.ln2_b, h2, d, B, d, eps, nullptr, s));
        GNNLM_TRY(linear(h2, d, w.w1, w.b1, b.wide, B, m.ffn, d, nullptr, ALPHA_UNSET, s));
        GNNLM_TRY(m.act == 0 ? relu(b.wide, (int64_t)B * m.ffn, s) : gelu(b.wide, (int64_t)B * m.ffn, s));
        float* dst = !last ? b.x : (io.last_inner ? io.last_inner : (m.ln_out_g ? b.x : io.out));
        GNNLM_TRY(linear(b.wide, m.ffn, w.w2, w.b2, dst, B, d, m.ffn, b.x, ALPHA_UNSET, s));
        if (last) {
            if (m.ln_out_g) GNNLM_TRY(layernorm(dst, d, m.ln_out_g, m.ln_out_b, io.out, d, B, d, eps, nullptr, s));
            else if (dst != io.out) GNNLM_HIP(hipMemcpyAsync(io.out, dst, (size_t)B * d * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    GNNLM_TRY(kv_len_advance(c, (int)io.max_len, s));
    return OK;
}

}  // namespace

int relu(float* x, int64_t n, hipStream_t stream) {
    GNNLM_REQUIRE(n >= 0, "relu: bad size");
    if (n == 0) return OK;
    GNNLM_REQUIRE(x && (uintptr_t)x % 4 == 0, "relu: null or misaligned");
    ProfScope prof(K_MISC, stream, 0.0, 8.0 * n);
    if ((uintptr_t)x % 16 == 0 && n % 4 == 0) {
        GNNLM_REQUIRE(cdiv(n / 4, 256) < (1ll << 31), "relu: too many elements for one launch");
        hipLaunchKernelGGL(relu4_kernel, dim3((unsigned)cdiv(n / 4, 256)), dim3(256), 0, stream, reinterpret_cast<float4*>(x), n / 4);
    } else {
        GNNLM_REQUIRE(cdiv(n, 256) < (1ll << 31), "relu: too many elements for one launch");
        hipLaunchKernelGGL(relu1_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, x, n);
    }
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm

using namespace gnnlm;

extern "C" {

int gnnlm_lm_embed(const gnnlm_lm_embed_t* desc, const gnnlm_ragged_t* blocks, void* stream) {
    GNNLM_DESC(desc);
    GNNLM_DESC(blocks);
    const int rc = check_embed(*desc, *blocks);
    return rc != OK ? rc : launch_embed(*desc, *blocks, (hipStream_t)stream);
}
int gnnlm_relu(float* x, int64_t n, void* stream) { return relu(x, n, (hipStream_t)stream); }
size_t gnnlm_transformer_lm_workspace_bytes(const gnnlm_tlm_t* m, const gnnlm_tlm_io_t* io) {
    if (!m || !io || m->d <= 0 || m->ffn <= 0 || io->blocks.n_tok < 0) return 0;
    TlmBufs b;
    return carve_tlm(*m, io->blocks.n_tok, nullptr, b);
}
int gnnlm_transformer_lm_forward(const gnnlm_tlm_t* m, const gnnlm_tlm_io_t* io, void* workspace, size_t workspace_bytes, void* stream) {
    GNNLM_DESC(m);
    GNNLM_DESC(io);
    return tlm_forward(*m, *io, workspace, workspace_bytes, (hipStream_t)stream);
}
int gnnlm_transformer_lm_prefill(const gnnlm_tlm_t* m, const gnnlm_tlm_io_t* io, const gnnlm_kv_cache_t* cache, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    GNNLM_DESC(m);
    GNNLM_DESC(io);
    GNNLM_DESC(cache);
    return tlm_forward(*m, *io, workspace, workspace_bytes, (hipStream_t)stream, cache);
}
size_t gnnlm_transformer_lm_step_workspace_bytes(const gnnlm_tlm_t* m, const gnnlm_kv_cache_t* c, const gnnlm_tlm_step_io_t* io) {
    if (!m || !c || !io || m->d <= 0 || m->ffn <= 0 || m->H <= 0 || c->B < 0 || io->max_len < 0 || io->max_len > c->cap) return 0;
    TlmBufs b;
    return carve_step(*m, c->B, (int)io->max_len, nullptr, b, nullptr, nullptr);
}
int gnnlm_transformer_lm_step(const gnnlm_tlm_t* m, const gnnlm_kv_cache_t* c, const gnnlm_tlm_step_io_t* io, void* workspace,
                              size_t workspace_bytes, void* stream) {
    GNNLM_DESC(m);
    GNNLM_DESC(c);
    GNNLM_DESC(io);
    return tlm_step(*m, *c, *io, workspace, workspace_bytes, (hipStream_t)stream);
}
int gnnlm_transformer_lm_step_beam(const gnnlm_tlm_t* m, const gnnlm_kv_cache_t* c, const gnnlm_tlm_step_io_t* io, const int32_t* src,
                                   int64_t ld_src, void* workspace, size_t workspace_bytes, void* stream) {
    GNNLM_DESC(m);
    GNNLM_DESC(c);
    GNNLM_DESC(io);
    return tlm_step(*m, *c, *io, workspace, workspace_bytes, (hipStream_t)stream, true, src, ld_src);
}

}  // extern "C"
