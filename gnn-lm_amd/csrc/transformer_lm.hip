// Base transformer LM (include/gnnlm.h: gnnlm_lm_embed, gnnlm_relu, gnnlm_transformer_lm_forward): the decoder-only, pre-norm
// language model of fairseq's transformer_lm in eval mode -- TransformerDecoder.extract_features (fairseq/models/transformer.py:
// 700-841) over TransformerDecoderLayer.forward (fairseq/modules/transformer_layer.py:223-331) -- on PACKED blocks.
//
// New device code: two row kernels.  Everything heavy is an entry point the library already has (gemm_nt with bias / residual,
// causal_attn_varlen, layernorm, gelu); the orchestrator only enqueues them on the caller's stream.  The forward (prefill) and the
// decoding step are ONE layer loop (tlm_layers) over n rows; they differ in their checks, their embed launch and the attention stage.
#include "host.h"

namespace gnnlm {
namespace {

struct EmbedParams {
    const int64_t* tokens;
    const float* E; int64_t ld_e; int n_vocab, d4;
    const float* P; int64_t ld_p, p_rows; int pad_idx;
    float scale;
    float* out; int64_t ldo;
    const int32_t* block_off; int n_blocks;                // lm_embed_kernel only: a row's position is its place in its block
    int64_t n;                                             // rows: packed tokens, or the sequences of a step
    int32_t* n_bad;
    const int32_t* len; int cap;                           // lm_embed_step_kernel only: sequence b stands at len[b], in [0, cap)
};

// One wave writes row r, the token at place at() of its sequence: scale * E[tok] (+ P[pad_idx + 1 + at()]); at is asked only when
// there is a table.  Two roundings per element: __fmul_rn / __fadd_rn are never contracted.  !ok, an id outside the vocabulary or a
// position outside the table: a zero row, counted.
template <class At>
__device__ __forceinline__ void embed_row(const EmbedParams& p, int64_t r, bool ok, At at) {
    const int lane = threadIdx.x & 63;
    float4* o = reinterpret_cast<float4*>(p.out + r * p.ldo);
    const int64_t tok = p.tokens[r];
    ok = ok && tok >= 0 && tok < p.n_vocab;
    const float4* pr = nullptr;
    if (p.P) {
        const int64_t pos = (int64_t)p.pad_idx + 1 + at();
        ok = ok && pos >= 0 && pos < p.p_rows;             // (the host refused a sequence longer than the table: memory safety only)
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

// One wave per packed row.  The row's block is found by bisection of the (wave-uniform) offset table; only differences of
// block_off are read, as everywhere (gnnlm_ragged_t).
__global__ __launch_bounds__(256) void lm_embed_kernel(EmbedParams p) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.n) return;
    embed_row(p, r, true, [&] {
        const int64_t base = p.block_off[0];
        return r - ((int64_t)p.block_off[last_block(p.block_off, p.n_blocks, r, base)] - base);
    });
}

// lm_embed_kernel for a decoding step: one wave per sequence, which stands at len[b], read here.  A len[b] the cache cannot hold is a
// zero row and counted, as an id outside the vocabulary is.
__global__ __launch_bounds__(256) void lm_embed_step_kernel(EmbedParams p) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= p.n) return;
    const int len = p.len[b];
    embed_row(p, b, len >= 0 && len < p.cap, [&] { return (int64_t)len; });
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

// The E / P tables of an embed over sequences of up to e.max_len tokens; `who` is the caller's prefix, `full` its words for a
// position table that is too short.  (ldo is the caller's own in gnnlm_lm_embed only; the orchestrators pass d.)
int check_tables(const gnnlm_lm_embed_t& e, const char* who, const char* full) {
    const std::string w(who);
    GNNLM_REQUIRE(e.E && e.ld_e >= e.d && e.ld_e % 4 == 0 && (uintptr_t)e.E % 16 == 0 && e.n_vocab > 0, w + ": E must be [n_vocab, d], 16-byte aligned, ld_e % 4 == 0");
    GNNLM_REQUIRE(e.ldo >= e.d && e.ldo % 4 == 0, w + ": ldo must be a multiple of 4 and >= d");
    if (e.P) {
        GNNLM_REQUIRE(e.ld_p >= e.d && e.ld_p % 4 == 0 && (uintptr_t)e.P % 16 == 0, w + ": P must be [p_rows, d], 16-byte aligned, ld_p % 4 == 0");
        GNNLM_REQUIRE(e.pad_idx >= 0 && e.max_len >= 0, w + ": bad pad_idx / max_len");
        GNNLM_REQUIRE((int64_t)e.pad_idx + 1 + e.max_len <= e.p_rows, w + full);
    }
    return OK;
}

int check_embed(const gnnlm_lm_embed_t& e, const gnnlm_ragged_t& rg) {
    GNNLM_REQUIRE(rg.n_tok >= 0 && rg.n_tok < (1ll << 31) && rg.n_blocks >= 0, "lm_embed: bad block table");
    GNNLM_REQUIRE(e.d > 0 && e.d % 4 == 0, "lm_embed: d % 4 != 0");
    GNNLM_REQUIRE(e.n_vocab > 0, "lm_embed: empty vocabulary");
    GNNLM_TRY(check_tables(e, "lm_embed", ": a block is longer than the position table holds (pad_idx + 1 + max_len > p_rows)"));
    if (rg.n_tok == 0) return OK;
    GNNLM_REQUIRE(e.tokens && e.out && (uintptr_t)e.out % 16 == 0, "lm_embed: tokens / out missing or out not 16-byte aligned");
    GNNLM_REQUIRE(!e.P || (rg.block_off && rg.n_blocks >= 1 && rg.n_blocks <= rg.n_tok), "lm_embed: positions need block_off with 1 .. n_tok blocks");
    return OK;
}

EmbedParams embed_params(const gnnlm_lm_embed_t& e, int64_t n) {
    return EmbedParams{e.tokens, e.E, e.ld_e, e.n_vocab, e.d / 4, e.P, e.ld_p, e.p_rows, e.pad_idx, e.scale, e.out, e.ldo, nullptr, 0,
                       n, e.n_bad, nullptr, 0};
}

int launch_embed(const gnnlm_lm_embed_t& e, const gnnlm_ragged_t& rg, hipStream_t stream) {
    if (rg.n_tok == 0) return OK;
    EmbedParams p = embed_params(e, rg.n_tok);
    p.block_off = rg.block_off; p.n_blocks = rg.n_blocks;
    ProfScope prof(K_MISC, stream, (e.P ? 2.0 : 1.0) * rg.n_tok * e.d, (e.P ? 12.0 : 8.0) * rg.n_tok * e.d + 8.0 * rg.n_tok);
    hipLaunchKernelGGL(lm_embed_kernel, dim3((unsigned)cdiv(rg.n_tok, 4)), dim3(256), 0, stream, p);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int launch_embed_step(const gnnlm_lm_embed_t& e, const gnnlm_kv_cache_t& c, hipStream_t stream) {
    EmbedParams p = embed_params(e, c.B);
    p.len = c.len; p.cap = (int)e.max_len;
    ProfScope prof(K_MISC, stream, (e.P ? 2.0 : 1.0) * c.B * e.d, (e.P ? 12.0 : 8.0) * c.B * e.d + 12.0 * c.B);
    hipLaunchKernelGGL(lm_embed_step_kernel, dim3((unsigned)cdiv(c.B, 4)), dim3(256), 0, stream, p);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

// the row buffers of n rows, and -- attn_len >= 0 -- the scratch of decode_attn for n sequences of up to attn_len keys behind them
struct TlmBufs { float *x, *h, *a, *wide, *attn_ws; size_t attn_bytes; };
size_t carve_tlm(const gnnlm_tlm_t& m, int64_t n, int attn_len, char* base, TlmBufs& b) {
    Carver c(base);
    b.x = c.take<float>(n * m.d);
    b.h = c.take<float>(n * m.d);
    b.a = c.take<float>(n * m.d);
    b.wide = c.take<float>(n * std::max<int64_t>(3 * (int64_t)m.d, m.ffn));      // q | k | v of the attention block, then the fc1 output
    b.attn_ws = nullptr;
    b.attn_bytes = attn_len < 0 ? 0 : decode_attn_workspace_bytes((int)n, m.H, m.H > 0 ? m.d / m.H : 0, attn_len);
    if (attn_len >= 0) b.attn_ws = reinterpret_cast<float*>(c.take<char>((int64_t)b.attn_bytes));
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

// IO: gnnlm_tlm_io_t or gnnlm_tlm_step_io_t -- the members read here are common to both
template <class IO>
gnnlm_lm_embed_t embed_of(const gnnlm_tlm_t& m, const IO& io, float* out) {
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

template <class IO>
int check_outputs(const IO& io, const char* who) {
    const std::string w(who);
    GNNLM_REQUIRE(io.tokens && io.out, w + ": tokens / out missing");
    GNNLM_REQUIRE(((uintptr_t)io.out | (uintptr_t)io.last_inner | (uintptr_t)io.last_ffn_input) % 16 == 0, w + ": outputs must be 16-byte aligned");
    return OK;
}

int carve_checked(const gnnlm_tlm_t& m, int64_t n, int attn_len, void* ws, size_t ws_bytes, const char* who, TlmBufs& b) {
    GNNLM_REQUIRE(ws && (uintptr_t)ws % 16 == 0 && carve_tlm(m, n, attn_len, nullptr, b) <= ws_bytes,
                  std::string(who) + ": workspace missing, misaligned or too small");
    carve_tlm(m, n, attn_len, reinterpret_cast<char*>(ws), b);
    return OK;
}

// The decoder over the n embedded rows of b.x: the embed-norm, L pre-norm layers, the final norm or copy.  attn(l) enqueues layer l's
// attention stage, q | k | v rows b.wide -> b.a.  out / last_inner / last_ffn_input as gnnlm_tlm_io_t names them.
template <class IO, class Attn>
int tlm_layers(const gnnlm_tlm_t& m, int64_t n, const TlmBufs& b, const IO& io, const Attn& attn, hipStream_t s) {
    const int d = m.d;
    const float eps = m.ln_eps == 0.f ? 1e-5f : m.ln_eps;
    GemmPrecisionScope prec_scope(m.precision);
    if (m.ln_emb_g) GNNLM_TRY(layernorm(b.x, d, m.ln_emb_g, m.ln_emb_b, b.x, d, n, d, eps, nullptr, s));
    for (int l = 0; l < m.L; ++l) {
        const gnnlm_tlm_layer_t& w = m.layers[l];
        const bool last = l == m.L - 1;
        // self-attention block: x += out_proj(attn(LN(x)))
        GNNLM_TRY(layernorm(b.x, d, w.ln1_g, w.ln1_b, b.h, d, n, d, eps, nullptr, s));
        GNNLM_TRY(linear(b.h, d, w.wqkv, w.bqkv, b.wide, n, 3 * d, d, nullptr, ALPHA_UNSET, s));
        GNNLM_TRY(attn(l));
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
    return OK;
}

// Packed causal attention.  cache != nullptr (gnnlm_transformer_lm_prefill): block b is sequence b, its K' / V' rows are copied into
// the cache after each layer's q|k|v GEMM and len is set at the end; the launches of the forward itself are the same either way.
int tlm_forward(const gnnlm_tlm_t& m, const gnnlm_tlm_io_t& io, void* ws, size_t ws_bytes, hipStream_t s, const gnnlm_kv_cache_t* cache = nullptr) {
    GNNLM_TRY(check_tlm(m));
    const gnnlm_ragged_t& rg = io.blocks;
    if (cache) {
        GNNLM_TRY(check_tlm_cache(m, *cache));
        GNNLM_REQUIRE(rg.n_blocks == cache->B, "transformer_lm_prefill: n_blocks != the cache's B");
        GNNLM_REQUIRE(io.max_len >= 0 && io.max_len <= cache->cap, "transformer_lm_prefill: a block is longer than the cache (max_len > cap)");
    }
    const int64_t n = rg.n_tok;
    const int d = m.d;
    GNNLM_TRY(check_embed(embed_of(m, io, reinterpret_cast<float*>(ws)), rg));
    if (n == 0) return OK;
    GNNLM_TRY(check_outputs(io, "transformer_lm"));
    GNNLM_REQUIRE(rg.block_off && rg.tiles && rg.n_blocks >= 1 && rg.n_blocks <= n && rg.n_tiles >= rg.n_blocks &&
                  (int64_t)rg.n_tiles <= n / 32 + rg.n_blocks, "transformer_lm: block_off / tiles missing or inconsistent (see gnnlm_ragged_tiles)");
    TlmBufs b;
    GNNLM_TRY(carve_checked(m, n, -1, ws, ws_bytes, "transformer_lm", b));

    GNNLM_TRY(launch_embed(embed_of(m, io, b.x), rg, s));
    const auto attn = [&](int l) {
        if (cache) GNNLM_TRY(kv_cache_fill(b.wide + d, b.wide + 2 * d, 3 * (int64_t)d, *cache, l, rg, (int)io.max_len, s));
        return causal_attn_varlen(b.wide, b.wide + d, b.wide + 2 * d, 3 * (int64_t)d, b.a, d, rg, m.H, d / m.H, 0, s);
    };
    GNNLM_TRY(tlm_layers(m, n, b, io, attn, s));
    if (cache) GNNLM_TRY(kv_len_set(*cache, rg.block_off, (int)io.max_len, s));
    return OK;
}

// One new row per sequence against the cache.  tab (gnnlm_transformer_lm_step_beam): every layer's attention reads its cached rows
// through the table.
int tlm_step(const gnnlm_tlm_t& m, const gnnlm_kv_cache_t& c, const gnnlm_tlm_step_io_t& io, void* ws, size_t ws_bytes, hipStream_t s,
             const SlotTable* tab = nullptr) {
    GNNLM_TRY(check_tlm(m));
    GNNLM_TRY(check_tlm_cache(m, c));
    const int B = c.B, d = m.d;
    GNNLM_REQUIRE(io.max_len >= 1 && io.max_len <= c.cap, "transformer_lm_step: max_len outside [1, cap] (the cache is full)");
    GNNLM_TRY(check_tables(embed_of(m, io, nullptr), "transformer_lm_step",
                           ": the position table does not hold the next position (pad_idx + 1 + max_len > p_rows)"));
    if (B == 0) return OK;
    GNNLM_TRY(check_outputs(io, "transformer_lm_step"));
    TlmBufs b;
    GNNLM_TRY(carve_checked(m, B, (int)io.max_len, ws, ws_bytes, "transformer_lm_step", b));

    GNNLM_TRY(launch_embed_step(embed_of(m, io, b.x), c, s));
    gnnlm_decode_attn_t a{};
    a.q = b.wide; a.k_new = b.wide + d; a.v_new = b.wide + 2 * d; a.ld = 3 * (int64_t)d;
    a.out = b.a; a.ldo = d;
    a.cache = c; a.H = m.H; a.dk = d / m.H; a.max_len = (int32_t)io.max_len;
    a.workspace = b.attn_ws; a.workspace_bytes = b.attn_bytes;
    const auto attn = [&](int l) {
        a.layer = l;
        if (l > 0) a.cache.n_bad = nullptr;                 // a row out of range is counted once per step, not once per layer
        return decode_attn(a, tab, s);
    };
    GNNLM_TRY(tlm_layers(m, B, b, io, attn, s));
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
    return carve_tlm(*m, io->blocks.n_tok, -1, nullptr, b);
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
    return carve_tlm(*m, c->B, (int)io->max_len, nullptr, b);
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
    const SlotTable tab{src, ld_src};
    return tlm_step(*m, *c, *io, workspace, workspace_bytes, (hipStream_t)stream, &tab);
}

}  // extern "C"
