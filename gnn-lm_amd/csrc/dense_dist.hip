// Next-token DISTRIBUTIONS: the dense [rows, V] outputs of the scoring chain, where every other file of this library answers for
// the target column only.
//
//   gnnlm_adaptive_log_probs   out[r, v] = log p(v | x[r]), tied adaptive softmax       AdaptiveSoftmax.get_log_prob(input, None),
//                                                                                       fairseq/modules/adaptive_softmax.py:170-206
//   gnnlm_dense_log_probs      the same for the plain head (with or without xl_bias)    fairseq/models/transformer.py:843-852,1081-1085
//   gnnlm_knn_mix_dense        out[r, v] = logaddexp(lm[r, v] + log(1 - l), log(p_knn[r, v] + 1e-10) + log l) for EVERY v
//                                                                                       knn/knn_model.py:192-205 (targets None),
//                                                                                       fairseq/sequence_scorer.py:55-68,121
//   gnnlm_row_rank             rank of the target under gnnlm_topk_merge's order (larger value first, then smaller id)
//
// Heads.  Rows are cut into chunks (at most HEAD_CHUNK_ROWS, and rows * ldo < 2^31, so that no kernel sees an element offset
// of 2^31 or more: the host advances the base pointers per chunk).  Per chunk, from what exists:
//   head logits      gemm_nt (store flavour) -> workspace [rows, cutoff0 + n_bands - 1]
//   band b >= 1      gemm_nt x . proj_t[b]^T -> workspace [rows, dim_b], then gemm_nt . emb[b]^T written STRAIGHT into
//                    out[:, cutoff[b-1] : cutoff[b]) with ldc = ldo (the GEMM's C needs 4-byte alignment only)
//   row sums         row_lse_pick without a pick over the head logits and over every band's columns of out
//   finish           head_finish_kernel, the one new kernel: in place, a head column gets head[v] - lse_head, a band column
//                    + head[cutoff0 + b - 1] - lse_head - lse_band.  Pad columns (v >= V of ldo > V) are never written.
// The plain head is the same chain with one "band": gemm_nt (bias_mode 1) into out, row_lse_pick over out, the finish kernel.
//
// Mix.  A store-bound pass ([rows, V] written once, lm read once) in two launches ordered by the stream:
//   mix_fill_kernel  elementwise over [rows, V]: every column gets the NO-NEIGHBOUR value logaddexp(lm + log(1 - l),
//                    logf(1e-10f) + log l), out_pknn zero; 16-byte loads and stores when the bases and row strides allow
//   mix_rows_kernel  one workgroup per row: softmax over the k neighbours (knn_model.py:192-196, -1e10 for id == -1), the
//                    (label, column) pairs sorted by a bitonic network in LDS (the key (label << 32 | j) is unique, so the order
//                    is total), every run of equal labels summed in sorted order by one thread in float64 -- no floating-point
//                    atomics, the same bits on every call -- and its at most k label columns overwritten from lm_logp.
//                    A label outside [0, V) (and a row outside the shard / store, as for gnnlm_knn_interp) takes part in the
//                    softmax's denominator but writes nothing.

#include "host.h"

namespace gnnlm {
namespace {

constexpr int64_t HEAD_CHUNK_ROWS = 1024;        // default rows per chunk (a multiple of MIN_CHUNK_ROWS)
constexpr int64_t MIN_CHUNK_ROWS = 128;          // the least a call accepts (or n, if smaller)
constexpr int64_t OFFSET_CAP = (1ll << 31) - 1;  // element offsets inside one kernel stay below 2^31

struct FinishArgs {
    const float* head;  int64_t ld_head;          // head logits [rows, ...]; the plain head passes out itself
    float* out;  int64_t ldo;
    const float* lse;   int64_t ld_lse;           // lse[b * ld_lse + r]: b = 0 the head, b >= 1 the bands
    int32_t n_bands;
    int32_t cutoff[8];
};

// grid (column tiles of 4096, rows).  adj[b] is the row's additive term of band b.
__global__ __launch_bounds__(256) void head_finish_kernel(const FinishArgs p) {
    __shared__ float adj[8];
    const int64_t r = blockIdx.y;
    const float* head = p.head + r * p.ld_head;
    float* out = p.out + r * p.ldo;
    const int tid = threadIdx.x;
    if (tid < p.n_bands) {
        const float l0 = p.lse[r];
        adj[tid] = tid == 0 ? -l0 : head[p.cutoff[0] + tid - 1] - l0 - p.lse[(int64_t)tid * p.ld_lse + r];
    }
    __syncthreads();
    const int V = p.cutoff[p.n_bands - 1], c0 = p.cutoff[0];
    const int v_end = min(V, ((int)blockIdx.x + 1) * 4096);
    for (int v = (int)blockIdx.x * 4096 + tid; v < v_end; v += 256) {
        int b = 0;
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (i < p.n_bands && v >= p.cutoff[i - 1]) b = i;
        out[v] = (v < c0 ? head[v] : out[v]) + adj[b];
    }
}

int head_finish(const FinishArgs& a, int64_t rows, hipStream_t s) {
    const int V = a.cutoff[a.n_bands - 1];
    hipLaunchKernelGGL(head_finish_kernel, dim3((unsigned)cdiv(V, 4096), (unsigned)rows), dim3(256), 0, s, a);
    GNNLM_LAUNCH_CHECK();
    return OK;
}


// ---- adaptive head ----
struct AdaptiveBufs { float *head, *xi, *lse; };
int64_t pad4(int64_t v) { return (v + 3) & ~3ll; }
size_t carve_adaptive(const gnnlm_adaptive_softmax_t& w, int64_t chunk, void* ws, AdaptiveBufs& b) {
    int64_t max_dim = 0;
    for (int i = 1; i < w.n_bands; ++i) max_dim = std::max<int64_t>(max_dim, w.dim[i]);
    Carver c(ws);
    b.head = c.take<float>(chunk * pad4((int64_t)w.cutoff[0] + w.n_bands - 1));
    b.xi = c.take<float>(chunk * max_dim);
    b.lse = c.take<float>(chunk * w.n_bands);
    return c.off + 256;
}
bool adaptive_shape_ok(const gnnlm_adaptive_softmax_t& w) {
    if (w.n_bands < 1 || w.n_bands > 8 || w.d <= 0 || w.d % 4 || w.cutoff[0] < 1) return false;
    for (int i = 1; i < w.n_bands; ++i)
        if (w.cutoff[i] <= w.cutoff[i - 1] || w.dim[i] <= 0 || w.dim[i] % 4) return false;
    return true;
}
int64_t default_chunk(int64_t n) { return std::min(n, HEAD_CHUNK_ROWS); }
int64_t least_chunk(int64_t n) { return std::min(n, MIN_CHUNK_ROWS); }

// rows per chunk for a workspace of ws_bytes whose size is fixed + per_row * chunk (0: it does not fit MIN_CHUNK_ROWS)
template <class SizeFn>
int64_t fit_chunk(int64_t n, size_t ws_bytes, SizeFn size_of) {
    int64_t chunk = default_chunk(n);
    if (size_of(chunk) <= ws_bytes) return chunk;
    for (chunk = chunk / MIN_CHUNK_ROWS * MIN_CHUNK_ROWS; chunk >= MIN_CHUNK_ROWS; chunk -= MIN_CHUNK_ROWS)
        if (size_of(chunk) <= ws_bytes) return chunk;
    chunk = least_chunk(n);
    return size_of(chunk) <= ws_bytes ? chunk : 0;
}

int adaptive_dense_impl(const gnnlm_adaptive_softmax_t& w, const float* x, int64_t ldx, int64_t n, float* out, int64_t ldo, void* ws,
                        size_t ws_bytes, hipStream_t s) {
    // everything is checked here, in front of the first launch: what gemm_nt() would refuse half-way through the call included
    GNNLM_REQUIRE(adaptive_shape_ok(w), "adaptive_log_probs: bad bands (n_bands 1..8, d and tail dims positive multiples of 4, cutoffs ascending)");
    GNNLM_REQUIRE(w.gemm_precision >= 0 && w.gemm_precision <= 3, "adaptive_log_probs: gemm_precision must be 0, 1, 2 or 3");
    GNNLM_REQUIRE(w.head_w && (uintptr_t)w.head_w % 16 == 0, "adaptive_log_probs: head_w must be given and 16-byte aligned");
    for (int i = 1; i < w.n_bands; ++i)
        GNNLM_REQUIRE(w.proj_t[i] && w.emb[i] && (uintptr_t)w.proj_t[i] % 16 == 0 && (uintptr_t)w.emb[i] % 16 == 0,
                      "adaptive_log_probs: band weights must be given and 16-byte aligned");
    const int V = w.cutoff[w.n_bands - 1];
    GNNLM_REQUIRE(n >= 0 && n < (1ll << 31), "adaptive_log_probs: bad row count");
    GNNLM_REQUIRE(x && out, "adaptive_log_probs: null io");
    GNNLM_REQUIRE(ldx >= w.d && ldx % 4 == 0 && (uintptr_t)x % 16 == 0, "adaptive_log_probs: x must be 16-byte aligned with ldx >= d, ldx % 4 == 0");
    GNNLM_REQUIRE(ldo >= V && ldo <= OFFSET_CAP && (uintptr_t)out % 4 == 0, "adaptive_log_probs: out must be 4-byte aligned with V <= ldo < 2^31");
    if (n == 0) return OK;
    AdaptiveBufs b{};
    int64_t chunk = fit_chunk(n, ws_bytes, [&](int64_t c) { return carve_adaptive(w, c, nullptr, b); });
    GNNLM_REQUIRE(ws && chunk > 0, "adaptive_log_probs: workspace too small (see gnnlm_adaptive_log_probs_workspace_bytes / _min)");
    GNNLM_REQUIRE((uintptr_t)ws % 16 == 0, "adaptive_log_probs: the workspace must be 16-byte aligned");
    chunk = std::max<int64_t>(1, std::min(chunk, OFFSET_CAP / std::max(ldo, ldx)));
    carve_adaptive(w, chunk, ws, b);
    GemmPrecisionScope prec_scope(w.gemm_precision);
    const int nt = w.n_bands - 1, head_n = w.cutoff[0] + nt;
    const int64_t ld_head = pad4(head_n);
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t rows = std::min(chunk, n - r0);
        const float* xc = x + r0 * ldx;
        float* oc = out + r0 * ldo;
        {   // head: [E_0 ; class_proj] (adaptive_softmax.py:24-47,184-188), logits kept: the finish reads them
            GemmParams g{};
            g.A = xc; g.lda = ldx; g.W = w.head_w; g.ldw = w.d; g.C = b.head; g.ldc = ld_head;
            g.M = (int)rows; g.N = head_n; g.K = w.d;
            GNNLM_TRY(gemm_nt(g, s));
        }
        GNNLM_TRY(row_lse_pick(b.head, ld_head, rows, nullptr, head_n, nullptr, b.lse, nullptr, s));
        for (int i = 1; i < w.n_bands; ++i) {   // tails (adaptive_softmax.py:91-115,199-203), every row
            const int size = w.cutoff[i] - w.cutoff[i - 1];
            GemmParams g{};
            g.A = xc; g.lda = ldx; g.W = w.proj_t[i]; g.ldw = w.d; g.C = b.xi; g.ldc = w.dim[i];
            g.M = (int)rows; g.N = w.dim[i]; g.K = w.d;
            GNNLM_TRY(gemm_nt(g, s));
            GemmParams t{};
            t.A = b.xi; t.lda = w.dim[i]; t.W = w.emb[i]; t.ldw = w.dim[i]; t.C = oc + w.cutoff[i - 1]; t.ldc = ldo;
            t.M = (int)rows; t.N = size; t.K = w.dim[i];
            GNNLM_TRY(gemm_nt(t, s));
            GNNLM_TRY(row_lse_pick(oc + w.cutoff[i - 1], ldo, rows, nullptr, size, nullptr, b.lse + (int64_t)i * chunk, nullptr, s));
        }
        FinishArgs f{};
        f.head = b.head; f.ld_head = ld_head; f.out = oc; f.ldo = ldo; f.lse = b.lse; f.ld_lse = chunk; f.n_bands = w.n_bands;
        for (int i = 0; i < w.n_bands; ++i) f.cutoff[i] = w.cutoff[i];
        GNNLM_TRY(head_finish(f, rows, s));
    }
    return OK;
}

// ---- plain head ----
size_t carve_plain(int64_t chunk, void* ws, float*& lse) {
    Carver c(ws);
    lse = c.take<float>(chunk);
    return c.off + 256;
}
bool plain_shape_ok(const gnnlm_dense_softmax_t& w) {
    return w.d > 0 && w.d % 4 == 0 && w.vocab >= 1 && w.gemm_precision >= 0 && w.gemm_precision <= 3;
}
int plain_dense_impl(const gnnlm_dense_softmax_t& w, const float* x, int64_t ldx, int64_t n, float* out, int64_t ldo, void* ws,
                     size_t ws_bytes, hipStream_t s) {
    GNNLM_REQUIRE(plain_shape_ok(w), "dense_log_probs: d must be a positive multiple of 4, vocab >= 1, gemm_precision 0..3");
    GNNLM_REQUIRE(w.w && w.ldw >= w.d && w.ldw % 4 == 0 && (uintptr_t)w.w % 16 == 0, "dense_log_probs: w must be 16-byte aligned with ldw >= d, ldw % 4 == 0");
    GNNLM_REQUIRE(n >= 0 && n < (1ll << 31), "dense_log_probs: bad row count");
    GNNLM_REQUIRE(x && out, "dense_log_probs: null io");
    GNNLM_REQUIRE(ldx >= w.d && ldx % 4 == 0 && (uintptr_t)x % 16 == 0, "dense_log_probs: x must be 16-byte aligned with ldx >= d, ldx % 4 == 0");
    GNNLM_REQUIRE(ldo >= w.vocab && ldo <= OFFSET_CAP && (uintptr_t)out % 4 == 0, "dense_log_probs: out must be 4-byte aligned with V <= ldo < 2^31");
    if (n == 0) return OK;
    float* lse = nullptr;
    int64_t chunk = fit_chunk(n, ws_bytes, [&](int64_t c) { return carve_plain(c, nullptr, lse); });
    GNNLM_REQUIRE(ws && chunk > 0, "dense_log_probs: workspace too small (see gnnlm_dense_log_probs_workspace_bytes / _min)");
    GNNLM_REQUIRE((uintptr_t)ws % 16 == 0, "dense_log_probs: the workspace must be 16-byte aligned");
    chunk = std::max<int64_t>(1, std::min(chunk, OFFSET_CAP / std::max(ldo, ldx)));
    carve_plain(chunk, ws, lse);
    GemmPrecisionScope prec_scope(w.gemm_precision);
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t rows = std::min(chunk, n - r0);
        float* oc = out + r0 * ldo;
        GemmParams g{};
        g.A = x + r0 * ldx; g.lda = ldx; g.W = w.w; g.ldw = w.ldw; g.C = oc; g.ldc = ldo;
        if (w.bias) { g.bias = w.bias; g.bias_mode = 1; }       // xl_bias: added in f32 under every precision
        g.M = (int)rows; g.N = w.vocab; g.K = w.d;
        GNNLM_TRY(gemm_nt(g, s));
        GNNLM_TRY(row_lse_pick(oc, ldo, rows, nullptr, w.vocab, nullptr, lse, nullptr, s));
        FinishArgs f{};
        f.head = oc; f.ld_head = ldo; f.out = oc; f.ldo = ldo; f.lse = lse; f.ld_lse = chunk; f.n_bands = 1;
        f.cutoff[0] = w.vocab;
        GNNLM_TRY(head_finish(f, rows, s));
    }
    return OK;
}

// ---- kNN mix ----
typedef gnnlm_knn_mix_dense_t MixParams;
constexpr int MIX_MAX_K = 1024;

__device__ __forceinline__ float logaddexp_f(float a, float b) {      // sequence_scorer.py:55-68, as knn_interp_kernel
    const float m = fmaxf(a, b);
    return m + logf(expf(a - m) + expf(b - m));
}

// every column's no-neighbour value.  grid (column tiles, rows: grid-strided); VEC: float4 over the first V & ~3 columns
template <bool VEC>
__global__ __launch_bounds__(256) void mix_fill_kernel(const MixParams p, float log_1ml, float log_l) {
    const float none = logf(1e-10f) + log_l;                           // logf(p_knn + 1e-10f) + log(lmbda) with p_knn = 0
    const int tid = threadIdx.x;
    for (int64_t r = blockIdx.y; r < p.n; r += gridDim.y) {
        const float* lm = p.lm_logp + r * p.ld_lm;
        float* out = p.out + r * p.ldo;
        float* pk = p.out_pknn ? p.out_pknn + r * p.ld_pknn : nullptr;
        int v_scalar = 0;
        if constexpr (VEC) {
            const int nv = p.V >> 2;
            for (int g = (int)blockIdx.x * 256 + tid; g < nv; g += (int)gridDim.x * 256) {
                const float4 a = reinterpret_cast<const float4*>(lm)[g];
                float4 o;
                o.x = logaddexp_f(a.x + log_1ml, none);
                o.y = logaddexp_f(a.y + log_1ml, none);
                o.z = logaddexp_f(a.z + log_1ml, none);
                o.w = logaddexp_f(a.w + log_1ml, none);
                reinterpret_cast<float4*>(out)[g] = o;
                if (pk) reinterpret_cast<float4*>(pk)[g] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            v_scalar = nv << 2;
        }
        for (int v = v_scalar + (int)blockIdx.x * 256 + tid; v < p.V; v += (int)gridDim.x * 256) {
            out[v] = logaddexp_f(lm[v] + log_1ml, none);
            if (pk) pk[v] = 0.f;
        }
    }
}

constexpr uint32_t NO_LABEL = 0xFFFFFFFFu;     // sorts behind every label of [0, V)

// one workgroup per row
__global__ __launch_bounds__(256) void mix_rows_kernel(const MixParams p, float log_1ml, float log_l) {
    __shared__ uint64_t key[MIX_MAX_K];          // (label << 32) | neighbour column j: unique, so the sorted order is total
    __shared__ float ev[MIX_MAX_K];              // exp(s_j - max), by neighbour column
    __shared__ float red_m[4];
    __shared__ double red_s[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t i = blockIdx.x;
    const float* sims = p.sims + i * p.k;
    const int64_t* ids = p.ids + i * p.k;
    int P = 1;
    while (P < p.k) P <<= 1;

    float mx = -INFINITY;
    for (int j = tid; j < P; j += 256) {
        uint32_t label = NO_LABEL;
        if (j < p.k) {
            const int64_t id = ids[j];
            const float s = (id == -1 ? -1e10f : sims[j]) / p.temperature;      // knn_model.py:193,196
            ev[j] = s;
            mx = fmaxf(mx, s);
            int64_t val = -1;
            if (p.knn_vals) {
                val = p.knn_vals[i * p.k + j];
            } else {
                // numpy indexing semantics of vals[knns] (knn_model.py:198): -1 wraps to the last row
                const int64_t row = (id < 0 ? id + p.n_store : id) - p.row0;
                if (row >= 0 && row < p.n_local)
                    val = p.vals_itemsize == 2 ? (int64_t) reinterpret_cast<const int16_t*>(p.vals)[row]
                                               : (int64_t) reinterpret_cast<const int32_t*>(p.vals)[row];
            }
            if (val >= 0 && val < p.V) label = (uint32_t)val;
        }
        key[j] = ((uint64_t)label << 32) | (uint32_t)j;
    }
    mx = wave_max(mx);
    if (lane == 0) red_m[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    double part = 0.0;
    for (int j = tid; j < p.k; j += 256) {
        const float e = expf(ev[j] - mx);
        ev[j] = e;
        part += (double)e;
    }
    // denominator: a fixed tree (lanes, then waves) in float64
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (lane == 0) red_s[wave] = part;
    // bitonic sort of the P keys, ascending
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < (P >> 1); t += 256) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t a = key[lo], b = key[hi];
                if ((a > b) == up) { key[lo] = b; key[hi] = a; }
            }
        }
    __syncthreads();
    const double den = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    const float* lm = p.lm_logp + i * p.ld_lm;
    float* out = p.out + i * p.ldo;
    float* pk = p.out_pknn ? p.out_pknn + i * p.ld_pknn : nullptr;
    // the thread that owns the first pair of a run sums the run, in sorted order
    for (int q = tid; q < p.k; q += 256) {
        const uint32_t label = (uint32_t)(key[q] >> 32);
        if (label == NO_LABEL || (q > 0 && (uint32_t)(key[q - 1] >> 32) == label)) continue;
        double num = 0.0;
        for (int e = q; e < p.k && (uint32_t)(key[e] >> 32) == label; ++e) num += (double)ev[(uint32_t)key[e]];
        const float pv = (float)(num / den);
        if (pk) pk[label] = pv;
        out[label] = logaddexp_f(lm[label] + log_1ml, logf(pv + 1e-10f) + log_l);
    }
}

int knn_mix_dense(const MixParams& p, hipStream_t s) {
    GNNLM_REQUIRE(p.lm_logp && p.sims && p.ids && p.out, "knn_mix_dense: null operand");
    GNNLM_REQUIRE(p.knn_vals || p.vals, "knn_mix_dense: need vals or pre-fetched knn_vals");
    GNNLM_REQUIRE(p.knn_vals || (p.n_local > 0 && p.n_store > 0 && p.row0 >= 0), "knn_mix_dense: vals needs n_store / row0 / n_local");
    GNNLM_REQUIRE(p.knn_vals || p.vals_itemsize == 2 || p.vals_itemsize == 4, "knn_mix_dense: vals must be int16 or int32");
    GNNLM_REQUIRE(p.k >= 1 && p.k <= MIX_MAX_K, "knn_mix_dense: k must be in 1..1024");
    GNNLM_REQUIRE(p.temperature > 0.f && p.lmbda > 0.0 && p.lmbda < 1.0, "knn_mix_dense: need temperature > 0 and 0 < lmbda < 1");
    GNNLM_REQUIRE(p.n >= 0 && p.n < (1ll << 31) && p.V >= 1, "knn_mix_dense: bad n / V");
    GNNLM_REQUIRE(p.ld_lm >= p.V && p.ldo >= p.V && (!p.out_pknn || p.ld_pknn >= p.V), "knn_mix_dense: a row stride is smaller than V");
    GNNLM_REQUIRE((uintptr_t)p.lm_logp % 4 == 0 && (uintptr_t)p.out % 4 == 0 && (uintptr_t)p.out_pknn % 4 == 0 && (uintptr_t)p.sims % 4 == 0 &&
                  (uintptr_t)p.ids % 8 == 0 && (uintptr_t)p.knn_vals % 4 == 0 && (uintptr_t)p.vals % (p.vals_itemsize == 2 ? 2 : 4) == 0,
                  "knn_mix_dense: misaligned operand");
    GNNLM_REQUIRE(p.out != p.lm_logp && p.out_pknn != p.lm_logp && p.out_pknn != p.out, "knn_mix_dense: out, out_pknn and lm_logp must not alias");
    if (p.n == 0) return OK;
    const float log_1ml = (float)log(1.0 - p.lmbda), log_l = (float)log(p.lmbda);
    const bool vec = (uintptr_t)p.lm_logp % 16 == 0 && (uintptr_t)p.out % 16 == 0 && (uintptr_t)p.out_pknn % 16 == 0 && p.ld_lm % 4 == 0 &&
                     p.ldo % 4 == 0 && p.ld_pknn % 4 == 0;
    // a thread takes up to 4 float4 (or 4 scalars) of a row
    const dim3 grid((unsigned)std::max<int64_t>(1, cdiv(vec ? p.V >> 2 : p.V, 1024)), (unsigned)std::min<int64_t>(p.n, 65535));
    if (vec) hipLaunchKernelGGL(mix_fill_kernel<true>, grid, dim3(256), 0, s, p, log_1ml, log_l);
    else hipLaunchKernelGGL(mix_fill_kernel<false>, grid, dim3(256), 0, s, p, log_1ml, log_l);
    GNNLM_LAUNCH_CHECK();
    hipLaunchKernelGGL(mix_rows_kernel, dim3((unsigned)p.n), dim3(256), 0, s, p, log_1ml, log_l);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

// ---- rank ----
// a column is PRESENT under gnnlm_topk_merge's rules (largest first) unless its value is NaN or -inf
__device__ __forceinline__ bool rank_present(float v) { return v == v && v != -INFINITY; }

// one workgroup per row: the number of present columns in front of the target, (value descending, id ascending).  A target
// whose own value is absent comes behind every present column.
__global__ __launch_bounds__(256) void row_rank_kernel(const float* logp, int64_t ld, int V, const int64_t* target, int32_t* rank) {
    __shared__ int red[4];
    const int64_t r = blockIdx.x;
    const int64_t t = target[r];
    const int tid = threadIdx.x;
    if (t < 0 || t >= V) {
        if (tid == 0) rank[r] = -1;
        return;
    }
    const float* row = logp + r * ld;
    const float tv = row[t];
    const bool t_present = rank_present(tv);
    int cnt = 0;
    for (int v = tid; v < V; v += 256) {
        const float x = row[v];
        cnt += rank_present(x) && (!t_present || x > tv || (x == tv && v < (int)t));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) rank[r] = red[0] + red[1] + red[2] + red[3];
}

int row_rank(const float* logp, int64_t ld, int64_t n, int V, const int64_t* target, int32_t* rank, hipStream_t s) {
    GNNLM_REQUIRE(logp && target && rank, "row_rank: null operand");
    GNNLM_REQUIRE(n >= 0 && n < (1ll << 31) && V >= 1 && ld >= V, "row_rank: need 0 <= n < 2^31, V >= 1, ld >= V");
    GNNLM_REQUIRE((uintptr_t)logp % 4 == 0 && (uintptr_t)target % 8 == 0 && (uintptr_t)rank % 4 == 0, "row_rank: misaligned operand");
    if (n == 0) return OK;
    hipLaunchKernelGGL(row_rank_kernel, dim3((unsigned)n), dim3(256), 0, s, logp, ld, V, target, rank);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace
}  // namespace gnnlm

using namespace gnnlm;

extern "C" {

size_t gnnlm_adaptive_log_probs_workspace_bytes(const gnnlm_adaptive_softmax_t* w, int64_t n) {
    if (!w || n <= 0 || !adaptive_shape_ok(*w)) return 0;
    AdaptiveBufs b{};
    return carve_adaptive(*w, default_chunk(n), nullptr, b);
}
size_t gnnlm_adaptive_log_probs_workspace_bytes_min(const gnnlm_adaptive_softmax_t* w, int64_t n) {
    if (!w || n <= 0 || !adaptive_shape_ok(*w)) return 0;
    AdaptiveBufs b{};
    return carve_adaptive(*w, least_chunk(n), nullptr, b);
}
int gnnlm_adaptive_log_probs(const gnnlm_adaptive_softmax_t* w, const float* x, int64_t ldx, int64_t n, float* out, int64_t ldo,
                             void* workspace, size_t workspace_bytes, void* stream) {
    GNNLM_DESC(w);
    return adaptive_dense_impl(*w, x, ldx, n, out, ldo, workspace, workspace_bytes, (hipStream_t)stream);
}
size_t gnnlm_dense_log_probs_workspace_bytes(const gnnlm_dense_softmax_t* w, int64_t n) {
    float* lse;
    return !w || n <= 0 || !plain_shape_ok(*w) ? 0 : carve_plain(default_chunk(n), nullptr, lse);
}
size_t gnnlm_dense_log_probs_workspace_bytes_min(const gnnlm_dense_softmax_t* w, int64_t n) {
    float* lse;
    return !w || n <= 0 || !plain_shape_ok(*w) ? 0 : carve_plain(least_chunk(n), nullptr, lse);
}
int gnnlm_dense_log_probs(const gnnlm_dense_softmax_t* w, const float* x, int64_t ldx, int64_t n, float* out, int64_t ldo,
                          void* workspace, size_t workspace_bytes, void* stream) {
    GNNLM_DESC(w);
    return plain_dense_impl(*w, x, ldx, n, out, ldo, workspace, workspace_bytes, (hipStream_t)stream);
}
int gnnlm_knn_mix_dense(const gnnlm_knn_mix_dense_t* d, void* stream) { GNNLM_DESC(d); return knn_mix_dense(*d, (hipStream_t)stream); }
int gnnlm_row_rank(const float* logp, int64_t ld, int64_t n, int32_t V, const int64_t* target, int32_t* rank, void* stream) {
    return row_rank(logp, ld, n, V, target, rank, (hipStream_t)stream);
}

}  // extern "C"
