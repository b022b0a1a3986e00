// Plain (non-adaptive) output layer, target log-probability only:
//
//   lm_logp[r] = (x[r] . w[t]^T + bias[t]) - log sum_v exp(x[r] . w[v]^T + bias[v]),   t = target[r]
//
// Reference: TransformerDecoder.output_layer with adaptive_softmax None (fairseq/models/transformer.py:843-852:
// F.linear(features, embed_tokens.weight | embed_out) [+ xl_bias]), the log_softmax of get_normalized_probs (:1081-1085) and
// gather_target_probs (fairseq/sequence_scorer.py:48-53,89) -- what a `--arch transformer_lm` checkpoint (enwik8,
// gnnlm_scripts/enwik8/prepare_enwik8.sh:34-42) takes instead of the adaptive softmax.
//
// Two routes (gnnlm_dense_softmax_t.route):
//
// 1. One launch, vocab <= 512, precision 0 (f32 MFMA) or 3 (fp16 operands): dense_logp_kernel below.  A workgroup of 4 waves owns
//    32 TM rows and the WHOLE vocabulary of those rows, so the log-probability leaves the GEMM directly: no logit, no per-slab
//    partial in HBM, no reduce launch, no pick launch, no workspace.
//      tile      (32 TM) rows x (128 TN) columns, TN = ceil(vocab / 128) in 1..4; wave w owns the columns [32 TN w, 32 TN (w + 1))
//                of every row.  TM in {1, 2, 4}: every workgroup re-reads W ([vocab, d], <= 2 MiB) from L2 while x is read once,
//                so W's traffic per flop falls with the rows a workgroup owns; dense_tm() takes the largest TM that still gives
//                every CU two workgroups (TM <= 4 for vocab <= 256, <= 2 above), short inputs keep 32-row workgroups
//      MFMA      v_mfma_f32_32x32x2_f32 with the operands swapped (W is "A", x is "B"), so an accumulator tile is TRANSPOSED:
//                column (lane & 31) = row of x, accumulator row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = vocabulary entry; the
//                k order inside a group of 8 is k, k+4, k+1, k+5, ... exactly as in gemm_f32.hip, so precision 0 is the same
//                fmaf chain bit for bit.  Precision 3: both operands are rounded to IEEE half while staged (v_cvt under the
//                default rounding mode: nearest even, beyond +-65504 -> +-inf), v_mfma_f32_32x32x16_f16, f32 accumulation
//      registers 16 TM TN accumulator registers (AGPRs) + (TM + 4 TN) float4 of staging + 4 (TM + TN) of operand fragments +
//                row offsets.  hipcc -Rpass-analysis=kernel-resource-usage, VGPR + AGPR -> waves per SIMD, no scratch anywhere:
//                (TM, TN) = (1, 1) 52 + 16 -> 7, (1, 2) 86 + 32 -> 4, (1, 3) 109 + 48 -> 3, (1, 4) 140 + 64 -> 2,
//                (2, 2) 109 + 64 -> 2, (2, 3) 159 + 96 -> 2, (2, 4) 208 + 128 -> 1, (4, 1) 94 + 64 -> 3, (4, 2) 175 + 128 -> 1
//      LDS       one buffer of (32 TM + 128 TN) rows of 32 k: f32 rows of 36 floats (144 B: ds_read_b128 of 16 lanes lands on 16
//                distinct 16-B slots, 9 i mod 16), 23,040 B at (1, 1) .. 82,944 B at (2, 4); fp16 rows of 80 B, at most 46,080 B.
//                Above 64 KiB (TN = 4, f32) the kernel opts in to the large dynamic LDS.  The epilogue reuses the first
//                36 TM x 32 B: 4 x 32 TM maxima, 4 x 32 TM sums, 32 TM target logits.
//      epilogue  in registers and LDS only: + bias (f32, never rounded), columns >= vocab masked to -inf, row maximum (in-lane
//                over the registers, v_permlane32_swap between the two halves of a row, LDS across the 4 waves), sum of
//                exp2((x - max) log2 e), the target's logit picked from the register that holds it, then
//                out = (logit - max) - log(sum).  Vector stores only.
//
// 2. General route (every other vocab, precisions 1 and 2), from existing entry points: without a bias the LSE-epilogue GEMM
//    (lse_pick / lse_picked) + lse_reduce, the adaptive head's own path; with a bias, which the LSE epilogue cannot add, the
//    storing GEMM with bias_mode 1 into a [rows, vocab] chunk of the workspace + row_lse_pick.  This is the one case that writes
//    logits to HBM.  Rows are cut into chunks so that the logits of a chunk stay below LOGITS_CAP = 64 MiB (a quarter of the
//    256 MiB Infinity Cache: the row pass re-reads what the GEMM just wrote without going to HBM); a caller may hand in less
//    workspace, down to gnnlm_dense_workspace_bytes_min (128-row chunks).
#include <cstdlib>

#include "host.h"

namespace gnnlm {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

constexpr int BK = 32;
constexpr int F32_LD = BK + 4;            // floats per LDS row, f32 operands
constexpr int F16_LD = 20;                // floats (80 B) per LDS row of 32 halves
constexpr int MAX_ONE_LAUNCH_VOCAB = 512;
constexpr int AUTO_ONE_LAUNCH_VOCAB = 384;
constexpr int64_t LOGITS_CAP = 64ll << 20;
constexpr int64_t MIN_CHUNK_ROWS = 128;

struct DenseArgs {
    const float* x;  int64_t ldx;
    const float* w;  int64_t ldw;
    const float* bias;
    const int64_t* target;
    int64_t n;
    int d, vocab;
    float* out;
};

template <int TM, int TN, bool HALF>
constexpr size_t dense_lds_bytes() { return (size_t)(32 * TM + 128 * TN) * (HALF ? F16_LD : F32_LD) * sizeof(float); }

// TM: 32-row tiles of x per workgroup (every wave holds all of them), TN: 32-column tiles of the vocabulary per wave.
template <int TM, int TN, bool HALF>
__global__ __launch_bounds__(256) void dense_logp_kernel(const DenseArgs p) {
    constexpr int BM = 32 * TM;                          // rows of x per workgroup
    constexpr int WCOLS = 32 * TN;                       // vocabulary columns of one wave
    constexpr int ROWS = BM + 4 * WCOLS;                 // LDS rows: the rows of x, then the (padded) vocabulary
    constexpr int NLD = ROWS / 32;                       // staging float4 per thread and k-tile
    constexpr int ROW_F = HALF ? F16_LD : F32_LD;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int64_t m0 = (int64_t)blockIdx.x * BM;

    // staging: thread -> (row srow + 32 i, k offset kq); rows beyond n / vocab read a clamped (valid) row, whose logits are
    // masked (columns) or never stored (rows).  Rows as 32-bit byte offsets from the two bases (half the address registers of
    // a pointer per row; the host checked vocab * ldw < 2^30, and a workgroup's rows of x span 128 ldx < 2^30 elements)
    const int kq = (tid & 7) * 4, srow = tid >> 3;
    const int64_t row_lim = p.n - m0;                    // >= 1: rows of this workgroup that exist
    const char* xbase = reinterpret_cast<const char*>(p.x + m0 * p.ldx);
    const char* wbase = reinterpret_cast<const char*>(p.w);
    unsigned off[NLD];
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
        const int r = srow + 32 * (i < TM ? i : i - TM);
        off[i] = i < TM ? (unsigned)(r < row_lim ? r : 0) * (unsigned)p.ldx * 4u : (unsigned)(r < p.vocab ? r : 0) * (unsigned)p.ldw * 4u;
    }
    float4 rg[NLD];
    const int nk = (p.d + BK - 1) / BK;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // the k offset of a tile's loads is clamped into the row (d % 4 == 0: a float4 is inside or outside as a whole); what was
    // read beyond d is zeroed when it is written to LDS, so no select sits behind a load that is still in flight
#define GNNLM_DENSE_LOAD(kt)                                                                 \
    {                                                                                        \
        int k_ = (kt) * BK + kq;                                                             \
        k_ = k_ < p.d ? k_ : 0;                                                              \
        _Pragma("unroll") for (int i_ = 0; i_ < NLD; ++i_)                                   \
            rg[i_] = *reinterpret_cast<const float4*>((i_ < TM ? xbase : wbase) + (off[i_] + 4u * (unsigned)k_)); \
    }
#define GNNLM_DENSE_STORE(kt)                                                                \
    {                                                                                        \
        const bool kin_ = (kt) * BK + kq < p.d;                                              \
        _Pragma("unroll") for (int i_ = 0; i_ < NLD; ++i_) {                                 \
            float4 v_ = rg[i_];                                                              \
            if (!kin_) v_ = make_float4(0.f, 0.f, 0.f, 0.f);                                 \
            if constexpr (HALF) {                                                            \
                *reinterpret_cast<f16x4*>(reinterpret_cast<char*>(lds) + (srow + 32 * i_) * (ROW_F * 4) + kq * 2) = \
                    f16x4{(_Float16)v_.x, (_Float16)v_.y, (_Float16)v_.z, (_Float16)v_.w};   \
            } else {                                                                         \
                *reinterpret_cast<float4*>(&lds[(srow + 32 * i_) * ROW_F + kq]) = v_;        \
            }                                                                                \
        }                                                                                    \
    }

    GNNLM_DENSE_LOAD(0)
    for (int kt = 0; kt < nk; ++kt) {
        GNNLM_DENSE_STORE(kt)
        __syncthreads();
        if (kt + 1 < nk) GNNLM_DENSE_LOAD(kt + 1)
        if constexpr (HALF) {
            const char* base = reinterpret_cast<const char*>(lds);
#pragma unroll
            for (int ks = 0; ks < BK / 16; ++ks) {
                f16x8 hx[TM], hw[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    hx[i] = *reinterpret_cast<const f16x8*>(base + (32 * i + l32) * (ROW_F * 4) + 32 * ks + 16 * half);
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    hw[j] = *reinterpret_cast<const f16x8*>(base + (BM + wave * WCOLS + 32 * j + l32) * (ROW_F * 4) + 32 * ks + 16 * half);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(hw[j], hx[i], acc[i][j], 0, 0, 0);
            }
        } else {
            const float* xb = &lds[l32 * ROW_F + 4 * half];
            const float* wb = &lds[(BM + wave * WCOLS + l32) * ROW_F + 4 * half];
#pragma unroll
            for (int s = 0; s < BK / 8; ++s) {
                float4 a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) a[i] = *reinterpret_cast<const float4*>(xb + 32 * i * ROW_F + 8 * s);
#pragma unroll
                for (int j = 0; j < TN; ++j) b[j] = *reinterpret_cast<const float4*>(wb + 32 * j * ROW_F + 8 * s);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[j].x, a[i].x, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[j].y, a[i].y, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[j].z, a[i].z, acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[j].w, a[i].w, acc[i][j], 0, 0, 0);
                    }
            }
        }
        __syncthreads();          // the next tile's store (or the epilogue's arrays) overwrite the buffer
    }
#undef GNNLM_DENSE_LOAD
#undef GNNLM_DENSE_STORE

    // ---- epilogue: lane (l32, half) holds, for row m0 + 32 i + l32 of x, the logits of the columns c0 + 32 j + rowidx(r, half) ----
    float* redm = lds;                    // [4][BM] per-wave row maxima
    float* reds = lds + 4 * BM;           // [4][BM] per-wave sums
    float* spick = lds + 8 * BM;          // [BM] the target's logit
    const int c0 = wave * WCOLS;
    constexpr float LOG2E = 1.44269504088896341f;
    bool t_ok[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int tok = 32 * i + l32;
        const int64_t t = tok < row_lim ? p.target[m0 + tok] : -1;
        t_ok[i] = t >= 0 && t < p.vocab;
        const int tl = t_ok[i] ? (int)t - c0 : -1;       // the target's column inside this wave's slab (when in [0, WCOLS))
        float amax = -INFINITY, pv = 0.f;
        bool found = false;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int cl = j * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                const int c = c0 + cl;
                float v = -INFINITY;
                if (c < p.vocab) v = acc[i][j][r] + (p.bias ? p.bias[c] : 0.f);
                acc[i][j][r] = v;
                amax = fmaxf(amax, v);
                if (cl == tl) { pv = v; found = true; }
            }
        {
            const gnnlm_u32x2 e = __builtin_amdgcn_permlane32_swap(__float_as_uint(amax), __float_as_uint(amax), false, false);
            amax = fmaxf(__uint_as_float(e.x), __uint_as_float(e.y));
        }
        if (half == 0) redm[wave * BM + tok] = amax;
        if (found) spick[tok] = pv;       // exactly one (wave, half) holds a valid target's column
    }
    __syncthreads();
    float gmax[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int tok = 32 * i + l32;
        gmax[i] = fmaxf(fmaxf(redm[tok], redm[BM + tok]), fmaxf(redm[2 * BM + tok], redm[3 * BM + tok]));   // column 0 is valid: finite
        const float nml = -(gmax[i] * LOG2E);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) s += __builtin_amdgcn_exp2f(fmaf(acc[i][j][r], LOG2E, nml));    // masked columns: exp2(-inf) = 0
        {
            const gnnlm_u32x2 e = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false);
            s = __uint_as_float(e.x) + __uint_as_float(e.y);
        }
        if (half == 0) reds[wave * BM + tok] = s;
    }
    __syncthreads();
    if (wave == 0 && half == 0) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int tok = 32 * i + l32;
            if (tok < row_lim) {
                const float sum = (reds[tok] + reds[BM + tok]) + (reds[2 * BM + tok] + reds[3 * BM + tok]);
                p.out[m0 + tok] = t_ok[i] ? (spick[tok] - gmax[i]) - logf(sum) : -INFINITY;
            }
        }
    }
}

template <int TM, int TN, bool HALF>
int launch_dense(const DenseArgs& a, hipStream_t stream) {
    constexpr size_t lds_bytes = dense_lds_bytes<TM, TN, HALF>();
    if constexpr (lds_bytes > 64 * 1024) GNNLM_LDS_OPT_IN((&dense_logp_kernel<TM, TN, HALF>), lds_bytes);
    hipLaunchKernelGGL((dense_logp_kernel<TM, TN, HALF>), dim3((unsigned)cdiv(a.n, 32 * TM)), dim3(256), lds_bytes, stream, a);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

// Rows per workgroup: W is re-read (from L2) by every workgroup, so its traffic per flop falls with the rows a workgroup owns --
// 32 TM rows, TM <= 4 for vocab <= 256 (128 accumulator registers), <= 2 above (the 512-column tile already holds 64 per row
// tile) -- as long as the grid still gives every CU two workgroups (256 CUs); short inputs keep 32-row workgroups.
// GNNLM_DENSE_TM = 1 | 2 | 4 overrides the choice (A/B runs).
int dense_tm(int64_t n, int tn) {
    static const int forced = [] { const char* e = getenv("GNNLM_DENSE_TM"); return e ? atoi(e) : 0; }();
    const int cap = tn <= 2 ? 4 : 2;
    if (forced == 1 || forced == 2 || forced == 4) return std::min(forced, cap);
    int tm = cap;
    while (tm > 1 && cdiv(n, 32 * tm) < 512) tm >>= 1;
    return tm;
}

template <bool HALF>
int launch_dense_any(const DenseArgs& a, hipStream_t stream) {
    const int tn = (a.vocab + 127) / 128, tm = dense_tm(a.n, tn);
#define GNNLM_DENSE_CASE(TM_, TN_) if (tm == TM_ && tn == TN_) return launch_dense<TM_, TN_, HALF>(a, stream);
    GNNLM_DENSE_CASE(1, 1) GNNLM_DENSE_CASE(2, 1) GNNLM_DENSE_CASE(4, 1)
    GNNLM_DENSE_CASE(1, 2) GNNLM_DENSE_CASE(2, 2) GNNLM_DENSE_CASE(4, 2)
    GNNLM_DENSE_CASE(1, 3) GNNLM_DENSE_CASE(2, 3)
    GNNLM_DENSE_CASE(1, 4) GNNLM_DENSE_CASE(2, 4)
#undef GNNLM_DENSE_CASE
    set_error("dense: no kernel for this tile");
    return E_INVALID;
}

// ---- general route: glue around gemm_nt / lse_reduce / row_lse_pick ----
// pick[r] = target[r] as the GEMM's int32 column, 0 for a target outside [0, vocab) (a readable column; the row ends as -inf)
__global__ void dense_pick_kernel(const int64_t* target, int64_t n, int vocab, int32_t* pick) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int64_t t = target[i];
        pick[i] = (t >= 0 && t < vocab) ? (int32_t)t : 0;
    }
}
__global__ void dense_finish_kernel(const float* picked, const float* lse, const int64_t* target, int64_t n, int vocab, float* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int64_t t = target[i];
        out[i] = (t >= 0 && t < vocab) ? picked[i] - lse[i] : -INFINITY;
    }
}

struct GeneralBufs {
    int32_t* pick;
    float *picked, *lse, *part, *logits;
};
int64_t logits_ld(int vocab) { return ((int64_t)vocab + 3) & ~3ll; }
// the workspace of the general route for chunks of `chunk` rows (with a bias) -> bytes
size_t carve_general(const gnnlm_dense_softmax_t& w, int64_t n, int64_t chunk, void* ws, GeneralBufs& b) {
    Carver c(ws);
    b.pick = c.take<int32_t>(n);
    b.picked = c.take<float>(n);
    b.lse = c.take<float>(n);
    b.part = b.logits = nullptr;
    if (w.bias) b.logits = c.take<float>(chunk * logits_ld(w.vocab));
    else b.part = c.take<float>(n * 4 * cdiv(w.vocab, 128));
    return c.off + 256;
}
int64_t default_chunk(const gnnlm_dense_softmax_t& w, int64_t n) {
    const int64_t fit = LOGITS_CAP / (logits_ld(w.vocab) * 4);
    return std::min(n, std::max(MIN_CHUNK_ROWS, fit / MIN_CHUNK_ROWS * MIN_CHUNK_ROWS));
}

// 0: invalid (message set), 1 / 2: the route the descriptor takes
int dense_route(const gnnlm_dense_softmax_t& w) {
    const bool one_ok = w.vocab <= MAX_ONE_LAUNCH_VOCAB && (w.gemm_precision == 0 || w.gemm_precision == 3);
    if (w.route == 1) return one_ok ? 1 : 0;
    if (w.route == 2) return 2;
    // auto: the one-launch kernel only where it measured at least as fast as the general route on the no-bias problem
    // (tools/dense_head_bench.py): fp16 operands up to 3 column tiles per wave (0.63-0.69 x the general route's
    // time at V = 205 / 260); at f32 it ties at V = 205 (0.97-1.04) and loses from V = 260 on (1.03-1.25), at V = 512 under both
    return one_ok && w.gemm_precision == 3 && w.vocab <= AUTO_ONE_LAUNCH_VOCAB ? 1 : 2;
}

int dense_validate(const gnnlm_dense_softmax_t& w) {
    GNNLM_REQUIRE(w.d > 0 && w.d % 4 == 0, "dense: d must be a positive multiple of 4");
    GNNLM_REQUIRE(w.vocab >= 1, "dense: vocab must be >= 1");
    GNNLM_REQUIRE(w.gemm_precision >= 0 && w.gemm_precision <= 3, "dense: gemm_precision must be 0, 1, 2 or 3");
    GNNLM_REQUIRE(w.route >= 0 && w.route <= 2, "dense: route must be 0 (auto), 1 (one launch) or 2 (general)");
    GNNLM_REQUIRE(dense_route(w) != 0, "dense: route 1 (the one-launch kernel) needs vocab <= 512 and gemm_precision 0 or 3");
    GNNLM_REQUIRE(w.w != nullptr, "dense: null weight");
    GNNLM_REQUIRE(w.ldw >= w.d && w.ldw % 4 == 0 && (uintptr_t)w.w % 16 == 0, "dense: w must be 16-byte aligned with ldw >= d, ldw % 4 == 0");
    return OK;
}

int dense_impl(const gnnlm_dense_softmax_t& w, const float* x, int64_t ldx, const int64_t* target, int64_t n, float* lm_logp,
               void* ws, size_t ws_bytes, hipStream_t s) {
    GNNLM_TRY(dense_validate(w));
    GNNLM_REQUIRE(n >= 0 && n < (1ll << 31), "dense: bad row count");
    const int route = dense_route(w);
    GeneralBufs b{};
    int64_t chunk = 0;
    if (route == 2) {                                   // the workspace is checked before any pointer is touched
        chunk = w.bias ? default_chunk(w, n) : 0;
        if (w.bias && n > 0 && carve_general(w, n, chunk, nullptr, b) > ws_bytes) {     // less than the default: as many rows as fit
            const size_t fixed = carve_general(w, n, 0, nullptr, b);
            const int64_t fit = ws_bytes > fixed ? (int64_t)((ws_bytes - fixed) / (size_t)(logits_ld(w.vocab) * 4)) : 0;
            chunk = std::min(chunk, fit / MIN_CHUNK_ROWS * MIN_CHUNK_ROWS);
            if (fit >= n) chunk = n;
        }
        GNNLM_REQUIRE(n == 0 || (ws && (!w.bias || chunk > 0) && carve_general(w, n, chunk, nullptr, b) <= ws_bytes),
                      "dense: workspace too small (see gnnlm_dense_workspace_bytes / gnnlm_dense_workspace_bytes_min)");
    }
    GNNLM_REQUIRE(x && target && lm_logp, "dense: null io");
    GNNLM_REQUIRE(ldx >= w.d && ldx % 4 == 0 && (uintptr_t)x % 16 == 0, "dense: x must be 16-byte aligned with ldx >= d, ldx % 4 == 0");
    if (n == 0) return OK;

    if (route == 1) {
        GNNLM_REQUIRE((int64_t)w.vocab * w.ldw < (1ll << 30) && 128 * ldx < (1ll << 30),
                      "dense: the one-launch kernel addresses a workgroup's rows with 32-bit offsets (vocab * ldw, 128 * ldx < 2^30)");
        DenseArgs a{x, ldx, w.w, w.ldw, w.bias, target, n, w.d, w.vocab, lm_logp};
        ProfScope prof(K_GEMM, s, 2.0 * n * (double)w.vocab * w.d, 4.0 * ((double)n * w.d + (double)w.vocab * w.d + n));
        return w.gemm_precision == 3 ? launch_dense_any<true>(a, s) : launch_dense_any<false>(a, s);
    }

    carve_general(w, n, chunk, ws, b);
    GemmPrecisionScope prec_scope(w.gemm_precision);
    const unsigned blocks = (unsigned)cdiv(n, 256);
    hipLaunchKernelGGL(dense_pick_kernel, dim3(blocks), dim3(256), 0, s, target, n, w.vocab, b.pick);
    GNNLM_LAUNCH_CHECK();
    if (!w.bias) {                                      // the adaptive head's own path: logits reduced in the epilogue, never written
        GemmParams g{};
        g.A = x; g.lda = ldx; g.W = w.w; g.ldw = w.ldw;
        g.lse_part = b.part; g.lse_pick = b.pick; g.lse_picked = b.picked;
        g.M = (int)n; g.N = w.vocab; g.K = w.d;
        if (n >= 1024) g.tile_order = 2 + 4;            // as the adaptive head (adaptive_logp.hip): bands of 4 m-tiles
        GNNLM_TRY(gemm_nt(g, s));
        GNNLM_TRY(lse_reduce(b.part, 2 * (int)cdiv(w.vocab, 128), n, nullptr, b.lse, s));
    } else {                                            // xl_bias: logits of a chunk of rows through the workspace
        const int64_t ldc = logits_ld(w.vocab);
        for (int64_t r0 = 0; r0 < n; r0 += chunk) {
            const int64_t rows = std::min(chunk, n - r0);
            GemmParams g{};
            g.A = x + r0 * ldx; g.lda = ldx; g.W = w.w; g.ldw = w.ldw;
            g.C = b.logits; g.ldc = ldc; g.bias = w.bias; g.bias_mode = 1;
            g.M = (int)rows; g.N = w.vocab; g.K = w.d;
            GNNLM_TRY(gemm_nt(g, s));
            GNNLM_TRY(row_lse_pick(b.logits, ldc, rows, nullptr, w.vocab, b.pick + r0, b.lse + r0, b.picked + r0, s));
        }
    }
    hipLaunchKernelGGL(dense_finish_kernel, dim3(blocks), dim3(256), 0, s, b.picked, b.lse, target, n, w.vocab, lm_logp);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

size_t dense_workspace(const gnnlm_dense_softmax_t* w, int64_t n, bool least) {
    if (!w || n <= 0 || w->vocab < 1 || w->d <= 0 || w->gemm_precision < 0 || w->gemm_precision > 3 || w->route < 0 || w->route > 2) return 0;
    if (dense_route(*w) != 2) return 0;
    GeneralBufs b{};
    const int64_t chunk = w->bias ? (least ? std::min(n, MIN_CHUNK_ROWS) : default_chunk(*w, n)) : 0;
    return carve_general(*w, n, chunk, nullptr, b);
}

}  // namespace
}  // namespace gnnlm

using namespace gnnlm;

extern "C" {

size_t gnnlm_dense_workspace_bytes(const gnnlm_dense_softmax_t* w, int64_t n) { return dense_workspace(w, n, false); }
size_t gnnlm_dense_workspace_bytes_min(const gnnlm_dense_softmax_t* w, int64_t n) { return dense_workspace(w, n, true); }
int gnnlm_dense_target_logp(const gnnlm_dense_softmax_t* w, const float* x, int64_t ldx, const int64_t* target, int64_t n,
                            float* lm_logp, void* workspace, size_t workspace_bytes, void* stream) {
    GNNLM_DESC(w);
    return dense_impl(*w, x, ldx, target, n, lm_logp, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
