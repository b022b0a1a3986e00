// Exact kNN-LM similarities: recompute the similarity of every retrieved neighbour from its stored key (knn_model.py:161-175).
//
// knn_resim_kernel: one wave per (query, run of 64 neighbours).  The query row lives in registers; element e of a row belongs
// to lane (e / 8) % 64, chunk e / 512, so that a wave instruction reads 1 KiB of one fp16 row with 16 bytes per lane.  ROWS key
// rows are in flight per wave.  The row of neighbour j is wave-uniform (v_readlane of the id that lane j loaded), so an id out
// of range skips its loads as a scalar branch.
//
// ONE summation order for every shape, dtype, stride and mode: a lane runs one fma chain over its elements in ascending e,
// always 8 per chunk, elements at or beyond d standing in as exact zeros (fma(0, 0, acc) == acc); then a fixed 64-lane tree
// (the DPP / permlane-swap steps of common.h's wave_sum on 64-bit values).  The chains and the tree run in float64 (full-rate
// v_fma_f64 on this part; the kernel stays far from VALU-bound) and a result is rounded to float32 ONCE, after the division by
// the key norm where there is one: it is within half a float32 ulp (+ 2^-40) of the exact value whatever cancels inside the sum.  How a lane's 8 elements are fetched (one or two 16-byte loads when the row start is 16-byte aligned and the 8
// elements lie inside the row, element-wise loads otherwise) changes no value, so a result is a function of its query row and
// its key row only: not of n, k, the column, the neighbours beside it, direct or indexed mode, or the row stride.
//
// The lane that holds result j is lane j of the run: one coalesced 256-byte store per wave.
#include <float.h>
#include <hip/hip_fp16.h>

#include "kernels.h"

namespace gnnlm {

namespace {

struct KnnResimParams {
    const float* q;  int64_t ldq;
    const int64_t* ids;  int64_t ld_ids;
    const void* keys;  int64_t ld_keys, n_rows;
    int d;  int64_t n;  int k;
    int normalize;
    float* out;  int64_t ld_out;
    int n_seg;                     // runs of 64 neighbours per query
    int q_vec, key_vec;            // 16-byte loads are legal for every query row / key row start
};

typedef float resim_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 resim_f16x8 __attribute__((ext_vector_type(8)));

// wave_sum of common.h, step for step, on doubles (two 32-bit DPP moves / swaps per step)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)u, (int)(unsigned)u, CTRL, 0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(u >> 32), (int)(unsigned)(u >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += dpp_f64<0xB1>(v);       // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);       // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);      // row_half_mirror
    v += dpp_f64<0x140>(v);      // row_mirror
    {
        const uint64_t u = (uint64_t)__double_as_longlong(v);
        const gnnlm_u32x2 lo = __builtin_amdgcn_permlane16_swap((unsigned)u, (unsigned)u, false, false);
        const gnnlm_u32x2 hi = __builtin_amdgcn_permlane16_swap((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);
        v = __longlong_as_double((long long)(((uint64_t)hi.x << 32) | lo.x)) + __longlong_as_double((long long)(((uint64_t)hi.y << 32) | lo.y));
    }
    {
        const uint64_t u = (uint64_t)__double_as_longlong(v);
        const gnnlm_u32x2 lo = __builtin_amdgcn_permlane32_swap((unsigned)u, (unsigned)u, false, false);
        const gnnlm_u32x2 hi = __builtin_amdgcn_permlane32_swap((unsigned)(u >> 32), (unsigned)(u >> 32), false, false);
        v = __longlong_as_double((long long)(((uint64_t)hi.x << 32) | lo.x)) + __longlong_as_double((long long)(((uint64_t)hi.y << 32) | lo.y));
    }
    return v;
}

typedef float resim_f32x8 __attribute__((ext_vector_type(8)));
template <typename T> struct Raw8;
template <> struct Raw8<_Float16> { typedef resim_f16x8 type; };
template <> struct Raw8<float> { typedef resim_f32x8 type; };

// row[e0 .. e0 + 8) as stored (the widening happens where a value is used: 4 / 8 registers per row piece in flight), exact
// zeros at and beyond d
template <typename T>
__device__ __forceinline__ typename Raw8<T>::type load8(const T* __restrict__ row, int e0, int d, bool vec) {
    typename Raw8<T>::type v;
    if (vec && e0 + 8 <= d) {
        if constexpr (sizeof(T) == 2) {
            v = *reinterpret_cast<const resim_f16x8*>(row + e0);
        } else {
            const resim_f32x4 a = *reinterpret_cast<const resim_f32x4*>(row + e0);
            const resim_f32x4 b = *reinterpret_cast<const resim_f32x4*>(row + e0 + 4);
            v = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
        }
    } else {
#pragma unroll
        for (int t = 0; t < 8; ++t) v[t] = e0 + t < d ? row[e0 + t] : (T)0;
    }
    return v;
}

// NCH > 0: d <= 512 * NCH (<= 1024), the query stays in registers as doubles.  NCH == 0: any d, a query chunk is re-read (L1 / L2)
// per group of key rows -- the registers of a wider query would cost the occupancy the gather lives on.
template <typename T, int NCH, int ROWS, int METRIC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void knn_resim_kernel(KnnResimParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t i = w / p.n_seg;
    if (i >= p.n) return;
    const int j0 = (int)(w % p.n_seg) * 64;
    const int cnt = min(64, p.k - j0);
    const int d = p.d;
    const float* __restrict__ qrow = p.q + i * p.ldq;
    const int nch = NCH > 0 ? NCH : (d + 511) / 512;

    // the run's rows: lane j resolves neighbour j0 + j to a key row, or -1 (touch nothing, -FLT_MAX)
    int64_t row = -1;
    if (lane < cnt) {
        if (p.ids) {
            const int64_t id = p.ids[i * p.ld_ids + j0 + lane];
            row = id < 0 ? id + p.n_rows : id;                  // numpy's wrap of a negative index
            if (row < 0 || row >= p.n_rows) row = -1;
        } else {
            row = i * p.k + j0 + lane;                          // direct mode (n * k <= n_rows is checked on the host)
        }
    }

    double q[NCH > 0 ? NCH : 1][8];
    if constexpr (NCH > 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const resim_f32x8 qf = load8<float>(qrow, c * 512 + lane * 8, d, p.q_vec);
#pragma unroll
            for (int t = 0; t < 8; ++t) q[c][t] = (double)qf[t];
        }
    }

    double res = 0.0, res_nrm = 1.0;        // lane j: the sum and the squared key norm of neighbour j0 + j
    bool res_ok = false;
    for (int jb = 0; jb < cnt; jb += ROWS) {
        const T* krow[ROWS];
        bool ok[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int j = min(jb + r, cnt - 1);                 // a short last group repeats its last row (cached)
            const unsigned lo = __builtin_amdgcn_readlane((unsigned)(uint64_t)row, j);
            const unsigned hi = __builtin_amdgcn_readlane((unsigned)((uint64_t)row >> 32), j);
            const int64_t rr = (int64_t)(((uint64_t)hi << 32) | lo);
            ok[r] = rr >= 0;
            krow[r] = reinterpret_cast<const T*>(p.keys) + (ok[r] ? rr : 0) * p.ld_keys;
        }
        double acc[ROWS], nrm[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[r] = 0.0, nrm[r] = 0.0;
        if constexpr (NCH > 0) {
            typename Raw8<T>::type kv[ROWS][NCH];
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    if (ok[r]) kv[r][c] = load8<T>(krow[r], c * 512 + lane * 8, d, p.key_vec);
                    else kv[r][c] = (T)0;
                }
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
#pragma unroll
                for (int c = 0; c < NCH; ++c)
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const double kx = (double)(float)kv[r][c][t];
                        if constexpr (METRIC == 0) {
                            acc[r] = fma(kx, q[c][t], acc[r]);
                            nrm[r] = fma(kx, kx, nrm[r]);
                        } else {
                            const double df = q[c][t] - kx;
                            acc[r] = fma(df, df, acc[r]);
                        }
                    }
        } else {
            for (int c = 0; c < nch; ++c) {
                const resim_f32x8 qc = load8<float>(qrow, c * 512 + lane * 8, d, p.q_vec);
                typename Raw8<T>::type kv[ROWS];
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    if (ok[r]) kv[r] = load8<T>(krow[r], c * 512 + lane * 8, d, p.key_vec);
                    else kv[r] = (T)0;
                }
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
#pragma unroll
                    for (int t = 0; t < 8; ++t) {
                        const double kx = (double)(float)kv[r][t], qx = (double)qc[t];
                        if constexpr (METRIC == 0) {
                            acc[r] = fma(kx, qx, acc[r]);
                            nrm[r] = fma(kx, kx, nrm[r]);
                        } else {
                            const double df = qx - kx;
                            acc[r] = fma(df, df, acc[r]);
                        }
                    }
            }
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const double s = wave_sum_f64(acc[r]);
            double s2 = 1.0;
            if constexpr (METRIC == 0) {
                if (p.normalize) s2 = wave_sum_f64(nrm[r]);
            }
            if (lane == jb + r) res = s, res_nrm = s2, res_ok = ok[r];
        }
    }
    // one division and one rounding per result, by the lane that holds it
    if constexpr (METRIC == 0) {
        if (p.normalize) res = res / sqrt(res_nrm);                     // knn_model.py:172-173
    } else {
        res = -res;                                                     // :166
    }
    if (lane < cnt) p.out[i * p.ld_out + j0 + lane] = res_ok ? (float)res : -FLT_MAX;
}

template <typename T, int ROWS, int METRIC>
void launch(const KnnResimParams& p, hipStream_t stream) {
    const dim3 grid((unsigned)cdiv(p.n * p.n_seg, 4)), block(256);
    if (p.d <= 512) hipLaunchKernelGGL((knn_resim_kernel<T, 1, ROWS, METRIC>), grid, block, 0, stream, p);
    else if (p.d <= 1024) hipLaunchKernelGGL((knn_resim_kernel<T, 2, ROWS, METRIC>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((knn_resim_kernel<T, 0, ROWS, METRIC>), grid, block, 0, stream, p);
}

}  // namespace

int knn_recompute_sims(const gnnlm_knn_resim_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.d >= 1 && d.n >= 0 && d.k >= 1, "knn_recompute_sims: need d >= 1, n >= 0, k >= 1");
    GNNLM_REQUIRE(d.keys_itemsize == 2 || d.keys_itemsize == 4, "knn_recompute_sims: keys must be fp16 (2) or f32 (4)");
    GNNLM_REQUIRE(d.metric == 0 || d.metric == 1, "knn_recompute_sims: metric is 0 (ip) or 1 (l2)");
    GNNLM_REQUIRE(d.normalize_keys == 0 || d.metric == 0, "knn_recompute_sims: l2 never normalises keys");
    GNNLM_REQUIRE(d.ldq >= d.d && d.ld_keys >= d.d && d.ld_out >= d.k, "knn_recompute_sims: a row stride is shorter than its row");
    GNNLM_REQUIRE(d.ids == nullptr || d.ld_ids >= d.k, "knn_recompute_sims: ld_ids < k");
    GNNLM_REQUIRE(d.n_rows >= 0, "knn_recompute_sims: n_rows < 0");
    GNNLM_REQUIRE(d.ids != nullptr || d.n <= d.n_rows / d.k, "knn_recompute_sims: direct mode needs n * k rows of keys");
    if (d.n == 0) return OK;
    GNNLM_REQUIRE(d.queries && d.out, "knn_recompute_sims: null operand");
    GNNLM_REQUIRE(d.keys || d.n_rows == 0, "knn_recompute_sims: null keys");
    KnnResimParams p{};
    p.q = d.queries, p.ldq = d.ldq, p.ids = d.ids, p.ld_ids = d.ld_ids;
    p.keys = d.keys, p.ld_keys = d.ld_keys, p.n_rows = d.n_rows;
    p.d = d.d, p.n = d.n, p.k = d.k, p.normalize = d.normalize_keys;
    p.out = d.out, p.ld_out = d.ld_out;
    p.n_seg = (int)cdiv(d.k, 64);
    GNNLM_REQUIRE(cdiv(d.n * p.n_seg, 4) < (1ll << 31), "knn_recompute_sims: too many (query, neighbour) pairs for one launch");
    p.q_vec = (reinterpret_cast<uintptr_t>(d.queries) % 16 == 0) && (d.ldq % 4 == 0);
    p.key_vec = (reinterpret_cast<uintptr_t>(d.keys) % 16 == 0) && (d.ld_keys % (16 / d.keys_itemsize) == 0);
    ProfScope prof(K_KNN_RESIM, stream, 2.0 * d.n * d.k * d.d,
                   (double)d.n * d.k * ((double)d.d * d.keys_itemsize + 12.0) + 4.0 * d.n * d.d);
    if (d.keys_itemsize == 2) {
        if (d.metric == 0) launch<_Float16, 4, 0>(p, stream);
        else launch<_Float16, 4, 1>(p, stream);
    } else {
        if (d.metric == 0) launch<float, 2, 0>(p, stream);
        else launch<float, 2, 1>(p, stream);
    }
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
