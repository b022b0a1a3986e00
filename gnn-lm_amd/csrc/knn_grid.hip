// kNN-LM tuning grid: every point of ks x temperatures x lmbdas from ONE read of a search result.
//
// knn_interp_grid_kernel is knn_interp_regs_kernel (rowops.hip) with the three knobs turned into loops over registers: one
// wave per token, a lane loads its (id, sim, label) columns lane + 64 j once, folds the -1 mask into the similarity and the
// target match into one bit per column, and then walks the grid.  A point (k', t, l) is what gnnlm_knn_interp returns for the
// first k' columns -- same column order per lane, maximum over the prefix, sv / t as a division, same wave reductions, same
// float32 log(1 - l) / log(l) from the host -- so the two agree bit for bit where both are defined (0 < l < 1).  The ends
// l = 0 / l = 1 need no special case: log 0 = -inf drops its term out of m + logf(expf(a - m) + expf(b - m)).
//
// Labels come with the neighbours (knn_vals: the IVF-PQ search delivers them) or from the label table by the plain 4-byte
// gather with the n_store / row0 / n_local rules of the single-setting kernel.  The tag table and the routed look-ups of
// knn_bucket.hip are NOT part of this kernel: a sweep over a label table of hundreds of MB pays the one-by-one gathers.
//
// Several language-model rows (gnnlm_knn_interp_grid_lm: the base-LM / GNN mixture at n_lm ratios, transformer.py:1056-1077):
// nothing of a (k', t) pair but its final mixes depends on the lm row, so the exponentials, the prefix sums and the wave
// reductions are computed once per pair and the n_lm * n_l mixes are spread over the lanes (lane a * n_l + l mixes lm row a
// with lmbda l; more than 64 of them take a second round).  n_lm = 1 is the plain grid, lane for lane.
//
// rows_sum_f64_kernel adds up every row of the [G, n] result in one launch, each row in masked_sum_f64_kernel's order.
#include "kernels.h"

namespace gnnlm {

namespace {

constexpr int GRID_KS = 8, GRID_T = 16, GRID_L = 16;      // capacities of gnnlm_knn_interp_grid_t

struct KnnGridParams {
    const float* lm_logp;  int n_lm;  int64_t ld_lm;  const float* sims;  const int64_t* ids;
    const void* vals;  int vals_itemsize;  int64_t n_store, row0, n_local;
    const int32_t* knn_vals;  const int64_t* targets;
    int64_t n;  int k;
    int n_ks, n_t, n_l;
    int ks[GRID_KS];  float t[GRID_T];  float log_1ml[GRID_L], log_l[GRID_L];
    float* out_logp;  float* out_pknn;  int64_t* out_recall;
};

// one wave per token; k <= 64 * JMAX
template <int JMAX>
__global__ __launch_bounds__(256) void knn_interp_grid_kernel(KnnGridParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= p.n) return;
    const float* sims = p.sims + i * p.k;
    const int64_t* ids = p.ids + i * p.k;
    int64_t id[JMAX];
    float sv[JMAX];
    int64_t val[JMAX];
#pragma unroll
    for (int t = 0; t < JMAX; ++t) {
        const int j = lane + 64 * t;
        id[t] = j < p.k ? ids[j] : -1;
        sv[t] = j < p.k ? sims[j] : 0.f;
    }
    const int64_t tgt = p.targets[i];
#pragma unroll
    for (int t = 0; t < JMAX; ++t) {
        const int j = lane + 64 * t;
        val[t] = -1;
        if (j < p.k) {
            if (p.knn_vals) {
                val[t] = p.knn_vals[i * p.k + j];
            } else {
                // numpy indexing semantics of vals[knns] (knn_model.py:198): -1 wraps to the last row
                const int64_t row = (id[t] < 0 ? id[t] + p.n_store : id[t]) - p.row0;
                if (row >= 0 && row < p.n_local)
                    val[t] = p.vals_itemsize == 2 ? (int64_t) reinterpret_cast<const int16_t*>(p.vals)[row]
                                                  : (int64_t) reinterpret_cast<const int32_t*>(p.vals)[row];
            }
        }
    }
    // everything the grid needs from the loads: the masked similarity (knn_model.py:193) and one hit bit per column (:211)
    unsigned hits = 0;
#pragma unroll
    for (int t = 0; t < JMAX; ++t) {
        sv[t] = id[t] == -1 ? -1e10f : sv[t];
        if (lane + 64 * t < p.k && val[t] == tgt) hits |= 1u << t;
    }
    // mix `m` = a * n_l + l (lm row a, lmbda l) belongs to lane m % 64 in round m / 64: the lane keeps that lmbda's two coefficients,
    // that row's log-prob of the token and the mix's row of the result (without the (k', t) pair's offset)
    const int n_mix = p.n_lm * p.n_l;                      // <= 8 * 16: two rounds at most
    const int G = p.n_ks * p.n_t * p.n_l;
    float c_1ml[2] = {0.f, 0.f}, c_l[2] = {0.f, 0.f}, lm[2] = {0.f, 0.f};
    int out_row[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int m = lane + 64 * r;
        if (m < n_mix) {
            const int a = m / p.n_l, my_l = m - a * p.n_l;
            for (int li = 0; li < p.n_l; ++li)
                if (my_l == li) { c_1ml[r] = p.log_1ml[li]; c_l[r] = p.log_l[li]; }
            lm[r] = p.lm_logp[(int64_t)a * p.ld_lm + i];
            out_row[r] = a * G + my_l;
        }
    }

    if (p.out_recall)
        for (int ki = 0; ki < p.n_ks; ++ki) {
            const int kp = p.ks[ki];
            int rec = 0;
#pragma unroll
            for (int t = 0; t < JMAX; ++t)
                if (lane + 64 * t < kp) rec += (hits >> t) & 1u;
            rec = (int)wave_sum((float)rec);
            if (lane == 0) p.out_recall[(int64_t)ki * p.n + i] = rec;
        }

    for (int ti = 0; ti < p.n_t; ++ti) {
        const float temperature = p.t[ti];
        float s[JMAX];
#pragma unroll
        for (int t = 0; t < JMAX; ++t) s[t] = sv[t] / temperature;                      // :196
        for (int ki = 0; ki < p.n_ks; ++ki) {
            const int kp = p.ks[ki];
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < JMAX; ++t)
                if (lane + 64 * t < kp) mx = fmaxf(mx, s[t]);
            mx = wave_max(mx);
            float den = 0.f, num = 0.f;
#pragma unroll
            for (int t = 0; t < JMAX; ++t) {
                if (lane + 64 * t < kp) {
                    const float e = expf(s[t] - mx);
                    const bool hit = (hits >> t) & 1u;
                    den += e;
                    num += hit ? e : 0.f;
                }
            }
            den = wave_sum(den);
            num = wave_sum(num);
            const float pk = num / den;
            const int64_t kt = (int64_t)ki * p.n_t + ti;
            if (lane == 0 && p.out_pknn) p.out_pknn[kt * p.n + i] = pk;
            const float lpk = logf(pk + 1e-10f);
#pragma unroll
            for (int r = 0; r < 2; ++r)
                if (lane + 64 * r < n_mix) {
                    // sequence_scorer.py:55-68 with knn_probs = log(p + 1e-10) (:121)
                    const float a = lm[r] + c_1ml[r];
                    const float b = lpk + c_l[r];
                    const float m = fmaxf(a, b);
                    p.out_logp[(kt * p.n_l + out_row[r]) * p.n + i] = m + logf(expf(a - m) + expf(b - m));
                }
        }
    }
}

__global__ __launch_bounds__(1024) void rows_sum_f64_kernel(const float* x, int64_t ld, int64_t n, double* out) {
    __shared__ double red[1024];
    x += (int64_t)blockIdx.x * ld;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += (double)x[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] += red[0];
}

}  // namespace

int knn_interp_grid(const gnnlm_knn_interp_grid_t& d, int n_lm, int64_t ld_lm, hipStream_t stream) {
    GNNLM_REQUIRE(n_lm >= 1 && n_lm <= 8, "knn_interp_grid: 1 .. 8 lm rows per call");
    GNNLM_REQUIRE(n_lm == 1 || ld_lm >= d.n, "knn_interp_grid: the lm rows overlap (ld_lm < n)");
    GNNLM_REQUIRE(d.lm_logp && d.sims && d.ids && d.targets && d.out_logp, "knn_interp_grid: null operand");
    GNNLM_REQUIRE(d.knn_vals || d.vals, "knn_interp_grid: need vals or pre-fetched knn_vals");
    GNNLM_REQUIRE(d.knn_vals || (d.n_local > 0 && d.n_store > 0 && d.row0 >= 0), "knn_interp_grid: vals needs n_store / row0 / n_local");
    GNNLM_REQUIRE(d.vals_itemsize == 2 || d.vals_itemsize == 4, "knn_interp_grid: vals must be int16 or int32");
    GNNLM_REQUIRE(d.n >= 0 && d.k > 0, "knn_interp_grid: need n >= 0, k > 0");
    GNNLM_REQUIRE(d.k <= 1024, "knn_interp_grid: k > 1024 is not built (gnnlm_knn_interp serves it, one setting per call)");
    GNNLM_REQUIRE(d.n_ks >= 1 && d.n_ks <= GRID_KS, "knn_interp_grid: 1 .. 8 values of k per call");
    GNNLM_REQUIRE(d.n_temperatures >= 1 && d.n_temperatures <= GRID_T, "knn_interp_grid: 1 .. 16 temperatures per call");
    GNNLM_REQUIRE(d.n_lmbdas >= 1 && d.n_lmbdas <= GRID_L, "knn_interp_grid: 1 .. 16 lmbdas per call");
    KnnGridParams p{};
    for (int j = 0; j < d.n_ks; ++j) {
        GNNLM_REQUIRE(d.ks[j] >= 1 && d.ks[j] <= d.k, "knn_interp_grid: every k' must lie in 1 .. k");
        p.ks[j] = d.ks[j];
    }
    for (int j = 0; j < d.n_temperatures; ++j) {
        GNNLM_REQUIRE(d.temperatures[j] > 0.f, "knn_interp_grid: every temperature must be > 0");
        p.t[j] = d.temperatures[j];
    }
    for (int j = 0; j < d.n_lmbdas; ++j) {
        GNNLM_REQUIRE(d.lmbdas[j] >= 0.0 && d.lmbdas[j] <= 1.0, "knn_interp_grid: every lmbda must lie in 0 .. 1");
        // float32 roundings of the float64 logs, as in coeffs[0] = np.log(1 - coeff); log 0 = -inf at the two ends
        p.log_1ml[j] = (float)log(1.0 - d.lmbdas[j]);
        p.log_l[j] = (float)log(d.lmbdas[j]);
    }
    if (d.n == 0) return OK;
    GNNLM_REQUIRE(cdiv(d.n, 4) < (1ll << 31), "knn_interp_grid: too many tokens for one launch");
    p.lm_logp = d.lm_logp, p.n_lm = n_lm, p.ld_lm = n_lm == 1 ? 0 : ld_lm, p.sims = d.sims, p.ids = d.ids;
    p.vals = d.vals, p.vals_itemsize = d.vals_itemsize, p.n_store = d.n_store, p.row0 = d.row0, p.n_local = d.n_local;
    p.knn_vals = d.knn_vals, p.targets = d.targets;
    p.n = d.n, p.k = d.k;
    p.n_ks = d.n_ks, p.n_t = d.n_temperatures, p.n_l = d.n_lmbdas;
    p.out_logp = d.out_logp, p.out_pknn = d.out_pknn, p.out_recall = d.out_recall;
    const double G = (double)n_lm * d.n_ks * d.n_temperatures * d.n_lmbdas;
    ProfScope prof(K_KNN_GRID, stream, 0.0,
                   (double)d.n * d.k * (12.0 + (d.knn_vals ? 4.0 : d.vals_itemsize)) + (8.0 + 4.0 * n_lm + 4.0 * G) * d.n);
    const dim3 grid((unsigned)cdiv(d.n, 4)), block(256);
    if (d.k <= 256) hipLaunchKernelGGL(knn_interp_grid_kernel<4>, grid, block, 0, stream, p);
    else hipLaunchKernelGGL(knn_interp_grid_kernel<16>, grid, block, 0, stream, p);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int rows_sum_f64(const float* x, int64_t ld, int64_t rows, int64_t n, double* out, hipStream_t stream) {
    GNNLM_REQUIRE(rows >= 0 && n >= 0 && ld >= n && rows < (1ll << 31), "rows_sum_f64: bad shape");
    if (rows == 0) return OK;
    GNNLM_REQUIRE(x && out, "rows_sum_f64: null");
    hipLaunchKernelGGL(rows_sum_f64_kernel, dim3((unsigned)rows), dim3(1024), 0, stream, x, ld, n, out);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
