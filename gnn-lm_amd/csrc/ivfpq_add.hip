// Adding keys to an IVF-PQ index (the add phase of faiss's IndexIVFPQ behind knn/index_builder.py:97-109, `add_with_ids`): the
// residual PQ encode of rows whose list is known, and the merge of the new rows behind the old rows of their lists.
//
//   ivfpq_encode_rows: codes[r][m] = argmin_c norm2[m][c] - 2 <x[r]_m - coarse[assign[r]]_m, pq[m][c]>, the dot product an fmaf
//     chain over e ascending from 0, the residual rounded to float32 once, ties to the lowest c: gnnlm_pq_encode's arithmetic on
//     the materialised residual, bit for bit.  A workgroup of 256 threads owns a TILE of 64 rows and walks the sub-quantizers; per
//     step (one sub-quantizer, up to 16 of its dimensions) the 256 x 16 centroid slice and the tile's residuals stand in LDS,
//     TRANSPOSED ([e][c], [e][row]: a lane's 4 centroids / 8 rows are one 16-byte read each, lanes next to each other 16 bytes
//     apart), and every thread keeps 8 rows x 8 centroids of running dot products in registers: 64 FMAs (v_pk_fma_f32, two IEEE FMAs
//     per lane) per 4 LDS reads.  Centroid bytes leave the cache once per tile, not once per key.  The next step's global loads are
//     issued before the arithmetic of this one and land in LDS after it.  Two workgroups per CU (218 VGPRs, no scratch): one per CU
//     measured 1.8x slower.  The argmin of a row is two DPP reductions over the 32 lanes of its row group (the smallest value, then
//     the lowest index that has it).  (The f32 matrix instructions run at the vector rate on this chip: nothing to gain from
//     them here, plain FMAs.)
//   ivfpq_list_merge: one pass, 16 bytes of a code row per thread; an old row finds its list by bisection of the old offsets.
#include "kernels.h"

namespace gnnlm {
namespace {

constexpr int ENC_ROWS = 64;          // rows of a tile
constexpr int ENC_EC = 16;            // dimensions of a sub-quantizer per step
constexpr int ENC_LDP = 256 + 4;      // floats per [e] row of the centroid slice (the pad spreads the staging stores over the banks)
constexpr int ENC_LDX = ENC_ROWS + 4; // ... of the residual tile
constexpr int ENC_UNROLL = 2;         // dimensions whose operands are in flight (4: 256 registers and spills; 1 and 4 measured slower)

__global__ __launch_bounds__(256, 2) void ivfpq_encode_rows_kernel(gnnlm_ivfpq_encode_t p) {
    __shared__ __attribute__((aligned(16))) float s_pq[ENC_EC * ENC_LDP];
    __shared__ __attribute__((aligned(16))) float s_x[ENC_EC * ENC_LDX];
    __shared__ float s_n2[256];
    __shared__ int s_list[ENC_ROWS];                                  // the row's list, -1: no such row / list

    const int t = threadIdx.x;
    const int tc = t & 31, tr = t >> 5;                               // centroids 4 tc .. + 3 and 128 + 4 tc .. + 3, rows 8 tr .. + 7
    const int64_t row0 = (int64_t)blockIdx.x * ENC_ROWS;
    const int dsub = p.dsub, M = p.M;
    const int n_chunks = (dsub + ENC_EC - 1) / ENC_EC;

    if (t < ENC_ROWS) {
        const int64_t r = row0 + t;
        int l = -1;
        if (r < p.n) {
            const int64_t a = p.assign[r];
            if (a >= 0 && a < p.nlist) {
                l = (int)a;
                if (p.list_cnt) atomicAdd(reinterpret_cast<unsigned long long*>(p.list_cnt) + a, 1ull);
            } else if (p.n_bad) {
                atomicAdd(p.n_bad, 1);
            }
        }
        s_list[t] = l;
    }
    __syncthreads();

    // what a thread stages per step: dimension te of centroids tq + 16 k (16 values) and of rows tq + 16 k (4 values) of the tile
    const int te = t & 15, tq = t >> 4;
    float g_pq[16], g_x[4], g_n2 = 0.f;
    auto fetch = [&](int m, int ch) {
        const int e0 = ch * ENC_EC;
        const bool live = e0 + te < dsub;
        const float* cen = p.pq + ((int64_t)m * 256 + tq) * dsub + e0 + te;
#pragma unroll
        for (int k = 0; k < 16; ++k) g_pq[k] = live ? cen[(int64_t)k * 16 * dsub] : 0.f;
        const int64_t col = (int64_t)m * dsub + e0 + te;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = tq + 16 * k, l = s_list[r];
            g_x[k] = live && l >= 0 ? p.x[(row0 + r) * p.ldx + col] - p.coarse[(int64_t)l * p.d + col] : 0.f;
        }
        if (ch == 0) g_n2 = p.norm2[m * 256 + t];
    };
    auto stage = [&](int ch) {
#pragma unroll
        for (int k = 0; k < 16; ++k) s_pq[te * ENC_LDP + tq + 16 * k] = g_pq[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) s_x[te * ENC_LDX + tq + 16 * k] = g_x[k];
        if (ch == 0) s_n2[t] = g_n2;
    };

    fetch(0, 0);
    for (int m = 0; m < M; ++m) {
        float acc[8][8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
        for (int ch = 0; ch < n_chunks; ++ch) {
            __syncthreads();                                          // the previous step's readers are done with LDS
            stage(ch);
            __syncthreads();
            if (ch + 1 < n_chunks) fetch(m, ch + 1);
            else if (m + 1 < M) fetch(m + 1, 0);
            const int ec = min(ENC_EC, dsub - ch * ENC_EC);
            for (int e4 = 0; e4 < ec; e4 += ENC_UNROLL) {                       // (ec % 4 == 0)
#pragma unroll
                for (int u = 0; u < ENC_UNROLL; ++u) {
                    const int e = e4 + u;
                    const float4 xa = *reinterpret_cast<const float4*>(&s_x[e * ENC_LDX + tr * 8]);
                    const float4 xb = *reinterpret_cast<const float4*>(&s_x[e * ENC_LDX + tr * 8 + 4]);
                    const float4 ca = *reinterpret_cast<const float4*>(&s_pq[e * ENC_LDP + tc * 4]);
                    const float4 cb = *reinterpret_cast<const float4*>(&s_pq[e * ENC_LDP + 128 + tc * 4]);
                    const float xv[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
                    const float cv[8] = {ca.x, ca.y, ca.z, ca.w, cb.x, cb.y, cb.z, cb.w};
#pragma unroll
                    for (int i = 0; i < 8; ++i)
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[i][j] = fmaf(xv[i], cv[j], acc[i][j]);
                }
            }
        }
        // smallest distance, lowest index on ties: the smallest value over the thread's eight and the row group's 32 lanes (DPP, no LDS),
        // then the lowest index among the centroids that have it (indices <= 255 are exact as floats)
        float n2[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) n2[j] = s_n2[(j >> 2) * 128 + tc * 4 + (j & 3)];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float dis[8], best = INFINITY;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                dis[j] = n2[j] - 2.f * acc[i][j];
                best = dis[j] < best ? dis[j] : best;
            }
            const float mn = -half32_max(-best);
            float cand = 256.f;                                        // no distance below +inf anywhere: code 0, as gnnlm_pq_encode
#pragma unroll
            for (int j = 7; j >= 0; --j) cand = (dis[j] == mn && mn < INFINITY) ? (float)((j >> 2) * 128 + tc * 4 + (j & 3)) : cand;
            const int bi = (int)(-half32_max(-cand)) & 255;
            const int r = tr * 8 + i;
            if (tc == 0 && s_list[r] >= 0) p.codes[(row0 + r) * p.ld_codes + m] = (uint8_t)bi;
        }
    }
}

__device__ __forceinline__ uint4 load16(const uint8_t* src, bool aligned) {
    if (aligned) return *reinterpret_cast<const uint4*>(src);
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (uint32_t)src[4 * k] | (uint32_t)src[4 * k + 1] << 8 | (uint32_t)src[4 * k + 2] << 16 | (uint32_t)src[4 * k + 3] << 24;
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ __launch_bounds__(256) void ivfpq_list_merge_kernel(gnnlm_ivfpq_list_merge_t p, bool new_aligned) {
    const int per_row = p.M >> 4;                                    // 16-byte pieces of a code row
    const int64_t n_all = p.N0 + p.n, total = n_all * per_row;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (int64_t)gridDim.x * 256) {
        const int64_t s = g / per_row;
        const int part = (int)(g - s * per_row);
        int64_t pos, id;
        uint4 v;
        if (s < p.N0) {                                               // old row s of list l: the last l with list_off_old[l] <= s
            int lo = 0, hi = p.nlist;
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (p.list_off_old[mid] <= s) lo = mid; else hi = mid;
            }
            pos = p.new_off[lo] + (s - p.list_off_old[lo]);
            id = p.ids_old[s];
            v = *reinterpret_cast<const uint4*>(p.codes_old + s * p.M + 16 * part);
        } else {
            const int64_t i = s - p.N0;
            pos = p.dest[i];
            id = p.ids_new[i];
            v = load16(p.codes_new + i * p.ld_new + 16 * part, new_aligned);
        }
        if (pos < 0 || pos >= n_all) {
            if (part == 0 && p.n_bad) atomicAdd(p.n_bad, 1);
            continue;
        }
        *reinterpret_cast<uint4*>(p.codes + pos * p.M + 16 * part) = v;
        if (part == 0) p.ids[pos] = id;
    }
}

}  // namespace

int ivfpq_encode_rows(const gnnlm_ivfpq_encode_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.n >= 0 && d.nlist >= 0 && d.M > 0 && d.dsub > 0 && d.d > 0 && d.ldx >= 0 && d.ld_codes >= 0, "ivfpq_encode_rows: negative size");
    GNNLM_REQUIRE(d.M % 16 == 0 && d.dsub % 4 == 0 && (int64_t)d.d == (int64_t)d.M * d.dsub, "ivfpq_encode_rows: need M % 16 == 0, dsub % 4 == 0 and d == M * dsub");
    if (d.n == 0) return OK;
    GNNLM_REQUIRE(d.x && d.assign && d.pq && d.norm2 && d.codes && (d.coarse || d.nlist == 0), "ivfpq_encode_rows: null operand");
    GNNLM_REQUIRE(d.ldx >= d.d && d.ld_codes >= d.M, "ivfpq_encode_rows: row strides shorter than the rows");
    GNNLM_REQUIRE(cdiv(d.n, (int64_t)ENC_ROWS) < (1ll << 31), "ivfpq_encode_rows: too many rows for one launch");
    hipLaunchKernelGGL(ivfpq_encode_rows_kernel, dim3((unsigned)cdiv(d.n, (int64_t)ENC_ROWS)), dim3(256), 0, stream, d);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int ivfpq_list_merge(const gnnlm_ivfpq_list_merge_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.N0 >= 0 && d.n >= 0 && d.nlist > 0 && d.M > 0 && d.ld_new >= 0, "ivfpq_list_merge: negative size");
    GNNLM_REQUIRE(d.M % 16 == 0, "ivfpq_list_merge: need M % 16 == 0");
    if (d.N0 + d.n == 0) return OK;
    GNNLM_REQUIRE(d.ids && d.codes && d.new_off && (uintptr_t)d.codes % 16 == 0, "ivfpq_list_merge: null / misaligned output");
    GNNLM_REQUIRE(d.N0 == 0 || (d.list_off_old && d.ids_old && d.codes_old && (uintptr_t)d.codes_old % 16 == 0), "ivfpq_list_merge: null / misaligned old rows");
    GNNLM_REQUIRE(d.n == 0 || (d.dest && d.ids_new && d.codes_new && d.ld_new >= d.M), "ivfpq_list_merge: null new rows / ld_new < M");
    GNNLM_REQUIRE(d.codes != d.codes_old && d.codes != d.codes_new && d.ids != d.ids_old && d.ids != d.ids_new, "ivfpq_list_merge: the outputs are buffers of their own");
    const bool new_aligned = (uintptr_t)d.codes_new % 16 == 0 && d.ld_new % 16 == 0;
    const int64_t total = (d.N0 + d.n) * (d.M >> 4);
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(total, 256), 256 * 64);
    hipLaunchKernelGGL(ivfpq_list_merge_kernel, dim3(blocks), dim3(256), 0, stream, d, new_aligned);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm

using namespace gnnlm;

extern "C" {
int gnnlm_ivfpq_encode_rows(const gnnlm_ivfpq_encode_t* d, void* stream) {
    if (!d) { set_error("invalid argument: null descriptor"); return E_INVALID; }
    return ivfpq_encode_rows(*d, (hipStream_t)stream);
}
int gnnlm_ivfpq_list_merge(const gnnlm_ivfpq_list_merge_t* d, void* stream) {
    if (!d) { set_error("invalid argument: null descriptor"); return E_INVALID; }
    return ivfpq_list_merge(*d, (hipStream_t)stream);
}
}
