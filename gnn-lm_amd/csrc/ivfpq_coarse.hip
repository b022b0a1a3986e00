// The coarse step of an IVF-PQ index with many lists (the reference's One Billion Word recipe, gnnlm_scripts/one_billion/find_knn.sh:8-21:
// IVF1048576, nprobe 32): the k best lists of every row WITHOUT the [n, nlist] score matrix.  The contract is gnnlm_ivfpq_select_probes
// over gnnlm_gemm_nt(x, coarse) (include/gnnlm.h, gnnlm_ivfpq_coarse_t).
//
//   ivfpq_coarse_kernel: a workgroup of 256 threads owns a TILE of 64 rows and one SLAB of the lists, streamed through LDS in chunks of
//     64 lists x 64 dimensions, transposed ([e][list]: a lane's four lists of one dimension are one 16-byte read).  A wave owns 16 rows
//     against the chunk's 64 lists: four accumulators of v_mfma_f32_16x16x4_f32 with the LISTS as the matrix rows and the wave's rows as
//     its columns -- a lane's 16 results all belong to ONE row of x, so that row's threshold is one register.  d <= 64: the lane's
//     operands of x stay in registers for the whole slab; beyond, x goes through LDS block by block of 64 dimensions like the lists.
//     Dimensions are summed in ascending order (k-step s adds dimensions 4 s .. 4 s + 3).
//   The running k-best of a row: a threshold (the k-th best value so far, -inf until there are k) and an append buffer in LDS of
//     cap = k + SLACK + 64 (value, list) records.  A score strictly above the threshold is appended (a later list that EQUALS the k-th
//     best loses the tie to every kept entry: strict is exact; NaN and -inf never pass).  After a chunk, a row with more than
//     k + SLACK records is compacted by its wave: every record is ranked among the row's records by (value, lower list) -- one 64-bit
//     key, read out of the lanes' registers -- and the k best are stored in rank order, the k-th value the new threshold.  Rows are private to a wave:
//     no barrier but the two of the chunk's staging.  At most 64 records join between checks, so the buffer never overflows (and an
//     append beyond cap is dropped, never stored out of bounds).
//   The slab's k best leave sorted, padded with (-inf, -1): to out_val / out_id (one slab) or to the [n, slabs, k] partial that
//     gnnlm_topk_merge folds (ids = the partial's lists): the same rules, so no second merge kernel.
#include "kernels.h"

namespace gnnlm {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int CO_ROWS = 64;            // rows of x per workgroup (16 per wave)
constexpr int CO_COLS = 64;            // lists per chunk
constexpr int CO_KB = 64;              // dimensions per staged block
constexpr int CO_LD = CO_COLS + 4;     // floats per [e] row in LDS: 4 e-rows of a k-step land 16 banks apart
constexpr int CO_SLACK = 16;           // records beyond k a row may hold before it is compacted
constexpr int CO_MAXK = 64;

__host__ __device__ constexpr int co_cap(int k) { return k + CO_SLACK + CO_COLS; }
__host__ __device__ constexpr size_t co_lds_bytes(int k, bool resident) {
    return (size_t)CO_ROWS * co_cap(k) * 8 + (size_t)CO_KB * CO_LD * 4 * (resident ? 1 : 2);
}

// larger key = better: value descending (-0 was made +0 when the record was appended), then the lower list
__device__ __forceinline__ uint64_t co_key(float v, uint32_t id) {
    const uint32_t b = __float_as_uint(v);
    const uint32_t m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((uint64_t)m << 32) | (uint32_t)~id;
}

// One row's records -> its k best in rank order (the whole wave; cnt <= cap <= 3 * 64).  -> the new count
__device__ __forceinline__ int co_compact(uint2* buf, int cnt, int k, int lane, float* thr_out) {
    uint64_t key[3];
    uint2 rec[3];
    int rank[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int e = lane + 64 * i;
        rec[i] = e < cnt ? buf[e] : make_uint2(0u, 0u);
        key[i] = e < cnt ? co_key(__uint_as_float(rec[i].x), rec[i].y) : 0ull;
        rank[i] = 0;
    }
    // record j of the row against the lane's records: its key comes out of the registers of lane j & 63 (v_readlane, j is uniform), no
    // LDS round trip per record; a lane's second and third records only exist beyond 64 / 128 records
#pragma unroll
    for (int src = 0; src < 3; ++src) {
        const int lim = min(64, cnt - 64 * src);                       // (<= 0: no such records)
        const int hi = (int)(key[src] >> 32), lo = (int)key[src];
        for (int j = 0; j < lim; ++j) {
            const uint64_t kj = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, j) << 32) | (uint32_t)__builtin_amdgcn_readlane(lo, j);
            rank[0] += kj > key[0] ? 1 : 0;
            if (cnt > 64) rank[1] += kj > key[1] ? 1 : 0;
            if (cnt > 128) rank[2] += kj > key[2] ? 1 : 0;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();                                   // every lane has read the row before any lane stores into it
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int e = lane + 64 * i;
        if (e < cnt && rank[i] < k) {
            buf[rank[i]] = rec[i];
            if (rank[i] == k - 1) *thr_out = __uint_as_float(rec[i].x);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return cnt < k ? cnt : k;
}

template <bool RESIDENT>
__global__ __launch_bounds__(256) void ivfpq_coarse_kernel(gnnlm_ivfpq_coarse_t p, int slab_cols) {
    extern __shared__ __attribute__((aligned(16))) unsigned char co_lds[];
    const int k = p.k, cap = co_cap(k);
    uint2* s_buf = reinterpret_cast<uint2*>(co_lds);                                  // [CO_ROWS][cap]
    float* s_c = reinterpret_cast<float*>(co_lds + (size_t)CO_ROWS * cap * 8);        // [CO_KB][CO_LD] the chunk's lists
    float* s_x = s_c + CO_KB * CO_LD;                                                 // [CO_KB][CO_LD] the tile's rows (not RESIDENT)
    __shared__ int s_cnt[CO_ROWS];
    __shared__ float s_thr[CO_ROWS];
    __shared__ __attribute__((aligned(16))) float s_bias[CO_COLS];

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int lr = lane & 15, g = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * CO_ROWS;
    const int slab = blockIdx.y;
    const int64_t c_lo = (int64_t)slab * slab_cols;
    const int64_t c_hi = min((int64_t)p.nlist, c_lo + slab_cols);
    const int d = p.d;
    const int n_kb = (d + CO_KB - 1) / CO_KB;
    const int qrow = w * 16 + lr;                                     // the row of the tile this lane's results belong to
    const bool has_bias = p.col_bias != nullptr;

    if (t < CO_ROWS) { s_cnt[t] = 0; s_thr[t] = -INFINITY; }
    __syncthreads();

    // the lane's operands of x: dimension 4 s + g of its row, k-step s
    float xb[16];
    if (RESIDENT) {
        const int64_t r = row0 + qrow;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int e = 4 * s + g;
            xb[s] = (r < p.n && e < d) ? p.x[r * p.ldx + e] : 0.f;
        }
    }

    // what a thread stages per block: 16 dimensions (4 float4) of list t >> 2, and of row t >> 2 of the tile
    const int sc = t >> 2, se = (t & 3) * 4;
    float4 g_c[4];
    float g_x[16], g_b = 0.f;
    auto fetch = [&](int64_t col0, int kb) {
        const int64_t col = col0 + sc;
        const int e0 = kb * CO_KB;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = e0 + se + 16 * q;
            g_c[q] = (col < c_hi && e < d) ? *reinterpret_cast<const float4*>(p.coarse + col * d + e) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (!RESIDENT) {
            const int64_t r = row0 + sc;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = e0 + se + 16 * q + i;
                    g_x[4 * q + i] = (r < p.n && e < d) ? p.x[r * p.ldx + e] : 0.f;
                }
        }
        if (kb == 0 && t < CO_COLS) g_b = (has_bias && col0 + t < c_hi) ? p.col_bias[col0 + t] : 0.f;
    };
    auto stage = [&](int kb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = se + 16 * q;
            s_c[(e + 0) * CO_LD + sc] = g_c[q].x;
            s_c[(e + 1) * CO_LD + sc] = g_c[q].y;
            s_c[(e + 2) * CO_LD + sc] = g_c[q].z;
            s_c[(e + 3) * CO_LD + sc] = g_c[q].w;
        }
        if (!RESIDENT) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 4; ++i) s_x[(se + 16 * q + i) * CO_LD + sc] = g_x[4 * q + i];
        }
        if (kb == 0 && t < CO_COLS) s_bias[t] = g_b;
    };

    float thr = -INFINITY;
    if (c_lo < c_hi) fetch(c_lo, 0);
    for (int64_t col0 = c_lo; col0 < c_hi; col0 += CO_COLS) {
        f32x4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int kb = 0; kb < n_kb; ++kb) {
            __syncthreads();                                          // the previous block's readers are done with LDS
            stage(kb);
            __syncthreads();
            if (kb + 1 < n_kb) fetch(col0, kb + 1);
            else if (col0 + CO_COLS < c_hi) fetch(col0 + CO_COLS, 0);
            const int steps = min(CO_KB, d - kb * CO_KB) >> 2;        // (d % 4 == 0)
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                if (s < steps) {
                    // lists 4 lr .. 4 lr + 3 of the chunk at dimension 4 s + g: the A operands of the four accumulators
                    const float4 a = *reinterpret_cast<const float4*>(&s_c[(4 * s + g) * CO_LD + 4 * lr]);
                    const float b = RESIDENT ? xb[s] : s_x[(4 * s + g) * CO_LD + qrow];
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b, acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b, acc[1], 0, 0, 0);
                    acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b, acc[2], 0, 0, 0);
                    acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b, acc[3], 0, 0, 0);
                }
            }
        }
        // accumulator c, register r of this lane: list col0 + 4 (4 g + r) + c of row qrow
        uint2* buf = s_buf + (size_t)qrow * cap;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float4 bias = make_float4(0.f, 0.f, 0.f, 0.f);
            if (has_bias) bias = *reinterpret_cast<const float4*>(&s_bias[4 * (4 * g + r)]);
            const float bv[4] = {bias.x, bias.y, bias.z, bias.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t col = col0 + 4 * (4 * g + r) + c;
                float v = acc[c][r];
                if (has_bias) v = v + bv[c];
                if (col < c_hi && v > thr) {
                    const int pos = atomicAdd(&s_cnt[qrow], 1);
                    if (pos < cap) buf[pos] = make_uint2(__float_as_uint(v + 0.f), (uint32_t)col);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // the wave's rows that hold more than k + SLACK records are compacted (rows are private to the wave)
        uint64_t full = __ballot(lane < 16 && s_cnt[w * 16 + lane] > k + CO_SLACK);
        if (full) {
            while (full) {
                const int rr = w * 16 + (__ffsll((unsigned long long)full) - 1);
                full &= full - 1;
                const int m = co_compact(s_buf + (size_t)rr * cap, min(s_cnt[rr], cap), k, lane, &s_thr[rr]);
                if (lane == 0) s_cnt[rr] = m;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            thr = s_thr[qrow];
        }
    }

    // the slab's k best of every row, sorted, padded
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int i = 0; i < 16; ++i) {
        const int rr = w * 16 + i;
        const int64_t r = row0 + rr;
        if (r >= p.n) break;                                          // (wave-uniform)
        uint2* buf = s_buf + (size_t)rr * cap;
        const int m = co_compact(buf, min(s_cnt[rr], cap), k, lane, &s_thr[rr]);
        if (lane < k) {
            const uint2 rec = lane < m ? buf[lane] : make_uint2(0u, 0u);
            const float v = lane < m ? __uint_as_float(rec.x) : -INFINITY;
            const int64_t id = lane < m ? (int64_t)rec.y : -1;
            const int64_t o = p.slabs > 1 ? (r * p.slabs + slab) * k + lane : r * k + lane;
            (p.slabs > 1 ? p.part_val : p.out_val)[o] = v;
            (p.slabs > 1 ? p.part_id : p.out_id)[o] = id;
        }
    }
}

// a pointer into device (or managed) memory; six queries per call did not show in the timings (tools/ivfpq_coarse_bench.py)
bool co_device_ptr(const void* ptr) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

}  // namespace

int ivfpq_coarse_probes(const gnnlm_ivfpq_coarse_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.k >= 1 && d.k <= CO_MAXK, "ivfpq_coarse_probes: need 1 <= k <= 64");
    GNNLM_REQUIRE(d.d > 0 && d.d % 4 == 0, "ivfpq_coarse_probes: need d > 0 and d % 4 == 0");
    GNNLM_REQUIRE(d.n >= 0 && d.nlist >= 0 && d.ldx >= d.d, "ivfpq_coarse_probes: negative size / row stride shorter than the rows");
    GNNLM_REQUIRE(d.slabs >= 1 && d.slabs * d.k <= 4096, "ivfpq_coarse_probes: need 1 <= slabs <= 4096 / k");
    if (d.n == 0) return OK;
    GNNLM_REQUIRE(d.x && d.out_val && d.out_id && (d.coarse || d.nlist == 0) && (d.slabs == 1 || (d.part_val && d.part_id)),
                  "ivfpq_coarse_probes: null operand");
    GNNLM_REQUIRE(co_device_ptr(d.x) && co_device_ptr(d.out_val) && co_device_ptr(d.out_id) && (d.nlist == 0 || co_device_ptr(d.coarse)) &&
                  (!d.col_bias || co_device_ptr(d.col_bias)) && (d.slabs == 1 || (co_device_ptr(d.part_val) && co_device_ptr(d.part_id))),
                  "ivfpq_coarse_probes: host pointer (operands live in device memory)");
    GNNLM_REQUIRE((uintptr_t)d.coarse % 16 == 0, "ivfpq_coarse_probes: coarse must be 16-byte aligned");
    const int64_t tiles = cdiv(d.n, (int64_t)CO_ROWS);
    GNNLM_REQUIRE(tiles < (1ll << 31), "ivfpq_coarse_probes: too many rows for one launch");
    const int slab_cols = (int)(cdiv(cdiv((int64_t)d.nlist, (int64_t)d.slabs), (int64_t)CO_COLS) * CO_COLS);
    const bool resident = d.d <= CO_KB;
    const size_t lds = co_lds_bytes(d.k, resident);
    {
        ProfScope prof(K_TOPK, stream, 2.0 * (double)d.n * d.nlist * d.d,
                       4.0 * ((double)d.n * d.ldx + (double)tiles * d.nlist * d.d) + 12.0 * (double)d.n * d.slabs * d.k);
        const dim3 grid((unsigned)tiles, (unsigned)d.slabs), block(256);
        if (resident) {
            GNNLM_LDS_OPT_IN(ivfpq_coarse_kernel<true>, co_lds_bytes(CO_MAXK, true));
            hipLaunchKernelGGL(ivfpq_coarse_kernel<true>, grid, block, lds, stream, d, slab_cols);
        } else {
            GNNLM_LDS_OPT_IN(ivfpq_coarse_kernel<false>, co_lds_bytes(CO_MAXK, false));
            hipLaunchKernelGGL(ivfpq_coarse_kernel<false>, grid, block, lds, stream, d, slab_cols);
        }
        GNNLM_LAUNCH_CHECK();
    }
    if (d.slabs == 1) return OK;
    gnnlm_topk_t m{};
    m.scores = d.part_val;  m.ld = (int64_t)d.slabs * d.k;  m.n = d.n;  m.ncols = d.slabs * d.k;
    m.ids = d.part_id;  m.ld_ids = m.ld;
    m.k = d.k;  m.largest = 1;  m.init = 1;
    m.best_val = d.out_val;  m.best_id = d.out_id;
    return topk_merge(m, stream);
}

}  // namespace gnnlm

using namespace gnnlm;

extern "C" {
int gnnlm_ivfpq_coarse_probes(const gnnlm_ivfpq_coarse_t* d, void* stream) {
    if (!d) { set_error("invalid argument: null descriptor"); return E_INVALID; }
    return ivfpq_coarse_probes(*d, (hipStream_t)stream);
}
}
