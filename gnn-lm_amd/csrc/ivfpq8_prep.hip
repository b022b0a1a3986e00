// The int8 IVF-PQ search (scheme: ivfpq8_scan.hip; buffer shapes and launch arithmetic: ivfpq8_layout.h), what is prepared before a scan:
// the index's code rows as tiles (per index), the queries' ADC tables with their byte images (per query block), the task table (per scan).
#include "kernels.h"
#include "ivfpq8_layout.h"

namespace gnnlm {
namespace {

// codes [N, 64] row-major -> tiles of 16 rows, [tile][g 0..3][i 0..15][p 0..15] = code[16 tile + i][16 g + (i + p) % 16];
// rows beyond N are zero.  One thread per (row, g).
__global__ __launch_bounds__(256) void pack_tiles_kernel(const uint8_t* __restrict__ codes, int64_t N, uint8_t* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = e >> 2;
    const int g = (int)(e & 3);
    if (row >= ((N + 15) >> 4 << 4)) return;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (row < N) {
        const uint8_t* src = codes + row * 64 + 16 * g;
        const int i = (int)(row & 15);
#pragma unroll
        for (int p = 0; p < 16; ++p) v[p >> 2] |= (uint32_t)src[(i + p) & 15] << (8 * (p & 3));
    }
    *reinterpret_cast<uint4*>(out + (((row >> 4) * 4 + g) * 16 + (row & 15)) * 16) = uint4{v[0], v[1], v[2], v[3]};
}

// One workgroup per query: L [64][256] f32 -> u8 [half][code][32 slots] + {delta, sum_lo, absmax, 0}.
__global__ __launch_bounds__(256) void quantize_lut_kernel(const float* __restrict__ lut, int64_t ld, uint8_t* __restrict__ qlut,
                                                           float* __restrict__ qmeta) {
    __shared__ __attribute__((aligned(16))) float tab[64 * 256];
    __shared__ float lo_s[64], rng_s[64], amax_s[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    {
        const float4* src = reinterpret_cast<const float4*>(lut + q * ld);
        float4* dst = reinterpret_cast<float4*>(tab);
        for (int e = tid; e < 64 * 64; e += 256) dst[e] = src[e];
    }
    __syncthreads();
    for (int m = wave; m < 64; m += 4) {
        float mn = INFINITY, mx = -INFINITY;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const float v = tab[m * 256 + lane + 64 * x];
            mn = fminf(mn, v);
            mx = fmaxf(mx, v);
        }
        mn = -wave_max(-mn);
        mx = wave_max(mx);
        if (lane == 0) { lo_s[m] = mn; rng_s[m] = mx - mn; amax_s[m] = fmaxf(fabsf(mn), fabsf(mx)); }
    }
    __syncthreads();
    float maxrange = 0.f, sum_lo = 0.f, amax = 0.f;
    for (int m = 0; m < 64; ++m) {                       // every thread, same order: sum_lo is one fixed f32 chain
        maxrange = fmaxf(maxrange, rng_s[m]);
        sum_lo += lo_s[m];
        amax = fmaxf(amax, amax_s[m]);
    }
    // inv a little below 255 / maxrange, delta a little above maxrange / 255: (u + 1) delta bounds L - lo from above whatever
    // the rounding of the two float operations of the quantisation did (see ivfpq8_scan.hip's header comment; delta * inv >= 1 + 2^-19)
    const bool flat = !(maxrange > 0.f);
    const float inv = flat ? 0.f : (255.f / maxrange) * (1.f - 3.8146973e-6f);          // 1 - 2^-18
    const float delta = flat ? 1e-30f : (maxrange / 255.f) * (1.f + 7.6293945e-6f);     // 1 + 2^-17
    if (tid == 0) {
        qmeta[q * 4 + 0] = delta;
        qmeta[q * 4 + 1] = sum_lo;
        qmeta[q * 4 + 2] = amax;
        qmeta[q * 4 + 3] = 0.f;
    }
    uint8_t* dst = qlut + q * QLUT_BYTES;
    for (int hc = tid; hc < 512; hc += 256) {           // row (half, code): 32 slots = 32 bytes
        const int h = hc >> 8, c = hc & 255;
        uint32_t o[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            uint32_t pk = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int m = 32 * h + 4 * w + b;
                const float y = (tab[m * 256 + c] - lo_s[m]) * inv;
                const int u = min(255, max(0, (int)floorf(y)));
                pk |= (uint32_t)(u ^ 0x80) << (8 * b);            // stored as the SIGNED byte u - 128: the i8 MFMA reads signed operands
            }
            o[w] = pk;
        }
        uint4* d4 = reinterpret_cast<uint4*>(dst + hc * 32);
        d4[0] = uint4{o[0], o[1], o[2], o[3]};
        d4[1] = uint4{o[4], o[5], o[6], o[7]};
    }
}

// ADC tables and their int8 image in ONE launch (gnnlm_ivfpq_tables): the pair gnnlm_gemm_nt (M = 64 batched [n x 256] GEMMs,
// K = dsub) + quantize_lut_kernel wrote the f32 tables (2 GiB at 32768 queries) and read them back.  Here a workgroup owns
// TQ = 32 queries and computes their tiles twice from the operands (qr rows and the 1-MiB codebook: L2-resident):
//   pass 1: lut = every [32 x 256] tile of every sub-quantizer, stored (a query's 64-KiB row, full 128-B lines), and per
//           (query, m) the min and max over the 256 codes (one wave owns all codes of its m: in-wave reductions only);
//   meta:   delta, sum_lo, amax, inv per query -- quantize_lut_kernel's formulas and its left-to-right chain over m;
//   pass 2: the same tiles again, quantised, transposed to [code][slot] through LDS in eight (half, 64-code) pieces, 2 KiB
//           contiguous per query and piece.
// Bits: the f32 tiles are those of gemm_nt_f32_kernel (gemm_f32.hip, the kernel gemm_nt picks for K <= 32: ragged K, no LDS-DMA)
// -- the same v_mfma_f32_32x32x2_f32 with A = query rows, B = codebook rows, lane half h supplying k = 8 s + 4 h + {x, y, z, w}
// (zero beyond dsub), the same instruction order per accumulator.  Its k-steps s >= ceil(dsub / 8) multiply zeros only; they
// are not issued here: they add +0 to an accumulator that is never -0 (it starts at +0, and a round-to-nearest sum is -0 only
// if both addends are), which leaves it unchanged.  Min / max do not depend on the order they are taken in (no -0, no NaN in
// a table), so the quantisation sees the values quantize_lut_kernel sees and applies the same two f32 operations to them.
constexpr int TAB_STAGE = TQ * 64 * 32;                 // pass 2 staging: [query][64 codes][32 slots] bytes = 64 KiB
constexpr int TABLES_LDS = TAB_STAGE + 64 * TQ * 4 + TQ * 4;       // + lo [64][TQ] + inv [TQ] (hi [64][TQ]: in the staging area, free until
                                                                     // pass 2) = 72.1 KiB: 2 workgroups per CU
static_assert(2 * TABLES_LDS <= 160 * 1024, "two workgroups of the tables kernel per CU");

template <int DSUB>
__global__ __launch_bounds__(256, 2) void ivfpq_tables_kernel(const gnnlm_ivfpq_tables_t p) {
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    constexpr int S = (DSUB + 7) / 8;                   // k-steps of 8 that hold data
    extern __shared__ __attribute__((aligned(16))) unsigned char tlds[];
    uint32_t* stage = reinterpret_cast<uint32_t*>(tlds);
    float* lo_s = reinterpret_cast<float*>(tlds + TAB_STAGE);                 // [m][query]
    float* hi_s = reinterpret_cast<float*>(tlds);                             // [m][query], read by the meta step only
    float* inv_s = lo_s + 64 * TQ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l32 = lane & 31;
    const int64_t q0 = (int64_t)blockIdx.x * TQ;
    const int nrow = (int)min((int64_t)TQ, p.n - q0);
    // the lane's A row (rows beyond n read the last query: computed, never stored)
    const float* arow = p.qr + (q0 + min(l32, nrow - 1)) * p.ld_qr;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load_a = [&](int m, float4 (&a)[S]) __attribute__((always_inline)) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int k = 8 * s + 4 * half;
            a[s] = k < DSUB ? *reinterpret_cast<const float4*>(arow + m * DSUB + k) : z4;
        }
    };
    auto load_b = [&](int m, int c, float4 (&b)[S]) __attribute__((always_inline)) {     // codebook row (m, c)
        const float* brow = p.pq + ((int64_t)m * 256 + c) * DSUB;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int k = 8 * s + 4 * half;
            b[s] = k < DSUB ? *reinterpret_cast<const float4*>(brow + k) : z4;
        }
    };
    auto mfma = [&](const float4 (&a)[S], const float4 (&b)[S], f32x16& acc) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].x, b[s].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].y, b[s].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].z, b[s].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s].w, b[s].w, acc, 0, 0, 0);
        }
    };
    // C/D layout of the 32x32 MFMA: col = lane & 31 (code), row = (r & 3) + 8 (r >> 2) + 4 half (query)
    auto row_of = [&](int r) __attribute__((always_inline)) { return (r & 3) + 8 * (r >> 2) + 4 * half; };

    // ---- pass 1: f32 tables + per-(query, m) min / max.  Wave w: m = w, w + 4, ...; all 256 codes, two tiles of 32 at a time
    for (int m = wave; m < 64; m += 4) {
        float4 a[S];
        load_a(m, a);
        float mn[16], mx[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) { mn[r] = INFINITY; mx[r] = -INFINITY; }
#pragma unroll
        for (int t0 = 0; t0 < 8; t0 += 2) {
            float4 b[2][S];
#pragma unroll
            for (int t = 0; t < 2; ++t) load_b(m, 32 * (t0 + t) + l32, b[t]);
            f32x16 acc[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) mfma(a, b[t], acc[t]);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float* dst = p.lut + q0 * p.ld_lut + m * 256 + 32 * (t0 + t) + l32;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row_of(r);
                    if (row < nrow) dst[row * p.ld_lut] = acc[t][r];
                    mn[r] = fminf(mn[r], acc[t][r]);
                    mx[r] = fmaxf(mx[r], acc[t][r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float lo = -half32_max(-mn[r]), hi = half32_max(mx[r]);
            if (l32 == 0) { lo_s[m * TQ + row_of(r)] = lo; hi_s[m * TQ + row_of(r)] = hi; }
        }
    }
    __syncthreads();
    // ---- meta: quantize_lut_kernel's per-query reduction, same chain
    if (tid < TQ) {
        float maxrange = 0.f, sum_lo = 0.f, amax = 0.f;
        for (int m = 0; m < 64; ++m) {
            const float mn = lo_s[m * TQ + tid], mx = hi_s[m * TQ + tid];
            maxrange = fmaxf(maxrange, mx - mn);
            sum_lo += mn;
            amax = fmaxf(amax, fmaxf(fabsf(mn), fabsf(mx)));
        }
        const bool flat = !(maxrange > 0.f);
        const float inv = flat ? 0.f : (255.f / maxrange) * (1.f - 3.8146973e-6f);          // 1 - 2^-18
        const float delta = flat ? 1e-30f : (maxrange / 255.f) * (1.f + 7.6293945e-6f);     // 1 + 2^-17
        inv_s[tid] = inv;
        if (tid < nrow) *reinterpret_cast<float4*>(p.qmeta + (q0 + tid) * 4) = make_float4(delta, sum_lo, amax, 0.f);
    }
    __syncthreads();
    float inv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) inv[r] = inv_s[row_of(r)];

    // ---- pass 2: (half h, codes 64 cq ..): wave w quantises m = 32 h + 8 w + j (j = 0..7) of the piece's two tiles and packs
    // four consecutive m of a (query, code) into the dword of slots 8 w + 4 jj ..  Staging dword d of (query, code cl) sits at
    // d' = (d + cl / 8 + 4 ((query >> 2) & 1)) & 7 of the code's 32-byte row: the 64 lanes of a store (and of a read below)
    // hit 64 different banks.
    for (int h = 0; h < 2; ++h) {
        for (int cq = 0; cq < 4; ++cq) {
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                uint32_t pk[2][16];
#pragma unroll
                for (int r = 0; r < 16; ++r) pk[0][r] = pk[1][r] = 0u;
#pragma nounroll
                for (int j = 0; j < 4; ++j) {                        // (rolled: unrolled, all four steps' loads are hoisted and spill)
                    const int m = 32 * h + 8 * wave + 4 * jj + j;
                    float4 a[S], b[2][S];
                    load_a(m, a);
#pragma unroll
                    for (int t = 0; t < 2; ++t) load_b(m, 64 * cq + 32 * t + l32, b[t]);
                    f32x16 acc[2];
#pragma unroll
                    for (int t = 0; t < 2; ++t) mfma(a, b[t], acc[t]);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float lo = lo_s[m * TQ + row_of(r)];
#pragma unroll
                        for (int t = 0; t < 2; ++t) {
                            const float y = (acc[t][r] - lo) * inv[r];
                            const uint32_t u = (uint32_t)min(255, max(0, (int)floorf(y))) ^ 0x80u;   // the SIGNED byte u - 128
                            pk[t][r] |= u << (8 * j);
                        }
                    }
                }
                const int d = 2 * wave + jj;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int cl = 32 * t + l32;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = row_of(r);
                        stage[(row * 64 + cl) * 8 + ((d + (cl >> 3) + 4 * ((row >> 2) & 1)) & 7)] = pk[t][r];
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < TQ * 64 / 256; ++i) {
                const int e = tid + 256 * i, row = e >> 6, cl = e & 63;
                const uint32_t* src = stage + (row * 64 + cl) * 8;
                const int rot = (cl >> 3) + 4 * ((row >> 2) & 1);
                uint32_t o[8];
#pragma unroll
                for (int dd = 0; dd < 8; ++dd) o[dd] = src[(dd + rot) & 7];
                if (row < nrow) {
                    uint4* dst = reinterpret_cast<uint4*>(p.qlut + (q0 + row) * QLUT_BYTES + h * 8192 + (64 * cq + cl) * 32);
                    dst[0] = uint4{o[0], o[1], o[2], o[3]};
                    dst[1] = uint4{o[4], o[5], o[6], o[7]};
                }
            }
            __syncthreads();
        }
    }
}

// ---- the scan's task table (gnnlm_ivfpq_build_groups): pairs per list, group offsets, scatter.  cnt / fill: [nlist + 1] each
__global__ __launch_bounds__(256) void groups_fill_kernel(int32_t* grp_list, int32_t* grp_q, int64_t* grp_out, int64_t G, int32_t* scratch, int nlist) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < G) grp_list[e] = -1;
    if (e < G * QG) { grp_q[e] = -1; if (grp_out) grp_out[e] = -1; }
    if (e < 2 * (int64_t)(nlist + 1)) scratch[e] = 0;
}
__global__ __launch_bounds__(256) void groups_count_kernel(const int64_t* __restrict__ pl, int64_t ld, int64_t n, int P, int nlist, int32_t* cnt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * P) return;
    const int64_t l = pl[(e / P) * ld + e % P];
    if (l >= 0 && l < nlist) atomicAdd(&cnt[l], 1);
}
// one workgroup: cnt[l] -> the first group of list l (exclusive prefix of ceil(cnt / 8)), in place; n_groups = the total
__global__ __launch_bounds__(1024) void groups_scan_kernel(int32_t* cnt, int nlist, int32_t* n_groups) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (nlist + 1023) / 1024, lo = tid * per, hi = min(nlist, lo + per);
    int mine = 0;
    for (int l = lo; l < hi; ++l) mine += (cnt[l] + QG - 1) / QG;
    part[tid] = mine;
    __syncthreads();
    for (int step = 1; step < 1024; step <<= 1) {                            // inclusive prefix over the threads
        const int other = tid >= step ? part[tid - step] : 0;
        __syncthreads();
        part[tid] += other;
        __syncthreads();
    }
    int at = part[tid] - mine;
    for (int l = lo; l < hi; ++l) { const int g = (cnt[l] + QG - 1) / QG; cnt[l] = at; at += g; }
    if (tid == 1023) *n_groups = part[1023];
}
__global__ __launch_bounds__(256) void groups_scatter_kernel(const int64_t* __restrict__ pl, int64_t ld, int64_t n, int P, int nlist, int64_t seg,
                                                             const int32_t* __restrict__ goff, int32_t* fill, int32_t* grp_list, int32_t* grp_q,
                                                             int64_t* grp_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * P) return;
    const int64_t q = e / P, l = pl[q * ld + e % P];
    if (l < 0 || l >= nlist) return;
    const int pos = atomicAdd(&fill[l], 1);
    const int64_t g = goff[l] + pos / QG;
    grp_list[g] = (int32_t)l;
    grp_q[g * QG + pos % QG] = (int32_t)q;
    if (grp_out) grp_out[g * QG + pos % QG] = e * seg;
}

}  // namespace

int ivfpq_pack_tiles(const uint8_t* codes, int64_t N, int M, uint8_t* out, hipStream_t stream) {
    GNNLM_REQUIRE(codes && out && N >= 0 && M == 64, "ivfpq_pack_tiles: need M = 64");
    GNNLM_REQUIRE((uintptr_t)out % 16 == 0, "ivfpq_pack_tiles: 16-byte aligned output");
    const int64_t threads = ((N + 15) >> 4 << 4) * 4;
    if (threads == 0) return OK;
    GNNLM_REQUIRE(cdiv(threads, (int64_t)256) < (1ll << 31), "ivfpq_pack_tiles: too many rows for one launch");
    hipLaunchKernelGGL(pack_tiles_kernel, dim3((unsigned)cdiv(threads, (int64_t)256)), dim3(256), 0, stream, codes, N, out);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int ivfpq_build_groups(const int64_t* pl, int64_t ld, int64_t n, int P, int nlist, int64_t seg, int32_t* grp_list, int32_t* grp_q,
                       int64_t* grp_out, int32_t* n_groups, int32_t* scratch, hipStream_t stream) {
    GNNLM_REQUIRE(n >= 0 && P > 0 && nlist > 0 && n * P < (1ll << 31) && ld >= P, "ivfpq_build_groups: bad shape");
    GNNLM_REQUIRE(pl && grp_list && grp_q && n_groups && scratch, "ivfpq_build_groups: null operand");
    const int64_t G = groups_cap(n, P, nlist), pairs = n * P;
    const int64_t fill = groups_fill(G, nlist);
    hipLaunchKernelGGL(groups_fill_kernel, dim3((unsigned)cdiv(fill, (int64_t)256)), dim3(256), 0, stream, grp_list, grp_q, grp_out, G, scratch, nlist);
    if (pairs > 0)
        hipLaunchKernelGGL(groups_count_kernel, dim3((unsigned)cdiv(pairs, (int64_t)256)), dim3(256), 0, stream, pl, ld, n, P, nlist, scratch);
    hipLaunchKernelGGL(groups_scan_kernel, dim3(1), dim3(1024), 0, stream, scratch, nlist, n_groups);
    if (pairs > 0)
        hipLaunchKernelGGL(groups_scatter_kernel, dim3((unsigned)cdiv(pairs, (int64_t)256)), dim3(256), 0, stream, pl, ld, n, P, nlist, seg, scratch,
                           scratch + nlist + 1, grp_list, grp_q, grp_out);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int ivfpq_quantize_lut(const float* lut, int64_t ld_lut, int64_t n, int M, uint8_t* qlut, float* qmeta, hipStream_t stream) {
    GNNLM_REQUIRE(lut && qlut && qmeta && n >= 0 && n < (1ll << 31) && M == 64 && ld_lut >= 64 * 256 && ld_lut % 4 == 0 &&
                      (uintptr_t)lut % 16 == 0 && (uintptr_t)qlut % 16 == 0,
                  "ivfpq_quantize_lut: need M = 64 and 16-byte aligned tables");
    if (n == 0) return OK;
    hipLaunchKernelGGL(quantize_lut_kernel, dim3((unsigned)n), dim3(256), 0, stream, lut, ld_lut, qlut, qmeta);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int ivfpq_tables(const gnnlm_ivfpq_tables_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.qr && d.pq && d.lut && d.qlut && d.qmeta && d.n >= 0 && d.n < (1ll << 31), "ivfpq_tables: null operand or bad n");
    GNNLM_REQUIRE(d.M == 64 && (d.dsub == 4 || d.dsub == 8 || d.dsub == 16 || d.dsub == 32),
                  "ivfpq_tables: need M = 64 and dsub in {4, 8, 16, 32} (other shapes: gnnlm_gemm_nt + gnnlm_ivfpq_quantize_lut)");
    GNNLM_REQUIRE(d.ld_qr >= 64 * d.dsub && d.ld_qr % 4 == 0 && d.ld_lut >= 64 * 256 && d.ld_lut % 4 == 0 &&
                      (uintptr_t)d.qr % 16 == 0 && (uintptr_t)d.pq % 16 == 0 && (uintptr_t)d.lut % 16 == 0 &&
                      (uintptr_t)d.qlut % 16 == 0 && (uintptr_t)d.qmeta % 16 == 0,
                  "ivfpq_tables: rows of qr / lut must be 16-byte aligned and hold 64 * dsub / 64 * 256 floats");
    if (d.n == 0) return OK;
    const dim3 grid((unsigned)tables_grid(d.n));
#define GNNLM_TABLES_LAUNCH(DS)                                                                                 \
    GNNLM_LDS_OPT_IN(&ivfpq_tables_kernel<DS>, TABLES_LDS);                                                     \
    hipLaunchKernelGGL(ivfpq_tables_kernel<DS>, grid, dim3(256), TABLES_LDS, stream, d);
    if (d.dsub == 4) { GNNLM_TABLES_LAUNCH(4) }
    else if (d.dsub == 8) { GNNLM_TABLES_LAUNCH(8) }
    else if (d.dsub == 16) { GNNLM_TABLES_LAUNCH(16) }
    else { GNNLM_TABLES_LAUNCH(32) }
#undef GNNLM_TABLES_LAUNCH
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
