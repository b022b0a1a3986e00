// gnnlm_pack_rows (include/gnnlm.h): the scored rows of packed samples -- every sample a run of context rows followed by the rows
// that are scored -- as one contiguous query matrix, and / or the same rows at unit length for a cosine index.  One launch
// replaces one slice per sample + torch.cat + the four launches and three temporaries of knn/knn_model.py:181-184.
//
// Memory-bound row kernel: one wave per output row, 16-byte accesses, the row held in registers between the sum and the scaling
// (d <= 1024; longer rows are read a second time, from L2).
#include "host.h"

namespace gnnlm {
namespace {

struct PackParams {
    const float* src; int64_t ld_src;
    const int32_t* block_off; const int32_t* skip; const int32_t* out_off;
    float* dst; int64_t ld_dst;
    float* unit; int64_t ld_unit;
    int n_blocks, d;
    int64_t n_tok, n_out;
};

// One block.  Everything the pack kernel relies on is counted, nothing is followed: only the tables are read.
__global__ __launch_bounds__(256) void pack_check_kernel(PackParams p, int32_t* n_bad) {
    int bad = 0;
    for (int b = threadIdx.x; b < p.n_blocks; b += 256) {
        const int64_t len = (int64_t)p.block_off[b + 1] - p.block_off[b];
        const int64_t sk = p.skip ? p.skip[b] : 0;
        const int64_t take = (int64_t)p.out_off[b + 1] - p.out_off[b];
        bad += (len < 0) + (sk < 0) + (sk > len) + (take != len - sk);
    }
    if (threadIdx.x == 0) bad += (p.out_off[0] != 0) + ((int64_t)p.out_off[p.n_blocks] != p.n_out);
    bad = (int)wave_sum((float)bad);                 // (at most 4 per block entry and lane: exact in float32 far beyond any table)
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(n_bad, bad);
}

// -> the source row of output row r, or -1 when the tables do not describe one inside [0, n_tok) (wave-uniform).
__device__ __forceinline__ int64_t source_row(const PackParams& p, int64_t r) {
    const int lo = last_block(p.out_off, p.n_blocks, r);    // (empty blocks repeat an offset: the last one wins)
    const int64_t j = r - p.out_off[lo];
    const int64_t b0 = (int64_t)p.block_off[lo] - p.block_off[0], b1 = (int64_t)p.block_off[lo + 1] - p.block_off[0];
    const int64_t sk = p.skip ? p.skip[lo] : 0;
    const bool ok = j >= 0 && r < p.out_off[lo + 1] && b0 >= 0 && b1 <= p.n_tok && sk >= 0 && sk <= b1 - b0 && j < b1 - b0 - sk;
    return ok ? b0 + sk + j : -1;
}

__device__ __forceinline__ float sq4(float4 v) { return v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }
__device__ __forceinline__ float4 div4(float4 v, float n) {
    return make_float4(__fdiv_rn(v.x, n), __fdiv_rn(v.y, n), __fdiv_rn(v.z, n), __fdiv_rn(v.w, n));
}

constexpr int HELD = 4;                               // float4 per lane kept between the two passes: rows of up to 1024 floats

__global__ __launch_bounds__(256) void pack_rows4_kernel(PackParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.n_out) return;
    const int64_t s_row = source_row(p, r);
    if (s_row < 0) return;
    const int d4 = p.d >> 2;
    const float4* s = reinterpret_cast<const float4*>(p.src + s_row * p.ld_src);
    float4* o = p.dst ? reinterpret_cast<float4*>(p.dst + r * p.ld_dst) : nullptr;
    float4* u = p.unit ? reinterpret_cast<float4*>(p.unit + r * p.ld_unit) : nullptr;
    if (d4 <= 64 * HELD) {
        float4 v[HELD];
#pragma unroll
        for (int i = 0; i < HELD; ++i) {
            const int e = lane + 64 * i;
            v[i] = e < d4 ? s[e] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < HELD; ++i) {
            const int e = lane + 64 * i;
            if (o && e < d4) o[e] = v[i];
            acc += sq4(v[i]);
        }
        if (!u) return;
        const float n = __fsqrt_rn(wave_sum(acc));
#pragma unroll
        for (int i = 0; i < HELD; ++i) {
            const int e = lane + 64 * i;
            if (e < d4) u[e] = div4(v[i], n);
        }
        return;
    }
    float acc = 0.f;
    for (int e = lane; e < d4; e += 64) {
        const float4 v = s[e];
        if (o) o[e] = v;
        acc += sq4(v);
    }
    if (!u) return;
    const float n = __fsqrt_rn(wave_sum(acc));
    for (int e = lane; e < d4; e += 64) u[e] = div4(s[e], n);
}

// Any d, any stride, pointers aligned to 4 bytes only.
__global__ __launch_bounds__(256) void pack_rows1_kernel(PackParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.n_out) return;
    const int64_t s_row = source_row(p, r);
    if (s_row < 0) return;
    const float* s = p.src + s_row * p.ld_src;
    float* o = p.dst ? p.dst + r * p.ld_dst : nullptr;
    float acc = 0.f;
    for (int e = lane; e < p.d; e += 64) {
        const float v = s[e];
        if (o) o[e] = v;
        acc += v * v;
    }
    if (!p.unit) return;
    float* u = p.unit + r * p.ld_unit;
    const float n = __fsqrt_rn(wave_sum(acc));
    for (int e = lane; e < p.d; e += 64) u[e] = __fdiv_rn(s[e], n);
}

int pack_rows(const gnnlm_pack_rows_t& q, hipStream_t stream) {
    GNNLM_REQUIRE(q.d > 0, "pack_rows: d <= 0");
    GNNLM_REQUIRE(q.n_blocks >= 0 && q.n_tok >= 0 && q.n_tok < (1ll << 31) && q.n_out >= 0 && q.n_out < (1ll << 31), "pack_rows: bad counts");
    GNNLM_REQUIRE(q.dst || q.dst_unit, "pack_rows: both outputs are NULL");
    GNNLM_REQUIRE(q.ld_src >= q.d, "pack_rows: ld_src < d");
    GNNLM_REQUIRE(!q.dst || q.ld_dst >= q.d, "pack_rows: ld_dst < d");
    GNNLM_REQUIRE(!q.dst_unit || q.ld_unit >= q.d, "pack_rows: ld_unit < d");
    GNNLM_REQUIRE(q.block_off && q.out_off, "pack_rows: block_off / out_off missing");
    GNNLM_REQUIRE(q.src || q.n_out == 0, "pack_rows: src missing");
    GNNLM_REQUIRE(((uintptr_t)q.src | (uintptr_t)q.dst | (uintptr_t)q.dst_unit | (uintptr_t)q.block_off | (uintptr_t)q.skip |
                   (uintptr_t)q.out_off | (uintptr_t)q.n_bad) % 4 == 0, "pack_rows: a pointer is not 4-byte aligned");
    GNNLM_REQUIRE(!q.wait || q.n_bad, "pack_rows: wait needs n_bad");
    PackParams p{q.src, q.ld_src, q.block_off, q.skip, q.out_off, q.dst, q.ld_dst, q.dst_unit, q.ld_unit, q.n_blocks, q.d, q.n_tok, q.n_out};
    if (q.n_bad) {
        hipLaunchKernelGGL(pack_check_kernel, dim3(1), dim3(256), 0, stream, p, q.n_bad);
        GNNLM_LAUNCH_CHECK();
        if (q.wait) {
            int32_t bad = 0;
            GNNLM_HIP(hipMemcpyAsync(&bad, q.n_bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
            GNNLM_HIP(hipStreamSynchronize(stream));
            GNNLM_REQUIRE(bad == 0, "pack_rows: the tables do not describe the rows (a negative skip, a skip longer than its block, or an "
                                    "out_off that is not the prefix sum of length - skip ending at n_out)");
        }
    }
    if (q.n_out == 0 || q.n_blocks == 0) return OK;
    const bool vec = q.d % 4 == 0 && q.ld_src % 4 == 0 && (uintptr_t)q.src % 16 == 0 &&
                     (!q.dst || (q.ld_dst % 4 == 0 && (uintptr_t)q.dst % 16 == 0)) &&
                     (!q.dst_unit || (q.ld_unit % 4 == 0 && (uintptr_t)q.dst_unit % 16 == 0));
    const double outs = (q.dst ? 1.0 : 0.0) + (q.dst_unit ? 1.0 : 0.0);
    ProfScope prof(K_MISC, stream, 3.0 * q.n_out * q.d, 4.0 * (1.0 + outs) * q.n_out * q.d);
    if (vec) hipLaunchKernelGGL(pack_rows4_kernel, dim3((unsigned)cdiv(q.n_out, 4)), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(pack_rows1_kernel, dim3((unsigned)cdiv(q.n_out, 4)), dim3(256), 0, stream, p);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace
}  // namespace gnnlm

using namespace gnnlm;

extern "C" int gnnlm_pack_rows(const gnnlm_pack_rows_t* desc, void* stream) {
    GNNLM_DESC(desc);
    return pack_rows(*desc, (hipStream_t)stream);
}
