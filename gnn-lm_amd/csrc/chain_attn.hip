// ('ntgt','intra','ntgt') attention of the HGT layer (fairseq/models/hgt.py:341-386; the edge types: star_attn.hip): each group
// of 1+l+r context nodes is a path graph with self loops (token_block_dataset.py:395-398): <= 3 incoming edges per node, one
// wave per (group, head), operands live in registers.
#include <algorithm>
#include "kernels.h"

namespace gnnlm {
namespace {

constexpr int MAX_NG = 8;
constexpr int MAX_EPT = 4;

// One wave per (group, head).  Position order along the path: o-l .. o-1, o, o+1 .. o+r.
__global__ __launch_bounds__(256) void chain_attn_kernel(ChainAttnParams p) {
    const int lane = threadIdx.x & 63;
    // (a device-side group count -- ABI 9 -- comes with a capped grid: the waves then walk the tasks)
    const int64_t n_tasks = (p.n_groups_dev ? min(p.n_groups, (int64_t)*p.n_groups_dev) : p.n_groups) * p.H;
  for (int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); task < n_tasks; task += (int64_t)gridDim.x * 4) {
    const int64_t g = task / p.H;
    const int h = (int)(task - g * p.H);
    const int n_g = 1 + p.left + p.right;
    const int dk = p.dk;
    const float scale = p.scale ? p.scale[h] : 1.f;

    // radius_p1 = r + 1 > 0: only the positions within r of the centre are destinations (a later layer reads nothing else);
    // their sources lie within r + 1, and only those rows of Q / K / V exist
    const int rad = p.radius_p1 > 0 ? p.radius_p1 - 1 : MAX_NG;
    float q[MAX_NG][MAX_EPT], k[MAX_NG][MAX_EPT], v[MAX_NG][MAX_EPT];
    bool ok[MAX_NG], dst[MAX_NG];
    int64_t slot_of[MAX_NG];
#pragma unroll
    for (int pos = 0; pos < MAX_NG; ++pos) {
        ok[pos] = dst[pos] = false;
        slot_of[pos] = 0;
        if (pos < n_g) {
            const int c = pos < p.left ? pos + 1 : (pos == p.left ? 0 : pos);
            const int64_t s = g * n_g + c;
            const int dist = pos < p.left ? p.left - pos : pos - p.left;
            slot_of[pos] = s;
            dst[pos] = dist <= rad;
            // (ABI 11: K / V keyed by datastore row -- slot s reads row kv_index[s]; a valid slot always has one.  The index is loaded
            // BESIDE the validity byte, not behind it: gated by `ok` it was a third dependent round trip per task and the layer-0 launch of
            // the 3-layer recipe took 20 ms instead of 10)
            const int32_t kvr = (p.kv_index && dist <= rad + 1) ? p.kv_index[s] : 0;
            ok[pos] = dist <= rad + 1 && p.valid[s] != 0;
            const int64_t row_kv = p.kv_index ? (int64_t)max(kvr, 0) : s;
#pragma unroll
            for (int t = 0; t < MAX_EPT; ++t) {
                const int e = lane + 64 * t;
                const bool in = ok[pos] && e < dk;
                const int64_t off = s * p.ld + h * dk + (in ? e : 0);
                const int64_t off_kv = row_kv * p.ld + h * dk + (in ? e : 0);
                q[pos][t] = in && dst[pos] ? p.Q[off] : 0.f;
                k[pos][t] = in ? p.K[off_kv] : 0.f;
                v[pos][t] = in ? p.V[off_kv] : 0.f;
            }
        }
    }
#pragma unroll
    for (int pos = 0; pos < MAX_NG; ++pos) {
        if (pos >= n_g) break;
        if (!dst[pos]) continue;
        float sc[3];
        bool has[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int u = pos + d - 1;
            has[d] = false;
            sc[d] = -INFINITY;
            if (u >= 0 && u < MAX_NG) {
                if (u < n_g && ok[u] && ok[pos]) {
                    float a = 0.f;
#pragma unroll
                    for (int t = 0; t < MAX_EPT; ++t) a = fmaf(q[pos][t], k[u][t], a);
                    a = wave_sum(a);
                    sc[d] = a * scale;
                    has[d] = true;
                }
            }
        }
        const float mx = fmaxf(sc[0], fmaxf(sc[1], sc[2]));
        float e[3], den = 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            e[d] = has[d] ? expf(sc[d] - mx) : 0.f;
            den += e[d];
        }
        const float inv = den > 0.f ? 1.f / den : 0.f;
#pragma unroll
        for (int t = 0; t < MAX_EPT; ++t) {
            const int el = lane + 64 * t;
            if (el < dk) {
                float o = 0.f;
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const int u = pos + d - 1;
                    if (u >= 0 && u < MAX_NG) {
                        if (has[d]) o = fmaf(e[d] * inv, v[u][t], o);
                    }
                }
                p.out[slot_of[pos] * p.ldo + h * dk + el] = o;
            }
        }
    }
  }
}

}  // namespace

int chain_attn(const ChainAttnParams& p, hipStream_t stream) {
    GNNLM_REQUIRE(p.Q && p.K && p.V && p.valid && p.out, "chain_attn: null operand");
    GNNLM_REQUIRE(1 + p.left + p.right <= MAX_NG, "chain_attn: 1+left+right must be <= 8");
    GNNLM_REQUIRE(p.dk > 0 && p.dk <= 64 * MAX_EPT && p.H > 0, "chain_attn: d_k must be <= 256");
    const int64_t tasks = p.n_groups * p.H;
    if (tasks == 0) return OK;
    const double slots = (double)p.n_groups * (1 + p.left + p.right);
    ProfScope prof(K_CHAIN, stream, slots * p.H * p.dk * 12.0, slots * (16.0 * p.H * p.dk + 1.0));
    const int64_t wgs = cdiv(tasks, 4);
    hipLaunchKernelGGL(chain_attn_kernel, dim3((unsigned)(p.n_groups_dev ? std::min<int64_t>(wgs, 256 * 32) : wgs)), dim3(256), 0, stream, p);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
