// Base-LM / GNN mixture of two target log-probabilities (transformer.py:1056-1062 `combinetow_probs`, :1075-1077), at up to 8
// ratios from ONE read of the two inputs: out[a, i] = logsumexp(log(alpha_a) + base[i], log(1 - alpha_a) + gnn[i]).
//
// A thread owns four consecutive tokens: one 16-byte load per input where the row allows it, then per ratio the four mixes and
// one 16-byte store (row a of `out` starts at a * n floats, so the wide form needs n % 4 == 0 and 16-byte aligned pointers; any
// other shape takes the same arithmetic through 4-byte accesses).  The coefficients are the float32 roundings of the float64
// logs, formed on the host and passed by value (wave-uniform indices: scalar loads).  alpha = 0 / 1 need no special case:
// log 0 = -inf drops its term out of m + logf(expf(x - m) + expf(y - m)), and the other term comes back bit for bit
// (m + logf(0 + 1) = m), as in knn_interp_grid_kernel.
#include "kernels.h"

namespace gnnlm {

namespace {

constexpr int MIX_A = 8;

struct LogpMixParams {
    const float* gnn;  const float* base;  float* out;
    int64_t n;  int n_a;  int wide;
    float c_base[MIX_A], c_gnn[MIX_A];
};

__device__ __forceinline__ float mix2(float x, float y) {
    const float m = fmaxf(x, y);
    return m + logf(expf(x - m) + expf(y - m));
}

__global__ __launch_bounds__(256) void logp_mix_kernel(LogpMixParams p) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= p.n) return;
    float g[4], b[4];
    const bool full = p.wide && i0 + 4 <= p.n;
    if (full) {
        const float4 gv = *reinterpret_cast<const float4*>(p.gnn + i0), bv = *reinterpret_cast<const float4*>(p.base + i0);
        g[0] = gv.x, g[1] = gv.y, g[2] = gv.z, g[3] = gv.w;
        b[0] = bv.x, b[1] = bv.y, b[2] = bv.z, b[3] = bv.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool in = i0 + j < p.n;
            g[j] = in ? p.gnn[i0 + j] : 0.f;
            b[j] = in ? p.base[i0 + j] : 0.f;
        }
    }
    for (int a = 0; a < p.n_a; ++a) {
        const float cb = p.c_base[a], cg = p.c_gnn[a];
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = mix2(cb + b[j], cg + g[j]);
        float* o = p.out + (int64_t)a * p.n + i0;
        if (full) {
            *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < p.n) o[j] = r[j];
        }
    }
}

}  // namespace

int logp_mix(const float* gnn_logp, const float* base_logp, int64_t n, const double* alphas, int n_alphas, float* out, hipStream_t stream) {
    GNNLM_REQUIRE(n_alphas >= 1 && n_alphas <= MIX_A, "logp_mix: 1 .. 8 ratios per call");
    GNNLM_REQUIRE(alphas, "logp_mix: null ratios");
    LogpMixParams p{};
    for (int a = 0; a < n_alphas; ++a) {
        GNNLM_REQUIRE(alphas[a] >= 0.0 && alphas[a] <= 1.0, "logp_mix: every ratio must lie in 0 .. 1");
        // float32 roundings of the float64 logs, as coeffs[0] = math.log(p1_coeff) lands in a float32 tensor; log 0 = -inf at the ends
        p.c_base[a] = (float)log(alphas[a]);
        p.c_gnn[a] = (float)log(1.0 - alphas[a]);
    }
    GNNLM_REQUIRE(n >= 0, "logp_mix: n < 0");
    if (n == 0) return OK;
    GNNLM_REQUIRE(gnn_logp && base_logp && out, "logp_mix: null operand");
    GNNLM_REQUIRE(cdiv(n, 1024) < (1ll << 31), "logp_mix: too many tokens for one launch");
    p.gnn = gnn_logp, p.base = base_logp, p.out = out, p.n = n, p.n_a = n_alphas;
    p.wide = n % 4 == 0 && ((reinterpret_cast<uintptr_t>(gnn_logp) | reinterpret_cast<uintptr_t>(base_logp) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    // (the kernel-id table ends at knn_resim_kernel, which tests/test_knn_resim_cpu.py holds it to: the mix is timed as "misc")
    ProfScope prof(K_MISC, stream, 0.0, 4.0 * (2.0 + n_alphas) * n);
    hipLaunchKernelGGL(logp_mix_kernel,dim3((unsigned)cdiv(n, 1024)), dim3(256), 0, stream, p);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
