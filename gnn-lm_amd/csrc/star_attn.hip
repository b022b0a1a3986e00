// HGT attention kernels (reference: HGTLayer.forward, fairseq/models/hgt.py:341-386).
//
// The three edge types of the token/neighbour graph (fairseq/models/transformer.py:913-918) each get
// the kernel their shape asks for -- the graph is implicit, no edge list is ever built:
//   ('ntgt','inter','tgt')   star_attn (this file: the dispatch and the generic kernel; star_tab.hip, star_dense.hip):
//        every token attends over its kg neighbour centres.  The
//        per-neighbour K/V projections are absorbed into the query side (exact algebra):
//          score = q.(x W_k' ) = x.(W_k' q) = x.u,   sum_j a_j (x_j W_v') = (sum_j a_j x_j) W_v'
//        so the kernel only needs the raw neighbour rows x_j -- PQ codes decoded on the fly from the
//        HBM-resident store (layer 1, fused gather + decode) or the previous layer's ntgt states.
//   ('ntgt','intra','ntgt')  chain_attn (chain_attn.hip)
//   ('tgt','intra','tgt')    causal_softmax, causal_attn_fused (causal_attn.hip), causal_attn_varlen (causal_varlen.hip)
#include "kernels.h"
#include "star_route.h"

namespace gnnlm {
namespace {


// One workgroup (4 waves) per token.  QPL = float4 chunks of the feature row held per lane: lane l owns
// the contiguous floats [16*QPL*l/4 ...), i.e. (for dsub = 8, QPL = 4) the two sub-quantizers 2l, 2l+1.
// The token's kg code rows (kg x M bytes = 16 KiB at 128 x 128) are staged into LDS once with
// coalesced 16-B loads -- one full 128-B line per neighbour, the only HBM traffic of the kernel --
// so the per-neighbour dependent chain is LDS byte -> L2 centroid gather, and two neighbours are in
// flight per wave to cover the L2 latency.
//
// Measured dead ends (round 1, 2048 tokens x 128 neighbours, this kernel = 405 us): streaming the centroid
// table through LDS in 32/64-dim chunks with lane = neighbour (no cross-lane reduction) and U either on
// the scalar path (s_load -> SGPR operands; 1230 us: SGPR spills + exposed scalar latency at 1 wave/SIMD)
// or broadcast from LDS with two neighbours per lane (640 us: random 32-B LDS reads conflict, 128 barriers
// per workgroup, 1 workgroup per CU).  The L2 gather below moves a 128-B line per 32 useful bytes but keeps
// 8 waves per CU in flight; it stays until a formulation with >= 2 workgroups per CU is found.
template <int QPL>
__global__ __launch_bounds__(256) void star_attn_kernel(StarAttnParams p, bool stage_codes) {
    // stage_codes = false (k_g too large for LDS, e.g. the k_g = 1024 stress): code bytes are read from
    // the store directly
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sc = smem;                               // [HB][kg] scores, then alphas
    float* zred = smem + HB * p.kg;                 // [HB][D]  cross-wave reduction of Z
    int* okf = reinterpret_cast<int*>(zred + HB * p.D);          // [kg] neighbour validity
    uint8_t* lcodes = reinterpret_cast<uint8_t*>(okf + ((p.kg + 3) & ~3));   // [kg][M] (PQ source only)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x;
    const int D = p.D, kg = p.kg, nq = D / 4, M = p.M;
    const int64_t* ids = p.ids + (int64_t)i * kg;
    const int q_per_m = p.codes ? p.dsub / 4 : 1;

    for (int j = tid; j < kg; j += 256) okf[j] = star_nb_ok(p, i, j, ids[j]);
    __syncthreads();
    if (p.codes && stage_codes) {
        if ((M & 15) == 0) {
            const int per_row = M >> 4;
            for (int e = tid; e < kg * per_row; e += 256) {
                const int j = e / per_row, part = e - j * per_row;
                const int64_t id = ids[j];
                const int64_t lrow = p.codes_direct ? (p.codes_index ? (int64_t)p.codes_index[((int64_t)i * kg + j) * p.codes_direct] : ((int64_t)i * kg + j) * p.codes_direct) : id - p.row0;
                uint4 v = make_uint4(0, 0, 0, 0);
                if (okf[j]) v = *reinterpret_cast<const uint4*>(p.codes + lrow * M + 16 * part);
                *reinterpret_cast<uint4*>(lcodes + j * M + 16 * part) = v;
            }
        } else {
            for (int e = tid; e < kg * M; e += 256) {
                const int j = e / M, m = e - j * M;
                const int64_t id = ids[j];
                const int64_t lrow = p.codes_direct ? (p.codes_index ? (int64_t)p.codes_index[((int64_t)i * kg + j) * p.codes_direct] : ((int64_t)i * kg + j) * p.codes_direct) : id - p.row0;
                lcodes[e] = okf[j] ? p.codes[lrow * M + m] : 0;
            }
        }
    }
    __syncthreads();

    // x_j chunk of this lane (zero for invalid neighbours / lanes beyond D)
    auto load_x = [&](int j, float4 (&x)[QPL]) {
        const bool ok = j < kg && okf[j];
#pragma unroll
        for (int t = 0; t < QPL; ++t) {
            const int q = QPL * lane + t;
            x[t] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok && q < nq) {
                if (p.codes) {
                    const int m = q / q_per_m;
                    const int within = (q - m * q_per_m) * 4;
                    int code;
                    if (stage_codes) {
                        code = lcodes[j * M + m];
                    } else {
                        const int64_t lrow = p.codes_direct ? (p.codes_index ? (int64_t)p.codes_index[((int64_t)i * kg + j) * p.codes_direct] : ((int64_t)i * kg + j) * p.codes_direct) : ids[j] - p.row0;
                        code = p.codes[lrow * M + m];
                    }
                    x[t] = *reinterpret_cast<const float4*>(p.centroids + ((int64_t)(m * 256 + code)) * p.dsub + within);
                } else {
                    x[t] = *reinterpret_cast<const float4*>(p.X + star_group(p, i, j) * p.x_group_stride * p.ldx + 4 * q);
                }
            }
        }
    };

    for (int h0 = 0; h0 < p.H; h0 += HB) {
        // ---- pass 1: scores s[h][j] = x_j . U[i,h,:]
        {
            float4 u[HB][QPL];
#pragma unroll
            for (int h = 0; h < HB; ++h)
#pragma unroll
                for (int t = 0; t < QPL; ++t) {
                    const int q = QPL * lane + t;
                    u[h][t] = (h0 + h < p.H && q < nq)
                                  ? *reinterpret_cast<const float4*>(p.U + ((int64_t)i * p.H + h0 + h) * D + 4 * q)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            for (int j = wave; j < kg; j += 8) {
                float4 xa[QPL], xb[QPL];
                load_x(j, xa);
                load_x(j + 4, xb);
                float pa[HB], pb[HB];
#pragma unroll
                for (int h = 0; h < HB; ++h) {
                    float a = 0.f, b = 0.f;
#pragma unroll
                    for (int t = 0; t < QPL; ++t) {
                        a = fmaf(xa[t].x, u[h][t].x, a); b = fmaf(xb[t].x, u[h][t].x, b);
                        a = fmaf(xa[t].y, u[h][t].y, a); b = fmaf(xb[t].y, u[h][t].y, b);
                        a = fmaf(xa[t].z, u[h][t].z, a); b = fmaf(xb[t].z, u[h][t].z, b);
                        a = fmaf(xa[t].w, u[h][t].w, a); b = fmaf(xb[t].w, u[h][t].w, b);
                    }
                    pa[h] = a;
                    pb[h] = b;
                }
                const float ta = reduce8(pa, lane), tb = reduce8(pb, lane);
                if ((lane & 7) == 0) {
                    sc[(lane >> 3) * kg + j] = okf[j] ? ta : -INFINITY;
                    if (j + 4 < kg) sc[(lane >> 3) * kg + j + 4] = okf[j + 4] ? tb : -INFINITY;
                }
            }
        }
        __syncthreads();
        // ---- softmax over j per head (wave w: heads w, w+4)
        for (int h = wave; h < HB; h += 4) {
            float mx = -INFINITY;
            for (int j = lane; j < kg; j += 64) mx = fmaxf(mx, sc[h * kg + j]);
            mx = wave_max(mx);
            float sum = 0.f;
            int cnt = 0;
            for (int j = lane; j < kg; j += 64) {
                const float s = sc[h * kg + j];
                const bool ok = s != -INFINITY;
                const float e = ok ? expf(s - mx) : 0.f;
                cnt += ok;
                sum += e;
                sc[h * kg + j] = e;
            }
            sum = wave_sum(sum);
            const float inv = sum > 0.f ? 1.f / sum : 0.f;
            for (int j = lane; j < kg; j += 64) sc[h * kg + j] *= inv;
            if (h == 0 && h0 == 0) {
                cnt = (int)wave_sum((float)cnt);
                if (lane == 0 && p.has_nb) p.has_nb[i] = cnt > 0 ? 1.f : 0.f;
            }
        }
        __syncthreads();
        // ---- pass 2: Z[h,:] = sum_j alpha[h][j] x_j   (alpha = 0 and x = 0 for invalid neighbours)
        {
            float4 z[HB][QPL];
#pragma unroll
            for (int h = 0; h < HB; ++h)
#pragma unroll
                for (int t = 0; t < QPL; ++t) z[h][t] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int j = wave; j < kg; j += 8) {
                float4 xa[QPL], xb[QPL];
                load_x(j, xa);
                load_x(j + 4, xb);
                const bool hb = j + 4 < kg;
#pragma unroll
                for (int h = 0; h < HB; ++h) {
                    const float a = sc[h * kg + j];
                    const float b = hb ? sc[h * kg + j + 4] : 0.f;
#pragma unroll
                    for (int t = 0; t < QPL; ++t) {
                        z[h][t].x = fmaf(a, xa[t].x, z[h][t].x); z[h][t].x = fmaf(b, xb[t].x, z[h][t].x);
                        z[h][t].y = fmaf(a, xa[t].y, z[h][t].y); z[h][t].y = fmaf(b, xb[t].y, z[h][t].y);
                        z[h][t].z = fmaf(a, xa[t].z, z[h][t].z); z[h][t].z = fmaf(b, xb[t].z, z[h][t].z);
                        z[h][t].w = fmaf(a, xa[t].w, z[h][t].w); z[h][t].w = fmaf(b, xb[t].w, z[h][t].w);
                    }
                }
            }
            // deterministic cross-wave reduction: waves add in order 0,1,2,3
            for (int w = 0; w < 4; ++w) {
                if (wave == w) {
#pragma unroll
                    for (int h = 0; h < HB; ++h)
#pragma unroll
                        for (int t = 0; t < QPL; ++t) {
                            const int q = QPL * lane + t;
                            if (q < nq) {
                                float4* dst = reinterpret_cast<float4*>(zred + h * D + 4 * q);
                                if (w == 0) {
                                    *dst = z[h][t];
                                } else {
                                    float4 c = *dst;
                                    c.x += z[h][t].x; c.y += z[h][t].y; c.z += z[h][t].z; c.w += z[h][t].w;
                                    *dst = c;
                                }
                            }
                        }
                }
                __syncthreads();
            }
            for (int e = tid; e < HB * nq; e += 256) {
                const int h = e / nq, q = e - h * nq;
                if (h0 + h < p.H)
                    *reinterpret_cast<float4*>(p.Z + ((int64_t)i * p.H + h0 + h) * D + 4 * q) =
                        *reinterpret_cast<const float4*>(zred + h * D + 4 * q);
            }
        }
        __syncthreads();
    }
}

}  // namespace

int star_attn(const StarAttnParams& p, hipStream_t stream) {
    GNNLM_REQUIRE(p.U && p.ids && p.Z, "star_attn: null operand");
    GNNLM_REQUIRE(p.T >= 0 && p.H > 0 && p.kg > 0 && p.D > 0 && p.D % 4 == 0 && p.D <= 1024,
                  "star_attn: need D % 4 == 0 and D <= 1024");
    const bool pq = p.codes != nullptr || p.shards != nullptr;
    GNNLM_REQUIRE(pq != (p.X != nullptr), "star_attn: exactly one of codes (or mapped shards) / X");
    GNNLM_REQUIRE(!p.shards || (!p.codes_direct && p.n_store > 0), "star_attn: a shard table needs n_store and no fetched codes");
    if (pq) {
        GNNLM_REQUIRE(p.centroids && p.M > 0 && p.dsub % 4 == 0 && p.M * p.dsub == p.D,
                      "star_attn: PQ source needs centroids and M*dsub == D, dsub % 4 == 0");
    } else {
        GNNLM_REQUIRE(p.ldx % 4 == 0 && (uintptr_t)p.X % 16 == 0, "star_attn: X alignment");
    }
    // every kernel moves U, Z and the centroid rows 16 bytes at a time, and the code rows too when M % 16 == 0
    GNNLM_REQUIRE((uintptr_t)p.U % 16 == 0 && (uintptr_t)p.Z % 16 == 0 && (uintptr_t)p.centroids % 16 == 0 &&
                      (p.M % 16 != 0 || (uintptr_t)p.codes % 16 == 0),
                  "star_attn: U, Z, centroids (and codes when M % 16 == 0) must be 16-byte aligned");
    if (p.T == 0) return OK;
    const StarPlan plan = star_route(p, star_switches());
    GNNLM_REQUIRE(!p.shards || star_route_is_tab(plan.route),
                  "star_attn: mapped shards need the table-resident kernel (k_g <= 128, dsub 4 / 8, M % 16 == 0)");
    GNNLM_REQUIRE(plan.lds_bytes <= (size_t)STAR_LDS_MAX, "star_attn: kg too large for LDS");
    const double rows = (double)p.T * p.kg;
    ProfScope prof(K_STAR, stream, 4.0 * rows * p.H * p.D, rows * (8.0 + (p.X ? 4.0 * p.D : (double)p.M)) + 8.0 * p.T * p.H * p.D);
    const dim3 grid(p.T), block(plan.threads);
    switch (plan.route) {
        case StarRoute::NONE: return OK;                        // (T == 0: returned above)
        case StarRoute::TAB8M:
        case StarRoute::TAB8:
        case StarRoute::TAB4: return star_attn_tab(p, plan, stream);
        case StarRoute::DENSE1:
        case StarRoute::DENSE2:
        case StarRoute::DENSE4: return star_attn_dense(p, plan, stream);
        case StarRoute::GENERIC1: hipLaunchKernelGGL(star_attn_kernel<1>, grid, block, plan.lds_bytes, stream, p, plan.staged); break;
        case StarRoute::GENERIC2: hipLaunchKernelGGL(star_attn_kernel<2>, grid, block, plan.lds_bytes, stream, p, plan.staged); break;
        case StarRoute::GENERIC4: hipLaunchKernelGGL(star_attn_kernel<4>, grid, block, plan.lds_bytes, stream, p, plan.staged); break;
    }
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
