// Token-embedding neighbour features (`--reinit-nfeat`: "use word embedding as neighbor node feature instead of cached
// representation", fairseq/tasks/language_modeling.py:151-153).
//
// Replaces, per token block, the label gathers of the reference's graph builder
//   neighbor_tokens[offset]                                   fairseq/data/token_block_dataset.py:369-371,392-394,407-410
// (the only thing it attaches to the ntgt nodes when no quantized-keys.npy is loaded, language_modeling.py:273-278) and
//   ntgt_feat = self.embed_tokens(graph.nodes["ntgt"].data["labels"])        fairseq/models/transformer.py:1046-1048
// with `embed_tokens` materialised once as a [V, d] f32 table (gnn-lm_amd/token_embed.py, imported as gnnlm_amd.token_embed).
// Slot order and validity are those of gather_decode_kernel (gather_decode.hip): slot c of a group is row o (c = 0),
// o-left .. o-1, o+1 .. o+right.
//
// HBM-bound: a row is d * 4 bytes (4 KB at d = 1024) read from a random place of the table and written once.  One wave per
// GROUP: its 1 + left + right labels come from one load instruction (lane c holds slot c), then the rows are copied with
// 16 B per lane, up to four independent loads in flight per lane before the first store (a 4-KB row is one trip).
#include "kernels.h"

namespace gnnlm {
namespace {

__device__ __forceinline__ int32_t load_label(const void* vals, int itemsize, int64_t row) {
    return itemsize == 2 ? (int32_t) reinterpret_cast<const int16_t*>(vals)[row] : reinterpret_cast<const int32_t*>(vals)[row];
}

__global__ __launch_bounds__(256) void token_gather_kernel(gnnlm_token_gather_t p) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const int n_g = 1 + p.left + p.right;
    const int64_t n_groups = p.n_groups_dev ? min(p.n_groups, (int64_t)*p.n_groups_dev) : p.n_groups;
    const int nq = p.d / 4;                     // float4 per row

    for (int64_t g = wave; g < n_groups; g += nwaves) {
        const int64_t centre = p.ids[g];
        const bool centre_ok = centre >= 0 && centre < p.n_store + p.left;       // (beyond: no slot can be a row; keeps centre + delta in range)
        for (int c0 = 0; c0 < n_g; c0 += 64) {
            const int c = c0 + lane;
            int32_t lab = -1;
            if (c < n_g) {
                const int delta = c == 0 ? 0 : (c <= p.left ? c - 1 - p.left : c - p.left);
                const int64_t row = centre + delta;
                if (centre_ok && row >= 0 && row < p.n_store) {
                    lab = load_label(p.vals, p.vals_itemsize, row);
                    if (lab < 0 || lab >= p.n_vocab) lab = -1;                   // memory safety: never an index outside the table
                }
                const int64_t s = g * n_g + c;
                if (p.out_labels) p.out_labels[s] = lab;
                if (p.out_valid) p.out_valid[s] = lab >= 0 ? 1 : 0;
            }
            if (!p.out_x) continue;
            const int cn = min(64, n_g - c0);
            for (int cc = 0; cc < cn; ++cc) {
                const int32_t l = __shfl(lab, cc, 64);                           // wave-uniform
                const float4* src = reinterpret_cast<const float4*>(p.embed + (int64_t)max(l, 0) * p.ld_embed);      // (not dereferenced unless l >= 0)
                float4* dst = reinterpret_cast<float4*>(p.out_x + (g * n_g + c0 + cc) * p.ld_x);
                for (int q0 = lane; q0 < nq; q0 += 256) {
                    float4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int q = q0 + 64 * u;
                        v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (l >= 0 && q < nq) v[u] = src[q];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int q = q0 + 64 * u;
                        if (q < nq) dst[q] = v[u];
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void neighbor_labels_kernel(const int64_t* ids, int64_t n, int64_t n_store, const void* vals, int itemsize,
                                                              int n_vocab, int32_t* out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t id = ids[e];
        int32_t lab = -1;
        if (id >= 0 && id < n_store) {
            lab = load_label(vals, itemsize, id);
            if (lab < 0 || lab >= n_vocab) lab = -1;
        }
        out[e] = lab;
    }
}

}  // namespace

int token_gather(const gnnlm_token_gather_t& p, hipStream_t stream) {
    GNNLM_REQUIRE(p.left >= 0 && p.right >= 0 && p.n_groups >= 0 && p.n_store >= 0, "token_gather: bad shape");
    if (p.n_groups == 0) return OK;
    GNNLM_REQUIRE(p.ids && p.vals, "token_gather: null ids / vals");
    GNNLM_REQUIRE(p.vals_itemsize == 2 || p.vals_itemsize == 4, "token_gather: vals must be int16 or int32");
    GNNLM_REQUIRE(p.n_vocab > 0, "token_gather: n_vocab must be positive");
    GNNLM_REQUIRE(!p.out_x || (p.embed && p.d > 0 && p.d % 4 == 0 && p.ld_embed >= p.d && p.ld_embed % 4 == 0 && p.ld_x >= p.d && p.ld_x % 4 == 0 &&
                               (uintptr_t)p.embed % 16 == 0 && (uintptr_t)p.out_x % 16 == 0),
                  "token_gather: out_x needs embed, d % 4 == 0, ld_embed / ld_x >= d and multiples of 4, 16-byte alignment");
    GNNLM_REQUIRE((1 + (int64_t)p.left + p.right) * p.n_groups < (1ll << 40), "token_gather: too many slots");
    if (!p.out_x && !p.out_labels && !p.out_valid) return OK;
    const int64_t n_slots = p.n_groups * (1 + p.left + p.right);
    const double row_bytes = (double)p.vals_itemsize + (p.out_x ? 8.0 * p.d : 0.0) + (p.out_labels ? 4.0 : 0.0) + (p.out_valid ? 1.0 : 0.0);
    ProfScope prof(K_GATHER, stream, 0.0, row_bytes * n_slots + 8.0 * p.n_groups);
    const int64_t blocks = std::min<int64_t>(cdiv(p.n_groups, 4), 256 * 16);
    hipLaunchKernelGGL(token_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, p);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

int neighbor_labels(const int64_t* ids, int64_t n, int64_t n_store, const void* vals, int itemsize, int n_vocab, int32_t* out,
                    hipStream_t stream) {
    GNNLM_REQUIRE(n >= 0 && n_store >= 0 && n_vocab > 0, "neighbor_labels: bad shape");
    if (n == 0) return OK;
    GNNLM_REQUIRE(ids && vals && out, "neighbor_labels: null operand");
    GNNLM_REQUIRE(itemsize == 2 || itemsize == 4, "neighbor_labels: vals must be int16 or int32");
    const int64_t blocks = std::min<int64_t>(cdiv(n, 256), 256 * 16);
    ProfScope prof(K_MISC, stream, 0.0, (12.0 + itemsize) * n);
    hipLaunchKernelGGL(neighbor_labels_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, ids, n, n_store, vals, itemsize, n_vocab, out);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm
