// Removing keys from an IVF-PQ index (faiss's `remove_ids`; the reference only trains and adds, knn/index_builder.py): which rows of
// the list-ordered arrays survive a set of id ranges, and the compaction of the survivors, list by list, order kept.
//
//   ivfpq_keep_flags: one thread per row; its id is looked up in the sorted ranges by bisection, its list in the offsets by
//     bisection.  The survivors of a list are counted per wave (rows of a wave are consecutive, so the lanes of one list are one
//     run: two ballots, one 64-bit atomic per (wave, list)) into list_keep, which a launch of its own zeroes first.
//   ivfpq_list_compact: a scan in separate launches -- no workgroup waits for another one.  The rows are cut into CHUNKS of 1024,
//     whatever the lists are (one list of 10^7 rows is 10^4 chunks, a million lists of 100 rows are ten lists per chunk):
//       count    per chunk: the survivors of the chunk -> prefix[c]; and, from the in-chunk scan, for every list boundary that
//                lies in the chunk the survivors between the chunk's first row and the boundary -> list_part[l]
//       scan     one workgroup: prefix[] <- its exclusive sum (4 M chunks at 2^32 rows: 512 tiles of 8192)
//       scatter  per chunk: G(row) = prefix[c] + in-chunk rank is the survivors ahead of the row in the whole index, G(off[l]) =
//                prefix[chunk of off[l]] + list_part[l] those ahead of its list; their difference r is the row's rank in its list
//                and new_off[l] + r its place, taken only if r < new_off[l + 1] - new_off[l].  Places stand in LDS; then the
//                chunk's code rows move 16 bytes per lane (4 KiB contiguous per step of the workgroup) and the ids 8 bytes.
//     Every number is an integer sum over fixed index sets: the result does not depend on the grid or on what else runs.
#include "kernels.h"

namespace gnnlm {
namespace {

constexpr int RM_CHUNK = 1024;        // rows of a chunk: 256 threads x 4 rows
constexpr int RM_SCAN_ITEMS = 8;      // chunk counts per thread and tile of the scan launch (1024 threads)

// the last l in [0, nlist) with off[l] <= s (the list of row s when off is monotone from 0; always inside [0, nlist))
__device__ __forceinline__ int list_of_row(const int64_t* off, int nlist, int64_t s) {
    int lo = 0, hi = nlist;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= s) lo = mid; else hi = mid;
    }
    return lo;
}
// the first l in [0, nlist] with off[l] >= x (nlist + 1: none)
__device__ __forceinline__ int first_list_from(const int64_t* off, int nlist, int64_t x) {
    int lo = 0, hi = nlist + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] >= x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void ivfpq_keep_zero_kernel(int64_t* list_keep, int nlist) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < nlist) list_keep[l] = 0;
}

__global__ __launch_bounds__(256) void ivfpq_keep_flags_kernel(gnnlm_ivfpq_keep_flags_t p) {
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < p.N; base += (int64_t)gridDim.x * 256) {   // (uniform per workgroup: whole waves vote)
        const int64_t s = base + threadIdx.x;
        const bool live = s < p.N;
        bool kept = false;
        int l = -1;
        if (live) {
            const int64_t id = p.ids[s];
            int64_t lo = 0, hi = p.n_ranges;                          // the first range whose lo lies above id
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (p.ranges[2 * mid] <= id) lo = mid + 1; else hi = mid;
            }
            kept = !(lo > 0 && id < p.ranges[2 * (lo - 1) + 1]);
            p.keep[s] = kept ? 1 : 0;
            l = list_of_row(p.list_off, p.nlist, s);
        }
        if (!p.list_keep) continue;
        const unsigned long long K = __ballot(kept);
        const int lprev = __shfl_up(l, 1);
        const bool head = live && (lane == 0 || l != lprev);          // first lane of its list's run in this wave
        const unsigned long long H = __ballot(head);
        if (head) {
            const unsigned long long from = ~0ull << lane;            // lanes >= this one
            const unsigned long long above = lane == 63 ? 0ull : H & (~0ull << (lane + 1));
            const unsigned long long run = above ? from & ((1ull << __builtin_ctzll(above)) - 1) : from;
            const int c = __popcll(K & run);
            if (c) atomicAdd(reinterpret_cast<unsigned long long*>(p.list_keep) + l, (unsigned long long)c);
        }
    }
}

// bit k: row s0 + k survives (rows from N0 on: no)
__device__ __forceinline__ unsigned keep4(const uint8_t* keep, int64_t s0, int64_t N0, bool aligned) {
    if (s0 + 4 <= N0 && aligned) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(keep + s0);
        return (w & 0xffu ? 1u : 0u) | (w & 0xff00u ? 2u : 0u) | (w & 0xff0000u ? 4u : 0u) | (w & 0xff000000u ? 8u : 0u);
    }
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (s0 + k < N0 && keep[s0 + k]) m |= 1u << k;
    return m;
}

// exclusive sum of v over the 256 threads of the workgroup, and the total (s_w: 4 ints, free again after the caller's next barrier)
__device__ __forceinline__ int block_scan_256(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int n = __shfl_up(inc, d);
        if (lane >= d) inc += n;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < w) base += s_w[i];
        total += s_w[i];
    }
    return base + inc - v;
}

// the lists whose old offset lies in chunk c: [begin, end) of l in [0, nlist]; the last chunk also takes the offsets equal to N0
__device__ __forceinline__ void chunk_lists(const int64_t* off, int nlist, int64_t N0, int64_t start, bool last, int& begin, int& end) {
    begin = first_list_from(off, nlist, start);
    end = last ? nlist + 1 : first_list_from(off, nlist, min(start + RM_CHUNK, N0));
}

__global__ __launch_bounds__(256) void ivfpq_compact_count_kernel(gnnlm_ivfpq_list_compact_t p, int64_t* prefix, int64_t* list_part, bool keep_aligned) {
    __shared__ int s_w[4];
    __shared__ uint16_t s_rank[RM_CHUNK + 1];                         // survivors of the chunk ahead of row i of it
    const int t = threadIdx.x;
    const int64_t start = (int64_t)blockIdx.x * RM_CHUNK;
    const unsigned m = keep4(p.keep, start + 4 * t, p.N0, keep_aligned);
    int total;
    const int ex = block_scan_256(__popc(m), s_w, total);
#pragma unroll
    for (int k = 0; k < 4; ++k) s_rank[4 * t + k] = (uint16_t)(ex + __popc(m & ((1u << k) - 1)));
    if (t == 0) {
        s_rank[RM_CHUNK] = (uint16_t)total;
        prefix[blockIdx.x] = total;
    }
    __syncthreads();
    int begin, end;
    chunk_lists(p.list_off_old, p.nlist, p.N0, start, blockIdx.x == gridDim.x - 1, begin, end);
    for (int l = begin + t; l < end; l += 256) {
        const int64_t i = p.list_off_old[l] - start;
        list_part[l] = s_rank[i < 0 ? 0 : i > RM_CHUNK ? RM_CHUNK : i];
    }
}

__global__ __launch_bounds__(1024) void ivfpq_compact_scan_kernel(int64_t* prefix, int64_t n) {
    __shared__ int64_t s_w[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    int64_t carry = 0;
    for (int64_t tile = 0; tile < n; tile += 1024 * RM_SCAN_ITEMS) {
        const int64_t i0 = tile + (int64_t)t * RM_SCAN_ITEMS;
        int64_t v[RM_SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int k = 0; k < RM_SCAN_ITEMS; ++k) {
            v[k] = i0 + k < n ? prefix[i0 + k] : 0;
            sum += v[k];
        }
        int64_t inc = sum;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        int64_t run = carry, tile_total = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < w) run += s_w[i];
            tile_total += s_w[i];
        }
        run += inc - sum;
#pragma unroll
        for (int k = 0; k < RM_SCAN_ITEMS; ++k) {
            if (i0 + k < n) prefix[i0 + k] = run;
            run += v[k];
        }
        carry += tile_total;
        __syncthreads();                                              // s_w is written again by the next tile
    }
}

__global__ __launch_bounds__(256) void ivfpq_compact_scatter_kernel(gnnlm_ivfpq_list_compact_t p, const int64_t* prefix, const int64_t* list_part, bool keep_aligned) {
    __shared__ int s_w[4];
    __shared__ int64_t s_dst[RM_CHUNK];                               // where row i of the chunk goes, -1: nowhere
    const int t = threadIdx.x;
    const int64_t n_chunks = gridDim.x;
    const int64_t start = (int64_t)blockIdx.x * RM_CHUNK, s0 = start + 4 * t;
    const int64_t n_new = p.new_off[p.nlist];
    // survivors ahead of list l in the whole index (an offset equal to N0 was counted by the last chunk)
    auto ahead_of_list = [&](int l) {
        const int64_t c = p.list_off_old[l] >> 10;
        return prefix[c < 0 ? 0 : c >= n_chunks ? n_chunks - 1 : c] + list_part[l];
    };
    const unsigned m = keep4(p.keep, s0, p.N0, keep_aligned);
    int total;
    const int ex = block_scan_256(__popc(m), s_w, total);
    const int64_t ahead = prefix[blockIdx.x] + ex;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int64_t d = -1;
        if (m >> k & 1) {
            const int l = list_of_row(p.list_off_old, p.nlist, s0 + k);
            const int64_t r = ahead + __popc(m & ((1u << k) - 1)) - ahead_of_list(l);
            const int64_t at = p.new_off[l], len = p.new_off[l + 1] - at;
            if (r >= 0 && r < len && at >= 0 && at + r < n_new) d = at + r;   // a list writes inside its own slot only
        }
        s_dst[4 * t + k] = d;
    }
    __syncthreads();
    if (p.n_bad) {                                                    // every list is checked by the chunk its old offset lies in
        int begin, end;
        chunk_lists(p.list_off_old, p.nlist, p.N0, start, blockIdx.x == gridDim.x - 1, begin, end);
        end = min(end, p.nlist);
        for (int l = begin + t; l < end; l += 256)
            if (ahead_of_list(l + 1) - ahead_of_list(l) != p.new_off[l + 1] - p.new_off[l]) atomicAdd(p.n_bad, 1);
    }
    const int per_row = p.M >> 4;                                     // 16-byte pieces of a code row
    const int rows = (int)min((int64_t)RM_CHUNK, p.N0 - start);
    const int pieces = rows * per_row;
#pragma unroll 4
    for (int i = t; i < pieces; i += 256) {
        const int row = i / per_row, part = i - row * per_row;
        const int64_t d = s_dst[row];
        if (d >= 0)
            *reinterpret_cast<uint4*>(p.codes + d * p.M + 16 * part) = *reinterpret_cast<const uint4*>(p.codes_old + (start + row) * p.M + 16 * part);
    }
    for (int i = t; i < rows; i += 256) {
        const int64_t d = s_dst[i];
        if (d >= 0) p.ids[d] = p.ids_old[start + i];
    }
}

}  // namespace

int ivfpq_keep_flags(const gnnlm_ivfpq_keep_flags_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.N >= 0 && d.nlist >= 0 && d.n_ranges >= 0, "ivfpq_keep_flags: negative size");
    GNNLM_REQUIRE(d.N == 0 || d.nlist > 0, "ivfpq_keep_flags: rows without lists");
    GNNLM_REQUIRE(d.N == 0 || (d.ids && d.list_off && d.keep), "ivfpq_keep_flags: null operand");
    GNNLM_REQUIRE(d.n_ranges == 0 || d.ranges, "ivfpq_keep_flags: null ranges");
    if (d.list_keep && d.nlist > 0) {
        hipLaunchKernelGGL(ivfpq_keep_zero_kernel, dim3((unsigned)cdiv(d.nlist, 256)), dim3(256), 0, stream, d.list_keep, d.nlist);
        GNNLM_LAUNCH_CHECK();
    }
    if (d.N == 0) return OK;
    const unsigned blocks = (unsigned)std::min<int64_t>(cdiv(d.N, 256), 256 * 64);
    hipLaunchKernelGGL(ivfpq_keep_flags_kernel, dim3(blocks), dim3(256), 0, stream, d);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

size_t ivfpq_list_compact_workspace_bytes(int64_t N0, int nlist) {
    if (N0 <= 0 || nlist <= 0) return 0;
    return (size_t)(cdiv(N0, RM_CHUNK) + nlist + 1) * sizeof(int64_t);
}

int ivfpq_list_compact(const gnnlm_ivfpq_list_compact_t& d, hipStream_t stream) {
    GNNLM_REQUIRE(d.N0 >= 0 && d.nlist >= 0 && d.M > 0, "ivfpq_list_compact: negative size");
    GNNLM_REQUIRE(d.M % 16 == 0, "ivfpq_list_compact: need M % 16 == 0");
    GNNLM_REQUIRE(d.N0 == 0 || d.nlist > 0, "ivfpq_list_compact: rows without lists");
    if (d.N0 == 0) return OK;
    GNNLM_REQUIRE(d.list_off_old && d.ids_old && d.codes_old && d.keep && d.new_off && d.ids && d.codes, "ivfpq_list_compact: null operand");
    GNNLM_REQUIRE((uintptr_t)d.codes_old % 16 == 0 && (uintptr_t)d.codes % 16 == 0, "ivfpq_list_compact: code rows are 16-byte aligned");
    GNNLM_REQUIRE(d.codes != d.codes_old && d.ids != d.ids_old, "ivfpq_list_compact: the outputs are buffers of their own");
    const int64_t n_chunks = cdiv(d.N0, RM_CHUNK);
    GNNLM_REQUIRE(n_chunks < (1ll << 31), "ivfpq_list_compact: too many rows for one launch");
    GNNLM_REQUIRE(d.workspace && (uintptr_t)d.workspace % 8 == 0 && d.workspace_bytes >= ivfpq_list_compact_workspace_bytes(d.N0, d.nlist),
                  "ivfpq_list_compact: workspace of gnnlm_ivfpq_list_compact_workspace_bytes(N0, nlist), 8-byte aligned");
    int64_t* prefix = static_cast<int64_t*>(d.workspace);
    int64_t* list_part = prefix + n_chunks;
    const bool keep_aligned = (uintptr_t)d.keep % 4 == 0;
    hipLaunchKernelGGL(ivfpq_compact_count_kernel, dim3((unsigned)n_chunks), dim3(256), 0, stream, d, prefix, list_part, keep_aligned);
    GNNLM_LAUNCH_CHECK();
    hipLaunchKernelGGL(ivfpq_compact_scan_kernel, dim3(1), dim3(1024), 0, stream, prefix, n_chunks);
    GNNLM_LAUNCH_CHECK();
    hipLaunchKernelGGL(ivfpq_compact_scatter_kernel, dim3((unsigned)n_chunks), dim3(256), 0, stream, d, (const int64_t*)prefix, (const int64_t*)list_part, keep_aligned);
    GNNLM_LAUNCH_CHECK();
    return OK;
}

}  // namespace gnnlm

using namespace gnnlm;

extern "C" {
int gnnlm_ivfpq_keep_flags(const gnnlm_ivfpq_keep_flags_t* d, void* stream) {
    if (!d) { set_error("invalid argument: null descriptor"); return E_INVALID; }
    return ivfpq_keep_flags(*d, (hipStream_t)stream);
}
size_t gnnlm_ivfpq_list_compact_workspace_bytes(int64_t N0, int32_t nlist) { return ivfpq_list_compact_workspace_bytes(N0, nlist); }
int gnnlm_ivfpq_list_compact(const gnnlm_ivfpq_list_compact_t* d, void* stream) {
    if (!d) { set_error("invalid argument: null descriptor"); return E_INVALID; }
    return ivfpq_list_compact(*d, (hipStream_t)stream);
}
}
