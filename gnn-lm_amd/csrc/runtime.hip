// Process state of libgnnlm_hip.so: the last-error string, the per-device LDS opt-in table and the event profiler, with the C
// entries that read them (include/gnnlm.h).
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "kernels.h"

namespace gnnlm {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    char buf[512];
    snprintf(buf, sizeof(buf), "HIP error %d (%s) in `%s` at %s:%d", (int)e, hipGetErrorString(e), what, file, line);
    g_last_error = buf;
    return E_HIP;
}

int lds_opt_in(const void* kernel_fn, int bytes) {
    static std::mutex mu;
    static std::vector<std::pair<const void*, int>> done;       // (function, device) pairs already opted in
    int dev = 0;
    GNNLM_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& e : done)
        if (e.first == kernel_fn && e.second == dev) return OK;
    GNNLM_HIP(hipFuncSetAttribute(kernel_fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.emplace_back(kernel_fn, dev);
    return OK;
}

// ---------------------------------------------------------------------------------------------
// profiler: (start, stop) event pairs per launch, resolved at gnnlm_profile_end
// ---------------------------------------------------------------------------------------------
unsigned g_prof_mask = 0;
namespace {
struct ProfRec { int kid; hipEvent_t a, b; double flops, bytes; int32_t* host_scale; double den; };
std::vector<ProfRec> g_prof_recs;
std::vector<hipEvent_t> g_event_pool;
std::vector<int32_t*> g_pinned_pool;
// the start event of an open ProfScope is per host thread (one scope per kernel id at a time on a thread); the
// record list and the pools are shared and guarded by g_prof_mu, so launches from several host threads may be
// profiled together
thread_local hipEvent_t g_pending_start[K_COUNT];
std::mutex g_prof_mu;
hipEvent_t take_event() {           // g_prof_mu held; nullptr on failure
    if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}
int32_t* take_pinned() {            // g_prof_mu held; nullptr on failure
    // slots come from slabs of 1024 pinned ints: hipHostMalloc is a heavy, device-synchronising call that must not
    // happen per launch inside a timed region
    if (g_pinned_pool.empty()) {
        int32_t* slab = nullptr;
        if (hipHostMalloc((void**)&slab, 1024 * sizeof(int32_t), hipHostMallocDefault) != hipSuccess || !slab) return nullptr;
        for (int i = 0; i < 1024; ++i) g_pinned_pool.push_back(slab + i);
    }
    int32_t* p = g_pinned_pool.back();
    g_pinned_pool.pop_back();
    return p;
}
}  // namespace
void prof_start(int kid, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_pending_start[kid] = take_event();
    if (g_pending_start[kid]) (void)hipEventRecord(g_pending_start[kid], s);
}
int32_t* prof_take_slot() {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    return take_pinned();           // nullptr: the launch simply does not report its device-side count
}
void prof_stop(int kid, hipStream_t s, double flops, double bytes, const int32_t* scale_dev, double den, int32_t* host_slot) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ProfRec r{kid, g_pending_start[kid], take_event(), flops, bytes, nullptr, den};
    if (!r.a || !r.b) {             // event creation failed: this launch is not recorded
        if (r.a) g_event_pool.push_back(r.a);
        if (r.b) g_event_pool.push_back(r.b);
        if (host_slot) g_pinned_pool.push_back(host_slot);
        return;
    }
    (void)hipEventRecord(r.b, s);
    if (host_slot) {
        r.host_scale = host_slot;                       // written by the kernel itself
    } else if (scale_dev) {
        r.host_scale = take_pinned();
        if (r.host_scale) (void)hipMemcpyAsync(r.host_scale, scale_dev, sizeof(int32_t), hipMemcpyDeviceToHost, s);
    }
    g_prof_recs.push_back(r);
}

}  // namespace gnnlm

using namespace gnnlm;

extern "C" {

int gnnlm_profile_begin(uint32_t kernel_mask) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    GNNLM_REQUIRE(g_prof_recs.empty(), "profile_begin: a profile is already open");
    g_prof_mask = kernel_mask;
    return OK;
}
int gnnlm_profile_end(gnnlm_profile_entry_t* out, int32_t n_max, int32_t* n_out) {
    GNNLM_REQUIRE(out && n_out && n_max >= K_COUNT, "profile_end: need room for every kernel id");
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_mask = 0;
    for (int k = 0; k < K_COUNT; ++k) out[k] = gnnlm_profile_entry_t{k, 0, 0.0, 0.0, 0.0};
    for (auto& r : g_prof_recs) {
        GNNLM_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        GNNLM_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        double scale = 1.0;
        if (r.host_scale) {
            scale = std::min(1.0, (double)*r.host_scale / r.den);
            g_pinned_pool.push_back(r.host_scale);
        }
        out[r.kid].launches += 1;
        out[r.kid].total_ms += ms;
        out[r.kid].flops += r.flops * scale;
        out[r.kid].bytes += r.bytes * scale;
        g_event_pool.push_back(r.a);
        g_event_pool.push_back(r.b);
    }
    g_prof_recs.clear();
    *n_out = K_COUNT;
    return OK;
}

static const char* kKernelNames[K_COUNT] = {"gemm_nt_f32_kernel", "gather_decode_kernel", "star_attn_kernel",
                                            "chain_attn_kernel", "causal_attn_kernel", "layernorm_kernel",
                                            "row_lse_pick_kernel", "knn_interp_kernel", "misc", "split_planes_kernel",
                                            "topk_merge_kernel", "ivfpq_scan_kernel", "ivfpq_scan8_kernel", "ivfpq_rescore_kernel", "ivfpq_sums_kernel", "ivfpq_tau_kernel",
                                            "knn_interp_grid_kernel", "knn_resim_kernel"};
const char* gnnlm_kernel_name(int32_t kernel_id) {
    return kernel_id >= 0 && kernel_id < K_COUNT ? kKernelNames[kernel_id] : nullptr;
}

const char* gnnlm_last_error(void) { return g_last_error.c_str(); }
int gnnlm_abi_version(void) { return GNNLM_ABI_VERSION; }
const char* gnnlm_target_arch(void) { return "gfx950"; }
size_t gnnlm_sizeof(const char* name) {
    if (!name) return 0;
#define GNNLM_SZ(t) if (!strcmp(name, #t)) return sizeof(t);
    GNNLM_SZ(gnnlm_group_assign_t) GNNLM_SZ(gnnlm_gemm_t) GNNLM_SZ(gnnlm_gather_t) GNNLM_SZ(gnnlm_token_gather_t) GNNLM_SZ(gnnlm_star_attn_t) GNNLM_SZ(gnnlm_chain_attn_t)
    GNNLM_SZ(gnnlm_adaptive_softmax_t) GNNLM_SZ(gnnlm_dense_softmax_t) GNNLM_SZ(gnnlm_knn_interp_t) GNNLM_SZ(gnnlm_knn_interp_grid_t) GNNLM_SZ(gnnlm_knn_mix_dense_t) GNNLM_SZ(gnnlm_knn_resim_t) GNNLM_SZ(gnnlm_hgt_layer_t)
    GNNLM_SZ(gnnlm_hgt_t) GNNLM_SZ(gnnlm_hgt_io_t) GNNLM_SZ(gnnlm_profile_entry_t) GNNLM_SZ(gnnlm_topk_t) GNNLM_SZ(gnnlm_ivfpq_scan_t) GNNLM_SZ(gnnlm_ivfpq_scan8_t) GNNLM_SZ(gnnlm_ivfpq_rescore_t) GNNLM_SZ(gnnlm_ivfpq_tau_t) GNNLM_SZ(gnnlm_ivfpq_tables_t) GNNLM_SZ(gnnlm_peer_gather_t) GNNLM_SZ(gnnlm_shards_t) GNNLM_SZ(gnnlm_ragged_t)
    GNNLM_SZ(gnnlm_lm_embed_t) GNNLM_SZ(gnnlm_tlm_layer_t) GNNLM_SZ(gnnlm_tlm_t) GNNLM_SZ(gnnlm_tlm_io_t) GNNLM_SZ(gnnlm_pack_rows_t)
    GNNLM_SZ(gnnlm_kv_cache_t) GNNLM_SZ(gnnlm_decode_attn_t) GNNLM_SZ(gnnlm_tlm_step_io_t) GNNLM_SZ(gnnlm_sample_topk_t) GNNLM_SZ(gnnlm_sample_topp_t)
    GNNLM_SZ(gnnlm_beam_attn_t) GNNLM_SZ(gnnlm_beam_select_t) GNNLM_SZ(gnnlm_beam_select_diverse_t) GNNLM_SZ(gnnlm_ivfpq_select_probes_t) GNNLM_SZ(gnnlm_ivfpq_select_final_t)
    GNNLM_SZ(gnnlm_ivfpq_encode_t) GNNLM_SZ(gnnlm_ivfpq_list_merge_t) GNNLM_SZ(gnnlm_ivfpq_coarse_t)
    GNNLM_SZ(gnnlm_ivfpq_keep_flags_t) GNNLM_SZ(gnnlm_ivfpq_list_compact_t)
#undef GNNLM_SZ
    return 0;
}

}  // extern "C"
