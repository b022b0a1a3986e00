// gnnlm_store_*: a shard of the datastore's code and label rows in device memory, owned by the library (include/gnnlm.h).
#include <algorithm>

#include "kernels.h"

using namespace gnnlm;

struct gnnlm_store {
    int64_t n_store, row0, n_local;
    int32_t M, vals_itemsize, device;
    uint8_t* codes;
    void* vals;
};

extern "C" {

int gnnlm_store_create(int64_t n_store, int64_t row0, int64_t n_local, int32_t M, int32_t vals_itemsize,
                       int32_t device, gnnlm_store_t** out) {
    GNNLM_REQUIRE(out && n_store > 0 && row0 >= 0 && n_local >= 0 && row0 + n_local <= n_store && M > 0,
                  "store_create: bad shape");
    GNNLM_REQUIRE(vals_itemsize == 2 || vals_itemsize == 4, "store_create: vals must be int16 or int32");
    GNNLM_HIP(hipSetDevice(device));
    gnnlm_store* s = new gnnlm_store{n_store, row0, n_local, M, vals_itemsize, device, nullptr, nullptr};
    // an empty shard (more ranks than rows) keeps a 1-row allocation so that the pointers stay non-null
    hipError_t e = hipMalloc((void**)&s->codes, (size_t)std::max<int64_t>(n_local, 1) * M);
    if (e == hipSuccess) e = hipMalloc(&s->vals, (size_t)std::max<int64_t>(n_local, 1) * vals_itemsize);
    if (e != hipSuccess) {
        if (s->codes) (void)hipFree(s->codes);
        delete s;
        set_error(std::string("store_create: hipMalloc failed: ") + hipGetErrorString(e));
        return E_NOMEM;
    }
    *out = s;
    return OK;
}
int gnnlm_store_upload_codes(gnnlm_store_t* s, const uint8_t* host, int64_t first, int64_t n, void* stream) {
    GNNLM_REQUIRE(s && host && first >= 0 && n >= 0 && first + n <= s->n_local, "store_upload_codes: bad range");
    GNNLM_HIP(hipMemcpyAsync(s->codes + first * s->M, host, (size_t)n * s->M, hipMemcpyHostToDevice, (hipStream_t)stream));
    GNNLM_HIP(hipStreamSynchronize((hipStream_t)stream));
    return OK;
}
int gnnlm_store_upload_vals(gnnlm_store_t* s, const void* host, int64_t first, int64_t n, void* stream) {
    GNNLM_REQUIRE(s && host && first >= 0 && n >= 0 && first + n <= s->n_local, "store_upload_vals: bad range");
    GNNLM_HIP(hipMemcpyAsync((char*)s->vals + first * s->vals_itemsize, host, (size_t)n * s->vals_itemsize,
                             hipMemcpyHostToDevice, (hipStream_t)stream));
    GNNLM_HIP(hipStreamSynchronize((hipStream_t)stream));
    return OK;
}
const uint8_t* gnnlm_store_codes(const gnnlm_store_t* s) { return s ? s->codes : nullptr; }
const void* gnnlm_store_vals(const gnnlm_store_t* s) { return s ? s->vals : nullptr; }
int gnnlm_store_destroy(gnnlm_store_t* s) {
    if (!s) return OK;
    if (s->codes) (void)hipFree(s->codes);
    if (s->vals) (void)hipFree(s->vals);
    delete s;
    return OK;
}

}  // extern "C"
