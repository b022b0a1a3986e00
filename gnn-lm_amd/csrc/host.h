// Host-side tools of the orchestrator files (the ones that enqueue several launchers behind one C entry): the workspace
// carver, the early-return macros and the plain `C = A W^T + b` GEMM descriptor.  Kernel files do not include this.
#pragma once
#include <algorithm>

#include "kernels.h"

namespace gnnlm {

// bump allocator over a caller-provided workspace: offsets aligned to 256 bytes; a null base only measures (`off`)
struct Carver {
    char* base;
    size_t off = 0, cap;
    explicit Carver(void* b, size_t c = SIZE_MAX) : base(reinterpret_cast<char*>(b)), cap(c) {}
    template <class T>
    T* take(int64_t n) {
        off = (off + 255) & ~size_t(255);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += (size_t)std::max<int64_t>(n, 0) * sizeof(T);
        return p;
    }
    bool fits() const { return !base || off <= cap; }
};

#define GNNLM_TRY(x)                   \
    do {                               \
        int _rc = (x);                 \
        if (_rc != ::gnnlm::OK) return _rc; \
    } while (0)

#define GNNLM_DESC(d)                                            \
    if (!(d)) {                                                  \
        ::gnnlm::set_error("invalid argument: null descriptor"); \
        return ::gnnlm::E_INVALID;                               \
    }

// gnnlm_gemm_t.alpha left at 0: gemm_nt reads it as 1
constexpr float ALPHA_UNSET = 0.f;

// C[M, N] = alpha * A[M, K] W[N, K]^T (+ bias) (+ R), C and R with row stride N.  m_dev: the row count lives on the device (M is
// its bound); such a launch walks the tiles the way the host-side count would have picked (gemm_nt's default assumes a small
// device count)
inline int linear(const float* A, int64_t lda, const float* W, const float* bias, float* C, int64_t M, int N, int K, const float* R,
                  float alpha, hipStream_t s, const int32_t* m_dev = nullptr) {
    GemmParams g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.C = C; g.ldc = N;
    g.bias = bias; g.bias_mode = bias ? 1 : 0;
    g.R = R; g.ldr = N; g.alpha = alpha;
    g.M = (int)M; g.N = N; g.K = K;
    g.m_dev = m_dev;
    if (m_dev && M > N) g.tile_order = 1;
    return gemm_nt(g, s);
}

// the same on a subset of rows: logical row r reads A row rows[r] and writes C row rows[r] (both in their full layouts)
inline int linear_rows(const float* A, int64_t lda, const float* W, const float* bias, float* C, int64_t ldc, const int32_t* rows,
                       int64_t n_rows, int N, int K, float alpha, hipStream_t s, int64_t rows_bound = 0, const int32_t* m_dev = nullptr) {
    GemmParams g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = K; g.C = C; g.ldc = ldc;
    g.bias = bias; g.bias_mode = bias ? 1 : 0;
    g.alpha = alpha;
    g.a_rows = rows; g.c_rows = rows; g.a_rows_bound = rows_bound;
    g.M = (int)n_rows; g.N = N; g.K = K;
    g.m_dev = m_dev;
    if (m_dev && n_rows > N) g.tile_order = 1;
    return gemm_nt(g, s);
}

}  // namespace gnnlm
