// Strict scoring kernels (built with -ffp-contract=off): every row is summed
// by one thread in stored order, product then add, so the result is bitwise
// the oracle's sp_dot and a plain host loop.
#include "score.h"

namespace cocoa {

__global__ void __launch_bounds__(256) score_strict_kernel(const int64_t* __restrict__ row_ptr,
                                                           const int32_t* __restrict__ col,
                                                           const double* __restrict__ val,
                                                           const double* __restrict__ w, int64_t n,
                                                           double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const int64_t e1 = row_ptr[r + 1];
        double acc = 0.0;
        for (int64_t q = row_ptr[r]; q < e1; ++q) {
            const double p = val[q] * w[col[q]];
            acc = acc + p;
        }
        out[r] = acc;
    }
}

__global__ void __launch_bounds__(256) score_strict_dense_kernel(const double* __restrict__ X,
                                                                 const double* __restrict__ w, int64_t n, int32_t d,
                                                                 double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const double* x = X + r * (int64_t)d;
        double acc = 0.0;
        for (int32_t j = 0; j < d; ++j) {
            const double p = x[j] * w[j];
            acc = acc + p;
        }
        out[r] = acc;
    }
}

__global__ void __launch_bounds__(256) score_gather_w_kernel(const double* __restrict__ w_dev,
                                                             const int32_t* __restrict__ perm, int32_t d,
                                                             double* __restrict__ w_orig) {
    const int32_t j = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (j < d) w_orig[j] = w_dev[perm[j]];
}

static unsigned row_grid(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

void launch_score_strict(const int64_t* row_ptr, const int32_t* col, const double* val, const double* w, int64_t n,
                         double* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(score_strict_kernel, dim3(row_grid(n)), dim3(256), 0, s, row_ptr, col, val, w, n, out);
}

void launch_score_strict_dense(const double* X, const double* w, int64_t n, int32_t d, double* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(score_strict_dense_kernel, dim3(row_grid(n)), dim3(256), 0, s, X, w, n, d, out);
}

void launch_score_gather_w(const double* w_dev, const int32_t* perm, int32_t d, double* w_orig, hipStream_t s) {
    if (d <= 0) return;
    hipLaunchKernelGGL(score_gather_w_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, w_dev, perm, d,
                       w_orig);
}

}  // namespace cocoa
