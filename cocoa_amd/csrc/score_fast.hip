// Fast scoring kernels (built with -ffp-contract=fast).
//
// Sparse: the entries are cut into tiles of kScoreTile, one 256-thread
// workgroup per tile.  A workgroup finds its tile's row range by binary search
// over row_ptr (nothing is read back by the host), streams its entries once
// (4 + 8 B, coalesced scalar loads: no alignment beyond the natural one is
// assumed), gathers w, and leaves the products in LDS (16 KB).  The rows of the
// tile are then reduced by groups of 16 lanes (or whole waves when the tile
// holds few rows) and every row that lies inside the tile is written with one
// plain store.  A row that crosses a tile boundary leaves one partial per tile
// (head: it began in an earlier tile; tail: it begins here and goes on); the
// second kernel sums those partials in tile order and writes the row, so no
// workgroup waits for another, there are no atomics, and the same input gives
// the same bytes on every call.
#include "score.h"
#include "wave.h"

namespace cocoa {

template <int G>
__device__ __forceinline__ double group_sum(double x) {
    if (G == 16) return row16_sum(x);
    return wave_sum(x);
}

template <int G>
__device__ __forceinline__ void score_reduce_rows(const double* prod, const int64_t* __restrict__ row_ptr,
                                                  int64_t r_first, int64_t nrows, int64_t e0, int64_t e1, int64_t t,
                                                  double* __restrict__ out, double* __restrict__ head,
                                                  double* __restrict__ tail) {
    constexpr int NG = 256 / G;
    const int g = (int)threadIdx.x / G, l = (int)threadIdx.x % G;
    for (int64_t i = g; i < nrows; i += NG) {  // uniform over the G lanes of a group
        const int64_t r = r_first + i;
        const int64_t start = row_ptr[r], end = row_ptr[r + 1];
        const int64_t a = (start > e0 ? start : e0) - e0, b = (end < e1 ? end : e1) - e0;
        double acc = 0.0;
        for (int64_t k = a + l; k < b; k += G) acc += prod[k];
        acc = group_sum<G>(acc);
        if (l == 0) {
            if (start < e0) head[t] = acc;
            else if (end > e1) tail[t] = acc;
            else out[r] = acc;
        }
    }
}

__global__ void __launch_bounds__(256) score_fast_kernel(const int64_t* __restrict__ row_ptr,
                                                         const int32_t* __restrict__ col,
                                                         const double* __restrict__ val,
                                                         const double* __restrict__ w, int64_t n, int64_t nnz,
                                                         double* __restrict__ out, double* __restrict__ head,
                                                         double* __restrict__ tail, int64_t* __restrict__ tail_row) {
    __shared__ double prod[kScoreTile];
    __shared__ int64_t s_r[2];
    const int64_t t = blockIdx.x;
    const int64_t e0 = t * kScoreTile;
    const int64_t e1 = e0 + kScoreTile < nnz ? e0 + kScoreTile : nnz;
    const bool last = blockIdx.x == gridDim.x - 1;
    if (threadIdx.x < 2) {
        // first index i in [0, n] with row_ptr[i] >= key (row_ptr[n] = nnz >= key)
        const int64_t key = threadIdx.x == 0 ? e0 : e1;
        int64_t lo = 0, hi = n;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (row_ptr[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        s_r[threadIdx.x] = lo;
    }
    const int cnt = (int)(e1 - e0);
    for (int i = (int)threadIdx.x; i < cnt; i += 256) prod[i] = val[e0 + i] * w[col[e0 + i]];
    __syncthreads();
    // rows that begin in [e0, e1) (the last tile also takes the trailing empty
    // rows), preceded by the row that holds entry e0 when it began earlier
    const int64_t r_lo = s_r[0], r_hi = last ? n : s_r[1];
    const int64_t r_first = row_ptr[r_lo] > e0 ? r_lo - 1 : r_lo;
    const int64_t nrows = r_hi - r_first;
    if (threadIdx.x == 0) {
        int64_t tail_r = -1;
        if (nrows > 0 && row_ptr[r_hi] > e1 && row_ptr[r_hi - 1] >= e0) tail_r = r_hi - 1;
        tail_row[t] = tail_r;
    }
    if (nrows <= 16) score_reduce_rows<64>(prod, row_ptr, r_first, nrows, e0, e1, t, out, head, tail);
    else score_reduce_rows<16>(prod, row_ptr, r_first, nrows, e0, e1, t, out, head, tail);
}

// rows that cross a tile boundary: the thread of the tile the row begins in
// adds the following tiles' head partials in tile order
__global__ void __launch_bounds__(256) score_fixup_kernel(const int64_t* __restrict__ row_ptr, int64_t ntiles,
                                                          const double* __restrict__ head,
                                                          const double* __restrict__ tail,
                                                          const int64_t* __restrict__ tail_row,
                                                          double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles) return;
    const int64_t r = tail_row[t];
    if (r < 0) return;
    const int64_t end = row_ptr[r + 1];
    double acc = tail[t];
    for (int64_t t2 = t + 1; t2 < ntiles; ++t2) {
        acc += head[t2];
        if (end <= (t2 + 1) * kScoreTile) break;
    }
    out[r] = acc;
}

// dense rows: G lanes per row (G = 1 for d <= 4), lanes stride the row
template <int G>
__global__ void __launch_bounds__(256) score_fast_dense_kernel(const double* __restrict__ X,
                                                               const double* __restrict__ w, int64_t n, int32_t d,
                                                               double* __restrict__ out) {
    constexpr int NG = 256 / G;
    const int g = (int)threadIdx.x / G, l = (int)threadIdx.x % G;
    const int64_t stride = (int64_t)gridDim.x * NG;
    for (int64_t r = (int64_t)blockIdx.x * NG + g; r < n; r += stride) {  // uniform over a group
        const double* x = X + r * (int64_t)d;
        double a0 = 0.0, a1 = 0.0;
        int32_t j = l;
        for (; j + G < d; j += 2 * G) {
            a0 = fma(x[j], w[j], a0);
            a1 = fma(x[j + G], w[j + G], a1);
        }
        if (j < d) a0 = fma(x[j], w[j], a0);
        double acc = a0 + a1;
        if (G > 1) acc = group_sum<G>(acc);
        if (l == 0) out[r] = acc;
    }
}

void launch_score_fast(const int64_t* row_ptr, const int32_t* col, const double* val, const double* w, int64_t n,
                       int64_t nnz, double* out, double* head, double* tail, int64_t* tail_row, hipStream_t s) {
    if (n <= 0) return;
    const int64_t ntiles = score_tiles(nnz);
    hipLaunchKernelGGL(score_fast_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, row_ptr, col, val, w, n, nnz, out,
                       head, tail, tail_row);
    hipLaunchKernelGGL(score_fixup_kernel, dim3((unsigned)((ntiles + 255) / 256)), dim3(256), 0, s, row_ptr, ntiles,
                       head, tail, tail_row, out);
}

template <int G>
static void launch_dense_g(const double* X, const double* w, int64_t n, int32_t d, double* out, hipStream_t s) {
    constexpr int NG = 256 / G;
    int64_t b = (n + NG - 1) / NG;
    if (b > (1 << 18)) b = 1 << 18;
    hipLaunchKernelGGL(score_fast_dense_kernel<G>, dim3((unsigned)b), dim3(256), 0, s, X, w, n, d, out);
}

void launch_score_fast_dense(const double* X, const double* w, int64_t n, int32_t d, double* out, hipStream_t s) {
    if (n <= 0) return;
    if (d <= 4) launch_dense_g<1>(X, w, n, d, out, s);
    else if (d <= 64) launch_dense_g<16>(X, w, n, d, out, s);
    else launch_dense_g<64>(X, w, n, d, out, s);
}

}  // namespace cocoa
