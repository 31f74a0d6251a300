// score_bench -- times the scoring entry points on the C2-shaped synthetic
// train rows (cocoa_gen_synthetic kind 0: n 677399, d 47236, ~75.6 nnz/row),
// fast mode:
//   device  cocoa_score_device on device-resident rows, HIP events around
//           repeated calls on the context's stream;
//   host    cocoa_score on the same rows in host memory, wall clock, over a
//           sweep of chunk sizes (cocoa_score_set_chunk), beside the time a
//           pinned host-to-device copy of the same bytes takes;
//   eval    cocoa_kernel_stats(COCOA_K_EVAL) of cocoa_eval on the same rows as
//           the training set: the yardstick (10 B per entry, hot w in LDS).
// One JSON object per line.  Bytes of a scoring pass: 12 per entry, 8 per row
// pointer, 8 per output.  usage: score_bench [n [d [mean_nnz [reps]]]]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cocoa_capi.h"

#define HIPCHK(x)                                                                      \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            std::fprintf(stderr, "%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); \
            std::exit(2);                                                              \
        }                                                                              \
    } while (0)

static void ck(int rc, cocoa_ctx* ctx) {
    if (rc != COCOA_OK) {
        std::fprintf(stderr, "error %d: %s\n", rc, cocoa_last_error(ctx));
        std::exit(2);
    }
}

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv) {
    const int64_t n = argc > 1 ? std::atoll(argv[1]) : 677399;
    const int32_t d = argc > 2 ? std::atoi(argv[2]) : 47236;
    const double mean_nnz = argc > 3 ? std::atof(argv[3]) : 75.6;
    const int reps = argc > 4 ? std::atoi(argv[4]) : 20;
    const double kPeak = 8.0e12;  // HBM bytes/s of the MI355X

    cocoa_dataset ds{};
    ck(cocoa_gen_synthetic(0, n, d, mean_nnz, 64, 12345, 0, 16, &ds), nullptr);
    const int64_t nnz = ds.nnz;
    std::vector<double> w((size_t)d);
    uint64_t s = 88172645463325252ull;
    for (auto& x : w) {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        x = ((double)(s >> 11) / 9007199254740992.0 - 0.5) * 0.02;
    }
    const double bytes = 12.0 * (double)nnz + 8.0 * (double)(n + 1) + 8.0 * (double)n;

    hipStream_t st;
    HIPCHK(hipSetDevice(0));
    HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    cocoa_ctx* ctx = nullptr;
    ck(cocoa_create(0, 0, st, &ctx), nullptr);

    // ---- device-resident rows
    int64_t* d_rp;
    int32_t* d_col;
    double *d_val, *d_w, *d_out;
    HIPCHK(hipMalloc(&d_rp, sizeof(int64_t) * (size_t)(n + 1)));
    HIPCHK(hipMalloc(&d_col, sizeof(int32_t) * (size_t)nnz));
    HIPCHK(hipMalloc(&d_val, sizeof(double) * (size_t)nnz));
    HIPCHK(hipMalloc(&d_w, sizeof(double) * (size_t)d));
    HIPCHK(hipMalloc(&d_out, sizeof(double) * (size_t)n));
    HIPCHK(hipMemcpy(d_rp, ds.row_ptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_col, ds.col, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_val, ds.val, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_w, w.data(), sizeof(double) * (size_t)d, hipMemcpyHostToDevice));
    for (int i = 0; i < 3; ++i) ck(cocoa_score_device(ctx, d_w, d_rp, d_col, d_val, n, nnz, d, d_out), ctx);
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a));
    HIPCHK(hipEventCreate(&b));
    HIPCHK(hipEventRecord(a, st));
    for (int i = 0; i < reps; ++i) ck(cocoa_score_device(ctx, d_w, d_rp, d_col, d_val, n, nnz, d, d_out), ctx);
    HIPCHK(hipEventRecord(b, st));
    HIPCHK(hipEventSynchronize(b));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    const double dev_ms = ms / reps;
    std::vector<double> f_dev((size_t)n), f_host((size_t)n);
    HIPCHK(hipMemcpy(f_dev.data(), d_out, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    std::printf("{\"what\":\"device\",\"n\":%lld,\"d\":%d,\"nnz\":%lld,\"reps\":%d,\"ms\":%.4f,\"entries_per_s\":%.4g,"
                "\"bytes\":%.0f,\"frac_of_8TBs\":%.4f}\n",
                (long long)n, d, (long long)nnz, reps, dev_ms, nnz / (dev_ms * 1e-3), bytes,
                bytes / (dev_ms * 1e-3) / kPeak);
    std::fflush(stdout);

    // ---- a pinned host-to-device copy of the same input bytes
    const size_t piece = (size_t)64 << 20;
    void *hp, *dp;
    HIPCHK(hipHostMalloc(&hp, piece, hipHostMallocDefault));
    HIPCHK(hipMalloc(&dp, piece));
    const double in_bytes = 12.0 * (double)nnz + 8.0 * (double)(n + 1);
    const int pieces = (int)std::ceil(in_bytes / (double)piece);
    HIPCHK(hipMemcpyAsync(dp, hp, piece, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    double t0 = now_ms();
    for (int i = 0; i < pieces; ++i) HIPCHK(hipMemcpyAsync(dp, hp, piece, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    const double copy_ms = (now_ms() - t0) * in_bytes / ((double)pieces * (double)piece);
    std::printf("{\"what\":\"h2d_copy\",\"bytes\":%.0f,\"ms\":%.3f,\"GBs\":%.2f}\n", in_bytes, copy_ms,
                in_bytes / (copy_ms * 1e-3) / 1e9);
    std::fflush(stdout);

    // ---- host rows, chunk sweep (0 = the default)
    const int64_t chunks[] = {(int64_t)1 << 18, (int64_t)1 << 20, (int64_t)1 << 22, (int64_t)1 << 24, (int64_t)1 << 26, 0};
    for (int64_t c : chunks) {
        ck(cocoa_score_set_chunk(ctx, c), ctx);
        double best = 1e30;
        for (int i = 0; i < 3; ++i) {
            t0 = now_ms();
            ck(cocoa_score(ctx, w.data(), ds.row_ptr, ds.col, ds.val, n, d, f_host.data()), ctx);
            best = std::min(best, now_ms() - t0);
        }
        double md = 0;
        for (int64_t r = 0; r < n; ++r) md = std::max(md, std::fabs(f_host[(size_t)r] - f_dev[(size_t)r]));
        std::printf("{\"what\":\"host\",\"chunk_entries\":%lld,\"ms\":%.3f,\"entries_per_s\":%.4g,\"frac_of_8TBs\":%.5f,"
                    "\"pcie_copy_frac\":%.3f,\"max_abs_diff_vs_device\":%.3g}\n",
                    (long long)c, best, nnz / (best * 1e-3), bytes / (best * 1e-3) / kPeak, copy_ms / best, md);
        std::fflush(stdout);
    }

    // ---- the yardstick: cocoa_eval's kernels on the same rows
    ck(cocoa_set_train(ctx, ds.num_parts, ds.part_ptr, ds.row_ptr, ds.col, ds.val, ds.y, n, d, 0, ds.num_parts), ctx);
    cocoa_params P{(int32_t)n, 1, (int32_t)std::max<int64_t>(1, n / ds.num_parts), 0, 1e-4, 1.0, 1.0};
    cocoa_debug D{0, 0, 100, 0};
    ck(cocoa_init(ctx, &P, &D, COCOA_METHOD_COCOA_PLUS, w.data()), ctx);
    cocoa_eval_result ev{};
    for (int i = 0; i < 2; ++i) ck(cocoa_eval(ctx, &ev), ctx);
    ck(cocoa_stats_enable(ctx, 1), ctx);
    ck(cocoa_stats_kernels(ctx, 1u << COCOA_K_EVAL), ctx);
    ck(cocoa_stats_reset(ctx), ctx);
    const int evals = 10;
    for (int i = 0; i < evals; ++i) ck(cocoa_eval(ctx, &ev), ctx);
    double tot = 0;
    int64_t launches = 0;
    ck(cocoa_kernel_stats(ctx, COCOA_K_EVAL, &tot, &launches), ctx);
    ck(cocoa_stats_enable(ctx, 0), ctx);
    std::printf("{\"what\":\"eval_yardstick\",\"evals\":%d,\"launches\":%lld,\"ms_per_eval\":%.4f,"
                "\"entries_per_s\":%.4g,\"score_over_eval\":%.2f}\n",
                evals, (long long)launches, tot / evals, nnz / (tot / evals * 1e-3), dev_ms / (tot / evals));
    // scoring with the context's own w on the training set's device (gather + score)
    HIPCHK(hipEventRecord(a, st));
    for (int i = 0; i < reps; ++i) ck(cocoa_score_device(ctx, nullptr, d_rp, d_col, d_val, n, nnz, d, d_out), ctx);
    HIPCHK(hipEventRecord(b, st));
    HIPCHK(hipEventSynchronize(b));
    HIPCHK(hipEventElapsedTime(&ms, a, b));
    std::printf("{\"what\":\"device_context_w\",\"ms\":%.4f}\n", ms / reps);
    cocoa_destroy(ctx);
    cocoa_dataset_free(&ds);
    return 0;
}
