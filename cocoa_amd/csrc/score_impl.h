// Scoring entry points (cocoa_score*), included at the end of engine.hip.
//
// Scoring owns its buffers (ScoreState) and only enqueues on the context's
// stream behind whatever is queued there: it reads the context's w and writes
// nothing the rounds or the evaluations use, so it may run between rounds and
// while an evaluation is pending.
//
// Host variants: the rows go to the device in chunks of at most `chunk`
// entries (and rows) cut at row boundaries, a longer row being a chunk of its
// own.  Two slots, each a pinned host buffer and a device buffer of one
// layout, alternate: chunk i+1 is packed and uploaded on a copy stream while
// chunk i computes on the context's stream, and its scores come back through
// the slot's pinned tail.  Device memory is bounded by two chunks.
#pragma once
#include "score.h"

namespace {

// Default entries per host chunk: 4 Mi entries = 48 MiB per slot (see
// DESIGN.md "Scoring" for the sweep behind it).
constexpr int64_t kScoreChunkDefault = (int64_t)1 << 22;

struct ScoreSlot {
    void* h = nullptr;  // pinned
    size_t hbytes = 0;
    DevBuf d, head, tail, tail_row;
    hipEvent_t up = nullptr, done = nullptr;
    bool busy = false;
    int64_t r0 = 0, rows = 0;
    size_t out_off = 0;
};

}  // namespace

struct ScoreState {
    DevBuf w_orig;                // w in original feature order for the call in flight
    DevBuf head, tail, tail_row;  // tile partials of the device variant
    ScoreSlot slot[2];
    hipStream_t cstream = nullptr;
    int64_t chunk = 0;  // 0: kScoreChunkDefault
};

static void score_state_free(cocoa_ctx* c) {
    ScoreState* S = c->score;
    if (!S) return;
    for (ScoreSlot& sl : S->slot) {
        if (sl.done) (void)hipEventSynchronize(sl.done);
        if (sl.up) (void)hipEventDestroy(sl.up);
        if (sl.done) (void)hipEventDestroy(sl.done);
        if (sl.h) (void)hipHostFree(sl.h);
    }
    if (S->cstream) {
        (void)hipStreamSynchronize(S->cstream);
        (void)hipStreamDestroy(S->cstream);
    }
    delete S;
    c->score = nullptr;
}

static ScoreState& score_state(cocoa_ctx* c) {
    if (!c->score) c->score = new ScoreState();
    return *c->score;
}

static void score_grow(DevBuf& b, size_t bytes) {
    if (b.bytes < bytes) b.alloc(bytes);
}

// the model a call scores with, in original feature order on the device
static const double* score_w(cocoa_ctx* c, ScoreState& S, const double* w_host, int32_t d) {
    score_grow(S.w_orig, sizeof(double) * (size_t)d);
    if (w_host) {
        HIPCHK(hipMemcpyAsync(S.w_orig.p, w_host, sizeof(double) * (size_t)d, hipMemcpyHostToDevice, c->stream));
    } else {
        require(c->inited, COCOA_E_STATE, "cocoa_score: no w given and the context holds none (cocoa_init first)");
        launch_score_gather_w(c->w.as<double>(), c->d_perm.as<int32_t>(), d, S.w_orig.as<double>(), c->stream);
        HIPCHK(hipGetLastError());
    }
    return S.w_orig.as<double>();
}

static void score_check_d(const cocoa_ctx* c, int32_t d) {
    require(d >= 1, COCOA_E_ARG, "cocoa_score: num_features must be >= 1");
    require(c->d == 0 || d == c->d, COCOA_E_ARG,
            "cocoa_score: num_features " + std::to_string(d) + " differs from the training set's " +
                std::to_string(c->d));
}

static void score_launch_sparse(cocoa_ctx* c, const double* w, const int64_t* row_ptr, const int32_t* col,
                                const double* val, int64_t n, int64_t nnz, double* out, DevBuf& head, DevBuf& tail,
                                DevBuf& tail_row) {
    if (n <= 0) return;
    if (c->strict) {
        launch_score_strict(row_ptr, col, val, w, n, out, c->stream);
    } else {
        const size_t nt = (size_t)score_tiles(nnz);
        score_grow(head, sizeof(double) * nt);
        score_grow(tail, sizeof(double) * nt);
        score_grow(tail_row, sizeof(int64_t) * nt);
        launch_score_fast(row_ptr, col, val, w, n, nnz, out, head.as<double>(), tail.as<double>(),
                          tail_row.as<int64_t>(), c->stream);
    }
    HIPCHK(hipGetLastError());
}

static void score_launch_dense(cocoa_ctx* c, const double* w, const double* X, int64_t n, int32_t d, double* out) {
    if (n <= 0) return;
    if (c->strict) launch_score_strict_dense(X, w, n, d, out, c->stream);
    else launch_score_fast_dense(X, w, n, d, out, c->stream);
    HIPCHK(hipGetLastError());
}

// ---- host chunks ------------------------------------------------------------
static void score_slots_init(ScoreState& S) {
    if (!S.cstream) HIPCHK(hipStreamCreateWithFlags(&S.cstream, hipStreamNonBlocking));
    for (ScoreSlot& sl : S.slot) {
        if (!sl.up) HIPCHK(hipEventCreateWithFlags(&sl.up, hipEventDisableTiming));
        if (!sl.done) HIPCHK(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
        if (sl.busy) {  // left by a call that failed half way: let it finish, drop its scores
            HIPCHK(hipEventSynchronize(sl.done));
            sl.busy = false;
        }
    }
}

// wait for the slot's chunk and hand its scores to the caller
static void score_slot_collect(ScoreSlot& sl, double* out) {
    if (!sl.busy) return;
    HIPCHK(hipEventSynchronize(sl.done));
    std::memcpy(out + sl.r0, (const char*)sl.h + sl.out_off, sizeof(double) * (size_t)sl.rows);
    sl.busy = false;
}

static void score_slot_reserve(ScoreSlot& sl, size_t bytes) {
    if (sl.hbytes < bytes) {
        if (sl.h) HIPCHK(hipHostFree(sl.h));
        sl.h = nullptr;
        sl.hbytes = 0;
        HIPCHK(hipHostMalloc(&sl.h, bytes, hipHostMallocDefault));
        sl.hbytes = bytes;
    }
    score_grow(sl.d, bytes);
}

// upload the slot's first in_bytes on the copy stream, then (on the context's
// stream) run `launch` and bring rows scores back from out_off
template <class F>
static void score_slot_run(cocoa_ctx* c, ScoreState& S, ScoreSlot& sl, size_t in_bytes, F&& launch) {
    HIPCHK(hipMemcpyAsync(sl.d.p, sl.h, in_bytes, hipMemcpyHostToDevice, S.cstream));
    HIPCHK(hipEventRecord(sl.up, S.cstream));
    HIPCHK(hipStreamWaitEvent(c->stream, sl.up, 0));
    launch();
    HIPCHK(hipMemcpyAsync((char*)sl.h + sl.out_off, (char*)sl.d.p + sl.out_off, sizeof(double) * (size_t)sl.rows,
                          hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(sl.done, c->stream));
    sl.busy = true;
}

static size_t pad8(size_t x) { return (x + 7) & ~(size_t)7; }

// pageable -> pinned copy of a chunk's arrays; large ones on a few threads (one
// thread's memcpy moves less than half of what the host-to-device copy does)
static void score_pack(void* dst, const void* src, size_t bytes) {
    constexpr size_t kPiece = (size_t)4 << 20;
    const size_t nt = std::min<size_t>(4, bytes / kPiece);
    if (nt < 2) {
        std::memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> th;
    const size_t per = ((bytes + nt - 1) / nt + 63) & ~(size_t)63;
    for (size_t i = 1; i < nt; ++i) {
        const size_t b = i * per, e = std::min(bytes, b + per);
        th.emplace_back([=] { std::memcpy((char*)dst + b, (const char*)src + b, e - b); });
    }
    std::memcpy(dst, src, per);
    for (auto& t : th) t.join();
}

// rows [0, n) of a CSR whose row_ptr may start past 0 (a device's block of a
// multi-device call): col / val are indexed by row_ptr's absolute offsets
static void score_host_sparse(cocoa_ctx* c, const double* w_host, const int64_t* row_ptr, const int32_t* col,
                              const double* val, int64_t n, int32_t d, double* out) {
    ScoreState& S = score_state(c);
    score_slots_init(S);
    const double* w = score_w(c, S, w_host, d);
    const int64_t cap = S.chunk > 0 ? S.chunk : kScoreChunkDefault;
    int64_t r = 0;
    for (int i = 0; r < n; ++i) {
        const int64_t e0 = row_ptr[r];
        int64_t r1 = r;
        if (row_ptr[r + 1] - e0 > cap) r1 = r + 1;
        else
            while (r1 < n && row_ptr[r1 + 1] - e0 <= cap && r1 - r < cap) ++r1;
        const int64_t rows = r1 - r, ne = row_ptr[r1] - e0;
        ScoreSlot& sl = S.slot[i & 1];
        score_slot_collect(sl, out);
        const size_t o_val = sizeof(int64_t) * (size_t)(rows + 1), o_col = o_val + sizeof(double) * (size_t)ne;
        const size_t o_out = pad8(o_col + sizeof(int32_t) * (size_t)ne);
        score_slot_reserve(sl, o_out + sizeof(double) * (size_t)rows);
        int64_t* h_rp = (int64_t*)sl.h;
        for (int64_t k = 0; k <= rows; ++k) h_rp[k] = row_ptr[r + k] - e0;
        if (ne) {
            score_pack((char*)sl.h + o_val, val + e0, sizeof(double) * (size_t)ne);
            score_pack((char*)sl.h + o_col, col + e0, sizeof(int32_t) * (size_t)ne);
        }
        sl.r0 = r;
        sl.rows = rows;
        sl.out_off = o_out;
        char* dp = (char*)sl.d.p;
        score_slot_run(c, S, sl, o_out, [&] {
            score_launch_sparse(c, w, (const int64_t*)dp, (const int32_t*)(dp + o_col), (const double*)(dp + o_val),
                                rows, ne, (double*)(dp + o_out), sl.head, sl.tail, sl.tail_row);
        });
        r = r1;
    }
    for (ScoreSlot& sl : S.slot) score_slot_collect(sl, out);
    if (w_host) HIPCHK(hipStreamSynchronize(c->stream));  // (n = 0: the caller's w has been read)
}

static void score_host_dense(cocoa_ctx* c, const double* w_host, const double* X, int64_t n, int32_t d, double* out) {
    ScoreState& S = score_state(c);
    score_slots_init(S);
    const double* w = score_w(c, S, w_host, d);
    const int64_t cap = S.chunk > 0 ? S.chunk : kScoreChunkDefault;
    const int64_t per = std::max<int64_t>(1, cap / d);
    int64_t r = 0;
    for (int i = 0; r < n; ++i) {
        const int64_t rows = std::min(per, n - r);
        ScoreSlot& sl = S.slot[i & 1];
        score_slot_collect(sl, out);
        const size_t o_out = sizeof(double) * (size_t)rows * (size_t)d;
        score_slot_reserve(sl, o_out + sizeof(double) * (size_t)rows);
        score_pack(sl.h, X + r * (int64_t)d, o_out);
        sl.r0 = r;
        sl.rows = rows;
        sl.out_off = o_out;
        char* dp = (char*)sl.d.p;
        score_slot_run(c, S, sl, o_out, [&] { score_launch_dense(c, w, (const double*)dp, rows, d, (double*)(dp + o_out)); });
        r += rows;
    }
    for (ScoreSlot& sl : S.slot) score_slot_collect(sl, out);
    if (w_host) HIPCHK(hipStreamSynchronize(c->stream));
}

// a multi-device context: contiguous row blocks, one thread per device
template <class F>
static void score_group(cocoa_ctx* g, int64_t n, F&& block) {
    const int64_t N = (int64_t)g->subs.size();
    std::vector<int> rcs((size_t)N, COCOA_OK);
    std::vector<std::string> msgs((size_t)N);
    std::vector<std::thread> th;
    for (int64_t r = 0; r < N; ++r)
        th.emplace_back([&, r] {
            cocoa_ctx* sub = g->subs[(size_t)r];
            try {
                HIPCHK(hipSetDevice(sub->device));
                block(sub, n * r / N, n * (r + 1) / N);
            } catch (const Error& e) {
                rcs[(size_t)r] = e.code;
                msgs[(size_t)r] = e.what();
            } catch (const std::exception& e) {
                rcs[(size_t)r] = COCOA_E_ARG;
                msgs[(size_t)r] = e.what();
            }
        });
    for (auto& t : th) t.join();
    HIPCHK(hipSetDevice(g->device));
    for (int64_t r = 0; r < N; ++r)
        if (rcs[(size_t)r] != COCOA_OK) throw Error(rcs[(size_t)r], msgs[(size_t)r]);
}

extern "C" int cocoa_score(cocoa_ctx* ctx, const double* w, const int64_t* row_ptr, const int32_t* col,
                           const double* val, int64_t n_rows, int32_t num_features, double* out) {
    CAPI_BEGIN(ctx)
    require(row_ptr && n_rows >= 0 && (out || n_rows == 0), COCOA_E_ARG, "cocoa_score: bad argument");
    score_check_d(ctx, num_features);
    require(row_ptr[0] == 0 && ((col && val) || row_ptr[n_rows] == 0 || n_rows == 0), COCOA_E_ARG,
            row_ptr[0] == 0 ? "cocoa_score: null col / val" : "row_ptr[0] must be 0");
    check_csr(row_ptr, col, n_rows, num_features);
    if (ctx->is_group()) {
        require(w || ctx->subs[0]->inited, COCOA_E_STATE,
                "cocoa_score: no w given and the context holds none (cocoa_init first)");
        score_group(ctx, n_rows, [&](cocoa_ctx* sub, int64_t r0, int64_t r1) {
            score_host_sparse(sub, w, row_ptr + r0, col, val, r1 - r0, num_features, out + r0);
        });
        return COCOA_OK;
    }
    score_host_sparse(ctx, w, row_ptr, col, val, n_rows, num_features, out);
    CAPI_END(ctx)
}

extern "C" int cocoa_score_dense(cocoa_ctx* ctx, const double* w, const double* X, int64_t n_rows,
                                 int32_t num_features, double* out) {
    CAPI_BEGIN(ctx)
    require(n_rows >= 0 && ((X && out) || n_rows == 0), COCOA_E_ARG, "cocoa_score_dense: bad argument");
    score_check_d(ctx, num_features);
    if (ctx->is_group()) {
        require(w || ctx->subs[0]->inited, COCOA_E_STATE,
                "cocoa_score_dense: no w given and the context holds none (cocoa_init first)");
        score_group(ctx, n_rows, [&](cocoa_ctx* sub, int64_t r0, int64_t r1) {
            score_host_dense(sub, w, X + r0 * (int64_t)num_features, r1 - r0, num_features, out + r0);
        });
        return COCOA_OK;
    }
    score_host_dense(ctx, w, X, n_rows, num_features, out);
    CAPI_END(ctx)
}

extern "C" int cocoa_score_device(cocoa_ctx* ctx, const void* w_dev, const void* row_ptr_dev, const void* col_dev,
                                  const void* val_dev, int64_t n_rows, int64_t nnz, int32_t num_features,
                                  void* out_dev) {
    CAPI_BEGIN(ctx)
    GROUP_REJECT(ctx, "cocoa_score_device");
    require(n_rows >= 0 && nnz >= 0 && (n_rows == 0 || (row_ptr_dev && out_dev)) && (nnz == 0 || (col_dev && val_dev)),
            COCOA_E_ARG, "cocoa_score_device: bad argument");
    score_check_d(ctx, num_features);
    ScoreState& S = score_state(ctx);
    const double* w = w_dev ? (const double*)w_dev : score_w(ctx, S, nullptr, num_features);
    score_launch_sparse(ctx, w, (const int64_t*)row_ptr_dev, (const int32_t*)col_dev, (const double*)val_dev, n_rows,
                        nnz, (double*)out_dev, S.head, S.tail, S.tail_row);
    CAPI_END(ctx)
}

extern "C" int cocoa_score_dense_device(cocoa_ctx* ctx, const void* w_dev, const void* X_dev, int64_t n_rows,
                                        int32_t num_features, void* out_dev) {
    CAPI_BEGIN(ctx)
    GROUP_REJECT(ctx, "cocoa_score_dense_device");
    require(n_rows >= 0 && (n_rows == 0 || (X_dev && out_dev)), COCOA_E_ARG, "cocoa_score_dense_device: bad argument");
    score_check_d(ctx, num_features);
    ScoreState& S = score_state(ctx);
    const double* w = w_dev ? (const double*)w_dev : score_w(ctx, S, nullptr, num_features);
    score_launch_dense(ctx, w, (const double*)X_dev, n_rows, num_features, (double*)out_dev);
    CAPI_END(ctx)
}

extern "C" int cocoa_score_set_chunk(cocoa_ctx* ctx, int64_t max_entries) {
    CAPI_BEGIN(ctx)
    require(max_entries >= 0, COCOA_E_ARG, "cocoa_score_set_chunk: max_entries must be >= 0");
    score_state(ctx).chunk = max_entries;
    for (cocoa_ctx* sub : ctx->subs) score_state(sub).chunk = max_entries;
    CAPI_END(ctx)
}
