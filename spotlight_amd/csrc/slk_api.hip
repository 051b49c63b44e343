// slk_api.hip -- ctx lifetime, error text, scratch, event-based kernel timing.
#include <stdarg.h>

#include <stdlib.h>

#include "slk_common.h"

static char g_create_err[512] = {0};

int slk_fail(slk_ctx *ctx, int code, const char *fmt, ...) {
    char *dst = ctx ? ctx->err : g_create_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
    return code;
}

int slk_ensure(slk_ctx *ctx, slk_buf &b, size_t bytes) {
    if (bytes <= b.cap) return SLK_OK;
    if (b.p) {
        // hipFree waits for outstanding work that may still read the old block
        SLK_HIP(ctx, hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    void *p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) {
        (void)hipGetLastError();
        return slk_fail(ctx, SLK_ENOMEM, "hipMalloc of %zu scratch bytes failed", want);
    }
    b.p = p;
    b.cap = want;
    return SLK_OK;
}

int slk_ensure_lflags_host(slk_ctx *ctx, slk_prep_bufs &pb, size_t n) {
    if (n > pb.h_lflags_cap) {
        if (pb.h_lflags) (void)hipHostFree(pb.h_lflags);
        pb.h_lflags = nullptr;
        pb.h_lflags_cap = 0;
        void *p = nullptr;
        const size_t want = n + n / 4 + 64;
        if (hipHostMalloc(&p, want * sizeof(int), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return slk_fail(ctx, SLK_ENOMEM, "hipHostMalloc of %zu flag words failed", want);
        }
        pb.h_lflags = (int *)p;
        pb.h_lflags_cap = want;
    }
    for (size_t i = 0; i < n; ++i) pb.h_lflags[i] = 1;
    pb.h_lflags_n = n;
    return SLK_OK;
}

int slk_lflags_readback(slk_ctx *ctx, slk_prep_bufs &pb, size_t n, hipStream_t s) {
    int rc;
    if ((rc = slk_ensure_lflags_host(ctx, pb, n))) return rc;
    SLK_HIP(ctx, hipMemcpyAsync(pb.h_lflags, pb.lflags.p, n * 4, hipMemcpyDeviceToHost, s));
    if (!pb.ev_lflags) SLK_HIP(ctx, hipEventCreateWithFlags(&pb.ev_lflags, hipEventDisableTiming));
    SLK_HIP(ctx, hipEventRecord(pb.ev_lflags, s));
    return SLK_OK;
}

int slk_lflags_reserve(slk_ctx *ctx, slk_prep_bufs &pb, size_t n) {
    int rc;
    if ((rc = slk_ensure_lflags_host(ctx, pb, n))) return rc;
    pb.h_lflags_n = 0;
    if (!pb.ev_lflags) SLK_HIP(ctx, hipEventCreateWithFlags(&pb.ev_lflags, hipEventDisableTiming));
    return SLK_OK;
}

void slk_prof_begin(slk_ctx *ctx, int cls, hipStream_t s) {
    if (!ctx->prof_on) return;
    slk_prof_span sp;
    sp.cls = cls;
    for (hipEvent_t *e : {&sp.a, &sp.b}) {
        if (!ctx->ev_pool.empty()) {
            *e = ctx->ev_pool.back();
            ctx->ev_pool.pop_back();
        } else {
            (void)hipEventCreate(e);
        }
    }
    (void)hipEventRecord(sp.a, s);
    ctx->spans.push_back(sp);
}

void slk_prof_end(slk_ctx *ctx, hipStream_t s) {
    if (!ctx->prof_on) return;
    (void)hipEventRecord(ctx->spans.back().b, s);
    if (ctx->spans.size() >= 8192) slk_prof_drain(ctx);
}

int slk_prof_drain(slk_ctx *ctx) {
    for (slk_prof_span &sp : ctx->spans) {
        SLK_HIP(ctx, hipEventSynchronize(sp.b));
        float ms = 0.0f;
        SLK_HIP(ctx, hipEventElapsedTime(&ms, sp.a, sp.b));
        ctx->prof_launches[sp.cls] += 1;
        ctx->prof_ms[sp.cls] += (double)ms;
        ctx->ev_pool.push_back(sp.a);
        ctx->ev_pool.push_back(sp.b);
    }
    ctx->spans.clear();
    return SLK_OK;
}

int slk_prep_stream_init(slk_ctx *ctx) {
    if (ctx->prep_stream) return SLK_OK;
    // (CU-masked and high-priority prep streams were measured in round 3 and lost: a masked pass loses far more than its
    // share of CUs, a priority stream gains nothing beyond the plain one -- profiles/r03_a_*)
    SLK_HIP(ctx, hipStreamCreateWithFlags(&ctx->prep_stream, hipStreamNonBlocking));
    // the runtime sets a stream's hardware queue up at its first launch (measured: ~2 ms, once per stream -- the first
    // overlapped training call of a process ran 0.86 instead of 0.75 ms per step, profiles/r03_e_*): done here, in the
    // reserve / first-use path, not in a timed call
    SLK_HIP(ctx, hipMemsetAsync(&ctx->d_rng->sort_abort, 0, sizeof(int32_t), ctx->prep_stream));
    SLK_HIP(ctx, hipStreamSynchronize(ctx->prep_stream));
    for (hipEvent_t *e : {&ctx->ev_start, &ctx->ev_prep[0], &ctx->ev_prep[1], &ctx->ev_done[0], &ctx->ev_done[1]})
        if (!*e) SLK_HIP(ctx, hipEventCreateWithFlags(e, hipEventDisableTiming));
    return SLK_OK;
}

hipStream_t slk_copy_stream(slk_ctx *ctx) {
    if (!ctx->copy_stream && hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        ctx->copy_stream = nullptr;  // the null stream still gives correct results
    }
    return ctx->copy_stream;
}

SLK_EXPORT int slk_abi_version(void) { return SLK_ABI_VERSION; }

SLK_EXPORT int slk_ctx_create(slk_ctx **out, int device_id) {
    if (!out) return slk_fail(nullptr, SLK_EINVAL, "slk_ctx_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return slk_fail(nullptr, SLK_EIO, "slk_ctx_create: no HIP device visible");
    }
    if (device_id < 0 || device_id >= ndev)
        return slk_fail(nullptr, SLK_EINVAL, "slk_ctx_create: device %d out of range (%d devices)",
                        device_id, ndev);
    slk_ctx *ctx = new slk_ctx();
    ctx->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess) {
        delete ctx;
        return slk_fail(nullptr, SLK_EIO, "slk_ctx_create: hipSetDevice(%d) failed", device_id);
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) {
        ctx->num_cus = prop.multiProcessorCount;
        // LDS a workgroup may be granted (gfx950: the CU's whole 160 KB); kernels that pad their dynamic LDS request to cap
        // occupancy (slk_eval.hip) derive the pad from this, not from a constant
        if (prop.sharedMemPerBlock > 0) ctx->lds_per_block = prop.sharedMemPerBlock;
        if (prop.maxSharedMemoryPerMultiProcessor > 0) ctx->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
        if (ctx->lds_per_cu < ctx->lds_per_block) ctx->lds_per_cu = ctx->lds_per_block;
    }
    if (hipMalloc(reinterpret_cast<void **>(&ctx->d_rng), sizeof(slk_rng_dev)) != hipSuccess) {
        delete ctx;
        return slk_fail(nullptr, SLK_ENOMEM, "slk_ctx_create: hipMalloc(rng) failed");
    }
    // numpy's RandomState(0)-independent default: an all-zero key with pos = 624 is a valid
    // (if degenerate) state; callers are expected to slk_rng_set_state() before sampling.
    (void)hipMemset(ctx->d_rng, 0, sizeof(slk_rng_dev));
    int32_t pos = 624;
    (void)hipMemcpy(&ctx->d_rng->pos, &pos, sizeof(pos), hipMemcpyHostToDevice);
    *out = ctx;
    return SLK_OK;
}

SLK_EXPORT void slk_ctx_destroy(slk_ctx *ctx) {
    if (!ctx) return;
    if (ctx->shadow_active)  // (void function: the one loud channel left.  The scope is NOT written back -- its arrays may be gone.)
        fprintf(stderr, "libspotlight_hip: slk_ctx_destroy with an OPEN item-bias shadow (slk_bias_shadow_begin without _end): "
                        "the caller's item biases and their Adagrad accumulator keep their pre-scope values; the training of the "
                        "scope is lost\n");
    if (ctx->pp_active)
        fprintf(stderr, "libspotlight_hip: slk_ctx_destroy with an OPEN user-row ping-pong (slk_user_pingpong_begin without _end): "
                        "the rows whose current copy is the ctx's are not written back; the caller's user table is a mix of pre- and "
                        "in-scope rows -- the training of the scope is lost\n");
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    slk_prof_drain(ctx);
    for (hipEvent_t e : ctx->ev_pool) (void)hipEventDestroy(e);
    slk_buf *bufs[] = {&ctx->raw, &ctx->cnt, &ctx->neg32, &ctx->ukey[0], &ctx->ukey[1], &ctx->uval[0],
                       &ctx->uval[1], &ctx->uit, &ctx->ikey[0], &ctx->ikey[1], &ctx->ipay[0],
                       &ctx->ipay[1], &ctx->gk, &ctx->sk, &ctx->snap, &ctx->losspart,
                       &ctx->sort_tmp, &ctx->dgrad[0], &ctx->dgrad[1], &ctx->dgrad[2], &ctx->dgrad[3], &ctx->ipart,
                       &ctx->ipart_meta, &ctx->upart_meta, &ctx->pf_neg, &ctx->call_neg, &ctx->mt_tmp, &ctx->bias_shadow, &ctx->pp_alt,
                       &ctx->pp_flags};
    for (slk_buf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (slk_buf &b : ctx->extra)
        if (b.p) (void)hipFree(b.p);
    for (slk_prep_bufs &pb : ctx->pb) {
        slk_buf *pbs[] = {&pb.neg32, &pb.ukey[0], &pb.ukey[1], &pb.uval[0], &pb.uval[1], &pb.uit, &pb.ikey[0],
                          &pb.ikey[1], &pb.ipay[0], &pb.ipay[1], &pb.bik[0], &pb.bik[1], &pb.bip[0], &pb.bip[1],
                          &pb.buk[0], &pb.buk[1], &pb.bup[0], &pb.bup[1], &pb.lflags, &pb.mflag, &pb.msorted, &pb.mcount};
        for (slk_buf *b : pbs)
            if (b->p) (void)hipFree(b->p);
        if (pb.ev_lflags) (void)hipEventDestroy(pb.ev_lflags);
        if (pb.h_lflags) (void)hipHostFree(pb.h_lflags);
    }
    for (hipEvent_t e : {ctx->ev_start, ctx->ev_prep[0], ctx->ev_prep[1], ctx->ev_done[0], ctx->ev_done[1], ctx->ev_coef[0], ctx->ev_coef[1],
                         ctx->ev_sampled})
        if (e) (void)hipEventDestroy(e);
    for (void *h : ctx->h_coef)
        if (h) (void)hipHostFree(h);
    if (ctx->prep_stream) (void)hipStreamDestroy(ctx->prep_stream);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->d_rng) (void)hipFree(ctx->d_rng);
    for (uint32_t *j : ctx->d_jump)
        if (j) (void)hipFree(j);
    delete ctx;
}

SLK_EXPORT const char *slk_last_error(const slk_ctx *ctx) { return ctx ? ctx->err : g_create_err; }

// Options: one table for set and get (slk_ctx_get_option exists so that a caller can change an option for the duration of
// one piece of work and put the previous value back: spotlight_amd/_native.py, Engine.options).
namespace {
struct slk_opt_desc {
    const char *name;
    int64_t lo, hi;
    int64_t (*get)(const slk_ctx *);
    void (*set)(slk_ctx *, int64_t);
};
#define SLK_OPT(name_, member_, lo_, hi_)                                              \
    {name_, (int64_t)(lo_), (int64_t)(hi_), [](const slk_ctx *c) -> int64_t { return (int64_t)c->member_; }, \
     [](slk_ctx *c, int64_t v) { c->member_ = (decltype(c->member_))v; }}
const int64_t SLK_OPT_MAX = INT64_MAX;
const slk_opt_desc slk_options[] = {
    SLK_OPT("chunk_interactions", opt_chunk_interactions, 1, SLK_OPT_MAX),
    SLK_OPT("overlap_prep", opt_overlap_prep, 0, 2),
    SLK_OPT("overlap_min_batch", opt_overlap_min_batch, 0, SLK_OPT_MAX),
    SLK_OPT("prefetch_wait", opt_prefetch_wait, 0, 1),
    SLK_OPT("mt_long_min_blocks", opt_mt_long_min_blocks, 2, SLK_OPT_MAX),
    SLK_OPT("sort_big_min", opt_sort_big_min, 1, SLK_OPT_MAX),
    SLK_OPT("sort_debug", opt_sort_debug, 0, 3),
    SLK_OPT("item_grid_mult", opt_item_grid_mult, 1, 4096),
    SLK_OPT("user_grid_mult", opt_user_grid_mult, 1, 4096),
    SLK_OPT("seq_variant", opt_seq_variant, 0, 1),
    SLK_OPT("explicit_fused", opt_explicit_fused, 0, 1),
    SLK_OPT("epoch_kernel", opt_epoch_kernel, 0, 1),
    SLK_OPT("item_lat_max_tiles", opt_item_lat_max_tiles, 0, SLK_OPT_MAX),
    SLK_OPT("epoch_adaptive", opt_epoch_adaptive, 0, 1),
    SLK_OPT("epoch_adaptive_max_batch", opt_epoch_adaptive_max_batch, 1, (int64_t)1 << 20),
    SLK_OPT("epoch_max_batch", opt_epoch_max_batch, 1, (int64_t)1 << 20),
    SLK_OPT("epoch_max_grid", opt_epoch_max_grid, 1, 16384),
    SLK_OPT("epoch_barrier", opt_epoch_barrier, -1, 1),
    SLK_OPT("epoch_cooperative", opt_epoch_cooperative, 0, 1),
    SLK_OPT("epoch_debug", opt_epoch_debug, 0, 63),
    SLK_OPT("epoch_dense_elems", opt_epoch_dense_elems, 0, SLK_OPT_MAX),
    SLK_OPT("user_lat_max_batch", opt_user_lat_max_batch, 0, SLK_OPT_MAX),
    SLK_OPT("item_long_gate", opt_item_long_gate, 0, 1),
    SLK_OPT("adaptive_late_min_batch", opt_adaptive_late_min_batch, 0, SLK_OPT_MAX),
    SLK_OPT("shuffle_band", opt_shuffle_band, 0, 1024),
    SLK_OPT("nt", opt_nt, 0, 63),
    SLK_OPT("record_nt_min_bytes", opt_record_nt_min_bytes, 0, SLK_OPT_MAX),
    SLK_OPT("user_bias_zero_hint", opt_user_bias_zero_hint, 0, 1),
    SLK_OPT("user_grid_own_occ", opt_user_grid_own_occ, 0, 1),
    SLK_OPT("item_single_min_items", opt_item_single_min_items, 0, SLK_OPT_MAX),
};
#undef SLK_OPT
// An option of the EVALUATION side: it has nothing to say about training, so it is no row of the table above (whose rows
// tests/engine_checks.py trains under, one by one); that the top-k result does not depend on it is tests/topk_checks.py's
// chunking invariance, that scores and ranks do not depend on "eval_items_per_wg" is tests/sweep_checks.py.
const slk_opt_desc slk_eval_options[] = {
    {"topk_items_per_wg", 0, (int64_t)1 << 40, [](const slk_ctx *c) -> int64_t { return c->opt_topk_items_per_wg; },
     [](slk_ctx *c, int64_t v) { c->opt_topk_items_per_wg = v; }},
    {"eval_items_per_wg", 0, (int64_t)1 << 40, [](const slk_ctx *c) -> int64_t { return c->opt_eval_items_per_wg; },
     [](slk_ctx *c, int64_t v) { c->opt_eval_items_per_wg = v; }},
    // slk_bilinear_foldin's route choice: no row of the table above either (training never reads it).  The two routes add a
    // user's gradient terms in different orders, so the value is NOT bit-neutral; tests/foldin_checks.py runs every check under
    // the default, all-workgroup and all-wave
    {"foldin_wg_min_len", 0, (int64_t)1 << 40, [](const slk_ctx *c) -> int64_t { return c->opt_foldin_wg_min_len; },
     [](slk_ctx *c, int64_t v) { c->opt_foldin_wg_min_len = v; }},
    // slk_als_solve's route choice.  Both routes run the same chains of operations per element, so the value IS bit-neutral;
    // tests/als_checks.py solves every system under the default, all-workgroup and all-light
    {"als_wg_min_len", 0, (int64_t)1 << 40, [](const slk_ctx *c) -> int64_t { return c->opt_als_wg_min_len; },
     [](slk_ctx *c, int64_t v) { c->opt_als_wg_min_len = v; }},
    // slk_sample_items_weighted: values per internal draw (the split of a large count); tests/weighted_sampler_checks.py
    // draws the same ids and ends in the same state under a limit of 100
    {"weighted_max_values", 1, (int64_t)0x7ffffffe * 312, [](const slk_ctx *c) -> int64_t { return c->opt_weighted_max_values; },
     [](slk_ctx *c, int64_t v) { c->opt_weighted_max_values = v; }},
};
const slk_opt_desc *slk_find_option(const char *name) {
    for (const slk_opt_desc &d : slk_options)
        if (!strcmp(name, d.name)) return &d;
    for (const slk_opt_desc &d : slk_eval_options)
        if (!strcmp(name, d.name)) return &d;
    return nullptr;
}
}  // namespace

SLK_EXPORT int slk_ctx_set_option(slk_ctx *ctx, const char *name, int64_t value) {
    if (!ctx || !name) return SLK_EINVAL;
    const slk_opt_desc *d = slk_find_option(name);
    if (!d || value < d->lo || value > d->hi)
        return slk_fail(ctx, SLK_EINVAL, "slk_ctx_set_option: unknown option or bad value: %s = %lld", name,
                        (long long)value);
    d->set(ctx, value);
    return SLK_OK;
}

SLK_EXPORT int slk_ctx_get_option(slk_ctx *ctx, const char *name, int64_t *value) {
    if (!ctx || !name || !value) return SLK_EINVAL;
    const slk_opt_desc *d = slk_find_option(name);
    if (!d) return slk_fail(ctx, SLK_EINVAL, "slk_ctx_get_option: unknown option %s", name);
    *value = d->get(ctx);
    return SLK_OK;
}

SLK_EXPORT int slk_ctx_get_stat(slk_ctx *ctx, const char *name, int64_t *value) {
    if (!ctx || !name || !value) return SLK_EINVAL;
    if (!strcmp(name, "shuffle_sweeps")) *value = ctx->fy_sweeps;
    else if (!strcmp(name, "shuffle_fallbacks")) *value = ctx->fy_fallbacks;
    else if (!strcmp(name, "epoch_refused")) *value = ctx->epoch_refused ? 1 : 0;
    else if (!strcmp(name, "user_long_launches")) *value = ctx->stat_user_long;
    else if (!strcmp(name, "item_long_launches")) *value = ctx->stat_item_long;
    else if (!strcmp(name, "overlapped_chunks")) *value = ctx->stat_overlapped;
    else if (!strcmp(name, "prefetched_chunks")) *value = ctx->stat_prefetched;
    else if (!strcmp(name, "shadowed_calls")) *value = ctx->stat_shadowed;
    else if (!strcmp(name, "pingpong_calls")) *value = ctx->stat_pingpong;
    else if (!strcmp(name, "single_minibatches")) *value = ctx->stat_single;
    else if (!strcmp(name, "lds_per_block")) *value = (int64_t)ctx->lds_per_block;
    else if (!strcmp(name, "lds_per_cu")) *value = (int64_t)ctx->lds_per_cu;
    else if (!strcmp(name, "prefetch_pending")) *value = !ctx->pf.valid ? 0 : (ctx->pf.all ? 2 : 1);
    else if (!strcmp(name, "sort_finish_cap")) *value = slk_sort_finish_cap();
    else if (!strcmp(name, "sort_finish_sorts")) *value = ctx->stat_sort_finish_sorts;
    else if (!strcmp(name, "sort_finish_fallbacks")) {
        // counted on the device (the host never learns inside a sort whether its buckets fitted): wait for the sorts, then copy
        uint32_t h = 0;
        SLK_HIP(ctx, hipSetDevice(ctx->device));
        SLK_HIP(ctx, hipDeviceSynchronize());
        SLK_HIP(ctx, hipMemcpy(&h, &ctx->d_rng->sort_fallbacks, sizeof(h), hipMemcpyDeviceToHost));
        *value = (int64_t)h;
    }
    else return slk_fail(ctx, SLK_EINVAL, "slk_ctx_get_stat: unknown statistic %s", name);
    return SLK_OK;
}

SLK_EXPORT int slk_profile_enable(slk_ctx *ctx, int32_t on) {
    if (!ctx) return SLK_EINVAL;
    if (!on) slk_prof_drain(ctx);
    ctx->prof_on = on != 0;
    return SLK_OK;
}

SLK_EXPORT int slk_profile_read(slk_ctx *ctx, int32_t cls, int64_t *launches, double *total_ms) {
    if (!ctx || cls < 0 || cls >= SLK_K_COUNT) return SLK_EINVAL;
    int rc = slk_prof_drain(ctx);
    if (rc) return rc;
    if (launches) *launches = ctx->prof_launches[cls];
    if (total_ms) *total_ms = ctx->prof_ms[cls];
    return SLK_OK;
}

SLK_EXPORT int slk_profile_reset(slk_ctx *ctx) {
    if (!ctx) return SLK_EINVAL;
    int rc = slk_prof_drain(ctx);
    for (int i = 0; i < SLK_K_COUNT; ++i) {
        ctx->prof_launches[i] = 0;
        ctx->prof_ms[i] = 0.0;
    }
    return rc;
}
