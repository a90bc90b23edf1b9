// hfv_service.cpp -- the resident verify service (hfv_service_*).
// The host side of k_verify_service (hfv_service_kernel.hip): tickets 1, 2, ... go to ring slot
// (t - 1) % kSvcRing; ticket t is posted only once ticket t - kSvcRing is done.  Ring and
// completion words hold svc_tag | t, the tag changing with every grid, so nothing is cleared
// between grids.
#include <time.h>

#include "hfv_ctx.h"

// Grid-local batch t is complete once the relay has forwarded its completion (every block of
// the grid reported its share of it).
static bool svc_is_done(const hfv_ctx *ctx, uint64_t t)
{
    return __atomic_load_n(&ctx->svc_host->done[(t - 1) % kSvcRing], __ATOMIC_ACQUIRE) >= (ctx->svc_tag | t);
}

// The running grid has exited on the stop the host posted: it verified every batch before it
// (each block reaches the stop only after its share of all earlier batches), including those
// whose completion the relay did not forward (it leaves at the stop).
static bool svc_exited_clean(const hfv_ctx *ctx)
{
    return ctx->svc_running && ctx->svc_stop_posted && __atomic_load_n(&ctx->svc_host->status, __ATOMIC_ACQUIRE) == 0 &&
           hipStreamQuery(ctx->svc_stream) == hipSuccess;
}

// Device-side completion of grid-local batch t from a copy of SvcDev::done (after an idle or
// watchdog exit, when the relay may not have forwarded everything).
static bool svc_dev_done(const hfv_ctx *ctx, const std::vector<uint64_t> &done, uint64_t t)
{
    const uint64_t *d = &done[((t - 1) % kSvcRing) * kSvcMaxBlocks];
    for (unsigned k = 0; k < ctx->svc_grid; ++k)
        if (d[k] < (ctx->svc_tag | t)) return false;
    return true;
}

// Copy `bytes` at byte offset `off` of the ctx's SvcDev to host memory (diagnostics and the
// balance, after a grid; on the ctx's own stream, which a running grid does not occupy).
static int svc_dev_read(hfv_ctx *ctx, void *dst, size_t off, size_t bytes)
{
    if (!ctx->svc_dev) return fail(-EINVAL, "the verify service has not run");
    HIP_TRY(hipMemcpyAsync(dst, reinterpret_cast<const char *>(ctx->svc_dev) + off, bytes, hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// SvcDev::done into a host vector for svc_dev_done.
static int svc_read_done(hfv_ctx *ctx, std::vector<uint64_t> &done)
{
    done.assign((size_t)kSvcRing * kSvcMaxBlocks, 0);
    return svc_dev_read(ctx, done.data(), offsetof(SvcDev, done), done.size() * 8);
}

static int svc_wait_done(hfv_ctx *ctx, uint64_t t, int timeout_ms)
{
    struct timespec t0, now;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (uint64_t spin = 0;; ++spin) {
        if (svc_is_done(ctx, t)) return 0;
        if ((spin & 255) != 255) {
            __builtin_ia32_pause();
            continue;
        }
        if (hipStreamQuery(ctx->svc_stream) == hipSuccess) {   // the grid is gone
            if (svc_exited_clean(ctx)) return 0;
            std::vector<uint64_t> done;
            int rc = svc_read_done(ctx, done);
            if (rc) return rc;
            if (svc_dev_done(ctx, done, t)) return 0;
            const uint64_t st = __atomic_load_n(&ctx->svc_host->status, __ATOMIC_ACQUIRE);
            return fail(-EIO, "verify service exited (%s); ticket %llu will not complete",
                        st == kSvcIdleTimeout ? "idle timeout" : st == kSvcWatchdog ? "watchdog" : "grid ended",
                        (unsigned long long)(ctx->svc_base + t - 1));
        }
        clock_gettime(CLOCK_MONOTONIC, &now);
        double ms = (now.tv_sec - t0.tv_sec) * 1e3 + (now.tv_nsec - t0.tv_nsec) * 1e-6;
        if (timeout_ms >= 0 && ms > timeout_ms)
            return fail(-ETIMEDOUT, "ticket %llu not done after %d ms", (unsigned long long)(ctx->svc_base + t - 1),
                        timeout_ms);
    }
}

static int svc_post(hfv_ctx *ctx, uint64_t recs, uint64_t bits, uint64_t n, uint64_t stride, uint64_t *ticket)
{
    const uint64_t t = ctx->svc_next;   // grid-local batch number
    if (t > kSvcRing) {   // the slot's previous batch must be done (and its descriptor read)
        int rc = svc_wait_done(ctx, t - kSvcRing, 60000);
        if (rc) return rc;
    }
    SvcDesc *d = &ctx->svc_host->desc[(t - 1) % kSvcRing];
    d->recs = recs;
    d->bits = bits;
    d->n = n;
    d->stride = stride;
    __atomic_store_n(&d->seq, ctx->svc_tag | t, __ATOMIC_RELEASE);
    ctx->svc_next = t + 1;
    if (ticket) {   // a stop descriptor takes a grid slot but no ticket
        *ticket = ctx->svc_base + t - 1;
        ctx->svc_ticket = *ticket + 1;
    }
    return 0;
}

// Re-derive the block weights from the grid that just stopped (svc_run grids only: every batch
// was posted before the launch, so no block waited for the host and a block's tiles over its
// time from table fill to its last completed share is its verify rate).  Weights follow the
// XCDs' mean rates (block j on XCD j % 8) and block 0's own, averaged with the previous weights
// (halves run-to-run noise), clamped to [1/2, 2] of nominal.  Grids shorter than 50 us carry
// too little signal and leave them alone: with the grid's duration (grid_ns: its dispatch events;
// < 0 when it was not timed, then block 0's own stamps) below that, the G stamps are not even
// copied (a synchronous 16 KiB copy after every short grid).
static void svc_balance(hfv_ctx *ctx, double grid_ns)
{
    const uint64_t G = ctx->svc_grid;
    if (G < 16 || ctx->svc_run_ns.empty()) return;
    if (grid_ns >= 0.0 && grid_ns < 50000.0) return;
    if (grid_ns < 0.0) {   // untimed grid: block 0's span first (s_memrealtime, 100 MHz)
        uint64_t b0[2] = {0, 0};
        if (svc_dev_read(ctx, &b0[0], offsetof(SvcDev, blk_start), 8) ||
            svc_dev_read(ctx, &b0[1], offsetof(SvcDev, blk_fin), 8) || b0[1] < b0[0] + 5000)
            return;
    }
    std::vector<uint64_t> bt(2 * kSvcMaxBlocks);   // blk_start[0..G), blk_fin[0..G) (adjacent in SvcDev)
    static_assert(offsetof(SvcDev, blk_fin) == offsetof(SvcDev, blk_start) + kSvcMaxBlocks * 8, "layout");
    if (svc_dev_read(ctx, bt.data(), offsetof(SvcDev, blk_start), G * 8) ||
        svc_dev_read(ctx, bt.data() + kSvcMaxBlocks, offsetof(SvcDev, blk_fin), G * 8))
        return;
    const uint64_t *blk_start = bt.data(), *blk_fin = bt.data() + kSvcMaxBlocks;
    const SvcWeights &wu = ctx->svc_w_used;
    std::vector<uint64_t> cum(G + 1, 0);
    for (uint64_t k = 0; k < G; ++k) cum[k + 1] = cum[k] + (k ? wu.w[k % 8] : wu.w0);
    const uint64_t W = cum[G];
    std::vector<double> tiles(G, 0.0);
    for (size_t i = 0; i < ctx->svc_run_ns.size();) {   // runs of equal batch sizes at once
        size_t j = i;
        while (j < ctx->svc_run_ns.size() && ctx->svc_run_ns[j] == ctx->svc_run_ns[i]) ++j;
        const uint64_t T = (ctx->svc_run_ns[i] + 63) / 64;
        for (uint64_t k = 0; k < G; ++k)
            tiles[k] += (double)(j - i) * (double)(T * cum[k + 1] / W - T * cum[k] / W);
        i = j;
    }
    double rx[8] = {0}, r0 = 0, rsum = 0;
    int cx[8] = {0};
    uint64_t span = 0;
    for (uint64_t k = 0; k < G; ++k) {
        const uint64_t a = blk_start[k], b = blk_fin[k];
        if (b <= a || tiles[k] <= 0) return;   // a block without a measurement: keep the weights
        if (b - a > span) span = b - a;
        const double r = tiles[k] / (double)(b - a);
        rsum += r;
        if (k == 0) r0 = r;
        else {
            rx[k % 8] += r;
            cx[k % 8] += 1;
        }
    }
    if (span < 5000) return;   // 100 MHz ticks: 50 us
    const double mean = rsum / (double)G;
    // A grid some of whose blocks ran far below the others was disturbed from outside (a
    // transient on the box: blocks' rates normally stay within a few % of each other); learning
    // from it would carry the disturbance into the next grids' shares.
    double rmin = 1e300, rmax = 0;
    for (uint64_t k = 0; k < G; ++k) {
        const uint64_t a = blk_start[k], b = blk_fin[k];
        const double r = tiles[k] / (double)(b - a);
        rmin = r < rmin ? r : rmin;
        rmax = r > rmax ? r : rmax;
    }
    if (rmax > 1.6 * rmin) return;
    auto blend = [&](uint32_t old, double rate) {
        double w = 0.5 * old + 0.5 * kSvcWeightUnit * rate / mean;
        if (w < kSvcWeightUnit / 2) w = kSvcWeightUnit / 2;
        if (w > kSvcWeightUnit * 2) w = kSvcWeightUnit * 2;
        return (uint32_t)(w + 0.5);
    };
    for (int x = 0; x < 8; ++x)
        if (cx[x]) ctx->svc_w.w[x] = blend(ctx->svc_w.w[x], rx[x] / cx[x]);
    ctx->svc_w.w0 = blend(ctx->svc_w.w0, r0);
}

static int svc_stop(hfv_ctx *ctx, float *kernel_ms)
{
    if (kernel_ms) *kernel_ms = 0.0f;
    if (!ctx->svc_running) return 0;
    const uint64_t last = ctx->svc_next - 1 - (ctx->svc_stop_posted ? 1 : 0);   // last batch posted
    int rc = 0;
    if (!ctx->svc_stop_posted && __atomic_load_n(&ctx->svc_host->status, __ATOMIC_ACQUIRE) == 0)
        rc = svc_post(ctx, 0, 0, kSvcStopN, 0, nullptr);
    // the grid exits on the stop descriptor, or on its idle timeout if the post failed.  Spin
    // on the stream for a while first: the blocking wait sleeps on an interrupt, whose wake-up
    // costs more than the last batches of a short run.
    hipError_t e = hipErrorNotReady;
    struct timespec t0, now;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (uint64_t spin = 0;; ++spin) {
        e = hipStreamQuery(ctx->svc_stream);
        if (e != hipErrorNotReady) break;
        __builtin_ia32_pause();
        if ((spin & 1023) == 1023) {
            clock_gettime(CLOCK_MONOTONIC, &now);
            if ((now.tv_sec - t0.tv_sec) * 1000000000ll + (now.tv_nsec - t0.tv_nsec) > 20000000ll) {   // 20 ms
                e = hipStreamSynchronize(ctx->svc_stream);
                break;
            }
        }
    }
    ctx->svc_running = false;
    if (e != hipSuccess) return hip_fail(e, "verify service");
    if (rc) return rc;
    if (kernel_ms && ctx->svc_timed) HIP_TRY(hipEventElapsedTime(kernel_ms, ctx->svc_ev[0], ctx->svc_ev[1]));
    if (ctx->svc_adapt && __atomic_load_n(&ctx->svc_host->status, __ATOMIC_ACQUIRE) == 0) {
        // the grid's own duration decides whether its stamps carry signal (the host
        // time since the launch call can be far longer than the grid ran): its dispatch events when
        // it was timed, else block 0's stamps (two words) before all G stamps are fetched
        double grid_ns = -1.0;
        float ms = 0.0f;
        if (ctx->svc_timed && hipEventElapsedTime(&ms, ctx->svc_ev[0], ctx->svc_ev[1]) == hipSuccess) grid_ns = ms * 1e6;
        svc_balance(ctx, grid_ns);
    }
    ctx->svc_adapt = false;
    // A grid that left on the stop descriptor verified every batch before it (each block
    // reaches the stop only after its share of all earlier batches).  An idle or watchdog
    // exit is clean unless it left a posted batch unverified (batches may complete out of
    // order; only the newest kSvcRing can still be open): scan those in a copy of the device
    // completion words (the relay may have left before forwarding them; not paid on a normal stop).
    if (__atomic_load_n(&ctx->svc_host->status, __ATOMIC_ACQUIRE) == 0) return 0;
    std::vector<uint64_t> done;
    rc = svc_read_done(ctx, done);
    if (rc) {
        // the completion words cannot be read: every ticket that may still have been open is
        // recorded as lost, so no poll or wait reports it done (fail closed)
        for (uint64_t t = last; t > 0 && t + kSvcRing > last; --t) {
            if (ctx->svc_lost.size() >= 4096) ctx->svc_lost.erase(ctx->svc_lost.begin(), ctx->svc_lost.begin() + 1024);
            ctx->svc_lost.push_back(ctx->svc_base + t - 1);
        }
        return rc;
    }
    uint64_t first_lost = 0;
    for (uint64_t t = last; t > 0 && t + kSvcRing > last; --t)
        if (!svc_dev_done(ctx, done, t)) {
            first_lost = ctx->svc_base + t - 1;
            if (ctx->svc_lost.size() >= 4096) ctx->svc_lost.erase(ctx->svc_lost.begin(), ctx->svc_lost.begin() + 1024);
            ctx->svc_lost.push_back(first_lost);
        }
    if (first_lost)
        return fail(-ETIMEDOUT, "verify service exited on its idle timeout before ticket %llu",
                    (unsigned long long)first_lost);
    return 0;
}

// Ticket state: 1 done, 0 pending, -EIO lost (its grid stopped without verifying it),
// -EINVAL never issued.  Tickets of stopped grids were verified unless they exited on a
// timeout (svc_lost); tickets of the running grid are done once their completion was
// forwarded, or once the grid has left on its stop.
static int svc_ticket_state(const hfv_ctx *ctx, uint64_t ticket)
{
    if (!ctx->svc_host || ticket == 0 || ticket >= ctx->svc_ticket) return -EINVAL;
    for (uint64_t l : ctx->svc_lost)
        if (l == ticket) return -EIO;
    if (ticket < ctx->svc_base || !ctx->svc_running) return 1;
    return svc_is_done(ctx, ticket - ctx->svc_base + 1) || svc_exited_clean(ctx) ? 1 : 0;
}

int svc_quiesce(hfv_ctx *ctx) { return ctx->svc_running ? svc_stop(ctx, nullptr) : 0; }

static bool svc_keys_changed(hfv_ctx *ctx)
{
    return ctx->dirty || (ctx->keymap && keymap_seq(ctx->keymap) != ctx->keymap_seq);
}

extern "C" {

// A new service grid in two halves, so that a submit can post its batches into the ring
// between them and the grid finds them there when it starts: svc_begin (generation tag, key
// table, bookkeeping) and svc_launch.
static int svc_begin(hfv_ctx *ctx, uint32_t idle_ms, DevState **ds)
{
    if (!ctx->svc_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&ctx->svc_stream, hipStreamNonBlocking));
        HIP_TRY(hipHostMalloc((void **)&ctx->svc_host, sizeof(SvcShared),
                              hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(hipHostGetDevicePointer((void **)&ctx->svc_host_dev, ctx->svc_host, 0));
        HIP_TRY(hipMalloc((void **)&ctx->svc_dev, sizeof(SvcDev)));
        for (int i = 0; i < 2; ++i) HIP_TRY(hipEventCreate(&ctx->svc_ev[i]));
        memset(ctx->svc_host, 0, sizeof(SvcShared));
        HIP_TRY(hipMemsetAsync(ctx->svc_dev, 0, sizeof(SvcDev), ctx->svc_stream));
    }
    // a new generation: words an earlier grid left in the ring, the mirror and the completion
    // tables carry a smaller tag and never match
    ctx->svc_tag += 1ull << 40;
    __atomic_store_n(&ctx->svc_host->status, 0, __ATOMIC_RELEASE);
    int rc = publish_keys(ctx, ctx->svc_stream, ds);
    if (rc) return rc;
    ctx->svc_keysel = ctx->keysel;
    ctx->svc_inf_off = ctx->inf_off;
    ctx->svc_hf_off = ctx->hf_off;
    ctx->svc_idle_ms = idle_ms ? idle_ms : 1000;
    ctx->svc_next = 1;
    ctx->svc_base = ctx->svc_ticket;
    ctx->svc_stop_posted = false;
    ctx->svc_adapt = false;
    return 0;
}

#ifdef HFV_TEST_HOOKS
static uint32_t g_svc_relay_delay_us = 0;   // hfv_debug_relay_delay
#else
static constexpr uint32_t g_svc_relay_delay_us = 0;
#endif

static inline uint64_t mono_ns()
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (uint64_t)t.tv_sec * 1000000000ull + (uint64_t)t.tv_nsec;
}

// call_ns (nullable): svc_run's phase stamps (hfv_debug_service_call_ns), [3] before and [4] after
// the launch call; other callers (submitv, start) leave them alone
static int svc_launch(hfv_ctx *ctx, DevState *ds, uint64_t *call_ns = nullptr)
{
    const bool noev = !ctx->svc_timing;
    ctx->svc_timed = !noev;
    // the batches (and the stop) the caller posted before the launch (svc_run, submitv): the
    // first kSvcInline travel in the kernel arguments, so the blocks start on them without any
    // host round trip; the relay fetches the rest
    SvcArgs a;
    memset(&a, 0, sizeof a);
    a.tab = &ds->keys;
    a.host = ctx->svc_host_dev;
    a.dev = ctx->svc_dev;
    a.inf_off = ctx->inf_off;
    a.hf_off = ctx->hf_off;
    a.idle_ticks = (uint64_t)ctx->svc_idle_ms * 100000ull;
    a.tag = ctx->svc_tag;
    ctx->svc_w_used = ctx->svc_w;
    a.weights = ctx->svc_w_used;
    const uint64_t posted = ctx->svc_next - 1;
    a.n_inline = (uint32_t)(posted < kSvcInline ? posted : kSvcInline);
    for (uint32_t i = 0; i < a.n_inline; ++i) {
        const SvcDesc &d = ctx->svc_host->desc[i];
        a.inl[i] = {d.recs, d.bits, d.n, d.stride};
    }
    a.relay_delay_us = g_svc_relay_delay_us;
    a.launch = ctx->svc_launches;
    // slot 0's device key rows as published for this grid (the host image is what the last
    // publish copied into the device table), and T0
    a.pro = key_prologue(&ctx->host_img->keys);
    if (call_ns) call_ns[3] = mono_ns();
    int e = launch_verify_service(ctx->geom, ctx->keysel, a, ctx->svc_stream, noev ? nullptr : ctx->svc_ev[0],
                                  noev ? nullptr : ctx->svc_ev[1], &ctx->svc_grid);
    if (call_ns) call_ns[4] = mono_ns();
    int rc = after_launch(ctx, ctx->svc_stream, e, "verify service launch");
    if (rc) return rc;
    ++ctx->svc_launches;
    ctx->svc_running = true;
    return 0;
}

int hfv_service_start(hfv_ctx *ctx, uint32_t idle_ms)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    DeviceGuard g(ctx->device);
    if (ctx->svc_running && ctx->svc_stop_posted) {   // a run_async grid leaving on its own stop
        int rc = svc_stop(ctx, nullptr);
        if (rc) return rc;
    }
    if (ctx->svc_running) return 0;
    DevState *ds;
    int rc = svc_begin(ctx, idle_ms, &ds);
    if (rc) return rc;
    return svc_launch(ctx, ds);
}

static int svc_check_batch(const hfv_ctx *ctx, const void *recs, size_t stride, size_t n, const uint64_t *pass_bits)
{
    if (n >= kSvcStopN / 2) return fail(-EINVAL, "batch too large");
    static const uint64_t none = 0;   // an empty batch may come without buffers; its stride is checked all the same
    return check_records(ctx, n || recs ? recs : &none, stride, n || pass_bits ? pass_bits : &none);
}

// Restart the grid if it left on its idle timeout or if keys/keysel/layout changed (a batch
// boundary); if no grid runs, begin one and return its table in *launch (the caller posts its
// batches, then launches it with svc_launch), else *launch = nullptr.
static int svc_ready(hfv_ctx *ctx, DevState **launch)
{
    *launch = nullptr;
    if (ctx->svc_running && ctx->svc_stop_posted) {
        // a grid started by hfv_service_run_async has its stop behind its batches and exits by
        // itself: nothing posted now would be read, so reap it and begin a fresh grid
        int rc = svc_stop(ctx, nullptr);
        if (rc) return rc;
    }
    if (ctx->svc_running && __atomic_load_n(&ctx->svc_host->status, __ATOMIC_ACQUIRE) != 0) {
        // the grid left on its idle timeout: reap it (batches it left unverified are recorded
        // as lost for hfv_service_wait/poll) and start a fresh one
        (void)svc_stop(ctx, nullptr);
    }
    // key, key-selection or layout changes take effect at this batch boundary; the grid's
    // batch counter is 32-bit, so the service also restarts every 2^31 batches
    if (ctx->svc_running && (svc_keys_changed(ctx) || ctx->svc_keysel != ctx->keysel ||
                             ctx->svc_inf_off != ctx->inf_off || ctx->svc_hf_off != ctx->hf_off ||
                             ctx->svc_next >= (1ull << 31))) {
        int rc = svc_stop(ctx, nullptr);
        if (rc) return rc;
    }
    if (!ctx->svc_running) return svc_begin(ctx, ctx->svc_idle_ms, launch);
    return 0;
}

int hfv_service_submit(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, uint64_t *pass_bits,
                       uint64_t *ticket)
{
    if (!ctx || !ticket) return fail(-EINVAL, "null argument");
    *ticket = 0;
    struct hfv_batch b = {recs, stride, n, pass_bits};
    return hfv_service_submitv(ctx, &b, 1, ticket);
}

int hfv_service_submitv(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, uint64_t *first_ticket)
{
    if (!ctx || !first_ticket || (!batches && count)) return fail(-EINVAL, "null argument");
    *first_ticket = 0;
    for (size_t i = 0; i < count; ++i) {
        int rc = svc_check_batch(ctx, batches[i].recs, batches[i].stride, batches[i].n, batches[i].pass_bits);
        if (rc) return count == 1 ? rc : fail_batch(rc, i);
    }
    if (count == 0) return 0;
    DeviceGuard g(ctx->device);
    DevState *launch = nullptr;
    int rc = svc_ready(ctx, &launch);
    if (rc) return rc;
    for (size_t i = 0; i < count; ++i) {
        // a new grid is launched once the ring holds the first batches (at most a ring's
        // worth: posting more waits for completions), so it finds them when it starts
        if (launch && i == (size_t)kSvcRing) {
            rc = svc_launch(ctx, launch);
            launch = nullptr;
            if (rc) return rc;
        }
        uint64_t t = 0;
        rc = svc_post(ctx, (uint64_t)(uintptr_t)batches[i].recs, (uint64_t)(uintptr_t)batches[i].pass_bits,
                      batches[i].n, batches[i].stride, &t);
        if (rc) return rc;   // batches 0..i-1 are posted (tickets *first_ticket ..)
        if (i == 0) *first_ticket = t;
    }
    return launch ? svc_launch(ctx, launch) : 0;
}

static int svc_run(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, uint64_t *first_ticket,
                   float *kernel_ms, bool wait);

int hfv_service_run(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, uint64_t *first_ticket,
                    float *kernel_ms)
{
    return svc_run(ctx, batches, count, first_ticket, kernel_ms, true);
}

int hfv_service_run_async(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, uint64_t *first_ticket)
{
    return svc_run(ctx, batches, count, first_ticket, nullptr, false);
}

static int svc_run(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, uint64_t *first_ticket,
                   float *kernel_ms, bool wait)
{
    if (!ctx || !first_ticket || (!batches && count)) return fail(-EINVAL, "null argument");
    ctx->svc_call_ns[0] = mono_ns();
    *first_ticket = 0;
    if (kernel_ms) *kernel_ms = 0.0f;
    for (size_t i = 0; i < count; ++i) {
        int rc = svc_check_batch(ctx, batches[i].recs, batches[i].stride, batches[i].n, batches[i].pass_bits);
        if (rc) return fail_batch(rc, i);
    }
    DeviceGuard g(ctx->device);
    int rc = svc_quiesce(ctx);
    if (rc) return rc;
    DevState *ds;
    ctx->svc_call_ns[1] = mono_ns();
    rc = svc_begin(ctx, ctx->svc_idle_ms, &ds);
    if (rc) return rc;
    ctx->svc_call_ns[2] = mono_ns();
    ctx->svc_adapt = true;   // every batch is in the ring before the grid starts: measure its balance
    ctx->svc_run_ns.resize(count);
    for (size_t i = 0; i < count; ++i) ctx->svc_run_ns[i] = batches[i].n;
    // the batches, then the stop right behind them, are in the ring before the grid starts (a
    // longer run launches once the ring is full): the grid exits as soon as its blocks finish
    // their share of the last batch, with no stop to post and relay afterwards
    bool launched = false;
    for (size_t i = 0; i <= count && !rc; ++i) {
        if (!launched && ctx->svc_next > (uint64_t)kSvcRing) {
            // a run longer than the ring: the grid is launched mid-post, so the phase stamps of
            // this call would mix posting and launching -- they are left at 0 for it
            memset(ctx->svc_call_ns, 0, sizeof ctx->svc_call_ns);
            rc = svc_launch(ctx, ds);
            launched = true;
            if (rc) break;
        }
        if (i == count) {
            rc = svc_post(ctx, 0, 0, kSvcStopN, 0, nullptr);
            ctx->svc_stop_posted = rc == 0;
            break;
        }
        uint64_t t = 0;
        rc = svc_post(ctx, (uint64_t)(uintptr_t)batches[i].recs, (uint64_t)(uintptr_t)batches[i].pass_bits,
                      batches[i].n, batches[i].stride, &t);
        if (i == 0) *first_ticket = t;
    }
    if (!launched) {
        int lr = svc_launch(ctx, ds, ctx->svc_call_ns);
        if (lr) return lr;
        ctx->svc_call_ns[5] = mono_ns();
    }
    if (!wait) return rc;   // the grid exits after the stop posted behind the batches
    int sr = svc_stop(ctx, kernel_ms);
    return rc ? rc : sr;
}

int hfv_service_poll(hfv_ctx *ctx, uint64_t ticket)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    int st = svc_ticket_state(ctx, ticket);
    // A pending ticket of a grid that left without its stop (idle timeout or watchdog: the grid
    // sets the status word in pinned memory first) would never complete: its relay wave stopped
    // forwarding completions when it published the stop.  Only then (a read of pinned memory
    // decides it, no HIP call on the poll path) reap the grid: svc_stop reads the
    // device completion words and records the tickets it left unverified.
    if (st == 0 && ctx->svc_running && __atomic_load_n(&ctx->svc_host->status, __ATOMIC_ACQUIRE) != 0 &&
        hipStreamQuery(ctx->svc_stream) == hipSuccess) {
        DeviceGuard g(ctx->device);
        const int rc = svc_stop(ctx, nullptr);
        // -ETIMEDOUT: the grid left tickets unverified, now recorded as lost (poll reports -EIO for
        // those below).  Any other failure means the lost tickets could not be read: report it rather
        // than fall through to a state that would call them done (fail closed).
        if (rc && rc != -ETIMEDOUT) return rc;
        st = svc_ticket_state(ctx, ticket);
    }
    if (st == -EINVAL) return fail(-EINVAL, "unknown ticket %llu", (unsigned long long)ticket);
    if (st == -EIO) return fail(-EIO, "verify service stopped before ticket %llu", (unsigned long long)ticket);
    return st;
}

int hfv_service_wait(hfv_ctx *ctx, uint64_t ticket, int timeout_ms)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    int st = svc_ticket_state(ctx, ticket);
    if (st == -EINVAL) return fail(-EINVAL, "unknown ticket %llu", (unsigned long long)ticket);
    if (st == -EIO) return fail(-EIO, "verify service stopped before ticket %llu", (unsigned long long)ticket);
    if (st == 1) return 0;
    if (!ctx->svc_running) return fail(-EIO, "verify service stopped before ticket %llu", (unsigned long long)ticket);
    return svc_wait_done(ctx, ticket - ctx->svc_base + 1, timeout_ms);
}

int hfv_service_stop(hfv_ctx *ctx, float *kernel_ms)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    DeviceGuard g(ctx->device);
    return svc_stop(ctx, kernel_ms);
}

int hfv_service_running(const hfv_ctx *ctx) { return ctx && ctx->svc_running ? 1 : 0; }

int hfv_service_set_timing(hfv_ctx *ctx, int enable)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    ctx->svc_timing = enable != 0;
    return 0;
}

int hfv_service_set_grid(hfv_ctx *ctx, int blocks)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (blocks < 0) return fail(-EINVAL, "blocks %d < 0", blocks);
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);   // the next grid takes the new shape
    ctx->geom.svc_blocks = blocks == 0 || blocks > ctx->geom.num_cus ? ctx->geom.num_cus : blocks;
    return 0;
}

// Diagnostic (not part of include/scion_hfv.h): the block weights the next service grid will
// use (w[0..7] per XCD, then block 0's), in units of 1/1024 of an equal share.
int hfv_debug_service_weights(hfv_ctx *ctx, uint32_t out[9])
{
    if (!ctx || !out) return fail(-EINVAL, "bad argument");
    for (int x = 0; x < 8; ++x) out[x] = ctx->svc_w.w[x];
    out[8] = ctx->svc_w.w0;
    return 0;
}

// Diagnostic (not part of include/scion_hfv.h): the weights the running / last service grid was
// launched with (svc_w_used, what svc_balance reads), in the same order.
int hfv_debug_service_weights_used(hfv_ctx *ctx, uint32_t out[9])
{
    if (!ctx || !out) return fail(-EINVAL, "bad argument");
    for (int x = 0; x < 8; ++x) out[x] = ctx->svc_w_used.w[x];
    out[8] = ctx->svc_w_used.w0;
    return 0;
}

// Diagnostic (not part of include/scion_hfv.h): out[i] = s_memrealtime (100 MHz) when block
// 0 loaded ring slot i's descriptor from the mirror (i < kSvcRing; inline batches are not
// loaded); out[kSvcRing .. kSvcRing + 3] = block 0 wave 0's s_memtime and s_memrealtime at its
// start and at its exit (the shader clock over the grid's life); out[kSvcRing + 4 + i] =
// s_memrealtime when the relay published slot i (2 * kSvcRing + 4 words).
int hfv_debug_service_clocks(hfv_ctx *ctx, uint64_t *out)
{
    if (!ctx || !out || !ctx->svc_dev) return fail(-EINVAL, "bad argument");
    static_assert(offsetof(SvcDev, relay) == offsetof(SvcDev, run_clock) + 32, "layout");
    int rc = svc_dev_read(ctx, out, offsetof(SvcDev, load_clock), kSvcRing * 8);
    if (!rc) rc = svc_dev_read(ctx, out + kSvcRing, offsetof(SvcDev, run_clock), 4 * 8);
    if (!rc) rc = svc_dev_read(ctx, out + kSvcRing + 4, offsetof(SvcDev, relay_clock), kSvcRing * 8);
    return rc;
}

// Diagnostic (not part of include/scion_hfv.h): the last grid's per-block stamps: out[0 .. G)
// = s_memrealtime (100 MHz) after the table fill, out[G .. 2G) = at the block's last completed
// share (what svc_balance reads); with words >= 4G also s_memtime (the shader clock) at those two
// points in out[2G .. 3G) and out[3G .. 4G).  Returns G in *grid.
int hfv_debug_service_blocks(hfv_ctx *ctx, uint64_t *out, size_t words, int *grid)
{
    if (!ctx || !out || !grid || !ctx->svc_dev) return fail(-EINVAL, "bad argument");
    const size_t g = ctx->svc_grid;
    if (words < 2 * g) return fail(-EINVAL, "need %zu words", 2 * g);
    *grid = (int)g;
    int rc = svc_dev_read(ctx, out, offsetof(SvcDev, blk_start), g * 8);
    if (!rc) rc = svc_dev_read(ctx, out + g, offsetof(SvcDev, blk_fin), g * 8);
    if (!rc && words >= 4 * g) rc = svc_dev_read(ctx, out + 2 * g, offsetof(SvcDev, blk_clk0), g * 8);
    if (!rc && words >= 4 * g) rc = svc_dev_read(ctx, out + 3 * g, offsetof(SvcDev, blk_clk1), g * 8);
    return rc;
}

// Diagnostic (not part of include/scion_hfv.h): the last grid's relay counters (SvcRelayStat,
// 8 words): the host round trip probed at grid start, host reads and their summed / longest
// round trips (100 MHz ticks), descriptors relayed, completions forwarded, waits of a block for
// a descriptor, descriptors in the kernel arguments.
int hfv_debug_service_relay(hfv_ctx *ctx, uint64_t out[8])
{
    if (!ctx || !out || !ctx->svc_dev) return fail(-EINVAL, "bad argument");
    int rc = svc_dev_read(ctx, out, offsetof(SvcDev, relay), 8 * 8);
    const uint32_t last = ctx->svc_launches ? ctx->svc_launches - 1 : 0;   // the last grid's area
    if (!rc)
        rc = svc_dev_read(ctx, &out[kRelayBlockWaits], offsetof(SvcDev, area) + (last & 1) * sizeof(SvcArea) +
                                                            offsetof(SvcArea, block_waits), 8);
    return rc;
}

// Diagnostic (not part of include/scion_hfv.h): INTEGRATION.md section 2's data-plane loop,
// timed -- per RX batch one hfv_service_submit, then hfv_service_wait on the ticket `depth`
// batches back (a feeder keeping `depth` batches in flight), the last tickets at the end; *ns =
// host nanoseconds from the first submit to the last wait's return.  The same public calls a C
// maintainer writes, without a foreign-function layer in between (bench.py's `per_call` leg).
int hfv_debug_feed_loop(hfv_ctx *ctx, const struct hfv_batch *b, size_t count, uint32_t depth, uint64_t *ns)
{
    if (!ctx || !ns || (!b && count) || depth == 0) return fail(-EINVAL, "bad argument");
    std::vector<uint64_t> t(count);
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    for (size_t i = 0; i < count; ++i) {
        int rc = hfv_service_submit(ctx, b[i].recs, b[i].stride, b[i].n, b[i].pass_bits, &t[i]);
        if (!rc && i >= depth) rc = hfv_service_wait(ctx, t[i - depth], 10000);
        if (rc) return rc;
    }
    for (size_t i = count > depth ? count - depth : 0; i < count; ++i) {
        int rc = hfv_service_wait(ctx, t[i], 10000);
        if (rc) return rc;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    *ns = (uint64_t)((t1.tv_sec - t0.tv_sec) * 1000000000ll + (t1.tv_nsec - t0.tv_nsec));
    return 0;
}

// Diagnostic (not part of include/scion_hfv.h): the host-side phases of the last
// hfv_service_run / run_async call in nanoseconds: [0] argument checks and stopping a previous
// grid, [1] the new grid's bookkeeping (svc_begin), [2] posting the batches and building the
// kernel arguments, [3] the launch call itself, [4] the rest (ticket state) to the return.  All 0
// for a call with more batches than the ring holds (its grid is launched mid-post).
int hfv_debug_service_call_ns(hfv_ctx *ctx, uint64_t out[5])
{
    if (!ctx || !out) return fail(-EINVAL, "bad argument");
    const uint64_t *c = ctx->svc_call_ns;
    for (int i = 0; i < 5; ++i) out[i] = c[i + 1] >= c[i] ? c[i + 1] - c[i] : 0;
    return 0;
}

#ifdef HFV_TEST_HOOKS
// Test hook (test build only): every host read of later service grids' relay wave takes `us`
// microseconds longer (a slow PCIe link), 0 = off.
int hfv_debug_relay_delay(uint32_t us)
{
    g_svc_relay_delay_us = us > 100000u ? 100000u : us;
    return 0;
}

// Test hook (test build only): the block weights the next service grid will use, in the order
// hfv_debug_service_weights reports them (w[0..7] per XCD, then block 0's).  Only values
// svc_balance can produce: each inside its clamp [kSvcWeightUnit / 2, 2 kSvcWeightUnit].
int hfv_debug_service_set_weights(hfv_ctx *ctx, const uint32_t w[9])
{
    if (!ctx || !w) return fail(-EINVAL, "bad argument");
    for (int x = 0; x < 9; ++x)
        if (w[x] < kSvcWeightUnit / 2 || w[x] > kSvcWeightUnit * 2)
            return fail(-EINVAL, "weight %d = %u outside [%u, %u]", x, w[x], kSvcWeightUnit / 2, kSvcWeightUnit * 2);
    for (int x = 0; x < 8; ++x) ctx->svc_w.w[x] = w[x];
    ctx->svc_w.w0 = w[8];
    return 0;
}
#endif

}  // extern "C"
