// hfv_host_path.cpp -- the entry points that take frames or records in host memory
// (hfv_br_process_host, hfv_verify_records_host, hfv_verify_frames_host, hfv_host_register), what
// their staging workers need of the machine (thread count, NUMA pinning), and the router stage of
// in-library pipelines (hfv_loop.cpp).  The three chunked calls run on the two-slot schedule and the
// worker pool of hfv_host_pipe.h and share the ctx's one staging set (host_stage).
#include <pthread.h>
#include <stdlib.h>

#include "hfv_ctx.h"
#include "hfv_host_pipe.h"

// Compact staging record of the host path: INF (8 B) at 0, HF (12 B) at 8, 4 B pad.
static constexpr size_t kHostRec = 24;

// Records per chunk of hfv_verify_records_host (a multiple of 64, so that no bitmap word straddles two
// chunks), frames per chunk and per retry round of hfv_br_process_host, and the row count below which
// host_rows runs inline.  kBrChunk is also the layout constant of the router's stage_out.
static const size_t kRecChunk = (size_t)1 << 18;
static const size_t kBrChunk = (size_t)1 << 16;
static const size_t kInlineRows = 8192;

// HFV_MUT_HOSTCHUNK (make hostchunk; 0 in every product build): one deliberately wrong step of the
// chunk pipelines, each in bounds of every buffer and with every synchronisation kept:
//   1  all three paths (two_slot_chunks, hfv_host_pipe.h): a retired chunk's results go to the place of
//      the chunk on the other slot (cut at item n)
//   2  records: a ragged chunk copies back cnt / 64 words (floor)
//   3  records: chunks after the first gather from recs + first * kHostRec instead of first * stride
//      (in bounds for stride >= kHostRec)
//   5  router: the verdict counters are zeroed before every chunk instead of once per call (after the
//      other stream has drained, so that the loss is the same in every run)
//   6  router: a retry round's results are scattered through idx[cnt - 1 - k]
// (4 was 1 in the router's own copy of the loop.)  tests/test_gpu_host_chunks.py must fail on every one,
// tests/test_gpu_frames_hostmem.py on 1.

#ifdef HFV_TEST_HOOKS
// hfv_debug_records_host_chunk / _br_host_chunk / _host_inline_rows: the three counts above made small,
// so that a few hundred records or frames span several chunks, reuse both stream slots, fill several
// retry rounds and go through the host pool's partition; 0 restores the default.  The staging buffers
// keep their full size: only the counts change.  hfv_debug_host_chunk_counts: what the last host-path
// call of the process ran (read-only): chunks launched in the first pass, retry rounds (second-run
// chunks of hfv_verify_frames_host), frames retried, chunks that reused a slot within the call.
static size_t g_rec_chunk = 0, g_br_chunk = 0, g_inline_rows = 0;
static uint64_t g_hc_counts[4] = {0, 0, 0, 0};
extern "C" int hfv_debug_records_host_chunk(size_t records)
{
    if ((records & 63) || records > kRecChunk) return fail(-EINVAL, "chunk must be a multiple of 64, at most %zu", kRecChunk);
    g_rec_chunk = records;
    return 0;
}
extern "C" int hfv_debug_br_host_chunk(size_t frames)
{
    if (frames > kBrChunk) return fail(-EINVAL, "chunk must be at most %zu", kBrChunk);
    g_br_chunk = frames;
    return 0;
}
extern "C" int hfv_debug_host_inline_rows(size_t rows)
{
    g_inline_rows = rows;
    return 0;
}
extern "C" int hfv_debug_host_chunk_counts(uint64_t out[4])
{
    if (!out) return fail(-EINVAL, "null buffer");
    memcpy(out, g_hc_counts, sizeof g_hc_counts);
    return 0;
}
static size_t rec_chunk() { return g_rec_chunk ? g_rec_chunk : kRecChunk; }
static size_t br_chunk() { return g_br_chunk ? g_br_chunk : kBrChunk; }
static size_t inline_rows() { return g_inline_rows ? g_inline_rows : kInlineRows; }
static void hc_reset() { memset(g_hc_counts, 0, sizeof g_hc_counts); }
static void hc_add(int k, uint64_t v) { g_hc_counts[k] += v; }
#else
static size_t rec_chunk() { return kRecChunk; }
static size_t br_chunk() { return kBrChunk; }
static size_t inline_rows() { return kInlineRows; }
static void hc_reset() {}
static void hc_add(int, uint64_t) {}
#endif
enum { kHcChunks = 0, kHcRounds = 1, kHcRetried = 2, kHcReuses = 3 };

// Host threads for staging copies: HFV_HOST_THREADS, default min(8, cores).
static int host_threads()
{
    static const int t = [] {
        const char *e = getenv("HFV_HOST_THREADS");
        int v = e ? atoi(e) : 0;
        if (v <= 0) {
            unsigned hc = std::thread::hardware_concurrency();
            v = hc ? (int)(hc < 8 ? hc : 8) : 4;
        }
        return v;
    }();
    return t;
}

// NUMA placement of the host-side workers: the staging copies of a GPU's host path run on
// the CPUs of the NUMA node its PCIe root port hangs off (one process per GPU, so the
// first ctx of the process decides).  HFV_NUMA_PIN=0 leaves the threads unpinned.
static std::mutex g_numa_m;
static cpu_set_t g_numa_cpus;
static bool g_numa_set = false;

static void pin_to_numa()
{
    std::lock_guard<std::mutex> g(g_numa_m);
    if (g_numa_set) (void)pthread_setaffinity_np(pthread_self(), sizeof g_numa_cpus, &g_numa_cpus);
}

// NUMA node of `device` (from its PCI bus id in sysfs) and that node's CPUs that this
// process may run on; -1 if unknown.
int device_numa(int device, cpu_set_t *cpus)
{
    char bus[64] = {0}, path[256];
    if (hipDeviceGetPCIBusId(bus, sizeof bus, device) != hipSuccess) return -1;
    for (char *p = bus; *p; ++p)
        if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    if (node < 0 || !cpus) return node;
    snprintf(path, sizeof path, "/sys/devices/system/node/node%d/cpulist", node);
    f = fopen(path, "r");
    if (!f) return node;
    cpu_set_t allowed;
    CPU_ZERO(cpus);
    if (sched_getaffinity(0, sizeof allowed, &allowed) != 0) CPU_ZERO(&allowed);
    int a, b;
    char sep;
    while (fscanf(f, "%d", &a) == 1) {
        b = a;
        if (fscanf(f, "%c", &sep) == 1 && sep == '-') {
            if (fscanf(f, "%d", &b) != 1) break;
            if (fscanf(f, "%c", &sep) != 1) sep = 0;
        }
        for (int c = a; c <= b && c < CPU_SETSIZE; ++c)
            if (CPU_ISSET(c, &allowed)) CPU_SET(c, cpus);
        if (sep != ',') break;
    }
    fclose(f);
    return node;
}

void note_numa(int device)
{
    const char *e = getenv("HFV_NUMA_PIN");
    if (e && atoi(e) == 0) return;
    cpu_set_t cpus;
    int node = device_numa(device, &cpus);
    std::lock_guard<std::mutex> g(g_numa_m);
    if (node >= 0 && !g_numa_set && CPU_COUNT(&cpus) > 0) {
        g_numa_cpus = cpus;
        g_numa_set = true;
    }
}

static HostPool &host_pool()
{
    static HostPool pool(host_threads(), pin_to_numa);
    return pool;
}

// fn(a, b) over [0, n) split into host_threads() contiguous parts (inline below kInlineRows items).
template <class F>
static void host_rows(size_t n, F fn)
{
    parallel_rows(host_threads(), inline_rows(), host_pool, n, fn);
}

// dst[i] = {INF, HF} of src record i (the verifier's 20 bytes).
static void gather_hf(uint8_t *dst, const uint8_t *src, size_t stride, uint32_t inf_off, uint32_t hf_off, size_t n)
{
    host_rows(n, [=](size_t a, size_t b) {
        for (size_t i = a; i < b; ++i) {
            const uint8_t *r = src + i * stride;
            uint8_t *d = dst + i * kHostRec;
            memcpy(d, r + inf_off, 8);
            memcpy(d + 8, r + hf_off, 12);
        }
    });
}

// Row copies between frames in their slots and packed windows: dst row i <- src row i.
static void copy_rows(uint8_t *dst, size_t dpitch, const uint8_t *src, size_t spitch, size_t width, size_t n)
{
    host_rows(n, [=](size_t a, size_t b) {
        for (size_t i = a; i < b; ++i) memcpy(dst + i * dpitch, src + i * spitch, width);
    });
}

static const size_t kBrStatWords = HFV_BR_STATS_IFINDEX * 2 * HFV_BR_COUNTERS;

// The device verdict counters of one host-path call: allocated on first use, zeroed on `st`.
static int brh_stats_buffer(hfv_ctx *ctx, hipStream_t st)
{
    if (!ctx->brh_dstats) HIP_TRY(hipMalloc((void **)&ctx->brh_dstats, kBrStatWords * 8));
    HIP_TRY(hipMemsetAsync(ctx->brh_dstats, 0, kBrStatWords * 8, st));
    return 0;
}

// ... added to the caller's (nullable) once the call's launches have completed.
static int brh_add_stats(hfv_ctx *ctx, uint64_t *stats)
{
    if (!stats) return 0;
    uint64_t tmp[kBrStatWords];
    HIP_TRY(hipMemcpy(tmp, ctx->brh_dstats, sizeof tmp, hipMemcpyDeviceToHost));
    for (size_t k = 0; k < kBrStatWords; ++k) stats[k] += tmp[k];
    return 0;
}

// The staging of one chunked call: both host streams exist and are idle (an earlier call that
// returned an error midway may have left work on them that still owns the staging), and each
// slot's pairs hold at least in_bytes and out_bytes.
static int host_stage(hfv_ctx *ctx, size_t in_bytes, size_t out_bytes)
{
    for (int i = 0; i < 2; ++i) {
        if (!ctx->hstream[i]) HIP_TRY(hipStreamCreateWithFlags(&ctx->hstream[i], hipStreamNonBlocking));
        HIP_TRY(hipStreamSynchronize(ctx->hstream[i]));
    }
    for (int i = 0; i < 2; ++i) {
        int rc = ctx->stage_in[i].reserve(in_bytes);
        if (!rc) rc = ctx->stage_out[i].reserve(out_bytes);
        if (rc) return rc;
    }
    return 0;
}

static int wait_slot(hfv_ctx *ctx, int sl)
{
    HIP_TRY(hipStreamSynchronize(ctx->hstream[sl]));
    return 0;
}

// The slot and window of a call over frames in their slots; window 0 is the default, min(slot, 256).
static int check_slot_window(size_t slot, size_t *window)
{
    if (slot < 64 || (slot & 7) || slot > 65535 * 8) return fail(-EINVAL, "slot must be >= 64 and a multiple of 8");
    if (*window == 0) *window = slot < 256 ? slot : 256;
    if (*window < 64 || (*window & 7) || *window > slot) return fail(-EINVAL, "window must be a multiple of 8 in [64, slot]");
    return 0;
}

// One chunk: frames[k * fstride] for k < cnt (window bytes each), metadata through pinned io.
static int brh_chunk(hfv_ctx *ctx, int sl, uint8_t *frames, size_t fstride, size_t maxlen, size_t window,
                     const uint16_t *len, const uint32_t *ifx, size_t cnt)
{
    hipStream_t st = ctx->hstream[sl];
    const StagePair &win = ctx->stage_in[sl], &io = ctx->stage_out[sl];
    memcpy(io.host, len, cnt * 2);
    memcpy(io.host + kBrChunk * 2, ifx, cnt * 4);
    HIP_TRY(hipMemcpyAsync(io.dev, io.host, kBrChunk * 6, hipMemcpyHostToDevice, st));
    // the header windows, packed by host threads into pinned staging, then one linear DMA
    copy_rows(win.host, window, frames, fstride, window, cnt);
    HIP_TRY(hipMemcpyAsync(win.dev, win.host, cnt * window, hipMemcpyHostToDevice, st));
    int rc = with_tables(ctx, st, "br_process launch", [&](DevState *ds) {
        return launch_br_process(br_geom(ctx), ds, win.dev, window, (uint32_t)maxlen, (uint32_t)window,
                                 (const uint16_t *)io.dev, (const uint32_t *)(io.dev + kBrChunk * 2), cnt,
                                 io.dev + kBrChunk * 6, io.dev + kBrChunk * 7, (int32_t *)(io.dev + kBrChunk * 8),
                                 ctx->brh_dstats, st);
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(win.host, win.dev, cnt * window, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(io.host + kBrChunk * 6, io.dev + kBrChunk * 6, kBrChunk * 6, hipMemcpyDeviceToHost, st));
    return 0;
}

// A retired chunk (its stream synchronized): the rewritten windows back into the frames
// (host threads), and the per-frame results.
static void brh_results(hfv_ctx *ctx, int sl, uint8_t *frames, size_t fstride, size_t window, size_t cnt,
                        uint8_t *action, uint8_t *verdict, int32_t *egress)
{
    copy_rows(frames, fstride, ctx->stage_in[sl].host, window, window, cnt);
    const uint8_t *hio = ctx->stage_out[sl].host;
    memcpy(action, hio + kBrChunk * 6, cnt);
    memcpy(verdict, hio + kBrChunk * 7, cnt);
    memcpy(egress, hio + kBrChunk * 8, cnt * 4);
}

uint8_t *host_dev_ptr(hfv_ctx *ctx, const void *p, size_t bytes)
{
    const uint8_t *q = (const uint8_t *)p;
    for (int i = 0; i < ctx->nhreg; ++i) {
        const hfv_ctx::HostRange &r = ctx->hreg[i];
        if (q >= r.host && q + bytes <= r.host + r.bytes) return r.dev + (q - r.host);
    }
    return nullptr;
}

// The zero-copy calls' device scratch holds at least `bytes`; after a failure it is null, its size 0.
static int zc_scratch(hfv_ctx *ctx, size_t bytes)
{
    if (ctx->zc_cap >= bytes) return 0;
    if (ctx->zc_meta) (void)hipFree(ctx->zc_meta);
    ctx->zc_meta = nullptr;
    ctx->zc_cap = 0;
    HIP_TRY(hipMalloc((void **)&ctx->zc_meta, bytes));
    ctx->zc_cap = bytes;
    return 0;
}

// The per-item arrays of one zero-copy call on stream st.  in / out give an array's device address:
// the array itself where it lies in a registered buffer, else its offset in the scratch (grown to
// `need` bytes when the first such array turns up), copied up at once for an input and copied back
// by copy_back for an output.  A null array stays null.  rc holds the first failure.
namespace {
struct ZcArrays {
    hfv_ctx *ctx;
    hipStream_t st;
    size_t need;
    int rc = 0;
    struct Back {
        void *host;
        const uint8_t *dev;
        size_t bytes;
    } back[3] = {};
    int nback = 0;

    uint8_t *place(const void *host, size_t bytes, size_t off, bool input)
    {
        if (!host || rc) return nullptr;
        if (uint8_t *d = host_dev_ptr(ctx, host, bytes)) return d;
        if ((rc = zc_scratch(ctx, need))) return nullptr;
        uint8_t *d = ctx->zc_meta + off;
        if (!input) {
            back[nback++] = {(void *)host, d, bytes};
        } else if (hipError_t e = hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, st)) {
            rc = hip_fail(e, "hipMemcpyAsync of a zero-copy input");
        }
        return d;
    }
    template <class T>
    const T *in(const T *host, size_t bytes, size_t off) { return (const T *)place(host, bytes, off, true); }
    template <class T>
    T *out(T *host, size_t bytes, size_t off) { return (T *)place(host, bytes, off, false); }
    int copy_back()
    {
        for (int k = 0; k < nback; ++k)
            HIP_TRY(hipMemcpyAsync(back[k].host, back[k].dev, back[k].bytes, hipMemcpyDeviceToHost, st));
        return 0;
    }
};
}  // namespace

// Zero-copy: the frames are in a registered (mapped) ring, so the kernel reads each header
// window across PCIe itself and writes back only the rewritten rows; no DMA of frame bytes and
// no retry pass (the whole frame stays addressable).  Per-frame metadata uses the caller's
// arrays in place when they are registered too, else one copy each way.
static int br_zero_copy(hfv_ctx *ctx, uint8_t *dframes, size_t slot, const uint16_t *len, const uint32_t *ifx,
                        size_t n, uint8_t *action, uint8_t *verdict, int32_t *egress, uint64_t *stats)
{
    hipStream_t st = ctx->stream;
    int rc = brh_stats_buffer(ctx, st);
    if (rc) return rc;
    ZcArrays z{ctx, st, n * 16};
    const uint16_t *dlen = z.in(len, n * 2, 0);
    const uint32_t *difx = z.in(ifx, n * 4, n * 4);
    uint8_t *dact = z.out(action, n, n * 2);
    uint8_t *dver = z.out(verdict, n, n * 3);
    int32_t *degr = z.out(egress, n * 4, n * 8);
    if (z.rc) return z.rc;
    rc = with_tables(ctx, st, "br_process launch", [&](DevState *ds) {
        return launch_br_process(br_geom(ctx), ds, dframes, slot, (uint32_t)slot, (uint32_t)slot, dlen, difx, n, dact,
                                 dver, degr, ctx->brh_dstats, st);
    });
    if (!rc) rc = z.copy_back();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return brh_add_stats(ctx, stats);
}

int hfv::br_zc_prepare(hfv_ctx *ctx)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    SVC_QUIESCE(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    return 0;
}

int hfv::br_dev_launch(hfv_ctx *ctx, void *stream, uint8_t *dframes, size_t slot, const uint16_t *dlen,
                       const uint32_t *difx, size_t n, uint8_t *dact, uint8_t *dver, int32_t *degr, uint64_t *dstats,
                       uint8_t *dout)
{
    if (n == 0) return 0;
    return with_tables(ctx, (hipStream_t)stream, "br_process launch", [&](DevState *ds) {
        return launch_br_process(br_geom(ctx), ds, dframes, slot, (uint32_t)slot, (uint32_t)slot, dlen, difx, n, dact,
                                 dver, degr, dstats, stream, nullptr, nullptr, dout);
    });
}

extern "C" {

// Windowed host path.  Per chunk of br_chunk() frames, on alternating streams: the windows packed
// into pinned staging, H2D of the windows + metadata, the kernel (stride = window, lengths clamped
// to the caller's slot), D2H of the rewritten windows + results.  Then frames marked
// HFV_BR_ACTION_RETRY (headers beyond the window) go through again with whole slots.
int hfv_br_process_host(hfv_ctx *ctx, uint8_t *frames, size_t slot, const uint16_t *len,
                        const uint32_t *ingress_ifindex, size_t n, size_t window, uint8_t *action,
                        uint8_t *verdict, int32_t *egress_ifindex, uint64_t *stats)
{
    if (n == 0) return ctx ? 0 : fail(-EINVAL, "ctx is NULL");
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (!frames || !len || !ingress_ifindex || !action || !verdict || !egress_ifindex) return fail(-EINVAL, "null buffer");
    int rc = check_slot_window(slot, &window);
    if (rc) return rc;
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    hc_reset();
    uint8_t *dframes = host_dev_ptr(ctx, frames, n * slot);
    if (dframes) return br_zero_copy(ctx, dframes, slot, len, ingress_ifindex, n, action, verdict, egress_ifindex, stats);
    rc = host_stage(ctx, kBrChunk * window, kBrChunk * 12);
    if (!rc) rc = brh_stats_buffer(ctx, ctx->hstream[0]);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(ctx->hstream[0]));
    const size_t chunk = br_chunk();
    hc_add(kHcChunks, (n + chunk - 1) / chunk);
    uint64_t reuses = 0;
    rc = two_slot_chunks(
        n, chunk, [&](int sl) { return wait_slot(ctx, sl); },
        [&](int sl, size_t first, size_t cnt) -> int {
            if (HFV_MUT_HOSTCHUNK == 5 && first) {
                HIP_TRY(hipStreamSynchronize(ctx->hstream[sl ^ 1]));
                HIP_TRY(hipMemsetAsync(ctx->brh_dstats, 0, kBrStatWords * 8, ctx->hstream[sl]));
            }
            return brh_chunk(ctx, sl, frames + first * slot, slot, slot, window, len + first, ingress_ifindex + first, cnt);
        },
        [&](int sl, size_t first, size_t cnt) {
            brh_results(ctx, sl, frames + first * slot, slot, window, cnt, action + first, verdict + first,
                        egress_ifindex + first);
            return 0;
        },
        &reuses);
    hc_add(kHcReuses, reuses);
    if (rc) return rc;
    // frames whose headers did not fit the window: whole slots, in rounds, through a bounce buffer
    size_t nretry = 0;
    for (size_t i = 0; i < n; ++i) nretry += action[i] == HFV_BR_ACTION_RETRY;
    hc_add(kHcRetried, nretry);
    if (nretry) {
        rc = host_stage(ctx, kBrChunk * slot, kBrChunk * 12);
        if (rc) return rc;
        uint8_t *bounce = nullptr;
        size_t cap = nretry < chunk ? nretry : chunk;
        // cap slots (slot is a multiple of 8), then ifindex u32[cap], then len u16[cap]: each part aligned
        HIP_TRY(hipHostMalloc((void **)&bounce, cap * slot + cap * 4 + cap * 2, hipHostMallocDefault));
        uint32_t *bif = (uint32_t *)(bounce + cap * slot);
        uint16_t *blen = (uint16_t *)(bounce + cap * slot + cap * 4);
        std::vector<size_t> idx(cap);   // where each frame of a round came from
        const uint8_t *hwin = ctx->stage_in[0].host, *hio = ctx->stage_out[0].host;
        size_t i = 0;
        while (rc == 0 && i < n) {
            size_t cnt = 0;
            for (; i < n && cnt < cap; ++i) {
                if (action[i] != HFV_BR_ACTION_RETRY) continue;
                memcpy(bounce + cnt * slot, frames + i * slot, slot);
                blen[cnt] = len[i];
                bif[cnt] = ingress_ifindex[i];
                idx[cnt++] = i;
            }
            if (!cnt) break;
            hc_add(kHcRounds, 1);
            if (HFV_MUT_HOSTCHUNK == 5 && hipMemsetAsync(ctx->brh_dstats, 0, kBrStatWords * 8, ctx->hstream[0]) != hipSuccess)
                rc = fail(-EIO, "retry chunk");
            if (rc == 0) rc = brh_chunk(ctx, 0, bounce, slot, slot, slot, blen, bif, cnt);
            if (rc == 0 && hipStreamSynchronize(ctx->hstream[0]) != hipSuccess) rc = fail(-EIO, "retry chunk");
            for (size_t k = 0; rc == 0 && k < cnt; ++k) {
                size_t j = idx[HFV_MUT_HOSTCHUNK == 6 ? cnt - 1 - k : k];
                memcpy(frames + j * slot, hwin + k * slot, slot);
                action[j] = hio[kBrChunk * 6 + k];
                verdict[j] = hio[kBrChunk * 7 + k];
                memcpy(&egress_ifindex[j], hio + kBrChunk * 8 + 4 * k, 4);
            }
        }
        (void)hipHostFree(bounce);
        if (rc) return rc;
    }
    return brh_add_stats(ctx, stats);
}

int hfv_host_register(hfv_ctx *ctx, void *ptr, size_t bytes)
{
    if (!ctx || !ptr || !bytes) return fail(-EINVAL, "bad argument");
    if (ctx->nhreg == 16) return fail(-ENOMEM, "at most 16 registered host buffers per ctx");
    DeviceGuard g(ctx->device);
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterMapped));
    void *dev = nullptr;
    hipError_t e = hipHostGetDevicePointer(&dev, ptr, 0);
    if (e != hipSuccess) {
        (void)hipHostUnregister(ptr);
        return hip_fail(e, "hipHostGetDevicePointer");
    }
    ctx->hreg[ctx->nhreg++] = {(uint8_t *)ptr, bytes, (uint8_t *)dev};
    return 0;
}

int hfv_host_unregister(hfv_ctx *ctx, void *ptr)
{
    if (!ctx || !ptr) return fail(-EINVAL, "bad argument");
    DeviceGuard g(ctx->device);
    for (int i = 0; i < ctx->nhreg; ++i) {
        if (ctx->hreg[i].host != ptr) continue;
        HIP_TRY(hipDeviceSynchronize());   // no launch may still address it
        HIP_TRY(hipHostUnregister(ptr));
        ctx->hreg[i] = ctx->hreg[--ctx->nhreg];
        return 0;
    }
    return fail(-EINVAL, "buffer was not registered with this ctx");
}

// Zero-copy host batch: the records lie in a registered (mapped) host buffer, so one verify
// launch reads each record's INF/HF words across PCIe itself (20 of the 64 bytes; no bulk
// H2D copy).  The bitmap is written in place when it is registered too, else to a device
// buffer and copied back.
static int verify_records_zero_copy(hfv_ctx *ctx, const uint8_t *drecs, size_t stride, size_t n, uint64_t *pass_bits)
{
    hipStream_t st = ctx->stream;
    ZcArrays z{ctx, st, (n + 63) / 64 * 8};
    uint64_t *dbits = z.out(pass_bits, z.need, 0);
    if (z.rc) return z.rc;
    const bool reader = launch_reads_tables(ctx->keysel);
    int rc = with_tables(ctx, st, "verify_records launch (zero-copy)", reader, [&](DevState *ds) {
        return launch_verify_records(batch_geom(ctx), &ds->keys, &ctx->host_img->keys, ctx->keysel, drecs, stride, n,
                                     ctx->inf_off, ctx->hf_off, dbits, st, nullptr, nullptr, /*interleaved=*/true);
    });
    if (!rc) rc = z.copy_back();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// Bitmap words a chunk of cnt records copies back.
static size_t rec_words(size_t cnt) { return HFV_MUT_HOSTCHUNK == 2 ? cnt / 64 : (cnt + 63) / 64; }

// Host batch: chunks of records go host -> pinned -> device, verified, bitmap back; two
// streams alternate so chunk k's copy-in overlaps chunk k-1's kernel and copy-out.  Records
// in a registered buffer (hfv_host_register) take the zero-copy path instead.
int hfv_verify_records_host(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, uint64_t *pass_bits)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    int rc = check_records(ctx, recs, stride, pass_bits);
    if (rc) return rc;
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    hc_reset();
    if (const uint8_t *drecs = host_dev_ptr(ctx, recs, (n - 1) * stride + ctx->hf_off + 12))
        return verify_records_zero_copy(ctx, drecs, stride, n, pass_bits);
    // Staging: each chunk's records are gathered on the host into a compact pinned layout of
    // kHostRec bytes per record (INF at 0, HF at 8: the 20 bytes the verifier reads), so
    // PCIe moves 24 B instead of the record stride; the gather is split over host threads
    // and chunk c's gather overlaps chunk c-1's copy, kernel and copy-back on the other stream.
    rc = host_stage(ctx, kRecChunk * kHostRec, kRecChunk / 8);
    if (rc) return rc;
    const size_t chunk = rec_chunk();   // records per chunk
    hc_add(kHcChunks, (n + chunk - 1) / chunk);
    const bool reader = launch_reads_tables(ctx->keysel);
    uint64_t reuses = 0;
    rc = two_slot_chunks(
        n, chunk, [&](int sl) { return wait_slot(ctx, sl); },
        [&](int sl, size_t first, size_t cnt) -> int {
            hipStream_t st = ctx->hstream[sl];
            const StagePair &in = ctx->stage_in[sl], &out = ctx->stage_out[sl];
            const size_t from = HFV_MUT_HOSTCHUNK == 3 ? first * kHostRec : first * stride;
            gather_hf(in.host, (const uint8_t *)recs + from, stride, ctx->inf_off, ctx->hf_off, cnt);
            HIP_TRY(hipMemcpyAsync(in.dev, in.host, cnt * kHostRec, hipMemcpyHostToDevice, st));
            int rc = with_tables(ctx, st, "verify_records launch", reader, [&](DevState *ds) {
                return launch_verify_records(batch_geom(ctx), &ds->keys, &ctx->host_img->keys, ctx->keysel, in.dev,
                                             kHostRec, cnt, 0, 8, (uint64_t *)out.dev, st);
            });
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync(out.host, out.dev, rec_words(cnt) * 8, hipMemcpyDeviceToHost, st));
            return 0;
        },
        [&](int sl, size_t first, size_t cnt) {
            memcpy(pass_bits + first / 64, ctx->stage_out[sl].host, rec_words(cnt) * 8);
            return 0;
        },
        &reuses);
    hc_add(kHcReuses, reuses);
    return rc;
}

}  // extern "C"

// ---- frames in host memory -> verdict bits (hfv_verify_frames_host) ----------------------------
// HFV_MUT_HOSTWIN: see hfv_frames_fused_kernel.hip (make hostwin; 0 in every product build).
#ifndef HFV_MUT_HOSTWIN
#define HFV_MUT_HOSTWIN 0
#endif

// Frames per chunk: a multiple of 64, so that no bitmap word straddles two chunks.
static const size_t kFhChunk = (size_t)1 << 16;
#ifdef HFV_TEST_HOOKS
// hfv_debug_frames_host_chunk: frames per chunk of hfv_verify_frames_host (a multiple of 64, at most
// the default; 0 restores it), so that a few hundred frames span several chunks and both streams.
static size_t g_fh_chunk = 0;
extern "C" int hfv_debug_frames_host_chunk(size_t frames)
{
    if ((frames & 63) || frames > kFhChunk) return fail(-EINVAL, "chunk must be a multiple of 64, at most %zu", kFhChunk);
    g_fh_chunk = frames;
    return 0;
}
static size_t fh_chunk() { return g_fh_chunk ? g_fh_chunk : kFhChunk; }
#else
static size_t fh_chunk() { return kFhChunk; }
#endif

static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Where a chunk of cnt frames keeps its parts.  In (one H2D copy of `in` bytes): len u16[cnt], the
// ifindex u32[cnt] (only where the caller gave one), then the rows, each part 16-byte aligned.
// Out (one D2H copy of `out` bytes): the verdict words, the retry words, then status u8[cnt] (only
// where wanted).
struct FhLayout {
    size_t ifx, rows, in;
    size_t words, status, out;
};
static FhLayout fh_layout(size_t cnt, size_t pitch, bool with_ifx, bool with_status)
{
    FhLayout l;
    l.ifx = up16(cnt * 2);
    l.rows = l.ifx + (with_ifx ? up16(cnt * 4) : 0);
    l.in = l.rows + cnt * pitch;
    l.words = (cnt + 63) / 64;
    l.status = l.words * 16;
    l.out = l.status + (with_status ? cnt : 0);
    return l;
}

// The staging for rows of `pitch` bytes: a full chunk with every optional part.
static int fh_stage(hfv_ctx *ctx, size_t pitch)
{
    return host_stage(ctx, fh_layout(kFhChunk, pitch, true, false).in, fh_layout(kFhChunk, 0, false, true).out);
}

// One chunk whose parts lie in slot sl's pinned staging as `l` says: the copy up, the launch, the
// copy back.  The launch is the windowed kernel over packed windows (it also writes the chunk's
// retry words: all zero where window == slot), or, for the second run's whole slots, the full-slot
// kernel of hfv_verify_frames_fused.
static int fh_run(hfv_ctx *ctx, int sl, const FhLayout &l, size_t slot, size_t window, bool whole, bool with_ifx,
                  bool with_status, size_t cnt)
{
    hipStream_t st = ctx->hstream[sl];
    const StagePair &in = ctx->stage_in[sl], &out = ctx->stage_out[sl];
    HIP_TRY(hipMemcpyAsync(in.dev, in.host, l.in, hipMemcpyHostToDevice, st));
    int rc = with_tables(ctx, st, "verify_frames_host launch", launch_reads_tables(ctx->keysel), [&](DevState *ds) {
        FusedWinArgs a;
        memset(&a, 0, sizeof a);
        a.f = fused_args(ctx, ds, in.dev + l.rows, slot, (const uint16_t *)in.dev,
                         with_ifx ? (const uint32_t *)(in.dev + l.ifx) : nullptr, cnt,
                         with_status ? out.dev + l.status : nullptr, (uint64_t *)out.dev);
        if (whole) return launch_verify_frames(batch_geom(ctx), ctx->keysel, a.f, &ctx->host_img->keys, st);
        a.window = (uint32_t)window;
        a.retry = (unsigned long long *)(out.dev + l.words * 8);
        return launch_verify_frames_win(batch_geom(ctx), ctx->keysel, a, &ctx->host_img->keys, st);
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out.host, out.dev, l.out, hipMemcpyDeviceToHost, st));
    return 0;
}

// Zero-copy: the frames lie in a registered (mapped) ring, so the full-slot kernel reads them in
// place over PCIe and nothing is packed or run again.  Each of len, ifindex, status and the bitmap
// is used in place where it is registered too, else it goes through zc_meta with one copy.
static int verify_frames_zero_copy(hfv_ctx *ctx, const uint8_t *dframes, size_t slot, const uint16_t *len,
                                   const uint32_t *ifx, size_t n, uint8_t *status, uint64_t *pass_bits)
{
    hipStream_t st = ctx->stream;
    const size_t words = (n + 63) / 64;
    const size_t o_ifx = words * 8, o_len = o_ifx + n * 4, o_status = o_len + n * 2;
    ZcArrays z{ctx, st, o_status + n};
    const uint16_t *dlen = z.in(len, n * 2, o_len);
    const uint32_t *difx = z.in(ifx, n * 4, o_ifx);
    uint64_t *dbits = z.out(pass_bits, words * 8, 0);
    uint8_t *dstatus = z.out(status, n, o_status);
    if (z.rc) return z.rc;
    int rc = with_tables(ctx, st, "verify_frames_host launch (zero-copy)", launch_reads_tables(ctx->keysel), [&](DevState *ds) {
        const FusedArgs a = fused_args(ctx, ds, dframes, slot, dlen, difx, n, dstatus, dbits);
        return launch_verify_frames(batch_geom(ctx), ctx->keysel, a, &ctx->host_img->keys, st);
    });
    if (!rc) rc = z.copy_back();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int hfv_verify_frames_host(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                                      const uint32_t *ingress_ifindex, size_t n, size_t window, uint8_t *status,
                                      uint64_t *pass_bits, size_t *retried)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!frames || !len || !pass_bits) return fail(-EINVAL, "null buffer");
    int rc = check_slot_window(slot, &window);
    if (rc) return rc;
    if ((uintptr_t)pass_bits & 7) return fail(-EINVAL, "bitmap must be 8-byte aligned");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    hc_reset();
    if (retried) *retried = 0;
    if (const uint8_t *dframes = host_dev_ptr(ctx, frames, n * slot))
        return verify_frames_zero_copy(ctx, dframes, slot, len, ingress_ifindex, n, status, pass_bits);
    rc = fh_stage(ctx, window);
    if (rc) return rc;
    const bool with_ifx = ingress_ifindex != nullptr, with_status = status != nullptr;
    const size_t chunk = fh_chunk();
    hc_add(kHcChunks, (n + chunk - 1) / chunk);
    // Chunk c is packed by the host threads while chunk c - 1's copy and kernel run on the other
    // stream; chunk c - 2 (same stream, same buffers) is retired first.
    std::vector<size_t> again;   // the frames to run again, in order
    uint64_t reuses = 0;
    rc = two_slot_chunks(
        n, chunk, [&](int sl) { return wait_slot(ctx, sl); },
        [&](int sl, size_t first, size_t cnt) {
            const FhLayout l = fh_layout(cnt, window, with_ifx, with_status);
            uint8_t *hin = ctx->stage_in[sl].host;
            memcpy(hin, len + first, cnt * 2);
            if (with_ifx) memcpy(hin + l.ifx, ingress_ifindex + first, cnt * 4);
            copy_rows(hin + l.rows, window, frames + first * slot, slot, window, cnt);
            return fh_run(ctx, sl, l, slot, window, /*whole=*/false, with_ifx, with_status, cnt);
        },
        [&](int sl, size_t first, size_t cnt) -> int {
            const FhLayout l = fh_layout(cnt, window, with_ifx, with_status);
            const uint8_t *hout = ctx->stage_out[sl].host;
            const uint64_t *w = (const uint64_t *)hout;
            memcpy(pass_bits + first / 64, w, l.words * 8);
            if (with_status) memcpy(status + first, hout + l.status, cnt);
            for (size_t k = 0; k < l.words; ++k) {
                uint64_t r = w[l.words + k];
                const size_t left = cnt - k * 64;
                if (left < 64 && (r >> left)) return fail(-EIO, "retry word %zu marks frames past the chunk's %zu", k, cnt);
                for (; r; r &= r - 1) again.push_back(first + k * 64 + (size_t)__builtin_ctzll(r));
            }
            return 0;
        },
        &reuses);
    hc_add(kHcReuses, reuses);
    if (rc) return rc;
    hc_add(kHcRetried, again.size());
    if (retried) *retried = again.size();
    if (again.empty()) return 0;
    // The second run: the marked frames' whole slots, gathered into the pinned staging chunk by
    // chunk, through the full-slot kernel; each verdict into the frame's own bit, each status into
    // its own byte.
    rc = fh_stage(ctx, slot);
    if (rc) return rc;
    for (size_t done = 0; done < again.size(); done += chunk) {
        const size_t cnt = again.size() - done < chunk ? again.size() - done : chunk;
        const size_t *idx = again.data() + done;
        const FhLayout l = fh_layout(cnt, slot, with_ifx, with_status);
        uint8_t *hin = ctx->stage_in[0].host;
        uint16_t *blen = (uint16_t *)hin;
        uint32_t *bifx = (uint32_t *)(hin + l.ifx);
        for (size_t k = 0; k < cnt; ++k) {
            blen[k] = len[idx[k]];
            if (with_ifx) bifx[k] = ingress_ifindex[idx[k]];
        }
        host_rows(cnt, [=](size_t a, size_t b) {
            for (size_t k = a; k < b; ++k) memcpy(hin + l.rows + k * slot, frames + idx[k] * slot, slot);
        });
        hc_add(kHcRounds, 1);
        rc = fh_run(ctx, 0, l, slot, slot, /*whole=*/true, with_ifx, with_status, cnt);
        if (!rc) rc = wait_slot(ctx, 0);
        if (rc) return rc;
        const uint8_t *hout = ctx->stage_out[0].host;
        const uint64_t *w = (const uint64_t *)hout;
        for (size_t k = 0; k < cnt; ++k) {
            const size_t j = HFV_MUT_HOSTWIN == 2 ? k : idx[k];
            const uint64_t bit = (uint64_t)1 << (j & 63);
            if ((w[k / 64] >> (k & 63)) & 1)
                pass_bits[j / 64] |= bit;
            else
                pass_bits[j / 64] &= ~bit;
            if (with_status) status[j] = hout[l.status + k];
        }
    }
    return 0;
}
