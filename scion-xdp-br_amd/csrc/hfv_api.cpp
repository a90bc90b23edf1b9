// hfv_api.cpp -- the C ABI of libscionhfv.so (include/scion_hfv.h): the error sink, the per-GPU
// context and its settings, the mac_key_map-equivalent key table, and the entry points of the
// device-resident data path.  The rest of the ABI lives beside it, around the same hfv_ctx
// (hfv_ctx.h): key-table publication in hfv_publish.cpp, the host-memory paths in
// hfv_host_path.cpp, the resident verify service in hfv_service.cpp.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "hfv_ctx.h"
#include "hfv_frame_desc.h"

namespace hfv {

static thread_local char g_err[256];

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

}  // namespace hfv

// Test hooks.  They change what the library does (delays, launch shapes) and exist only in the
// test build, lib/libscionhfv_test.so (make: -DHFV_TEST_HOOKS); the product library has none of
// them (tests/test_abi.py checks the exports).  The GPU tests that need one run in a child process
// on the test build (tests/conftest.py: rerun_on_test_build).
#ifdef HFV_TEST_HOOKS
// hfv_debug_br_grid: blocks per k_br_process launch (0 = one block per CU up to the tile count).
// With 1, a 1000-frame chunk runs as 16 active waves of one block -- the shape the round-2 loop
// failure ran in ("loop parity failure").
static unsigned g_br_grid = 0;
extern "C" int hfv_debug_br_grid(unsigned blocks)
{
    g_br_grid = blocks;
    return 0;
}
// hfv_debug_br_split: split launches that count verdicts into pieces of at most `frames` frames
// (0 = only where 32-bit block counters could overflow), so a test can check that split launches
// add up to the same counters and outputs.
static size_t g_br_split = 0;
extern "C" int hfv_debug_br_split(size_t frames)
{
    g_br_split = frames;
    return 0;
}
// hfv_debug_br_last_variant: the kernel the last k_br_process launch ran, 1 staged or 2 direct (0: no
// launch yet), so a test of one variant can assert that it ran that one (tests/test_gpu_br_deal.py).
static int g_br_variant = 0;
extern "C" int hfv_debug_br_last_variant(void) { return g_br_variant; }
LaunchGeom br_geom(const hfv_ctx *ctx)
{
    LaunchGeom g = ctx->geom;
    g.br_grid_cap = g_br_grid;
    g.br_split_cap = g_br_split;
    g.br_variant_out = &g_br_variant;
    return g;
}
// hfv_debug_batch_grid: blocks per k_verify_batches launch (0 = one block per CU up to the tile
// count), for every call that ends in launch_verify_batches.  With 1 to 3 blocks a list of a few
// thousand tiles gives every wave a hundred tiles and more over many batches -- the dealing the real
// grid reaches only at 2^24 records (tests/test_gpu_tile_deal.py).  The same cap holds for the
// k_verify_frames launch of hfv_verify_frames_fused (tests/test_gpu_frames_fused.py), the
// k_verify_frames_list launches of hfv_verify_frames_batches (tests/test_gpu_frames_list.py) and the
// k_verify_frames_desc launch of hfv_verify_frames_desc (tests/test_gpu_frames_desc.py).
static unsigned g_batch_grid = 0;
extern "C" int hfv_debug_batch_grid(unsigned blocks)
{
    g_batch_grid = blocks;
    return 0;
}
LaunchGeom batch_geom(const hfv_ctx *ctx)
{
    LaunchGeom g = ctx->geom;
    g.batch_grid_cap = g_batch_grid;
    return g;
}
// hfv_debug_aux_grid: blocks per k_macinputs, k_count_verdicts and k_gen_records launch (0 = today's
// grid; otherwise the smaller of that grid and `blocks`), for hfv_verify_macinputs, hfv_cmac_tags,
// hfv_verdict_counters and hfv_gen_records.  With 1 to 3 blocks of 512 threads a round holds 512 to
// 1536 items, so a few thousand items give every wave five rounds and more of its grid-stride loop --
// what the real grid reaches only past a million (tests/test_gpu_aux_edges.py).
static unsigned g_aux_grid = 0;
extern "C" int hfv_debug_aux_grid(unsigned blocks)
{
    g_aux_grid = blocks;
    return 0;
}
LaunchGeom aux_geom(const hfv_ctx *ctx)
{
    LaunchGeom g = ctx->geom;
    g.aux_grid_cap = g_aux_grid;
    return g;
}
#endif

int check_records(const hfv_ctx *ctx, const void *recs, size_t stride, const void *bits)
{
    if (!recs || !bits) return fail(-EINVAL, "null buffer");
    if (((uintptr_t)recs & 7) || (stride & 7) || ((uintptr_t)bits & 7))
        return fail(-EINVAL, "records, stride and bitmap must be 8-byte aligned");
    if (stride < (size_t)ctx->inf_off + 8 || stride < (size_t)ctx->hf_off + 12)
        return fail(-EINVAL, "stride %zu too small for INF@%u/HF@%u", stride, ctx->inf_off, ctx->hf_off);
    return 0;
}

// body(ev0, ev1), which records the ctx's two timing events (created on first use) at the start of its
// first launch and at the end of its last; then waits for ev1 and writes the milliseconds between them.
template <class Body>
static int timed(hfv_ctx *ctx, float *kernel_ms, Body body)
{
    DeviceGuard g(ctx->device);
    for (int i = 0; i < 2; ++i)
        if (!ctx->tev[i]) HIP_TRY(hipEventCreate(&ctx->tev[i]));
    int rc = body(ctx->tev[0], ctx->tev[1]);
    if (rc) return rc;
    HIP_TRY(hipEventSynchronize(ctx->tev[1]));
    HIP_TRY(hipEventElapsedTime(kernel_ms, ctx->tev[0], ctx->tev[1]));
    return 0;
}

extern "C" {

const char *hfv_last_error(void) { return g_err; }
int hfv_abi_version(void) { return HFV_ABI_VERSION; }

int hfv_ctx_create(int device, hfv_ctx **out)
{
    if (!out) return fail(-EINVAL, "out is NULL");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(-ENODEV, "no HIP device available");
    if (device < 0 || device >= count) return fail(-ENODEV, "device %d out of range (%d devices)", device, count);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(-ENODEV, "device %d is %s; libscionhfv is built for gfx950 only", device, prop.gcnArchName);
    DeviceGuard g(device);
    hfv_ctx *c = new (std::nothrow) hfv_ctx();
    if (!c) return fail(-ENOMEM, "ctx allocation");
    c->device = device;
    int rc = 0;
    do {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = -EIO; break; }
        if (hipHostMalloc((void **)&c->host_img, sizeof(DevState), hipHostMallocDefault) != hipSuccess) { rc = -ENOMEM; break; }
        if (hipEventCreateWithFlags(&c->img_free, hipEventDisableTiming) != hipSuccess) { rc = -EIO; break; }
        for (int i = 0; i < 2; ++i) {
            if (hipMalloc((void **)&c->dev_tab[i], sizeof(DevState)) != hipSuccess) { rc = -ENOMEM; break; }
            if (hipMemset(c->dev_tab[i], 0, sizeof(DevState)) != hipSuccess) { rc = -EIO; break; }
            for (int r = 0; r < 8 && !rc; ++r)
                if (hipEventCreateWithFlags(&c->reader_ev[i][r], hipEventDisableTiming) != hipSuccess) rc = -EIO;
        }
        if (rc) break;
        if (hipMalloc((void **)&c->bat_clk, kBatchClkWords * sizeof(uint64_t)) != hipSuccess) { rc = -ENOMEM; break; }
        if (hipMemset(c->bat_clk, 0, kBatchClkWords * sizeof(uint64_t)) != hipSuccess) { rc = -EIO; break; }
        if (query_geometry(device, &c->geom) != 0) {
            hfv_ctx_destroy(c);
            return fail(-EINVAL, "device %d cannot hold a 1024-thread verify block with 156 KiB of LDS", device);
        }
    } while (0);
    if (rc) {
        hfv_ctx_destroy(c);
        return fail(rc, "hfv_ctx_create failed on device %d", device);
    }
    memset(c->shadow, 0, sizeof c->shadow);
    note_numa(device);
    *out = c;
    return 0;
}

int hfv_ctx_destroy(hfv_ctx *ctx)
{
    if (!ctx) return 0;
    DeviceGuard g(ctx->device);
    (void)svc_quiesce(ctx);
    if (ctx->svc_stream) {
        (void)hipStreamSynchronize(ctx->svc_stream);
        (void)hipStreamDestroy(ctx->svc_stream);
    }
    if (ctx->svc_host) (void)hipHostFree(ctx->svc_host);
    if (ctx->svc_dev) (void)hipFree(ctx->svc_dev);
    for (int i = 0; i < 2; ++i)
        if (ctx->svc_ev[i]) (void)hipEventDestroy(ctx->svc_ev[i]);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 2; ++i) {
        if (ctx->hstream[i]) { (void)hipStreamSynchronize(ctx->hstream[i]); (void)hipStreamDestroy(ctx->hstream[i]); }
        ctx->stage_in[i].release();
        ctx->stage_out[i].release();
        for (int r = 0; r < 8; ++r)
            if (ctx->reader_ev[i][r]) (void)hipEventDestroy(ctx->reader_ev[i][r]);
        if (ctx->dev_tab[i]) (void)hipFree(ctx->dev_tab[i]);
    }
    if (ctx->brh_dstats) (void)hipFree(ctx->brh_dstats);
    if (ctx->zc_meta) (void)hipFree(ctx->zc_meta);
    if (ctx->bat_clk) (void)hipFree(ctx->bat_clk);
    keymap_close(ctx->keymap);
    brcfg_close(ctx->brmap);
    for (int i = 0; i < 2; ++i)
        if (ctx->tev[i]) (void)hipEventDestroy(ctx->tev[i]);
    if (ctx->img_free) { (void)hipEventSynchronize(ctx->img_free); (void)hipEventDestroy(ctx->img_free); }
    if (ctx->host_img) (void)hipHostFree(ctx->host_img);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return 0;
}

int hfv_ctx_device(const hfv_ctx *ctx) { return ctx ? ctx->device : -1; }
int hfv_ctx_numa_node(const hfv_ctx *ctx) { return ctx ? device_numa(ctx->device, nullptr) : -1; }
void *hfv_ctx_stream(hfv_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

int hfv_ctx_set_keysel(hfv_ctx *ctx, int keysel)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (keysel != HFV_KEYSEL_ZERO && keysel != HFV_KEYSEL_IFID) return fail(-EINVAL, "unknown keysel %d", keysel);
    ctx->keysel = keysel;
    return 0;
}

int hfv_ctx_set_record_layout(hfv_ctx *ctx, uint32_t inf_off, uint32_t hf_off)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if ((inf_off & 7) || (hf_off & 7)) return fail(-EINVAL, "INF/HF offsets must be multiples of 8");
    ctx->inf_off = inf_off;
    ctx->hf_off = hf_off;
    return 0;
}

int hfv_ctx_synchronize(hfv_ctx *ctx)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    DeviceGuard g(ctx->device);
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- key table ------------------------------------------------------------------------

int hfv_key_set_hop_key(hfv_ctx *ctx, uint32_t index, const struct hop_key *hk)
{
    if (!ctx || !hk) return fail(-EINVAL, "null argument");
    if (index >= HFV_MAX_KEYS) return fail(-EINVAL, "key index %u >= %d", index, HFV_MAX_KEYS);
    if (ctx->keymap) {
        int rc = hfv_keymap_update(ctx->keymap_path, index, hk);
        if (rc) return rc;
    }
    ctx->shadow[index] = *hk;
    ctx->valid[index >> 5] |= 1u << (index & 31);
    ctx->dirty = true;
    return 0;
}

int hfv_key_add(hfv_ctx *ctx, uint32_t index, const struct aes_key *key)
{
    if (!ctx || !key) return fail(-EINVAL, "null argument");
    hop_key hk;
    hop_key_from_key(key->b, &hk);   // aes_key_expansion + aes_cmac_subkeys, K1 kept
    return hfv_key_set_hop_key(ctx, index, &hk);
}

int hfv_key_add_b64(hfv_ctx *ctx, uint32_t index, const char *base64)
{
    struct aes_key k;
    int rc = hfv_decode_key_b64(base64, &k);
    if (rc) return rc;
    return hfv_key_add(ctx, index, &k);
}

int hfv_key_remove(hfv_ctx *ctx, uint32_t index)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (index >= HFV_MAX_KEYS) return fail(-EINVAL, "key index %u >= %d", index, HFV_MAX_KEYS);
    if (!((ctx->valid[index >> 5] >> (index & 31)) & 1u)) return fail(-ENOENT, "key slot %u is empty", index);
    if (ctx->keymap) {
        int rc = hfv_keymap_erase(ctx->keymap_path, index);
        if (rc) return rc;
    }
    ctx->valid[index >> 5] &= ~(1u << (index & 31));
    memset(&ctx->shadow[index], 0, sizeof(hop_key));
    ctx->dirty = true;
    return 0;
}

int hfv_ctx_attach_keymap(hfv_ctx *ctx, const char *path)
{
    if (!ctx || !path) return fail(-EINVAL, "null argument");
    if (strlen(path) >= sizeof ctx->keymap_path) return fail(-ENAMETOOLONG, "path too long");
    const void *m = nullptr;
    int rc = keymap_open_ro(path, &m);
    if (rc == -ENOENT) {   // create an empty pinned map, as attachBr creates mac_key_map
        rc = keymap_create(path, HFV_KEYMAP_SLOTS);   // header only: never touches a slot another process may write
        if (!rc) rc = keymap_open_ro(path, &m);
    }
    if (rc) return fail(rc, "cannot attach key map %s", path);
    keymap_close(ctx->keymap);
    ctx->keymap = m;
    strcpy(ctx->keymap_path, path);
    ctx->keymap_seq = keymap_snapshot(m, ctx->shadow, ctx->valid);
    ctx->dirty = true;
    return 0;
}

int hfv_key_get(hfv_ctx *ctx, uint32_t index, struct hop_key *out)
{
    if (!ctx || !out) return fail(-EINVAL, "null argument");
    if (index >= HFV_MAX_KEYS) return fail(-EINVAL, "key index %u >= %d", index, HFV_MAX_KEYS);
    if (!((ctx->valid[index >> 5] >> (index & 31)) & 1u)) return fail(-ENOENT, "key slot %u is empty", index);
    *out = ctx->shadow[index];
    return 0;
}

int hfv_key_add_batch(hfv_ctx *ctx, uint32_t first, const struct aes_key *keys, size_t n)
{
    if (!ctx || (!keys && n)) return fail(-EINVAL, "null argument");
    if ((size_t)first + n > HFV_MAX_KEYS) return fail(-EINVAL, "slots %u..%zu exceed %d", first, first + n, HFV_MAX_KEYS);
    if (n == 0) return 0;
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    uint8_t *d_raw = nullptr;
    hop_key *d_hk = nullptr;
    HIP_TRY(hipMalloc((void **)&d_raw, 16 * n));
    if (hipMalloc((void **)&d_hk, sizeof(hop_key) * n) != hipSuccess) {
        (void)hipFree(d_raw);
        return fail(-ENOMEM, "hipMalloc");
    }
    int rc = 0;
    if (hipMemcpyAsync(d_raw, keys, 16 * n, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = -EIO;
    if (!rc && launch_expand_keys(d_raw, n, d_hk, ctx->stream) != 0) rc = -EIO;
    hop_key *tmp = (hop_key *)malloc(sizeof(hop_key) * n);
    if (!tmp) rc = -ENOMEM;
    if (!rc && hipMemcpyAsync(tmp, d_hk, sizeof(hop_key) * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = -EIO;
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = -EIO;
    if (rc) rc = fail(rc, "device key expansion failed");
    for (size_t i = 0; !rc && i < n; ++i) rc = hfv_key_set_hop_key(ctx, first + (uint32_t)i, &tmp[i]);   // first error wins
    free(tmp);
    (void)hipFree(d_raw);
    (void)hipFree(d_hk);
    return rc;
}

// ---- data path ------------------------------------------------------------------------

// The data-path calls below that come in a plain and a *_timed form share one function taking
// two nullable events, which bracket its launches.  ctx is not NULL and n != 0.
static int verify_records(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, uint64_t *pass_bits, void *stream,
                          hipEvent_t ev0, hipEvent_t ev1)
{
    int rc = check_records(ctx, recs, stride, pass_bits);
    if (rc) return rc;
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    const bool reader = launch_reads_tables(ctx->keysel);
    return with_tables(ctx, (hipStream_t)stream, "verify_records launch", reader, [&](DevState *ds) {
        return launch_verify_records(batch_geom(ctx), &ds->keys, &ctx->host_img->keys, ctx->keysel, (const uint8_t *)recs,
                                     stride, n, ctx->inf_off, ctx->hf_off, pass_bits, stream, ev0, ev1);
    });
}

int hfv_verify_records(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, uint64_t *pass_bits, void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    return verify_records(ctx, recs, stride, n, pass_bits, stream, nullptr, nullptr);
}

int hfv_verify_records_timed(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, uint64_t *pass_bits,
                             void *stream, float *kernel_ms)
{
    if (!ctx || !kernel_ms) return fail(-EINVAL, "null argument");
    *kernel_ms = 0.0f;
    if (n == 0) return 0;
    return timed(ctx, kernel_ms, [&](hipEvent_t ev0, hipEvent_t ev1) {
        return verify_records(ctx, recs, stride, n, pass_bits, stream, ev0, ev1);
    });
}

// The batch list of hfv_verify_batches: checked as hfv_verify_records checks one batch; empty
// batches are dropped.
static int batches_check(const hfv_ctx *ctx, const struct hfv_batch *b, size_t count)
{
    if (!b && count) return fail(-EINVAL, "null batch list");
    for (size_t i = 0; i < count; ++i) {
        if (b[i].n == 0) continue;
        int rc = check_records(ctx, b[i].recs, b[i].stride, b[i].pass_bits);
        if (rc) return fail_batch(rc, i);
        if (b[i].stride > (1u << 24)) return fail(-EINVAL, "batch %zu: stride %zu > 16 MiB", i, b[i].stride);
        if (b[i].n > ((size_t)1 << 36)) return fail(-EINVAL, "batch %zu: %zu records (at most 2^36)", i, b[i].n);
    }
    return 0;
}

// One launch per kBatchMax non-empty batches (and at most 2^31 tiles); ev0/ev1 (nullable) bracket
// the first and the last launch.
static int batches_launch(hfv_ctx *ctx, const struct hfv_batch *b, size_t count, hipStream_t st, hipEvent_t ev0,
                          hipEvent_t ev1)
{
    size_t last = count;   // the last non-empty batch: its launch records ev1
    while (last > 0 && b[last - 1].n == 0) --last;
    // the block finish stamps are atomic maxima: cleared before timed launches (outside the events)
    if (ev0) HIP_TRY(hipMemsetAsync(ctx->bat_clk + 4 + kBatchStampBlocks, 0, kBatchStampBlocks * sizeof(uint64_t), st));
    const bool reader = launch_reads_tables(ctx->keysel);
    return with_tables(ctx, st, "verify_batches launch", reader, [&](DevState *ds) {
        if (last == 0) return (int)hipSuccess;   // nothing to launch: the tables are published all the same
        BatchArgs a;
        memset(&a, 0, sizeof a);
        a.tab = &ds->keys;
        a.inf_off = ctx->inf_off;
        a.hf_off = ctx->hf_off;
        a.clk = ctx->bat_clk;
        a.pro = key_prologue(&ctx->host_img->keys);
        for (size_t i = 0;;) {
            a.nb = 0;
            uint64_t tiles = 0;
            for (; i < last && a.nb < kBatchMax; ++i) {
                if (b[i].n == 0) continue;
                const uint64_t t = (b[i].n + 63) / 64;
                if (a.nb && tiles + t > (1ull << 31)) break;
                a.d[a.nb] = {(uint64_t)(uintptr_t)b[i].recs, (uint64_t)(uintptr_t)b[i].pass_bits, (uint64_t)b[i].n,
                             (uint64_t)b[i].stride};
                a.cum[a.nb] = (uint32_t)tiles;
                tiles += t;
                ++a.nb;
            }
            a.cum[a.nb] = (uint32_t)tiles;
            a.total = (uint32_t)tiles;
            const bool fin = i >= last;
            int e = launch_verify_batches(batch_geom(ctx), ctx->keysel, a, st, ev0, fin ? ev1 : nullptr);
            if (e != hipSuccess || fin) return e;   // with_tables notes the last launch
            if (reader) note_reader(ctx, st);
            ev0 = nullptr;
        }
    });
}

int hfv_verify_batches(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    int rc = batches_check(ctx, batches, count);
    if (rc) return rc;
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    return batches_launch(ctx, batches, count, (hipStream_t)stream, nullptr, nullptr);
}

int hfv_verify_batches_timed(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, void *stream,
                             float *kernel_ms)
{
    if (!ctx || !kernel_ms) return fail(-EINVAL, "null argument");
    *kernel_ms = 0.0f;
    int rc = batches_check(ctx, batches, count);
    if (rc) return rc;
    size_t nonempty = 0;
    for (size_t i = 0; i < count; ++i) nonempty += batches[i].n != 0;
    if (!nonempty) return 0;
    return timed(ctx, kernel_ms, [&](hipEvent_t ev0, hipEvent_t ev1) {
        SVC_QUIESCE(ctx);
        return batches_launch(ctx, batches, count, (hipStream_t)stream, ev0, ev1);
    });
}

// ---- frames -> records -> verdict bits ---------------------------------------------------

// What every frame call checks of the frames themselves.
static int frame_args_check(const uint8_t *frames, size_t slot, const uint16_t *len, size_t n)
{
    if (!frames || !len) return fail(-EINVAL, "null buffer");
    if ((slot & 7) || slot < 64) return fail(-EINVAL, "slot %zu: must be a multiple of 8, at least 64", slot);
    if (slot > (1u << 24)) return fail(-EINVAL, "slot %zu > 16 MiB", slot);
    if (n > ((size_t)1 << 36)) return fail(-EINVAL, "%zu frames (at most 2^36)", n);
    return 0;
}

static int frames_check(const hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len, size_t n,
                        const void *recs, size_t stride, const uint8_t *status)
{
    if (!status) return fail(-EINVAL, "null buffer");
    int rc = frame_args_check(frames, slot, len, n);
    if (rc) return rc;
    rc = check_records(ctx, recs, stride, recs);   // no bitmap here: hfv_verify_frames_rx checks its own
    if (rc) return rc;
    if (stride > (1u << 24)) return fail(-EINVAL, "stride %zu > 16 MiB", stride);
    return 0;
}

// The set hfv_extract_records_rx / hfv_verify_frames_rx test ingress_ifindex[i] against: host state,
// copied into the kernel arguments of every launch, so a change holds for calls enqueued after it.
int hfv_ctx_set_internal_ifindices(hfv_ctx *ctx, const uint32_t *ifindex, size_t n)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n > kRxSetMax) return fail(-EINVAL, "%zu internal ifindices (at most %u)", n, kRxSetMax);
    if (!ifindex && n) return fail(-EINVAL, "null ifindex list");
    ctx->rx_set.n = (uint32_t)n;
    for (size_t i = 0; i < kRxSetMax; ++i) ctx->rx_set.v[i] = i < n ? ifindex[i] : 0u;
    return 0;
}

// The extract kernel needs LDS on every CU it runs on, which a running service grid holds until
// it stops: like every other data-path call, these stop the service after its posted batches.
// The direction-blind calls are the direction-aware ones without an ifindex array.
static int extract_records_rx(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                              const uint32_t *ingress_ifindex, size_t n, void *recs, size_t stride, uint8_t *status,
                              void *stream, hipEvent_t ev0, hipEvent_t ev1)
{
    int rc = frames_check(ctx, frames, slot, len, n, recs, stride, status);
    if (rc) return rc;
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    int e = launch_extract_records_rx(frames, slot, len, ingress_ifindex, ctx->rx_set, n, (uint8_t *)recs, stride,
                                      ctx->inf_off, ctx->hf_off, status, stream, ev0, ev1);
    return e == hipSuccess ? 0 : hip_fail((hipError_t)e, "extract_records launch");
}

int hfv_extract_records_rx(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                           const uint32_t *ingress_ifindex, size_t n, void *recs, size_t stride, uint8_t *status,
                           void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    return extract_records_rx(ctx, frames, slot, len, ingress_ifindex, n, recs, stride, status, stream, nullptr, nullptr);
}

int hfv_extract_records_rx_timed(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                                 const uint32_t *ingress_ifindex, size_t n, void *recs, size_t stride,
                                 uint8_t *status, void *stream, float *kernel_ms)
{
    if (!ctx || !kernel_ms) return fail(-EINVAL, "null argument");
    *kernel_ms = 0.0f;
    if (n == 0) return 0;
    return timed(ctx, kernel_ms, [&](hipEvent_t ev0, hipEvent_t ev1) {
        return extract_records_rx(ctx, frames, slot, len, ingress_ifindex, n, recs, stride, status, stream, ev0, ev1);
    });
}

int hfv_verify_frames_rx(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                         const uint32_t *ingress_ifindex, size_t n, void *recs, size_t stride, uint8_t *status,
                         uint64_t *pass_bits, void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    int rc = frames_check(ctx, frames, slot, len, n, recs, stride, status);
    if (rc) return rc;
    const struct hfv_batch b = {recs, stride, n, pass_bits};
    rc = batches_check(ctx, &b, 1);   // the bitmap's pointer and alignment
    if (rc) return rc;
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    hipStream_t st = (hipStream_t)stream;
    int e = launch_extract_records_rx(frames, slot, len, ingress_ifindex, ctx->rx_set, n, (uint8_t *)recs, stride,
                                      ctx->inf_off, ctx->hf_off, status, st);
    if (e != hipSuccess) return hip_fail((hipError_t)e, "extract_records launch");
    rc = batches_launch(ctx, &b, 1, st, nullptr, nullptr);
    if (rc) return rc;
    e = launch_mask_status(status, n, pass_bits, st);
    return e == hipSuccess ? 0 : hip_fail((hipError_t)e, "status mask launch");
}

int hfv_extract_records(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len, size_t n, void *recs,
                        size_t stride, uint8_t *status, void *stream)
{
    return hfv_extract_records_rx(ctx, frames, slot, len, nullptr, n, recs, stride, status, stream);
}

int hfv_extract_records_timed(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len, size_t n,
                              void *recs, size_t stride, uint8_t *status, void *stream, float *kernel_ms)
{
    return hfv_extract_records_rx_timed(ctx, frames, slot, len, nullptr, n, recs, stride, status, stream, kernel_ms);
}

int hfv_verify_frames(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len, size_t n, void *recs,
                      size_t stride, uint8_t *status, uint64_t *pass_bits, void *stream)
{
    return hfv_verify_frames_rx(ctx, frames, slot, len, nullptr, n, recs, stride, status, pass_bits, stream);
}

// Frames in, verdict bits out, in one launch (k_verify_frames): no records, no scratch, the ctx's
// record layout plays no part.  frame_args_check bounds n at 2^36 frames = 2^30 tiles, below the
// 2^31 tiles one launch may take, so the call is always one launch.  Under KEYSEL_ZERO the kernel
// takes slot 0 from its arguments and reads no device table (launch_reads_tables).  ctx is not
// NULL and n != 0.
static int verify_frames_fused(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                               const uint32_t *ingress_ifindex, size_t n, uint8_t *status, uint64_t *pass_bits,
                               void *stream, hipEvent_t ev0, hipEvent_t ev1)
{
    int rc = frame_args_check(frames, slot, len, n);
    if (rc) return rc;
    if (!pass_bits) return fail(-EINVAL, "null buffer");
    if ((uintptr_t)pass_bits & 7) return fail(-EINVAL, "bitmap must be 8-byte aligned");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    const bool reader = launch_reads_tables(ctx->keysel);
    return with_tables(ctx, (hipStream_t)stream, "verify_frames_fused launch", reader, [&](DevState *ds) {
        const FusedArgs a = fused_args(ctx, ds, frames, slot, len, ingress_ifindex, n, status, pass_bits);
        return launch_verify_frames(batch_geom(ctx), ctx->keysel, a, &ctx->host_img->keys, stream, ev0, ev1);
    });
}

int hfv_verify_frames_fused(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                            const uint32_t *ingress_ifindex, size_t n, uint8_t *status, uint64_t *pass_bits,
                            void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    return verify_frames_fused(ctx, frames, slot, len, ingress_ifindex, n, status, pass_bits, stream, nullptr, nullptr);
}

int hfv_verify_frames_fused_timed(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                                  const uint32_t *ingress_ifindex, size_t n, uint8_t *status, uint64_t *pass_bits,
                                  void *stream, float *kernel_ms)
{
    if (!ctx || !kernel_ms) return fail(-EINVAL, "null argument");
    *kernel_ms = 0.0f;
    if (n == 0) return 0;
    return timed(ctx, kernel_ms, [&](hipEvent_t ev0, hipEvent_t ev1) {
        return verify_frames_fused(ctx, frames, slot, len, ingress_ifindex, n, status, pass_bits, stream, ev0, ev1);
    });
}

int hfv_frame_desc_ok(uint64_t addr, uint32_t len, size_t umem_bytes)
{
    return frame_desc_ok(addr, len, (uint64_t)umem_bytes) ? 1 : 0;
}

// Frames given by descriptors into one buffer, verified in place in one launch
// (k_verify_frames_desc): the preamble of verify_frames_fused.  What the descriptors hold is on the
// device and judged there, per frame.  ctx is not NULL and n != 0.
static int verify_frames_desc(hfv_ctx *ctx, const uint8_t *umem, size_t umem_bytes, const struct hfv_frame_desc *desc,
                              size_t n, uint8_t *status, uint64_t *pass_bits, void *stream, hipEvent_t ev0,
                              hipEvent_t ev1)
{
    if (!desc) return fail(-EINVAL, "null descriptor array");
    if ((uintptr_t)desc & 7) return fail(-EINVAL, "descriptors must be 8-byte aligned");
    if (!pass_bits) return fail(-EINVAL, "null buffer");
    if ((uintptr_t)pass_bits & 7) return fail(-EINVAL, "bitmap must be 8-byte aligned");
    if (!umem && umem_bytes) return fail(-EINVAL, "null buffer of %zu bytes", umem_bytes);
    if (n > ((size_t)1 << 36)) return fail(-EINVAL, "%zu frames (at most 2^36)", n);
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    const bool reader = launch_reads_tables(ctx->keysel);
    return with_tables(ctx, (hipStream_t)stream, "verify_frames_desc launch", reader, [&](DevState *ds) {
        DescArgs a;
        memset(&a, 0, sizeof a);
        a.umem = umem;
        a.umem_bytes = umem_bytes;
        a.desc = desc;
        a.n = n;
        a.status = status;
        a.bits = (unsigned long long *)pass_bits;
        a.tab = &ds->keys;
        a.set = ctx->rx_set;
        return launch_verify_frames_desc(batch_geom(ctx), ctx->keysel, a, &ctx->host_img->keys, stream, ev0, ev1);
    });
}

int hfv_verify_frames_desc(hfv_ctx *ctx, const uint8_t *umem, size_t umem_bytes, const struct hfv_frame_desc *desc,
                           size_t n, uint8_t *status, uint64_t *pass_bits, void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    return verify_frames_desc(ctx, umem, umem_bytes, desc, n, status, pass_bits, stream, nullptr, nullptr);
}

int hfv_verify_frames_desc_timed(hfv_ctx *ctx, const uint8_t *umem, size_t umem_bytes,
                                 const struct hfv_frame_desc *desc, size_t n, uint8_t *status, uint64_t *pass_bits,
                                 void *stream, float *kernel_ms)
{
    if (!ctx || !kernel_ms) return fail(-EINVAL, "null argument");
    *kernel_ms = 0.0f;
    if (n == 0) return 0;
    return timed(ctx, kernel_ms, [&](hipEvent_t ev0, hipEvent_t ev1) {
        return verify_frames_desc(ctx, umem, umem_bytes, desc, n, status, pass_bits, stream, ev0, ev1);
    });
}

// The batch list of hfv_verify_frames_batches: every non-empty batch checked as
// hfv_verify_frames_fused checks one, before anything is launched.
static int frames_batches_check(const struct hfv_frame_batch *b, size_t count)
{
    if (!b && count) return fail(-EINVAL, "null batch list");
    for (size_t i = 0; i < count; ++i) {
        if (b[i].n == 0) continue;
        int rc = frame_args_check(b[i].frames, b[i].slot, b[i].len, b[i].n);
        if (rc) return fail_batch(rc, i);
        if (!b[i].pass_bits) return fail(-EINVAL, "batch %zu: null buffer", i);
        if ((uintptr_t)b[i].pass_bits & 7) return fail(-EINVAL, "batch %zu: bitmap must be 8-byte aligned", i);
    }
    return 0;
}

// One k_verify_frames_list launch per run of consecutive non-empty batches that are all staged or
// all direct (the rule of launch_verify_frames), of at most kFrameBatchMax batches and 2^31 tiles,
// in list order; ev0/ev1 (nullable) bracket the first and the last launch.
static int frames_batches_launch(hfv_ctx *ctx, const struct hfv_frame_batch *b, size_t count, hipStream_t st,
                                 hipEvent_t ev0, hipEvent_t ev1)
{
    size_t last = count;   // the last non-empty batch: its launch records ev1
    while (last > 0 && b[last - 1].n == 0) --last;
    const bool reader = launch_reads_tables(ctx->keysel);
    return with_tables(ctx, st, "verify_frames_batches launch", reader, [&](DevState *ds) {
        if (last == 0) return (int)hipSuccess;   // nothing to launch: the tables are published all the same
        FusedListArgs a;
        memset(&a, 0, sizeof a);
        a.tab = &ds->keys;
        a.set = ctx->rx_set;
        const KeyPrologue pro = key_prologue(&ctx->host_img->keys);
        memcpy(a.key0, pro.key0, sizeof a.key0);
        a.key0_ok = pro.key0_ok;
        auto stageable = [](const struct hfv_frame_batch &x) { return frames_stageable(x.frames, x.slot); };
        for (size_t i = 0;;) {
            a.nb = 0;
            uint64_t tiles = 0;
            bool staged = false;
            for (; i < last && a.nb < kFrameBatchMax; ++i) {
                if (b[i].n == 0) continue;
                const uint64_t t = (b[i].n + 63) / 64;
                if (a.nb && (tiles + t > (1ull << 31) || stageable(b[i]) != staged)) break;
                staged = stageable(b[i]);
                // no set: every frame is external, and no ifindex is loaded
                const uint32_t *ifx = a.set.n ? b[i].ingress_ifindex : nullptr;
                a.d[a.nb] = {(uint64_t)(uintptr_t)b[i].frames, (uint64_t)(uintptr_t)b[i].len, (uint64_t)(uintptr_t)ifx,
                             (uint64_t)(uintptr_t)b[i].status, (uint64_t)(uintptr_t)b[i].pass_bits, (uint64_t)b[i].n,
                             (uint32_t)b[i].slot, 0u};
                a.cum[a.nb] = (uint32_t)tiles;
                tiles += t;
                ++a.nb;
            }
            a.cum[a.nb] = (uint32_t)tiles;
            a.total = (uint32_t)tiles;
            const bool fin = i >= last;
            int e = launch_verify_frames_list(batch_geom(ctx), ctx->keysel, staged, a, st, ev0, fin ? ev1 : nullptr);
            if (e != hipSuccess || fin) return e;   // with_tables notes the last launch
            if (reader) note_reader(ctx, st);
            ev0 = nullptr;
        }
    });
}

int hfv_verify_frames_batches(hfv_ctx *ctx, const struct hfv_frame_batch *batches, size_t count, void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    int rc = frames_batches_check(batches, count);
    if (rc) return rc;
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    return frames_batches_launch(ctx, batches, count, (hipStream_t)stream, nullptr, nullptr);
}

int hfv_verify_frames_batches_timed(hfv_ctx *ctx, const struct hfv_frame_batch *batches, size_t count, void *stream,
                                    float *kernel_ms)
{
    if (!ctx || !kernel_ms) return fail(-EINVAL, "null argument");
    *kernel_ms = 0.0f;
    int rc = frames_batches_check(batches, count);
    if (rc) return rc;
    size_t nonempty = 0;
    for (size_t i = 0; i < count; ++i) nonempty += batches[i].n != 0;
    if (!nonempty) return 0;
    return timed(ctx, kernel_ms, [&](hipEvent_t ev0, hipEvent_t ev1) {
        SVC_QUIESCE(ctx);
        return frames_batches_launch(ctx, batches, count, (hipStream_t)stream, ev0, ev1);
    });
}

// Diagnostic (not part of include/scion_hfv.h): the last step of hfv_verify_frames alone,
// pass_bits[i / 64] &= (status[i] == 0), so that scripts/frames_probe.py can time the mask kernel.
extern "C" int hfv_debug_mask_status(hfv_ctx *ctx, const uint8_t *status, size_t n, uint64_t *pass_bits, void *stream)
{
    if (!ctx || !status || !pass_bits || n == 0 || ((uintptr_t)pass_bits & 7)) return fail(-EINVAL, "bad argument");
    DeviceGuard g(ctx->device);
    int e = launch_mask_status(status, n, pass_bits, stream);
    return e == hipSuccess ? 0 : hip_fail((hipError_t)e, "status mask launch");
}

// Diagnostic (not part of include/scion_hfv.h): block 0's shader clock (s_memtime) and 100 MHz
// s_memrealtime at the start and at the end of the last hfv_verify_batches launch (out[0..3]);
// with words >= 4 + 2 * 1024 also every block's s_memrealtime at its entry (out[4 + k]) and when it
// finished (out[4 + 1024 + k]).  The caller has synchronized that launch.
extern "C" int hfv_debug_batches_clock(hfv_ctx *ctx, uint64_t *out, size_t words)
{
    if (!ctx || !out || words < 4) return fail(-EINVAL, "bad argument");
    DeviceGuard g(ctx->device);
    if (words > kBatchClkWords) words = kBatchClkWords;
    HIP_TRY(hipMemcpy(out, ctx->bat_clk, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

// Diagnostic (not part of include/scion_hfv.h): one dense non-temporal streaming read of `count`
// (<= 64) device buffers on `stream`, waited for; *kernel_ms = its dispatch time.  bench.py prices
// the verify kernel against this rate over the same resident batches (roofline.achievable_peak).
extern "C" int hfv_debug_stream_read(hfv_ctx *ctx, const void *const *bufs, const size_t *bytes, size_t count,
                                     void *stream, float *kernel_ms)
{
    if (!ctx || !bufs || !bytes || !kernel_ms || count == 0 || count > kBatchMax) return fail(-EINVAL, "bad argument");
    StreamArgs a;
    memset(&a, 0, sizeof a);
    a.nb = (uint32_t)count;
    a.sink = (uint32_t *)ctx->bat_clk;   // never written in practice (see k_stream_read)
    for (size_t i = 0; i < count; ++i) {
        if (((uintptr_t)bufs[i] & 15) || (bytes[i] & 15)) return fail(-EINVAL, "buffer %zu not 16-byte aligned", i);
        a.buf[i] = bufs[i];
        a.bytes[i] = bytes[i];
    }
    return timed(ctx, kernel_ms, [&](hipEvent_t ev0, hipEvent_t ev1) {
        SVC_QUIESCE(ctx);
        int e = launch_stream_read(ctx->geom, a, stream, ev0, ev1);
        return e == hipSuccess ? 0 : hip_fail((hipError_t)e, "stream read launch");
    });
}

// Diagnostic (not part of include/scion_hfv.h): the default KEYSEL_ZERO kernel with per-wave
// s_memrealtime stamps, for the timeline analysis in scripts/stamps.py.  stamps: device
// buffer of (grid * 16 waves) x 16 u64; returns the grid size in *grid.
extern "C" int hfv_debug_verify_stamped(hfv_ctx *ctx, const void *recs, size_t n, uint64_t *pass_bits,
                                        uint64_t *stamps, void *stream, int *grid)
{
    if (!ctx || !recs || !pass_bits || !stamps || !grid || n == 0) return fail(-EINVAL, "bad argument");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    return with_tables(ctx, (hipStream_t)stream, "stamped launch", [&](DevState *ds) {
        uint64_t tiles = (n + 63) / 64, blocks = (tiles + 15) / 16, cap = (uint64_t)ctx->geom.num_cus;
        *grid = (int)(blocks < cap ? blocks : cap);
        return launch_verify_stamped(ctx->geom, &ds->keys, &ctx->host_img->keys, (const uint8_t *)recs, n, pass_bits,
                                     stamps, stream);
    });
}

int hfv_ctx_describe(const hfv_ctx *ctx, char *buf, size_t len)
{
    if (!ctx || !buf || !len) return fail(-EINVAL, "null argument");
    snprintf(buf, len,
             "verify: 1024-thread blocks, one per CU (%d CUs), four 32x-replicated round tables in LDS (128 KiB), "
             "T0 and slot-0 key rows in the kernel arguments; keysel ifid: five 16 B LDS rows per slot "
             "(round-1 folded key, rk2, schedule words of rounds 3..10); service grid %d blocks; "
             "verify_frames_fused: one block per CU, two 8x-replicated round tables (16 KiB) beside 132 B staged "
             "rows per frame, 1024-thread blocks (keysel zero, 151556 B LDS) or 768-thread blocks with the "
             "per-slot key rows (keysel ifid, 138276 B LDS)",
             ctx->geom.num_cus, ctx->geom.svc_blocks);
    return 0;
}

int hfv_verify_macinputs(hfv_ctx *ctx, const struct macinput *mi, const uint64_t *expected, const uint8_t *key_index,
                         size_t n, uint64_t *pass_bits, void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!mi || !expected || !pass_bits) return fail(-EINVAL, "null buffer");
    if (((uintptr_t)mi & 15) || ((uintptr_t)expected & 7) || ((uintptr_t)pass_bits & 7))
        return fail(-EINVAL, "macinputs must be 16-byte aligned, expected/bitmap 8-byte aligned");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    return with_tables(ctx, (hipStream_t)stream, "verify_macinputs launch", [&](DevState *ds) {
        return launch_verify_macinputs(aux_geom(ctx), &ds->keys, mi, expected, key_index, n, pass_bits, stream);
    });
}

int hfv_cmac_tags(hfv_ctx *ctx, const struct macinput *mi, const uint8_t *key_index, size_t n, struct aes_cmac *tags,
                  void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!mi || !tags) return fail(-EINVAL, "null buffer");
    if (((uintptr_t)mi & 15) || ((uintptr_t)tags & 15)) return fail(-EINVAL, "macinputs/tags must be 16-byte aligned");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    return with_tables(ctx, (hipStream_t)stream, "cmac_tags launch", [&](DevState *ds) {
        return launch_cmac_tags(aux_geom(ctx), &ds->keys, mi, key_index, n, tags, stream);
    });
}

int hfv_expand_keys(hfv_ctx *ctx, const struct aes_key *keys, size_t n, struct hop_key *out, void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!keys || !out) return fail(-EINVAL, "null buffer");
    if (((uintptr_t)keys & 15) || ((uintptr_t)out & 15)) return fail(-EINVAL, "buffers must be 16-byte aligned");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    int e = launch_expand_keys((const uint8_t *)keys, n, out, stream);
    if (e != hipSuccess) return hip_fail((hipError_t)e, "expand_keys launch");
    return 0;
}

int hfv_gen_records(hfv_ctx *ctx, void *recs, size_t stride, size_t n, uint64_t seed, uint64_t first_index,
                    void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!recs) return fail(-EINVAL, "null buffer");
    if (((uintptr_t)recs & 15) || (stride & 15) || stride < 64)
        return fail(-EINVAL, "records must be 16-byte aligned with stride >= 64, multiple of 16");
    if (ctx->inf_off != HFV_REC_INF_OFF || ctx->hf_off != HFV_REC_HF_OFF)
        return fail(-EINVAL, "the generator writes the default 64 B layout only");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    return with_tables(ctx, (hipStream_t)stream, "gen_records launch", [&](DevState *ds) {
        return launch_gen_records(aux_geom(ctx), &ds->keys, ctx->keysel, (uint8_t *)recs, stride, n, seed, first_index,
                                  stream);
    });
}

int hfv_verdict_counters(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, const uint64_t *pass_bits,
                         uint64_t *counters, void *stream)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (n == 0) return 0;
    if (!counters) return fail(-EINVAL, "null buffer");
    int rc = check_records(ctx, recs, stride, pass_bits);   // the records hfv_verify_records took
    if (rc) return rc;
    if ((uintptr_t)counters & 7) return fail(-EINVAL, "bitmap and counters must be 8-byte aligned");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    int e = launch_count_verdicts(aux_geom(ctx), (const uint8_t *)recs, stride, n, ctx->inf_off, ctx->hf_off, pass_bits,
                                  counters, stream);
    if (e != hipSuccess) return hip_fail((hipError_t)e, "count_verdicts launch");
    return 0;
}

// ---- full border-router path (config 4) ---------------------------------------------------

int hfv_br_set_config(hfv_ctx *ctx, const struct hfv_br_config *cfg)
{
    if (!ctx || !cfg) return fail(-EINVAL, "null argument");
    if (br_config_check(cfg) == 0 && ctx->br.feat_off && hfv_br_config_check_options(cfg, ctx->br.feat_off))
        return -EINVAL;   // an address of a family the router is built without (br-loader's error)
    if (br_config_check(cfg))
        return fail(-EINVAL, "router table larger than the fixed capacity (%d interfaces, %d routes, %d tx ports)",
                    HFV_BR_MAX_IFACES, HFV_BR_MAX_ROUTES, HFV_BR_MAX_TXPORTS);
    const uint32_t off = ctx->br.hf_check_off, feat = ctx->br.feat_off;
    compile_br_config(cfg, &ctx->br);
    ctx->br.hf_check_off = off;
    ctx->br.feat_off = feat;
    ctx->cfg_src = *cfg;
    ctx->dirty = true;
    brcfg_close(ctx->brmap);   // explicit tables replace an attached pinned config
    ctx->brmap = nullptr;
    return 0;
}

int hfv_br_load_config(hfv_ctx *ctx, const char *toml_path, const struct hfv_br_next_hop *hops, size_t n_hops)
{
    if (!ctx || !toml_path) return fail(-EINVAL, "null argument");
    hfv_br_config cfg;
    int rc = hfv_br_config_load(toml_path, nullptr, 0, hops, n_hops, &cfg, nullptr, 0, nullptr, 0, nullptr, 0);
    if (rc) return rc;
    return hfv_br_set_config(ctx, &cfg);
}

int hfv_ctx_attach_brconfig(hfv_ctx *ctx, const char *path)
{
    if (!ctx || !path) return fail(-EINVAL, "null argument");
    const void *m = nullptr;
    int rc = brcfg_open_ro(path, &m);
    if (rc) return fail(rc, "cannot attach pinned router config %s", path);
    brcfg_close(ctx->brmap);
    ctx->brmap = m;
    ctx->brmap_seq = 0xffffffffu;   // loaded at the next batch boundary
    return 0;
}

int hfv_br_set_build_options(hfv_ctx *ctx, uint32_t disabled)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (hfv_br_config_check_options(&ctx->cfg_src, disabled)) return -EINVAL;
    ctx->br.feat_off = disabled;
    ctx->dirty = true;
    return 0;
}

int hfv_br_set_hf_check(hfv_ctx *ctx, int enable)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    ctx->br.hf_check_off = enable ? 0u : 1u;
    ctx->dirty = true;
    return 0;
}

static int br_args(hfv_ctx *ctx, uint8_t *pkts, size_t slot, const uint16_t *len, const uint32_t *ingress_ifindex,
                   uint8_t *action, uint8_t *verdict, int32_t *egress_ifindex)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    if (!pkts || !len || !ingress_ifindex || !action || !verdict || !egress_ifindex) return fail(-EINVAL, "null buffer");
    if (slot < 64 || (slot & 7) || ((uintptr_t)pkts & 7)) return fail(-EINVAL, "slot must be >= 64 and a multiple of 8, frames 8-byte aligned");
    if (((uintptr_t)len & 1) || ((uintptr_t)ingress_ifindex & 3) || ((uintptr_t)egress_ifindex & 3))
        return fail(-EINVAL, "misaligned length/ifindex array");
    return 0;
}

static int br_process(hfv_ctx *ctx, uint8_t *pkts, size_t slot, const uint16_t *len, const uint32_t *ingress_ifindex,
                      size_t n, uint8_t *action, uint8_t *verdict, int32_t *egress_ifindex, uint64_t *stats,
                      void *stream, hipEvent_t ev0, hipEvent_t ev1)
{
    int rc = br_args(ctx, pkts, slot, len, ingress_ifindex, action, verdict, egress_ifindex);
    if (rc) return rc;
    if ((uintptr_t)stats & 7) return fail(-EINVAL, "misaligned stats");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    return with_tables(ctx, (hipStream_t)stream, "br_process launch", [&](DevState *ds) {
        return launch_br_process(br_geom(ctx), ds, pkts, slot, (uint32_t)slot, (uint32_t)slot, len, ingress_ifindex, n,
                                 action, verdict, egress_ifindex, stats, stream, ev0, ev1);
    });
}

int hfv_br_process(hfv_ctx *ctx, uint8_t *pkts, size_t slot, const uint16_t *len, const uint32_t *ingress_ifindex,
                   size_t n, uint8_t *action, uint8_t *verdict, int32_t *egress_ifindex, uint64_t *stats,
                   void *stream)
{
    if (n == 0 || !ctx) return ctx ? 0 : fail(-EINVAL, "ctx is NULL");
    return br_process(ctx, pkts, slot, len, ingress_ifindex, n, action, verdict, egress_ifindex, stats, stream, nullptr,
                      nullptr);
}

int hfv_br_process_timed(hfv_ctx *ctx, uint8_t *pkts, size_t slot, const uint16_t *len,
                         const uint32_t *ingress_ifindex, size_t n, uint8_t *action, uint8_t *verdict,
                         int32_t *egress_ifindex, uint64_t *stats, void *stream, float *kernel_ms)
{
    if (!kernel_ms) return fail(-EINVAL, "kernel_ms is NULL");
    *kernel_ms = 0.0f;
    if (n == 0 || !ctx) return ctx ? 0 : fail(-EINVAL, "ctx is NULL");
    return timed(ctx, kernel_ms, [&](hipEvent_t ev0, hipEvent_t ev1) {
        return br_process(ctx, pkts, slot, len, ingress_ifindex, n, action, verdict, egress_ifindex, stats, stream, ev0,
                          ev1);
    });
}

// ---- memory helpers -------------------------------------------------------------------

int hfv_dev_alloc(hfv_ctx *ctx, size_t bytes, void **ptr)
{
    if (!ctx || !ptr) return fail(-EINVAL, "null argument");
    DeviceGuard g(ctx->device);
    if (hipMalloc(ptr, bytes ? bytes : 1) != hipSuccess) return fail(-ENOMEM, "hipMalloc(%zu)", bytes);
    return 0;
}

int hfv_dev_free(hfv_ctx *ctx, void *ptr)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    HIP_TRY(hipFree(ptr));
    return 0;
}

int hfv_memcpy_h2d(hfv_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

int hfv_memcpy_d2h(hfv_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx) return fail(-EINVAL, "ctx is NULL");
    DeviceGuard g(ctx->device);
    SVC_QUIESCE(ctx);
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

}  // extern "C"
