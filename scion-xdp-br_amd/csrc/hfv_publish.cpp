// hfv_publish.cpp -- key-table publication (replaces map updates under RCU,
// br_loader.cpp:221-222): key add/remove edit a host shadow; the next data-path call on any
// stream copies the shadow into the inactive one of two device tables (through a pinned staging
// image), then launches with it.  A device table is rewritten only after the work that last
// read it has completed (tracked with one event per reader stream), so in-flight batches keep a
// stable table.  The two stream fences below are this file's alone: `make nofence` and
// `make noreaderfence` rebuild it without one of them.
#include <utility>

#include "hfv_ctx.h"

// HFV_PUB_FENCE=0 builds the round-2 behaviour (no cross-stream wait for a publish copy) for the
// A/B that names the loop failure's cause (`make nofence`); never a product build.
#ifndef HFV_PUB_FENCE
#define HFV_PUB_FENCE 1
#endif
// HFV_READER_FENCE=0 drops the other half: a publish overwrites a device table without waiting for
// the launches that still read it (neither the per-stream events nor the overflow synchronize).
// `make noreaderfence` builds it so that tests/test_gpu_key_publish.py can be shown to fail
// without the fence; never a product build.
#ifndef HFV_READER_FENCE
#define HFV_READER_FENCE 1
#endif

#ifdef HFV_TEST_HOOKS
// Test hook (test build only, see hfv_api.cpp): every publish copy waits behind a spin of this
// many microseconds on its stream, so a test can make the cross-stream race deterministic.
static uint32_t g_pub_delay_us = 0;
extern "C" int hfv_debug_publish_delay(uint32_t us)
{
    g_pub_delay_us = us;
    return 0;
}
#else
static constexpr uint32_t g_pub_delay_us = 0;
#endif

// Make the shadow table visible to work enqueued next on `st` -- and, once the copy is queued,
// to work on any other stream (which waits for the copy until it has been seen complete);
// returns the table to use.  reader = false (launch_reads_tables): the launch that follows reads no
// device table, so `st` does not wait for a pending copy made on another stream; everything else
// -- the pick-up of attached maps, the rebuild of the staging image (the launch's key prologue is
// cut from it), the device copy and the fences of that copy -- is done all the same.
int publish_keys(hfv_ctx *ctx, hipStream_t st, DevState **out, bool reader)
{
    if (ctx->keymap) {   // pick up updates other processes made to the pinned map
        uint32_t seq = keymap_seq(ctx->keymap);
        if (seq != ctx->keymap_seq) {
            ctx->keymap_seq = keymap_snapshot(ctx->keymap, ctx->shadow, ctx->valid);
            ctx->dirty = true;
        }
    }
    if (ctx->brmap) {    // router tables republished by `hfv-loader attach`
        uint32_t seq = brcfg_seq(ctx->brmap);
        if (seq != ctx->brmap_seq) {
            hfv_br_config cfg;
            uint32_t detached = 0, feat_off = 0;
            ctx->brmap_seq = brcfg_snapshot(ctx->brmap, &cfg, &detached, &feat_off);
            if (br_config_check(&cfg) != 0)   // a corrupt or foreign file: keep the tables in use
                return fail(-EINVAL, "attached router config holds counts past the fixed capacity; "
                                     "previous tables kept");
            const uint32_t off = ctx->br.hf_check_off;
            ctx->cfg_src = cfg;   // what hfv_br_set_build_options checks against
            compile_br_config(&cfg, &ctx->br);
            ctx->br.hf_check_off = off;
            ctx->br.detached = detached;
            ctx->br.feat_off = feat_off & (HFV_BR_NO_IPV4 | HFV_BR_NO_IPV6 | HFV_BR_NO_SCION_PATH);
            ctx->dirty = true;
        }
    }
    if (ctx->dirty) {
        int next = ctx->active ^ 1;
        // wait (host) until the previous copy out of the staging image has been consumed
        HIP_TRY(hipEventSynchronize(ctx->img_free));
        for (uint32_t k = 0; k < HFV_MAX_KEYS; ++k) {
            uint32_t dk[4 * kDevKeyRows], t[8];
            if ((ctx->valid[k >> 5] >> (k & 31)) & 1u) {
                compile_dev_key(&ctx->shadow[k], dk);
                compile_dev_sched(&ctx->shadow[k], t);
            } else {
                memset(dk, 0, sizeof dk);
                memset(t, 0, sizeof t);
            }
            for (int r = 0; r < kDevKeyRows; ++r) memcpy(ctx->host_img->keys.rows[r][k], dk + 4 * r, 16);
            memcpy(ctx->host_img->keys.sched[0][k], t, 16);
            memcpy(ctx->host_img->keys.sched[1][k], t + 4, 16);
        }
        memcpy(ctx->host_img->keys.valid, ctx->valid, sizeof ctx->valid);
        ctx->host_img->br = ctx->br;
        // the device table may only be overwritten after every launch that read it completed
        if (!HFV_READER_FENCE) {
            // A/B build only: no write-after-read fence
        } else if (ctx->readers_overflow[next]) {
            HIP_TRY(hipDeviceSynchronize());
        } else {
            // the events were recorded after each reader's last launch with the table, so the
            // fence holds even for a reader stream the caller has destroyed since
            for (int r = 0; r < ctx->nreaders[next]; ++r) {
                hipStream_t rs = ctx->readers[next][r];
                if (rs == st) continue;   // same stream: ordered already
                // the ctx's own streams live as long as the ctx: mark them now; a caller's
                // stream carries the event recorded after its last launch with the table
                if (own_stream(ctx, rs)) HIP_TRY(hipEventRecord(ctx->reader_ev[next][r], rs));
                HIP_TRY(hipStreamWaitEvent(st, ctx->reader_ev[next][r], 0));
            }
        }
        ctx->nreaders[next] = 0;
        ctx->readers_overflow[next] = false;
        if (g_pub_delay_us) HIP_TRY((hipError_t)launch_debug_spin(st, g_pub_delay_us));
        HIP_TRY(hipMemcpyAsync(ctx->dev_tab[next], ctx->host_img, sizeof(DevState), hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(ctx->img_free, st));
        ctx->active = next;
        ctx->dirty = false;
        ctx->pub_pending = true;
    } else if (HFV_PUB_FENCE && ctx->pub_pending && reader) {
        // The copy into dev_tab[active] was enqueued on the stream that published it; work on any
        // other stream must not read the table before that copy lands.  (Round 2 skipped this: the
        // config-5 loop published on its chunk-0 stream and launched chunk 1 on a second stream,
        // whose kernel could read the half-written or previous table -- every MAC of that chunk
        // failed against a stale key, gpurun_out/r02c5: tx short by exactly one chunk.)
        if (hipEventQuery(ctx->img_free) == hipSuccess) ctx->pub_pending = false;
        else HIP_TRY(hipStreamWaitEvent(st, ctx->img_free, 0));
    }
    *out = ctx->dev_tab[ctx->active];
    return 0;
}

bool own_stream(const hfv_ctx *ctx, hipStream_t st)
{
    return st && (st == ctx->stream || st == ctx->svc_stream || st == ctx->hstream[0] || st == ctx->hstream[1]);
}

void note_reader(hfv_ctx *ctx, hipStream_t st)
{
    const int a = ctx->active;
    int r = 0;
    while (r < ctx->nreaders[a] && ctx->readers[a][r] != st) ++r;
    if (r == ctx->nreaders[a]) {
        if (r == 8) {
            ctx->readers_overflow[a] = true;
            return;
        }
        ctx->readers[a][ctx->nreaders[a]++] = st;
    }
    // a caller's stream may be destroyed before the next publish: remember where its launches
    // with this table end (one event record per launch; the ctx's own streams skip it)
    if (!own_stream(ctx, st) && hipEventRecord(ctx->reader_ev[a][r], st) != hipSuccess) ctx->readers_overflow[a] = true;
}

int after_launch(hfv_ctx *ctx, hipStream_t st, int err, const char *what, bool reader)
{
    if (err != hipSuccess) return hip_fail((hipError_t)err, what);
    if (reader) note_reader(ctx, st);
    return 0;
}

void hfv::forget_stream(hfv_ctx *ctx, void *stream)
{
    for (int a = 0; a < 2; ++a)
        for (int r = 0; r < ctx->nreaders[a];)
            if (ctx->readers[a][r] == (hipStream_t)stream) {
                // the last entry moves into slot r together with its fence event
                const int last = --ctx->nreaders[a];
                ctx->readers[a][r] = ctx->readers[a][last];
                std::swap(ctx->reader_ev[a][r], ctx->reader_ev[a][last]);
            } else {
                ++r;
            }
}
