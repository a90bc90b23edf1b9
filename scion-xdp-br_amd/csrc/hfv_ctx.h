// hfv_ctx.h -- the per-GPU context and what the host units of the C ABI share around it: hfv_api.cpp
// (lifecycle, keys, device-resident data path), hfv_publish.cpp (key-table publication), hfv_host_path.cpp
// (host-memory paths), hfv_service.cpp (resident service).  Not installed, and not for the .hip files.
#pragma once
#include <errno.h>
#include <sched.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include <hip/hip_runtime.h>

#include "hfv_internal.h"

namespace hfv {

static inline int hip_fail(hipError_t e, const char *what)
{
    return fail(-EIO, "%s: %s", what, hipGetErrorString(e));
}

#define HIP_TRY(expr)                                          \
    do {                                                       \
        hipError_t e_ = (expr);                                \
        if (e_ != hipSuccess) return hip_fail(e_, #expr);      \
    } while (0)

// Restores the caller's current device on scope exit.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// A pinned host buffer and its device twin of `cap` bytes: one stream slot's staging of the chunked
// host paths.  reserve grows only; a failure leaves null pointers beside a zero cap.
struct __attribute__((visibility("hidden"))) StagePair {
    uint8_t *host = nullptr, *dev = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return 0;
        release();
        hipError_t e = hipMalloc((void **)&dev, bytes);
        if (e == hipSuccess) e = hipHostMalloc((void **)&host, bytes, hipHostMallocDefault);
        if (e != hipSuccess) release();
        cap = e == hipSuccess ? bytes : 0;
        return e == hipSuccess ? 0 : hip_fail(e, "host-path staging");
    }
    void release()
    {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        host = dev = nullptr;
        cap = 0;
    }
};

}  // namespace hfv

using namespace hfv;   // every unit that includes this header is library code

struct hfv_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    LaunchGeom geom{};
    int keysel = HFV_KEYSEL_ZERO;
    uint32_t inf_off = HFV_REC_INF_OFF, hf_off = HFV_REC_HF_OFF;
    // host shadow of mac_key_map
    hop_key shadow[HFV_MAX_KEYS];
    uint32_t valid[8] = {0};
    bool dirty = true;
    // publication
    DevState *host_img = nullptr;         // pinned staging image
    hipEvent_t img_free = nullptr;        // staging image may be rewritten once this fires
                                          // (= the last publish copy into dev_tab[active] is done)
    bool pub_pending = false;             // img_free not yet seen complete: other streams wait on it
    DevState *dev_tab[2] = {nullptr, nullptr};
    hipStream_t readers[2][8] = {};                // streams that launched with dev_tab[i]
    hipEvent_t reader_ev[2][8] = {};               // caller streams: recorded after each such launch
    int nreaders[2] = {0, 0};
    bool readers_overflow[2] = {false, false};
    int active = 0;
    // The chunked host paths (hfv_verify_records_host, hfv_br_process_host, hfv_verify_frames_host):
    // two streams and each one's staging, what a chunk copies up and what it copies back.  The three
    // calls share it: none runs beside another on a ctx, and each waits for both streams before its
    // first chunk.  Records: in = the 24-byte compact records, out = the bitmap words.  Router: in =
    // the packed header windows (both ways), out = len u16 | ifindex u32 | action u8 | verdict u8 |
    // egress i32, each at its kBrChunk offset.  Frames: in and out as FhLayout says.
    hipStream_t hstream[2] = {nullptr, nullptr};
    StagePair stage_in[2], stage_out[2];
    // attached pinned key map
    const void *keymap = nullptr;
    uint32_t keymap_seq = 0xffffffffu;
    char keymap_path[4096] = {0};
    // attached pinned router tables (hfv_ctx_attach_brconfig)
    const void *brmap = nullptr;
    uint32_t brmap_seq = 0xffffffffu;
    // interfaces of the AS-internal link (hfv_ctx_set_internal_ifindices), for the *_rx frame calls
    RxSet rx_set{};
    // dispatch timing (hfv_verify_records_timed)
    hipEvent_t tev[2] = {nullptr, nullptr};
    uint64_t *bat_clk = nullptr;   // device: hfv_verify_batches' block-0 clock stamps (hfv_debug_batches_clock)
    // router tables for hfv_br_process (published with the key table)
    DevBrConfig br{};
    hfv_br_config cfg_src{};   // the tables as installed (checked against the build options)
    uint64_t *brh_dstats = nullptr;   // device verdict counters of one hfv_br_process_host call
    // host buffers registered with hfv_host_register (mapped: the kernels can address them)
    struct HostRange {
        uint8_t *host;
        size_t bytes;
        uint8_t *dev;
    };
    HostRange hreg[16] = {};
    int nhreg = 0;
    uint8_t *zc_meta = nullptr;   // zero-copy path: device len/ifindex/outputs for unregistered arrays
    size_t zc_cap = 0;
    // resident verify service (hfv_service_*)
    bool svc_running = false;
    int svc_keysel = HFV_KEYSEL_ZERO;
    uint32_t svc_inf_off = 0, svc_hf_off = 0, svc_idle_ms = 0;
    hipStream_t svc_stream = nullptr;
    SvcShared *svc_host = nullptr;   // descriptor ring + completions, coherent pinned memory
    SvcShared *svc_host_dev = nullptr;
    SvcDev *svc_dev = nullptr;       // device side: relayed descriptors, block completions, diagnostics
    uint32_t svc_launches = 0;       // grids launched (SvcArea parity)
    unsigned svc_grid = 0;           // blocks of the running grid (each reports its share)
    uint64_t svc_next = 1;           // next grid-local batch number (1, 2, ... per grid)
    uint64_t svc_base = 1;           // ticket of the running grid's batch 1 (tickets are monotonic per ctx)
    uint64_t svc_ticket = 1;         // next ticket
    std::vector<uint64_t> svc_lost;  // tickets of stopped grids that were never verified (bounded)
    uint64_t svc_tag = 0;            // generation of the running grid << 40 (see s_svc_tag)
    bool svc_stop_posted = false;    // the running grid's stop descriptor is already in the ring
    bool svc_timing = true;          // launch grids with dispatch start/stop events (hfv_service_set_timing)
    bool svc_timed = false;          // ... the running / last grid was
    hipEvent_t svc_ev[2] = {nullptr, nullptr};
    // work balance across the grid's blocks (SvcWeights, svc_balance)
    SvcWeights svc_w = {{kSvcWeightUnit, kSvcWeightUnit, kSvcWeightUnit, kSvcWeightUnit, kSvcWeightUnit,
                         kSvcWeightUnit, kSvcWeightUnit, kSvcWeightUnit},
                        kSvcWeightUnit, {0, 0, 0}};
    SvcWeights svc_w_used = svc_w;   // the running / last grid's
    bool svc_adapt = false;          // the running grid got all its batches up front (svc_run): measure it
    std::vector<uint64_t> svc_run_ns;   // ... their record counts
    uint64_t svc_call_ns[6] = {0, 0, 0, 0, 0, 0};   // hfv_debug_service_call_ns: the last svc_run's phases
};

// What the units call of each other; none of it is exported from the library.
#pragma GCC visibility push(hidden)

// hfv_host_path.cpp
int device_numa(int device, cpu_set_t *cpus);
void note_numa(int device);
// Device address of [p, p + bytes) if it lies in a mapped registered buffer, else NULL.
uint8_t *host_dev_ptr(hfv_ctx *ctx, const void *p, size_t bytes);

// hfv_service.cpp.  Any other data-path call on the ctx first stops a running service (after
// the batches already posted): its grid holds every CU's LDS, so other kernels could not start
// until it exits, and a call that waits for its own kernel would wait for the idle timeout.
int svc_quiesce(hfv_ctx *ctx);
#define SVC_QUIESCE(ctx)                         \
    do {                                         \
        int q_ = svc_quiesce(ctx);               \
        if (q_) return q_;                       \
    } while (0)

// hfv_publish.cpp.  after_launch turns a launcher's hipError_t into the call's result and notes
// `st` as a reader of the table publish_keys returned (note_reader).  reader: the launch's kernel
// dereferences the DevState it is given (launch_reads_tables below; true for every other launch).
int publish_keys(hfv_ctx *ctx, hipStream_t st, DevState **out, bool reader = true);
void note_reader(hfv_ctx *ctx, hipStream_t st);
bool own_stream(const hfv_ctx *ctx, hipStream_t st);
int after_launch(hfv_ctx *ctx, hipStream_t st, int err, const char *what, bool reader = true);

// hfv_api.cpp.  What every call taking records checks of them: null buffers, 8-byte alignment of
// records, stride and bitmap, the stride against the ctx's record layout (a call's own limits stay with it).
int check_records(const hfv_ctx *ctx, const void *recs, size_t stride, const void *bits);
// The router kernel's launch geometry: the ctx's, with the test build's hfv_debug_br_grid / br_split.
// The batch-list launch's (launch_verify_batches, also behind launch_verify_records): the ctx's, with
// the test build's hfv_debug_batch_grid.  The macinput, tag, verdict-counter and generator launches'
// (hfv_aux_kernels.hip): the ctx's, with the test build's hfv_debug_aux_grid.
#ifdef HFV_TEST_HOOKS
LaunchGeom br_geom(const hfv_ctx *ctx);
LaunchGeom batch_geom(const hfv_ctx *ctx);
LaunchGeom aux_geom(const hfv_ctx *ctx);
#else
#define br_geom(ctx) ((ctx)->geom)
#define batch_geom(ctx) ((ctx)->geom)
#define aux_geom(ctx) ((ctx)->geom)
#endif

#pragma GCC visibility pop

// The last error again behind "batch i: ", for the calls that check a list of batches.
static inline int fail_batch(int rc, size_t i)
{
    char why[256];
    snprintf(why, sizeof why, "%s", hfv_last_error());
    return fail(rc, "batch %zu: %s", i, why);
}

// Does the kernel of a record or batch-list verify launch (launch_verify_records,
// launch_verify_batches) under `keysel` dereference the DevState it is launched with?  Under
// KEYSEL_ZERO, k_verify_batches<ZERO> and k_verify_records<ZERO, *> take T0 and slot 0's key rows
// from their kernel arguments (KeyPrologue) and fill_block never touches `tab`, so such a launch
// is no reader of a device table: it neither waits for a publish copy pending on another stream
// nor leaves a fence event for the next publish to wait on.  THIS MUST TRACK WHAT THE KERNELS
// READ: a KEYSEL_ZERO verify kernel that starts reading the table has to make this true again.
// Every other launch of the library reads its DevState and goes through with_tables as a reader.
static inline bool launch_reads_tables(int keysel) { return keysel != HFV_KEYSEL_ZERO; }

// One launch (or several) with the published tables: publish, launch(ds) -> hipError_t as int,
// then note the stream as a reader of the table it launched with (reader = false: see above).
template <class Launch>
static inline int with_tables(hfv_ctx *ctx, hipStream_t st, const char *what, bool reader, Launch launch)
{
    DevState *ds;
    int rc = publish_keys(ctx, st, &ds, reader);
    if (rc) return rc;
    return after_launch(ctx, st, launch(ds), what, reader);
}

template <class Launch>
static inline int with_tables(hfv_ctx *ctx, hipStream_t st, const char *what, Launch launch)
{
    return with_tables(ctx, st, what, true, launch);
}

// What a caller fills of a frames-to-verdict-bits launch's argument (the launcher fills the key rows).
static inline FusedArgs fused_args(const hfv_ctx *ctx, const DevState *ds, const uint8_t *frames, size_t slot,
                                   const uint16_t *len, const uint32_t *ifx, size_t n, uint8_t *status, uint64_t *bits)
{
    FusedArgs a;
    memset(&a, 0, sizeof a);
    a.frames = frames;
    a.slot = slot;
    a.lens = len;
    a.ifindex = ifx;
    a.n = n;
    a.status = status;
    a.bits = (unsigned long long *)bits;
    a.tab = &ds->keys;
    a.set = ctx->rx_set;
    return a;
}
