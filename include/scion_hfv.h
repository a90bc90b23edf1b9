/*
 * scion_hfv.h -- C ABI of libscionhfv.so: SCION border-router hop-field (HF) AES-CMAC
 * verification on AMD MI355X (gfx950).
 *
 * What it replaces in the reference (netsys-lab/scion-xdp-br):
 *   - the per-packet data-plane call  int verify_hop_field(struct macinput*, u64 expected)
 *     (br/src/bpf/xdp.c:77-91) together with the macinput assembly and beta/SegID rule of
 *     defer_verify_hop_field / scion_as_ingress (br/src/bpf/path_processing.h:39-81),
 *     now executed for a whole batch per kernel launch;
 *   - the control-plane key table  mac_key_map  (br/src/bpf/maps.h:60-67) and its writers
 *     `br-loader key add|remove` (br/src/br_loader.cpp:182-261).
 *
 * Conventions
 *   - Status: 0 on success, a negative errno on failure (-EINVAL bad argument, -ENODEV no
 *     usable GPU, -ENOMEM allocation, -EIO HIP runtime error).  hfv_last_error() returns a
 *     human-readable message for the calling thread.  No C++ exception crosses the ABI.
 *   - Batch buffers (records, macinputs, tags, pass bitmaps) are DEVICE pointers (hipMalloc,
 *     hipMallocManaged or a framework allocation on the ctx's GPU) unless a function says
 *     otherwise.  `stream` is a hipStream_t passed as void*; NULL is HIP's default
 *     stream (hfv_ctx_stream() returns a private non-blocking stream of the ctx).  Calls enqueue work and return; completion is stream-ordered.
 *   - Verdict output: bit (i % 64) of pass_bits[i / 64] is 1 iff packet i's hop field
 *     verifies; bits for i >= n in the last word are 0.  A missing key fails closed
 *     (xdp.c:83-84).
 *   - Threading: one ctx per GPU, used by one host thread at a time (or externally
 *     serialised), like one XDP program instance per CPU queue.
 */
#ifndef SCION_HFV_H
#define SCION_HFV_H

#include <stddef.h>
#include <stdint.h>

#include "hfv_aes.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HFV_ABI_VERSION 3
#define HFV_MAX_KEYS 256          /* key slots; the reference map holds 8 (maps.h:60-67) */
#define HFV_REC_INF_OFF 40        /* default 64 B record layout, DESIGN.md section 3 */
#define HFV_REC_HF_OFF 48

/* struct macinput (include/bpf/scion.h:122-132): 16 B, wire byte order */
struct macinput {
    uint16_t null0;
    uint16_t beta;
    uint32_t ts;
    uint8_t null1;
    uint8_t exp;
    uint16_t ingress;
    uint16_t egress;
    uint16_t null2;
} __attribute__((packed));

/* struct hop_key (br/src/bpf/common.h:87-91): expanded key + CMAC subkey K1, 192 B */
struct hop_key {
    struct aes_key_schedule key;
    struct aes_block subkey;
};

/* Per-packet key selection (SURVEY.md 8b iii) */
enum hfv_keysel {
    HFV_KEYSEL_ZERO = 0,  /* mac_key_map[0] for every packet: the reference rule, xdp.c:82 */
    HFV_KEYSEL_IFID = 1,  /* slot = AS-ingress IFID & 0xff, IFID = Cons ? HF.ingress : HF.egress
                             (the hf_ingress rule of xdp.c:151-157) */
};

typedef struct hfv_ctx hfv_ctx;

/* ---- lifetime ----------------------------------------------------------------------
 * Replaces the mac_key_map creation/pinning part of attachBr (br_loader.cpp:88-151). */
int hfv_ctx_create(int device, hfv_ctx **out);
int hfv_ctx_destroy(hfv_ctx *ctx);
int hfv_ctx_device(const hfv_ctx *ctx);
/* NUMA node of the ctx's GPU (its PCIe root port), -1 if unknown.  The library's host worker
 * threads (staging copies of the host-memory paths) run on that node's CPUs (HFV_NUMA_PIN=0:
 * unpinned); a host feeder thread per GPU should be placed there too. */
int hfv_ctx_numa_node(const hfv_ctx *ctx);
void *hfv_ctx_stream(hfv_ctx *ctx);
int hfv_ctx_set_keysel(hfv_ctx *ctx, int keysel);
/* Offsets of the current InfoField / HopField inside each record (multiples of 8). */
int hfv_ctx_set_record_layout(hfv_ctx *ctx, uint32_t inf_off, uint32_t hf_off);
/* Wait for all work the ctx enqueued on its own stream. */
int hfv_ctx_synchronize(hfv_ctx *ctx);

/* ---- key table (mac_key_map) -------------------------------------------------------
 * Updates are made on a host shadow table and published to the GPU at the next batch
 * boundary (stream-ordered, double-buffered): batches already enqueued keep the table
 * they were launched with, like RCU readers of the BPF hash map. */
/* br-loader key add: decodeKey -> aes_key_expansion -> aes_cmac_subkeys -> keep K1
 * -> map update (br_loader.cpp:182-229). */
int hfv_key_add(hfv_ctx *ctx, uint32_t index, const struct aes_key *key);
/* Same, from the 24-character base64 form the CLI takes (decodeKey, br_loader.cpp:65-73). */
int hfv_key_add_b64(hfv_ctx *ctx, uint32_t index, const char *base64);
/* Map::update with a ready hop_key (what br-loader writes to the map). */
int hfv_key_set_hop_key(hfv_ctx *ctx, uint32_t index, const struct hop_key *hk);
/* br-loader key remove: Map::erase (br_loader.cpp:231-261); the slot then fails closed.
 * Returns -ENOENT if the slot was empty (the BPF map erase fails the same way). */
int hfv_key_remove(hfv_ctx *ctx, uint32_t index);
/* Map lookup: copies the slot's hop_key, -ENOENT if empty. */
int hfv_key_get(hfv_ctx *ctx, uint32_t index, struct hop_key *out);

/* ---- pinned key map ------------------------------------------------------------------
 * A file-backed mac_key_map that other processes update while the data plane runs, the
 * analogue of the bpffs-pinned map /sys/fs/bpf/<br>/mac_key_map (br_loader.cpp:119-126,
 * 191, 221-222).  Path: $HFV_PIN_DIR/<br>/mac_key_map, HFV_PIN_DIR defaults to /dev/shm/hfv.
 * Writers serialise with flock; readers see whole updates (seqlock). */
int hfv_keymap_path(const char *br, char *out, size_t len);
/* Map modes, fixed when the map is created:
 *   HFV_KEYMAP_SLOTS  256 direct slots, index 0..255 (per-interface keys, config 3);
 *   HFV_KEYMAP_HASH8  the reference map's semantics (maps.h:60-67: BPF_MAP_TYPE_HASH, u32
 *                     index, max_entries 8): any u32 index, a 9th new index fails with -E2BIG
 *                     as bpf_map_update_elem does.  The data plane reads indices < 256 (slot 0
 *                     in the reference's single-key mode, xdp.c:82); larger ones are kept and
 *                     listed but never looked up.  `hfv-loader` creates this mode. */
#define HFV_KEYMAP_SLOTS 0
#define HFV_KEYMAP_HASH8 1
/* Map::update (BPF_ANY) of one index, creating a SLOTS map file if needed. */
int hfv_keymap_update(const char *path, uint32_t index, const struct hop_key *hk);
/* An empty map (no slot written) if the file does not exist yet; an existing map is kept. */
int hfv_keymap_create(const char *path);
/* The same with the mode; an existing map without keys takes the mode, one with keys keeps its own. */
int hfv_keymap_create_mode(const char *path, int mode);
/* The map's mode (>= 0) or a negative errno. */
int hfv_keymap_mode(const char *path);
/* Map::erase of one index; -ENOENT if it was empty. */
int hfv_keymap_erase(const char *path, uint32_t index);
/* Every entry (index ascending) into indices[]/keys[] up to cap; *count = number of entries. */
int hfv_keymap_list(const char *path, uint32_t *indices, struct hop_key *keys, size_t cap, size_t *count);
/* Consistent snapshot of all HFV_MAX_KEYS slots and the 256-bit valid mask. */
int hfv_keymap_read(const char *path, struct hop_key *slots, uint32_t *valid);
/* reusePinnedMap: the ctx reloads its key table from the pinned map whenever the map
 * changed, at the next batch boundary; hfv_key_add/remove on the ctx then write through
 * to the map.  The map is created empty if it does not exist. */
int hfv_ctx_attach_keymap(hfv_ctx *ctx, const char *path);

/* ---- data path ----------------------------------------------------------------------
 * Fused per-packet verify over fixed-layout records: build macinput from the record's
 * InfoField/HopField with the AS-ingress beta rule (path_processing.h:39-81), select the
 * key (keysel), one-block CMAC (aes.h:129-141), 48-bit compare (xdp.c:89-90).
 * recs: n records of `stride` bytes (8-byte aligned, stride % 8 == 0). */
int hfv_verify_records(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, uint64_t *pass_bits,
                       void *stream);
/* One batch of records for the multi-batch calls (hfv_verify_batches, hfv_service_submitv,
 * hfv_service_run): n records of `stride` bytes at recs, verdicts into pass_bits. */
struct hfv_batch {
    const void *recs;
    size_t stride;
    size_t n;
    uint64_t *pass_bits;
};
/* hfv_verify_records over `count` batches in ONE stream-ordered launch (up to 64 batches per
 * launch; more are split): the round tables are written into LDS once for all of them, and
 * the batches' tiles are dealt to the CUs as one contiguous range.  Records written by earlier
 * work on `stream` are read, the bitmaps are complete for later work on it -- the fast path
 * for callers whose batches come from a copy or from hfv_extract_records on a stream (one
 * hfv_verify_records launch per batch pays the table fill and the grid's ramp and tail per
 * batch).  Each batch is checked as hfv_verify_records checks one; empty batches are skipped. */
int hfv_verify_batches(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, void *stream);
/* Same, then waits and stores the launches' execution time (dispatch start of the first to
 * dispatch end of the last) in *kernel_ms.  For benchmarks. */
int hfv_verify_batches_timed(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, void *stream,
                             float *kernel_ms);

/* ---- frames -> records -> verdict bits --------------------------------------------------
 * The producer in front of the record verify: parse_underlay + parse_scion + parse_scion_path
 * (br/src/bpf/parser.h:45-204) over raw Ethernet frames, and nothing else of process_packet (no
 * lookup, no rewrite, no counters).  Per frame a status: 0, or the verdict the router
 * (hfv_br_process) records when its parse fails at the same place.  The router's build options
 * (HFV_BR_NO_*) do not apply: IPv4, IPv6 and the standard SCION path type are always parsed. */
#define HFV_FRAME_OK 0
#define HFV_FRAME_PARSE_ERROR 17      /* a bound check of parse_scion / parse_scion_path failed */
#define HFV_FRAME_NOT_SCION 26        /* whatever parse_underlay rejects */
#define HFV_FRAME_NOT_IMPLEMENTED 34  /* SCION version != 0, or path type != 1 */
/* The compact record: InfoField at 0, HopField at 8, 4 bytes of padding.  Recommended with
 * hfv_ctx_set_record_layout(ctx, 0, 8): a wave's 64 records are 1536 contiguous bytes. */
#define HFV_FRAME_REC_STRIDE 24
/* Parse one frame on the host; *inf_off / *hf_off (the byte offsets of the current InfoField and
 * HopField) are valid when the result is HFV_FRAME_OK.  Returns the status (>= 0), or -EINVAL for
 * NULL arguments.  The scalar counterpart of the extract kernel, for control-plane checks. */
int hfv_frame_locate(const uint8_t *frame, size_t len, uint32_t *inf_off, uint32_t *hf_off);
/* Frame i at frames + i*slot (slot % 8 == 0, >= 64), len[i] its length (clamped to slot).  For
 * every frame: status[i], and into record i (recs + i*stride; recs and stride 8-byte aligned,
 * stride >= inf_off + 8 and >= hf_off + 12 of the ctx's record layout) the frame's current
 * InfoField (8 B at inf_off) and HopField (12 B at hf_off), both all zeros where status[i] != 0.
 * Record bytes outside the two fields are unspecified afterwards.  frames is never written, no
 * byte at or past frames + n*slot is read, and bytes of a slot at or past len[i] count as absent.
 * All pointers are device pointers; stream-ordered like hfv_verify_records; needs no key table.
 * Like every data-path call it first stops a running verify service (whose grid holds the LDS
 * the kernel needs).  n == 0 returns 0. */
int hfv_extract_records(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len, size_t n,
                        void *recs, size_t stride, uint8_t *status, void *stream);
/* Same, then waits and stores the kernel's execution time (dispatch start/stop) in *kernel_ms. */
int hfv_extract_records_timed(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len, size_t n,
                              void *recs, size_t stride, uint8_t *status, void *stream, float *kernel_ms);
/* Frames to verdict bits in one call: hfv_extract_records, hfv_verify_batches over recs (one batch;
 * the ctx's key table, keysel and record layout), then pass_bits &= (status == 0), all on `stream`
 * with no host synchronisation.  Bit i is 1 iff status[i] == 0 and the record verifies; bits >= n
 * of the last word are 0.  recs and status are the caller's scratch and outputs (the library
 * allocates nothing on this path). */
int hfv_verify_frames(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len, size_t n,
                      void *recs, size_t stride, uint8_t *status, uint64_t *pass_bits, void *stream);

/* ---- direction-aware frames: the AS-egress rule for frames from the internal link -------------
 * The calls above apply one MAC-chaining rule, the AS-ingress rule of scion_as_ingress
 * (path_processing.h:72-81): beta = SegID ^ MAC[0:2] for a Cons = 0 segment.  It holds for frames
 * received on an external interface.  A frame that arrives over the AS-internal link was processed
 * by a sibling router, which folded the MAC into the SegID already; the router verifies it in
 * scion_as_egress (path_processing.h:140-142) with the SegID as it stands, whatever Cons, and
 * chooses that rule where the receiving ifindex is in int_iface_map (xdp.c:129-131).  The *_rx calls
 * take that ifindex per frame and write a normalised record for such frames: where status is 0,
 * the frame is internal and its current InfoField has Cons = 0 (byte 0, bit 0), the record's SegID
 * (InfoField bytes 2-3) is the frame's SegID ^ the current HopField's bytes 6-7 (MAC[0:2]), which
 * the verify kernels' ingress rule undoes.  Every other byte, and every record of an external or
 * Cons = 1 frame, is what hfv_extract_records writes.  The record verify itself is unchanged.
 *
 * What these calls do NOT do (the router, hfv_br_process, does):
 *   - no ingress_map lookup and no VERDICT_NO_INTERFACE: any ifindex outside the set is external;
 *   - no router-alert check (a hop field with alert flags is verified like any other);
 *   - frames from the internal link whose AS-egress interface is not fwd_external (internal to
 *     internal) get no MAC check at all in the reference (xdp.c:202-233); here they are judged by
 *     the egress rule like every internal frame;
 *   - hfv_verdict_counters keys by the AS-ingress IFID of the record, which is not the receiving
 *     interface of an internal frame. */
/* The membership test of int_iface_map as a set of at most HFV_BR_MAX_IFACES ifindices, held on
 * the host in the ctx: pass cfg.int_ifaces[i].ifindex of the router's hfv_br_config (the set is
 * independent of hfv_br_set_config).  n == 0 clears it.  n > HFV_BR_MAX_IFACES, or NULL with
 * n > 0: -EINVAL, the set unchanged.  Takes effect for calls enqueued afterwards. */
int hfv_ctx_set_internal_ifindices(hfv_ctx *ctx, const uint32_t *ifindex, size_t n);
/* hfv_extract_records with the receiving interface: ingress_ifindex is a device uint32_t[n] (the
 * array hfv_br_process takes), never written, no element at or past n read; frame i is internal
 * iff ingress_ifindex[i] is in the ctx's set.  NULL, or an empty set: every frame is external and
 * the outputs are byte-identical to hfv_extract_records. */
int hfv_extract_records_rx(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                           const uint32_t *ingress_ifindex, size_t n, void *recs, size_t stride, uint8_t *status,
                           void *stream);
int hfv_extract_records_rx_timed(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                                 const uint32_t *ingress_ifindex, size_t n, void *recs, size_t stride,
                                 uint8_t *status, void *stream, float *kernel_ms);
/* hfv_verify_frames over hfv_extract_records_rx: the same three launches on `stream`, no host
 * synchronisation, no allocation, the same argument checks. */
int hfv_verify_frames_rx(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                         const uint32_t *ingress_ifindex, size_t n, void *recs, size_t stride, uint8_t *status,
                         uint64_t *pass_bits, void *stream);
/* Frames in, verdict bits out, in ONE launch on `stream`: the parse and the hop-field MAC in one
 * kernel, with no record in between.  No record buffer exists and the ctx's record layout plays no
 * part; status is optional (NULL: not written).  For every input that hfv_verify_frames_rx accepts,
 * pass_bits[0 .. (n+63)/64) is bit-identical to what that call writes (bits >= n of the last word
 * are 0) and status[0..n) likewise, for the same frames, slot, len, ingress_ifindex, n, key table,
 * keysel and internal-ifindex set.  Direction as above: ingress_ifindex NULL or an empty set means
 * every frame is external; otherwise a frame is internal iff its ifindex is in the ctx's set and is
 * judged with the SegID as it stands (path_processing.h:140-142), every other frame by the
 * AS-ingress rule (path_processing.h:73-77).  The limits are those of "What these calls do NOT do"
 * above.  Fail closed: KEYSEL_ZERO with slot 0 empty clears every bit (status is still written);
 * KEYSEL_IFID clears the bit of a frame whose key slot is empty.
 * Every bitmap word is written whole by one plain store, nothing is read-modify-written: the bitmap
 * needs no initialisation.  frames is never written; nothing at or past frames + n*slot, len + n or
 * ingress_ifindex + n is read; no bitmap word at or past (n+63)/64 and no status byte at or past n
 * is touched.  No allocation, no host synchronisation; like every data-path call it first stops a
 * running verify service.  Checks: frames, slot, len and n as hfv_extract_records; pass_bits
 * non-NULL and 8-byte aligned; n == 0 returns 0 and touches nothing, even with NULL buffers. */
int hfv_verify_frames_fused(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                            const uint32_t *ingress_ifindex, size_t n, uint8_t *status, uint64_t *pass_bits,
                            void *stream);
/* Same, then waits and stores the kernel's execution time (dispatch start/stop) in *kernel_ms. */
int hfv_verify_frames_fused_timed(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                                  const uint32_t *ingress_ifindex, size_t n, uint8_t *status, uint64_t *pass_bits,
                                  void *stream, float *kernel_ms);
/* One batch of the frame list of hfv_verify_frames_batches: the arguments hfv_verify_frames_fused
 * takes for one batch. */
struct hfv_frame_batch {            /* 56 bytes */
    const uint8_t *frames;          /* frame i at frames + i*slot */
    size_t slot;
    const uint16_t *len;
    const uint32_t *ingress_ifindex;/* nullable: every frame of this batch is external */
    size_t n;
    uint8_t *status;                /* nullable: not written */
    uint64_t *pass_bits;            /* (n+63)/64 words, 8-byte aligned */
};
/* hfv_verify_frames_fused over `count` batches in as few launches as the list allows: what
 * hfv_verify_batches is to hfv_verify_records.  The round tables are written into LDS once per
 * launch and the batches' tiles are dealt to the CUs as one contiguous range, so a list of ring
 * chunks pays the table fill, the grid's ramp and tail and the launch once, not once per chunk.
 * One launch holds up to 32 consecutive non-empty batches (and 2^31 tiles) that are all staged
 * (slot >= 128, slot % 16 == 0, frames 16-byte aligned) or all not; a longer or mixed list is split,
 * in list order.
 * For every batch j with n != 0, pass_bits and status hold bit for bit what
 * hfv_verify_frames_fused(ctx, frames, slot, len, ingress_ifindex, n, status, pass_bits, stream)
 * writes for that batch, under the ctx's key table, keysel and internal-ifindex set at the time of
 * the call: bits at or past n of a batch's last word are 0; every bitmap word is written whole by
 * one plain store, so no initialisation is needed; no bitmap word at or past (n+63)/64 and no
 * status byte at or past n is touched; nothing at or past frames + n*slot, len + n or
 * ingress_ifindex + n is read; no input is written.
 * Stream-ordered: the call reads what earlier work on `stream` wrote and its outputs are complete
 * for later work on it; it allocates nothing and does not synchronise the host.  Like every
 * data-path call it first stops a running verify service.  Key-table publication holds as for
 * hfv_verify_frames_fused: a launch keeps the table it was launched with.
 * Empty batches (n == 0) are skipped and their pointers are not looked at; count == 0, or a list of
 * empty batches only, returns 0 and launches nothing (the tables are still published).
 * All batches are checked before anything is launched: frames, slot, len and n as
 * hfv_extract_records; pass_bits non-NULL and 8-byte aligned.  A bad batch k returns -EINVAL with
 * "batch k: ..." in hfv_last_error(), and no output of any batch has been touched.  NULL ctx, or
 * NULL batches with count > 0: -EINVAL.
 * Outputs of different batches must not overlap.  Inputs may be shared: the same frames may appear
 * in two batches with different ifindex arrays. */
int hfv_verify_frames_batches(hfv_ctx *ctx, const struct hfv_frame_batch *batches, size_t count, void *stream);
/* Same, then waits and stores the launches' execution time (dispatch start of the first to
 * dispatch end of the last) in *kernel_ms; 0.0 and 0 when nothing is launched.  NULL kernel_ms:
 * -EINVAL. */
int hfv_verify_frames_batches_timed(hfv_ctx *ctx, const struct hfv_frame_batch *batches, size_t count,
                                    void *stream, float *kernel_ms);
/* Frames addressed by DESCRIPTORS into one buffer, verified in place in ONE launch on `stream`:
 * hfv_verify_frames_fused for a caller whose frames lie where the NIC put them -- an AF_XDP UMEM
 * (an RX ring hands out struct xdp_desc entries: chunk offset plus headroom, in whatever order the
 * fill ring recycled the chunks) or a DPDK mempool -- with no gather into slots first. */
#define HFV_FRAME_DESC_MAX_LEN 65535u
#define HFV_FRAME_BAD_DESC 255        /* status of a frame whose descriptor is rejected; no router verdict has this value */
struct hfv_frame_desc {               /* 16 bytes; the layout of AF_XDP's struct xdp_desc */
    uint64_t addr;                    /* byte offset of the frame's first byte inside the buffer */
    uint32_t len;                     /* frame length in bytes */
    uint32_t ifindex;                 /* receiving interface (xdp_desc's `options` word, filled by the caller) */
};
/* The validity rule, on the host (the kernel applies the same function per frame): 1 iff
 * len <= HFV_FRAME_DESC_MAX_LEN and addr <= umem_bytes and len <= umem_bytes - addr, else 0.  No
 * sum is formed, so nothing wraps at 2^64; len == 0 is valid (and reads nothing). */
int hfv_frame_desc_ok(uint64_t addr, uint32_t len, size_t umem_bytes);
/* umem, desc, status (nullable: not written) and pass_bits are device pointers.  Frame i is the
 * bytes [umem + desc[i].addr, umem + desc[i].addr + desc[i].len) when desc[i] is valid
 * (hfv_frame_desc_ok); descriptors may come in any order, may overlap and may repeat a frame; addr
 * and umem need no alignment (a umem that is not 16-byte aligned, or shorter than 128 bytes, takes
 * the kernel without 16-byte staging loads, with the same results).
 * Equivalence: take any slot that is a multiple of 8, at least 64 and at least every valid len,
 * copy each valid frame to frames + i*slot with len[i] = desc[i].len and ingress_ifindex[i] =
 * desc[i].ifindex: pass_bits[0 .. (n+63)/64) and status[0..n) are bit-identical to what
 * hfv_verify_frames_fused writes for that copy under the same key table, keysel and
 * internal-ifindex set, except at the indices of invalid descriptors, which get bit 0 and status
 * HFV_FRAME_BAD_DESC.  Bits at or past n of the last word are 0; every bitmap word is written whole
 * by one plain store, so the bitmap needs no initialisation.  Direction: a frame is internal iff
 * its ifindex is in the ctx's set (hfv_ctx_set_internal_ifindices); an empty set makes every frame
 * external.  The fail-closed rules are those of hfv_verify_frames_fused.
 * What is read: no byte outside [umem, umem + umem_bytes), and none at all on behalf of an invalid
 * descriptor; no descriptor at or past desc + n.  The outputs depend on no byte of the buffer
 * outside the frame's own [addr, addr + len): bytes past len count as absent although real memory
 * follows them.  umem and desc are never written; no bitmap word at or past (n+63)/64 and no
 * status byte at or past n is touched.
 * Stream-ordered: no allocation, no host synchronisation; like every data-path call it first stops
 * a running verify service.  Key-table publication holds as for hfv_verify_frames_fused.
 * Checks: NULL ctx is -EINVAL, even with n == 0; n == 0 returns 0 and touches nothing; with n > 0,
 * -EINVAL with a message in hfv_last_error() for a NULL desc, a desc that is not 8-byte aligned, a
 * pass_bits that is NULL or not 8-byte aligned, a NULL umem with umem_bytes > 0, or n > 2^36.
 * The descriptors' contents live on the device: they are judged per frame, never by the return
 * value. */
int hfv_verify_frames_desc(hfv_ctx *ctx, const uint8_t *umem, size_t umem_bytes, const struct hfv_frame_desc *desc,
                           size_t n, uint8_t *status, uint64_t *pass_bits, void *stream);
/* Same, then waits and stores the kernel's execution time (dispatch start/stop) in *kernel_ms.
 * NULL kernel_ms: -EINVAL. */
int hfv_verify_frames_desc_timed(hfv_ctx *ctx, const uint8_t *umem, size_t umem_bytes,
                                 const struct hfv_frame_desc *desc, size_t n, uint8_t *status, uint64_t *pass_bits,
                                 void *stream, float *kernel_ms);
/* One frame on the host: hfv_frame_locate, the copy of the two fields and, for from_internal != 0,
 * the normalisation above.  Returns the status; inf and hf are all zeros for a non-zero status;
 * -EINVAL for NULL arguments.  The scalar counterpart of hfv_extract_records_rx. */
int hfv_frame_extract(const uint8_t *frame, size_t len, int from_internal, uint8_t inf[8], uint8_t hf[12]);

/* Verdict counts for the verify-only paths, modelled on record_verdict (xdp.c:54-70) but NOT
 * its layout: counters[slot][0] += packets that verified, counters[slot][1] += packets dropped
 * as VERDICT_INVALID_HF, where slot is the packet's AS-ingress interface (IFID & 0xff,
 * Cons ? HF.ingress : HF.egress, xdp.c:151-157) -- an IFID-keyed approximation with packet
 * counts only; the reference's port_stats_map is keyed by the receiving ifindex and also counts
 * bytes, so these do not compare with it (hfv_br_process's counters do).
 * From the records and the verdict bitmap hfv_verify_records or the service wrote for them.
 * counters: device u64[256][2], added to.  Stream-ordered like hfv_verify_records. */
int hfv_verdict_counters(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, const uint64_t *pass_bits,
                         uint64_t *counters, void *stream);
/* verify_hop_field (xdp.c:77-91) for n prepared inputs: macinput[i] against the 48-bit
 * expected[i] (low 48 bits of the LE u64, as defer_verify_hop_field stores it).
 * key_index: per-packet slot (device u8 array) or NULL for slot 0. */
int hfv_verify_macinputs(hfv_ctx *ctx, const struct macinput *mi, const uint64_t *expected,
                         const uint8_t *key_index, size_t n, uint64_t *pass_bits, void *stream);
/* Parity mode: full 16-byte AES-CMAC tags of n one-block messages (aes_cmac_16bytes).
 * A missing key yields an all-zero tag. */
int hfv_cmac_tags(hfv_ctx *ctx, const struct macinput *mi, const uint8_t *key_index, size_t n,
                  struct aes_cmac *tags, void *stream);
/* Same as hfv_verify_records, then waits for it and stores the kernel's own execution
 * time (start/stop timestamps of the dispatch, hipExtLaunchKernel events) in *kernel_ms.
 * Used by the benchmark to price the kernel against its roofline. */
int hfv_verify_records_timed(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, uint64_t *pass_bits,
                             void *stream, float *kernel_ms);
/* Host-memory batch (config 5 path): records and bitmap in HOST memory; returns when
 * pass_bits is complete.  From pageable records, host threads (HFV_HOST_THREADS, default
 * min(8, cores)) gather each record's InfoField and HopField (the 20 bytes the verifier
 * reads) into 24-byte pinned staging records, chunk by chunk, with gather / H2D / kernel /
 * D2H overlapped over chunks on two streams; records inside a buffer registered with
 * hfv_host_register (an RX ring) are read by the kernel in place over PCIe (zero-copy),
 * and a registered pass_bits is written in place. */
int hfv_verify_records_host(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, uint64_t *pass_bits);
/* Frames in HOST memory in, verdict bits out: hfv_verify_frames_fused for a caller whose RX ring is
 * host memory and who wants the verdicts only (hfv_br_process_host also rewrites the frames and
 * copies every header window back).  All pointers are host pointers; frames needs no alignment;
 * ingress_ifindex, status and retried are nullable.  Synchronous: on return
 * pass_bits[0 .. (n+63)/64) is complete in host memory, and status[0..n) where given.
 * For every input the outputs are bit-identical to what hfv_verify_frames_fused writes for a device
 * copy of the same frames, len and ingress_ifindex, under the ctx's key table, keysel and
 * internal-ifindex set at the time of the call: bits at or past n of the last word are 0, the
 * bitmap needs no initialisation, no bitmap word or status byte past the end is touched, nothing at
 * or past frames + n*slot, len + n or ingress_ifindex + n is read, frames is never written, and
 * the fail-closed rules are those of hfv_verify_frames_fused.
 * Pageable frames: per chunk of 65536 frames, on two alternating streams, host threads
 * (HFV_HOST_THREADS) pack the first `window` bytes of each slot into pinned staging, one H2D copy
 * moves them with len and ingress_ifindex, a windowed kernel parses min(len, slot, window) bytes of
 * each frame, and one D2H copy brings back two bits per frame (verdict, run again) and, only where
 * status is given, a byte.  A frame whose headers pass the window (its parse stops at a bound
 * check while more of the frame lies past the window) is run again with its whole slot, and
 * *retried receives their number.  window: a multiple of 8 in [64, slot]; 0 means 256, capped at
 * slot (hfv_br_process_host's rule); the result never depends on it.  The staging belongs to the
 * ctx: allocated on first use, grown only when the window grows, freed by hfv_ctx_destroy.
 * Frames inside a buffer registered with hfv_host_register: the full-slot kernel reads them in
 * place over PCIe (zero-copy), nothing is packed or run again (*retried = 0), and each of len,
 * ingress_ifindex, status and pass_bits is used in place where it is registered too, else copied
 * once.
 * Checks: frames, slot, len and n as hfv_br_process_host; pass_bits non-NULL and 8-byte aligned;
 * a NULL ctx is -EINVAL even with n == 0, otherwise n == 0 returns 0 and touches nothing.  Like
 * every data-path call it first stops a running verify service. */
int hfv_verify_frames_host(hfv_ctx *ctx, const uint8_t *frames, size_t slot, const uint16_t *len,
                           const uint32_t *ingress_ifindex, size_t n, size_t window, uint8_t *status,
                           uint64_t *pass_bits, size_t *retried);

/* ---- resident verify service -----------------------------------------------------------
 * The GPU counterpart of the XDP program staying attached to the interface
 * (border_router, xdp.c:250-284, runs for every packet without a per-packet load): one
 * persistent grid per ctx keeps the AES tables (and, for KEYSEL_IFID, the key image)
 * resident in LDS and verifies batches as the host posts them, with the same verdict
 * semantics as hfv_verify_records.  Batches are posted into a 128-entry descriptor ring in
 * pinned host memory; no kernel launch or table fill per batch, and a batch's tail
 * overlaps the next batch's start.  Batches posted before the grid starts (hfv_service_run /
 * run_async, submitv on a stopped service) travel in the launch's kernel arguments (up to 64),
 * so those batches involve no PCIe round trip at all; batches posted to a running grid are
 * fetched by one relay wave, up to 64 per host read, and their completions are forwarded to
 * the ring by the same wave -- the verifying waves never access host memory.
 *   - Key-table, keysel or record-layout changes take effect at the next submit (the
 *     service is restarted there, after the batches already posted: a batch boundary).
 *   - Any other data-path call on the ctx (hfv_verify_records, hfv_br_process, ...) first
 *     stops the service after its posted batches; the next submit starts it again.
 *   - The grid exits by itself after idle_ms without a new batch (default 1000 ms), so a
 *     host that disappears never leaves it running; a later submit restarts it.
 *   - While the service runs it holds every CU's LDS: other kernels on this GPU wait for it
 *     to stop. */
/* Launch the service grid (no-op if running).  idle_ms 0: 1000 ms. */
int hfv_service_start(hfv_ctx *ctx, uint32_t idle_ms);
/* Post one batch (device pointers, as hfv_verify_records; starts the service if needed).
 * Returns its ticket (1, 2, ...) in *ticket.  Blocks only while 128 batches are in flight.
 * Host-ordered, not stream-ordered: the records must be in place and the bitmap must no
 * longer be written by other work when the call is made (synchronize their producers). */
int hfv_service_submit(hfv_ctx *ctx, const void *recs, size_t stride, size_t n, uint64_t *pass_bits,
                       uint64_t *ticket);
/* Post `count` batches in one call (tickets *first_ticket .. *first_ticket + count - 1), the
 * many-descriptor form of hfv_service_submit (recvmmsg-style: one call per burst of RX
 * batches).  All batches are checked before any is posted. */
int hfv_service_submitv(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, uint64_t *first_ticket);
/* One-shot run: the batches on a fresh grid (a running service is stopped first), with the
 * stop descriptor posted right behind them, so the grid exits as soon as the last batch is
 * verified; returns when it has (every ticket done) with the grid's lifetime in *kernel_ms
 * (nullable).  For a known set of batches it saves posting and relaying a stop afterwards. */
int hfv_service_run(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, uint64_t *first_ticket,
                    float *kernel_ms);
/* The same without the wait: returns once the grid is launched with the batches and the stop
 * behind them, so a caller that synchronizes the device (or the tickets) anyway does not wait
 * twice.  The grid exits by itself after the last batch; hfv_service_stop (or any later data-path
 * call) reaps it and reports its lifetime. */
int hfv_service_run_async(hfv_ctx *ctx, const struct hfv_batch *batches, size_t count, uint64_t *first_ticket);
/* Tickets are monotonic over the ctx's life, across service restarts (key changes, idle
 * exits): a ticket of a stopped grid reports done, or -EIO if that grid exited on its idle
 * timeout without verifying it. */
/* 1 if the ticket's verdicts are complete in pass_bits (visible to any stream and to
 * copies), 0 if not yet.  A grid that has exited on the stop a run / run_async posted has
 * verified every batch before it (its completions need not have been forwarded). */
int hfv_service_poll(hfv_ctx *ctx, uint64_t ticket);
/* Wait until the ticket is complete; timeout_ms < 0 waits indefinitely.  -ETIMEDOUT on
 * timeout, -EIO if the service stopped before completing it. */
int hfv_service_wait(hfv_ctx *ctx, uint64_t ticket, int timeout_ms);
/* Finish the posted batches and stop the grid; *kernel_ms (nullable) receives the grid's
 * lifetime (dispatch start/stop events).  -ETIMEDOUT if it had exited on its idle timeout. */
int hfv_service_stop(hfv_ctx *ctx, float *kernel_ms);
int hfv_service_running(const hfv_ctx *ctx);
/* Grids started from now on carry the dispatch start/stop events that hfv_service_stop /
 * hfv_service_run report as the lifetime (1, the default) or not (0: the lifetime reads 0).
 * The events cost the runtime ~12 us per launch-to-synchronize round trip on MI355X (7.5 us of
 * host time in the launch call, profiles/r03/launch_cost/), which a short run can leave out. */
int hfv_service_set_timing(hfv_ctx *ctx, int enable);
/* Service grids started from now on use `blocks` blocks (one per CU at most; 0 = one per CU,
 * the default).  For several processes sharing one GPU, each with its own service: every grid
 * holds the LDS of the CUs it runs on, so grids of cus/ranks blocks run side by side.  Stops
 * a running grid after its posted batches. */
int hfv_service_set_grid(hfv_ctx *ctx, int blocks);

/* ---- key-schedule kernels ------------------------------------------------------------
 * AES-128 key expansion + CMAC K1 on the GPU, one key per lane: device raw keys[n] ->
 * device hop_keys[n] (same bytes as aes_key_expansion + aes_cmac_subkeys). */
int hfv_expand_keys(hfv_ctx *ctx, const struct aes_key *keys, size_t n, struct hop_key *out, void *stream);
/* Bulk install: n raw host keys into slots first..first+n-1, expanded on the GPU. */
int hfv_key_add_batch(hfv_ctx *ctx, uint32_t first, const struct aes_key *keys, size_t n);

/* ---- synthetic traffic ---------------------------------------------------------------
 * Writes n synthetic 64 B SCION records with valid MACs under the
 * ctx's CURRENT key table and keysel (1/16 corrupted), records first_index.. of `seed`'s
 * stream.  stride >= 64, 16-byte aligned. */
int hfv_gen_records(hfv_ctx *ctx, void *recs, size_t stride, size_t n, uint64_t seed, uint64_t first_index,
                    void *stream);

/* ---- full BR per-packet path (config 4) -------------------------------------------------
 * border_router / process_packet (br/src/bpf/xdp.c:54-284) over a batch of Ethernet frames:
 * parse Eth/IPv4|IPv6/UDP/SCION (parser.h), AS ingress/egress processing with deferred HF
 * verification (path_processing.h), next-hop resolution, rewrite with incremental IP/UDP
 * checksums (rewrite.h), HF MAC verification (slot 0 of the ctx key table, xdp.c:259-274),
 * redirect decision and per-ingress-interface verdict counters (record_verdict).
 *
 * The BPF maps become one configuration struct.  bpf_fib_lookup (a kernel helper) is
 * replaced by a static next-hop table with longest-prefix match; an address with no route
 * behaves like BPF_FIB_LKUP_RET_NOT_FWDED.  Addresses and ports are in wire byte order. */
/* HFV_AF_*, HFV_BR_* limits and struct hfv_br_config with its entry types */
#include "hfv_br_config.h"

/* Install the router tables (copied; takes effect for batches enqueued afterwards).  Detaches
 * a pinned config attached with hfv_ctx_attach_brconfig. */
int hfv_br_set_config(hfv_ctx *ctx, const struct hfv_br_config *cfg);
/* The reference's ENABLE_HF_CHECK build switch (br/CMakeLists.txt:8,48-64) as a runtime
 * setting: enable = 0 skips the hop-field MAC check (defer_verify_hop_field and the MAC block
 * of border_router, path_processing.h:43-57 / xdp.c:259-274); default on.  Takes effect
 * for batches enqueued afterwards; survives hfv_br_set_config. */
int hfv_br_set_hf_check(hfv_ctx *ctx, int enable);
/* The reference's other build options (br/CMakeLists.txt:5-7, common.h:31-33), as a runtime
 * switch of the router: HFV_BR_NO_IPV4 / HFV_BR_NO_IPV6 compile that case of parse_underlay out
 * (parser.h:60,81: such frames fall to `default`, VERDICT_NOT_SCION, XDP_PASS), HFV_BR_NO_SCION_PATH
 * the standard SCION path type (parser.h:140: VERDICT_NOT_IMPLEMENTED).  Default 0: all built.
 * -EINVAL (tables unchanged) if the installed tables hold an address of a switched-off family,
 * which br-loader rejects (maps.cpp:68-80 "Border router configuration contains IPv4 address,
 * but IPv4 support is deactivated."); hfv_br_set_config checks the same against the options.
 * "Installed tables" are the ones last set by hfv_br_set_config or last loaded from an attached
 * pinned config (hfv_ctx_attach_brconfig); a republished pinned config carries the options
 * `hfv-loader attach` was given, and those replace the ones set here when it is reloaded. */
#define HFV_BR_NO_IPV4 1u
#define HFV_BR_NO_IPV6 2u
#define HFV_BR_NO_SCION_PATH 4u
int hfv_br_set_build_options(hfv_ctx *ctx, uint32_t disabled);
/* That check alone (for a loader): 0, or -EINVAL with br-loader's message in hfv_last_error(). */
int hfv_br_config_check_options(const struct hfv_br_config *cfg, uint32_t disabled);
/* ---- control plane: br-loader's configuration path ---------------------------------------
 * loadConfig + initializeMaps (br/src/config.cpp:212-262, maps.cpp:91-200, called by attachBr,
 * br_loader.cpp:88-151) for C hosts: the br-loader TOML file (`self`, `topology`,
 * `internal_interfaces`, br/README.md) and the SCION topology.json it names are parsed, each
 * local underlay address is resolved to the interface holding it, and the router tables are
 * built.  The next-hop table replaces bpf_fib_lookup (no kernel FIB on the GPU). */
struct hfv_br_ifaddr {             /* one address of the getifaddrs view (config.cpp:168-204) */
    char ifname[16];
    uint32_t ifindex;
    uint32_t family;               /* HFV_AF_INET / HFV_AF_INET6 */
    uint8_t addr[16];
};
struct hfv_br_next_hop {           /* one static FIB entry */
    uint32_t family;
    uint8_t prefix[16];
    uint32_t prefix_len;
    char ifname[16];
    uint8_t smac[6];
    uint8_t dmac[6];
    int32_t ret;                   /* BPF_FIB_LKUP_RET_*, 0 = forward */
};
/* ifaddrs NULL: this network namespace (getifaddrs + if_nametoindex).  self, listing and diag
 * (each nullable, NUL-terminated, truncated to their length) receive the BR name, the
 * "XDP Border Router ..." listing br-loader prints and br-loader's stderr messages (the error,
 * or the "WARNING: No interface has IP ..." lines).  Returns 0, -EINVAL for a configuration
 * br-loader rejects, -ENOSPC if the tables exceed the fixed capacity. */
int hfv_br_config_load(const char *toml_path, const struct hfv_br_ifaddr *ifaddrs, size_t n_ifaddrs,
                       const struct hfv_br_next_hop *hops, size_t n_hops, struct hfv_br_config *out,
                       char *self, size_t self_len, char *listing, size_t listing_len, char *diag, size_t diag_len);
/* The same with this namespace's interfaces, installed into ctx (hfv_br_set_config). */
int hfv_br_load_config(hfv_ctx *ctx, const char *toml_path, const struct hfv_br_next_hop *hops, size_t n_hops);
/* Pinned router tables, $HFV_PIN_DIR/<br>/br_config: `hfv-loader attach` publishes them (the
 * maps attachBr fills and pins), a data plane attached with hfv_ctx_attach_brconfig reloads
 * them whenever they are republished, at the next batch boundary.  Writers flock; readers see
 * whole tables (seqlock). */
int hfv_brconfig_path(const char *br, char *out, size_t len);
int hfv_brconfig_publish(const char *path, const struct hfv_br_config *cfg);
/* The same with the router's build options (HFV_BR_NO_*), which an attached ctx adopts. */
int hfv_brconfig_publish_opts(const char *path, const struct hfv_br_config *cfg, uint32_t disabled);
int hfv_brconfig_read(const char *path, struct hfv_br_config *cfg);
/* `hfv-loader detach`: marks the pinned tables detached (the file stays, so data planes that
 * attached it see the change): from their next batch an attached ctx passes every frame
 * (action XDP_PASS, verdict 0, egress -1, nothing counted), as the interface does once
 * detachBr removed the XDP program (br_loader.cpp:153-162); a later hfv_brconfig_publish
 * re-attaches.  -ENOENT if the file is missing or already detached.  Publish and read reject
 * tables whose counts exceed the fixed capacity (-EINVAL), and an attached ctx keeps its
 * previous tables (and fails that call) when it finds such a snapshot. */
int hfv_brconfig_detach(const char *path);
int hfv_ctx_attach_brconfig(hfv_ctx *ctx, const char *path);
/* Process n frames in place.  pkts: frame i at pkts + i*slot (slot % 8 == 0, >= 64);
 * len[i] its length (<= slot); ingress_ifindex[i] the receiving interface.  Outputs per
 * frame: action[i] = the XDP action returned (0 aborted, 1 drop, 2 pass, 4 redirect),
 * verdict[i] = the last enum verdict recorded, egress_ifindex[i] = redirect target or -1.
 * stats (nullable): u64 [HFV_BR_STATS_IFINDEX][2][HFV_BR_COUNTERS] (bytes, packets) to which
 * the batch's record_verdict calls are added.  All pointers are device pointers. */
int hfv_br_process(hfv_ctx *ctx, uint8_t *pkts, size_t slot, const uint16_t *len, const uint32_t *ingress_ifindex,
                   size_t n, uint8_t *action, uint8_t *verdict, int32_t *egress_ifindex, uint64_t *stats,
                   void *stream);
/* Config 5: frames in HOST memory (an RX ring of `slot`-byte slots).  Chunk by chunk, only
 * the first `window` bytes of each slot cross PCIe (host threads pack them into pinned
 * staging for one linear DMA each way and write the rewritten windows back; a ring
 * registered with hfv_host_register is instead read and written in place by the kernel over
 * PCIe), are processed
 * exactly as hfv_br_process does, and the rewritten window is copied back in place.  Frames
 * whose headers reach past the window are run again with the whole slot, so the result is
 * identical to hfv_br_process on the full frames.  len, ingress_ifindex, action, verdict,
 * egress_ifindex and stats (nullable, added to) are host arrays.  window: multiple of 8 with
 * 64 <= window <= slot, or 0 for 256 (capped at slot).  Synchronous: on return every output
 * is in host memory. */
int hfv_br_process_host(hfv_ctx *ctx, uint8_t *frames, size_t slot, const uint16_t *len,
                        const uint32_t *ingress_ifindex, size_t n, size_t window, uint8_t *action,
                        uint8_t *verdict, int32_t *egress_ifindex, uint64_t *stats);
/* ---- pinned verdict counters ----------------------------------------------------------
 * A file-backed port_stats_map (maps.h; pinned by br_loader.cpp:136-140, read by
 * `br-loader watch`, stats.cpp): $HFV_PIN_DIR/<br>/port_stats_map, same counter layout as the
 * `stats` buffer of hfv_br_process.  The data path adds its counters after a batch;
 * `hfv-loader watch <br> <iface>` prints them with per-second rates. */
int hfv_statsmap_path(const char *br, char *out, size_t len);
int hfv_statsmap_add(const char *path, const uint64_t *stats);   /* creates the map if needed */
int hfv_statsmap_read(const char *path, uint64_t *stats);

/* Page-lock and map an existing host buffer (e.g. the RX ring) for this ctx's GPU (at most 16
 * per ctx).  hfv_br_process_host on frames inside a registered buffer runs zero-copy: the
 * kernel reads the header windows across PCIe itself and writes back only rewritten rows
 * (`window` is then unused); registered len/ifindex/output arrays are used in place. */
int hfv_host_register(hfv_ctx *ctx, void *ptr, size_t bytes);
int hfv_host_unregister(hfv_ctx *ctx, void *ptr);

/* ---- config 5 in one process (br/evaluation/README.md:131-139) --------------------------
 * The reference measures its router with tcpreplay pushing gen_packets.py's frames into a veth
 * pair, the XDP program on the other end, and count_and_drop.py on the TX side.  hfv_loop_run
 * is that loop without the kernel's network stack: producer threads copy the frame list
 * (cycling, like `tcpreplay --loop`) into a registered RX ring of `chunks` x `chunk` slots,
 * the calling thread runs the router over each filled chunk (zero-copy like hfv_br_process_host,
 * or through HBM by DMA), `inflight` chunks at once on their own streams, and consumer
 * threads "transmit" redirected frames (count, bytes, optional digest) and drop the rest.
 * Producers and consumers run on the GPU's NUMA node. */
struct hfv_loop_config {
    const uint8_t *frames;       /* n_frames frames, frame_stride bytes apart */
    const uint16_t *lens;
    size_t n_frames, frame_stride;
    uint32_t rx_ifindex;         /* ingress interface of every frame */
    uint32_t slot;               /* ring slot bytes (multiple of 16, >= 128 and >= every len) */
    size_t chunk, chunks;        /* frames per chunk, chunks in the ring (>= 2) */
    uint64_t total;              /* frames to push through */
    int producers, consumers;    /* threads per side (0: 1) */
    int digest;                  /* 1: sum a 64-bit digest of every transmitted frame + egress */
    int inflight;                /* chunks on the GPU at once, each on its own stream (0: 2) */
    int dma;                     /* 0: the kernel reads/writes the ring over PCIe (zero-copy);
                                    1: each chunk is copied to HBM and back by the DMA engines;
                                    2: copied to HBM by DMA, the kernel writes the bytes it changes
                                       and its outputs straight back into the ring */
    uint64_t *stats;             /* nullable: per-ifindex verdict counters (added to), as hfv_br_process_host */
    /* Packet-socket I/O, the evaluation's veth loop (br/evaluation/veth_setup.bash,
     * README.md:131-139) -- NULL: the in-process frame list above.
     * rx_ifname: producers receive the frames tcpreplay pushes into the peer from an AF_PACKET
     *            socket on this interface (frames/lens/n_frames unused); `total` bounds them,
     *            and after idle_ms (0: 1000) without a frame the loop drains and returns.
     * tx_ifname: consumers send every redirected frame out of an AF_PACKET socket on this
     *            interface (count_and_drop.py counts them on the peer).
     * Needs CAP_NET_RAW; -EPERM (or the socket's errno) otherwise. */
    const char *rx_ifname, *tx_ifname;
    int idle_ms;
};
struct hfv_loop_stats {
    uint64_t rx_pkts, tx_pkts, tx_bytes, drop_pkts;
    uint64_t tx_digest;                         /* sum over transmitted frames (order-free) */
    uint64_t verdict_pkts[HFV_BR_COUNTERS];     /* frames per final verdict counter (verdict >> 3) */
    double seconds;                             /* wall time of the whole loop */
    double gpu_busy_s, gpu_wait_s;              /* router stage: inside hfv_br_process_host / waiting for RX */
    double producer_busy_s, consumer_busy_s;    /* summed over the threads of each side */
    uint64_t rx_truncated, tx_errors;           /* packet I/O: frames longer than a slot (dropped),
                                                   sends that failed after retries */
    int32_t numa_node;                          /* the GPU's NUMA node the threads were pinned to (-1: unknown) */
    uint32_t threads;                           /* producer + consumer threads */
    uint32_t threads_on_node;                   /* ... of which ended their work on a CPU of that node */
    uint32_t pad_;
};
int hfv_loop_run(hfv_ctx *ctx, const struct hfv_loop_config *cfg, struct hfv_loop_stats *out);

/* Same, then waits for the launch and returns its execution time (start/stop of the kernel
 * dispatch itself) in *kernel_ms.  For benchmarks. */
int hfv_br_process_timed(hfv_ctx *ctx, uint8_t *pkts, size_t slot, const uint16_t *len,
                         const uint32_t *ingress_ifindex, size_t n, uint8_t *action, uint8_t *verdict,
                         int32_t *egress_ifindex, uint64_t *stats, void *stream, float *kernel_ms);

/* ---- host helpers ---------------------------------------------------------------------- */
/* Scalar verify_hop_field on the host (SURVEY.md 8b v) for control-plane checks. */
int hfv_verify_macinput(const struct macinput *mi, uint64_t expected, const struct hop_key *key);
/* Base64 key decode with the reference's rules (exactly 24 chars, last two dropped). */
int hfv_decode_key_b64(const char *base64, struct aes_key *key);
/* Device memory helpers for C hosts without a framework allocator. */
int hfv_dev_alloc(hfv_ctx *ctx, size_t bytes, void **ptr);
int hfv_dev_free(hfv_ctx *ctx, void *ptr);
int hfv_memcpy_h2d(hfv_ctx *ctx, void *dst, const void *src, size_t bytes);
int hfv_memcpy_d2h(hfv_ctx *ctx, void *dst, const void *src, size_t bytes);
/* Writes a one-line description of the kernel variants the ctx launches. */
int hfv_ctx_describe(const hfv_ctx *ctx, char *buf, size_t len);
const char *hfv_last_error(void);
int hfv_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
