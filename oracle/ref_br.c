/*
 * ref_br.c -- TEST INFRASTRUCTURE ONLY.
 *
 * Driver that runs the reference's own router program (br/src/bpf/xdp.c with the BPF build of
 * aes/src/aes.c, compiled in place as host code by the Makefile's `ref` rule, never copied) over
 * the frame slots the CPU checker and the GPU router work on.  It supplies what the kernel gives
 * a loaded XDP program: the maps, filled from struct hfv_br_config, and the three helpers that
 * oracle/refbr/bpf_helpers.h maps onto the functions below.
 *
 *   - Map lookups dispatch on the address of the map object the program names.
 *   - bpf_fib_lookup is the static next-hop table of the config (scion_hfv.h, "full BR per-packet
 *     path"): longest prefix on (family, dst), the first entry wins a tie, no route gives
 *     BPF_FIB_LKUP_RET_NOT_FWDED (4).  A route with ret 0 fills dmac, smac and ifindex; any
 *     other ret is returned with the parameters left alone, as the kernel helper does for its
 *     failure codes.  (For a ret outside 0..8 the program then goes on with the ingress ifindex
 *     and zero MACs, which is not what the checker and the GPU router define for such a value:
 *     the comparison with this build covers ret 0..8 only, see hfv_br_config.h.)
 *   - bpf_redirect_map answers XDP_REDIRECT for a key below 128 that is in tx_ports, else the
 *     low two bits of flags.
 *   - The scratchpad is zeroed before each frame (the checker's one documented deviation from
 *     a per-CPU map, hfv_br_oracle.c); refbr_set_carry(1) keeps it across frames instead.
 *   - record_verdict cannot be intercepted, so each frame gets a private zeroed port_stats: the
 *     verdict is action | idx << 3 with idx the non-zero counter index that was bumped (0 if
 *     none: only the fall-through after VERDICT_ABORT records twice, both times index 0); the
 *     private counters are then added to stats[ifindex] for ifindex < 64.
 *   - struct xdp_md carries 32-bit packet pointers, so each slot is copied into a buffer mapped
 *     below 4 GiB and copied back.
 *
 * The driver keeps global state (maps, scratchpad, packet buffer): it is single-threaded, one
 * refbr_process call at a time per loaded library.
 *
 * It must be compiled with the same ENABLE_* definitions as the program it drives, because
 * they change the layout of the map values.
 */
#define _GNU_SOURCE
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <sys/mman.h>

#include "common.h"                       /* the reference's: map value types, struct scratchpad */
#include "../include/hfv_br_config.h"

/* the program's map objects; only their addresses are used */
extern char scratchpad_map[], port_stats_map[], int_iface_map[], ingress_map[], egress_map[], tx_port_map[];
extern char AES_SBox[];
#ifdef ENABLE_HF_CHECK
extern char mac_key_map[];
#endif
int border_router(struct xdp_md *ctx);

static struct {
    const struct hfv_br_config *cfg;
    uint32_t n_int, n_ing, n_egr, n_routes, n_tx;
    struct int_iface int_ifaces[HFV_BR_MAX_IFACES];
    struct ingress_addr ingress[HFV_BR_MAX_IFACES];
    struct fwd_info egress[HFV_BR_MAX_IFACES];
    struct scratchpad pad;
    struct port_stats stats;
    const void *key0;
    const uint8_t *sbox;
    int carry;
    uint8_t *low;
    size_t low_size;
} g;

static uint32_t min_u32(uint32_t a, uint32_t b) { return a < b ? a : b; }

static void fill_int_iface(struct int_iface *o, uint32_t family, const uint8_t addr[16], const uint8_t port[2])
{
    memset(o, 0, sizeof *o);
    o->ip_family = family;
#ifdef ENABLE_IPV6
    memcpy(o->ipv6, addr, 16);            /* the IPv4 member shares the first four bytes */
#else
    memcpy(&o->ipv4, addr, 4);
#endif
    memcpy(&o->port, port, 2);
}

static void build_maps(const struct hfv_br_config *cfg)
{
    g.cfg = cfg;
    g.n_int = min_u32(cfg->n_int_ifaces, HFV_BR_MAX_IFACES);
    g.n_ing = min_u32(cfg->n_ingress, HFV_BR_MAX_IFACES);
    g.n_egr = min_u32(cfg->n_egress, HFV_BR_MAX_IFACES);
    g.n_routes = min_u32(cfg->n_routes, HFV_BR_MAX_ROUTES);
    g.n_tx = min_u32(cfg->n_tx_ports, HFV_BR_MAX_TXPORTS);
    for (uint32_t i = 0; i < g.n_int; ++i)
        fill_int_iface(&g.int_ifaces[i], cfg->int_ifaces[i].family, cfg->int_ifaces[i].addr, cfg->int_ifaces[i].port);
    for (uint32_t i = 0; i < g.n_ing; ++i) {
        const struct hfv_br_ingress *e = &cfg->ingress[i];
        struct ingress_addr *o = &g.ingress[i];
        memset(o, 0, sizeof *o);          /* the key is compared whole: the unused family stays zero */
#ifdef ENABLE_IPV4
        if (e->family == HFV_AF_INET) memcpy(&o->ipv4, e->addr, 4);
#endif
#ifdef ENABLE_IPV6
        if (e->family != HFV_AF_INET) memcpy(o->ipv6, e->addr, 16);
#endif
        memcpy(&o->port, e->port, 2);
        o->ifindex = (u16)e->ifindex;
    }
    for (uint32_t i = 0; i < g.n_egr; ++i) {
        const struct hfv_br_egress *e = &cfg->egress[i];
        struct fwd_info *o = &g.egress[i];
        memset(o, 0, sizeof *o);
        o->fwd_external = e->fwd_external;
        if (!e->fwd_external) {
            fill_int_iface(&o->sibling, e->family, e->remote, e->remote_port);
            continue;
        }
        o->link.ip_family = e->family;
#ifdef ENABLE_IPV6
        if (e->family != HFV_AF_INET) {
            memcpy(o->link.ipv6.remote, e->remote, 16);
            memcpy(o->link.ipv6.local, e->local, 16);
        }
#endif
#ifdef ENABLE_IPV4
        if (e->family == HFV_AF_INET) {
            memcpy(&o->link.ipv4.remote, e->remote, 4);
            memcpy(&o->link.ipv4.local, e->local, 4);
        }
#endif
        memcpy(&o->link.remote_port, e->remote_port, 2);
        memcpy(&o->link.local_port, e->local_port, 2);
    }
}

void *refbr_map_lookup(const void *map, const void *key)
{
    uint32_t k32;
    if (map == (const void *)ingress_map) {
        for (uint32_t i = 0; i < g.n_ing; ++i)
            if (memcmp(&g.ingress[i], key, sizeof(struct ingress_addr)) == 0) return (void *)&g.cfg->ingress[i].ifid;
        return NULL;
    }
    memcpy(&k32, key, 4);
    if (map == (const void *)scratchpad_map) return k32 == 0 ? &g.pad : NULL;
    if (map == (const void *)port_stats_map) return &g.stats;
    if (map == (const void *)AES_SBox) return k32 == 0 ? (void *)g.sbox : NULL;
#ifdef ENABLE_HF_CHECK
    if (map == (const void *)mac_key_map) return k32 == 0 ? (void *)g.key0 : NULL;
#endif
    if (map == (const void *)int_iface_map) {
        for (uint32_t i = 0; i < g.n_int; ++i)
            if (g.cfg->int_ifaces[i].ifindex == k32) return &g.int_ifaces[i];
        return NULL;
    }
    if (map == (const void *)egress_map) {
        for (uint32_t i = 0; i < g.n_egr; ++i)
            if (g.cfg->egress[i].ifid == k32) return &g.egress[i];
        return NULL;
    }
    return NULL;
}

long refbr_redirect_map(const void *map, unsigned long long key, unsigned long long flags)
{
    if (map == (const void *)tx_port_map && key < HFV_BR_MAX_TXPORTS)
        for (uint32_t i = 0; i < g.n_tx; ++i)
            if (g.cfg->tx_ports[i] == key) return XDP_REDIRECT;
    return (long)(flags & 3);
}

long refbr_fib_lookup(void *ctx, void *params, int plen, unsigned int flags)
{
    struct bpf_fib_lookup *p = params;
    uint8_t dst[16] = {0};
    uint32_t width = p->family == HFV_AF_INET ? 32 : 128;
    const struct hfv_br_route *best = NULL;
    (void)ctx, (void)plen, (void)flags;
    if (p->family == HFV_AF_INET) memcpy(dst, &p->ipv4_dst, 4);
    else memcpy(dst, p->ipv6_dst, 16);
    for (uint32_t i = 0; i < g.n_routes; ++i) {
        const struct hfv_br_route *r = &g.cfg->routes[i];
        if (r->family != p->family || r->prefix_len > width) continue;
        if (best && r->prefix_len <= best->prefix_len) continue;      /* first entry wins a tie */
        uint32_t whole = r->prefix_len / 8, rest = r->prefix_len % 8;
        if (memcmp(r->prefix, dst, whole)) continue;
        if (rest && ((r->prefix[whole] ^ dst[whole]) >> (8 - rest))) continue;
        best = r;
    }
    if (!best) return BPF_FIB_LKUP_RET_NOT_FWDED;
    if (best->ret != BPF_FIB_LKUP_RET_SUCCESS) return best->ret;
    memcpy(p->dmac, best->dmac, 6);
    memcpy(p->smac, best->smac, 6);
    p->ifindex = best->ifindex;
    return BPF_FIB_LKUP_RET_SUCCESS;
}

/* 1: keep the scratchpad from frame to frame (and call to call), as a per-CPU map does */
void refbr_set_carry(int on)
{
    g.carry = on;
    memset(&g.pad, 0, sizeof g.pad);
}

/* Which build this is: bit 0 ENABLE_IPV4, 1 ENABLE_IPV6, 2 ENABLE_SCION_PATH, 3 ENABLE_HF_CHECK */
int refbr_build_flags(void)
{
    int f = 0;
#ifdef ENABLE_IPV4
    f |= 1;
#endif
#ifdef ENABLE_IPV6
    f |= 2;
#endif
#ifdef ENABLE_SCION_PATH
    f |= 4;
#endif
#ifdef ENABLE_HF_CHECK
    f |= 8;
#endif
    return f;
}

/* Like orc_br_process; key0 is the 192-byte struct hop_key of key 0 (NULL: no key installed),
 * sbox the 256-byte AES S-box for the program's AES_SBox map.  Returns 0, or -1 when no packet
 * buffer below 4 GiB could be mapped. */
int refbr_process(uint8_t *pkts, size_t slot, const uint16_t *len, const uint32_t *ingress_ifindex, size_t n,
                  const void *cfg, const void *key0, uint8_t *action, uint8_t *verdict, int32_t *egress_ifindex,
                  uint64_t *stats, const uint8_t *sbox)
{
    size_t need = slot + 4096;            /* zeroed room after the slot */
    if (g.low_size < need) {
        if (g.low) munmap(g.low, g.low_size);
        g.low = mmap(NULL, need, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_32BIT, -1, 0);
        if (g.low == MAP_FAILED || (uintptr_t)g.low + need > 0xffffffffull) {
            g.low = NULL;
            g.low_size = 0;
            return -1;
        }
        g.low_size = need;
    }
    build_maps(cfg);
    g.key0 = key0;
    g.sbox = sbox;
    for (size_t i = 0; i < n; ++i) {
        size_t ln = len[i] <= slot ? len[i] : slot;
        if (!g.carry) memset(&g.pad, 0, sizeof g.pad);
        memset(&g.stats, 0, sizeof g.stats);
        memcpy(g.low, pkts + i * slot, slot);
        struct xdp_md ctx;
        memset(&ctx, 0, sizeof ctx);
        ctx.data = (u32)(uintptr_t)g.low;
        ctx.data_end = (u32)((uintptr_t)g.low + ln);
        ctx.ingress_ifindex = ingress_ifindex[i];
        int a = border_router(&ctx);
        memcpy(pkts + i * slot, g.low, slot);
        unsigned idx = 0;
        for (unsigned c = 1; c < COUNTER_ENUM_COUNT; ++c)
            if (g.stats.verdict_pkts[c]) idx = c;
        action[i] = (uint8_t)a;
        verdict[i] = (uint8_t)((a & 7) | idx << 3);
        egress_ifindex[i] = g.pad.egress_ifindex;
        if (stats && ingress_ifindex[i] < HFV_BR_STATS_IFINDEX) {
            uint64_t *row = stats + (size_t)ingress_ifindex[i] * 2 * HFV_BR_COUNTERS;
            for (unsigned c = 0; c < COUNTER_ENUM_COUNT; ++c) {
                row[c] += g.stats.verdict_bytes[c];
                row[HFV_BR_COUNTERS + c] += g.stats.verdict_pkts[c];
            }
        }
    }
    return 0;
}
