/*
 * hfv_br_config.h -- the router tables of the config-4 path (struct hfv_br_config), part of
 * scion_hfv.h.  They live in a header of their own, free of any other declaration, so that
 * code which cannot include scion_hfv.h (the reference-router test driver, oracle/ref_br.c,
 * whose reference headers define their own struct hop_key and AES_SBox) shares the one
 * definition.  Include scion_hfv.h, not this file, to use the library.
 */
#ifndef HFV_BR_CONFIG_H
#define HFV_BR_CONFIG_H

#include <stdint.h>

#define HFV_AF_INET 2
#define HFV_AF_INET6 10
#define HFV_BR_MAX_IFACES 16
#define HFV_BR_MAX_ROUTES 64
#define HFV_BR_MAX_TXPORTS 128
#define HFV_BR_COUNTERS 11         /* enum counter (common.h:40-53) */
#define HFV_BR_STATS_IFINDEX 64    /* counters kept for ingress ifindex < 64 */
#define HFV_BR_ACTION_RETRY 0xff   /* internal to the windowed host path; never returned */

struct hfv_br_int_iface {          /* int_iface_map: ifindex -> internal address (common.h:116-128) */
    uint32_t ifindex;
    uint32_t family;
    uint8_t addr[16];              /* IPv4 in addr[0..3] */
    uint8_t port[2];
    uint8_t pad[2];
};
struct hfv_br_ingress {            /* ingress_map: {dst addr, dst port, ifindex} -> AS interface id (common.h:73-84) */
    uint32_t ifindex;
    uint32_t family;
    uint8_t addr[16];
    uint8_t port[2];
    uint8_t pad[2];
    uint32_t ifid;
};
struct hfv_br_egress {             /* egress_map: ifid -> fwd_info (common.h:131-145) */
    uint32_t ifid;
    uint32_t fwd_external;         /* 1: ext_link {remote, local}, 0: sibling BR {remote = its internal address} */
    uint32_t family;
    uint8_t remote[16];
    uint8_t local[16];
    uint8_t remote_port[2];
    uint8_t local_port[2];
};
struct hfv_br_route {              /* replaces bpf_fib_lookup (fib_lookup.h:74-261) */
    uint32_t family;
    uint8_t prefix[16];
    uint32_t prefix_len;
    /* BPF_FIB_LKUP_RET_*: 0 success, 1-3 drop (FIB_LKUP_DROP), 4-8 pass (FIB_LKUP_PASS).
     * Contract for any other value (negative, or above 8): the router treats it as success --
     * it takes this route's MACs and ifindex and goes on, as the fall-through of the
     * reference's switch does (fib_lookup.h:100-124).  The kernel helper never returns such
     * a code, so the reference program gives no behaviour to compare with there; the CPU
     * checker and the GPU router agree with each other by this rule. */
    int32_t ret;
    uint32_t ifindex;              /* an interface index: below 2^31 (the reference returns it as an int) */
    uint8_t smac[6];
    uint8_t dmac[6];
};
struct hfv_br_config {
    uint32_t n_int_ifaces, n_ingress, n_egress, n_routes, n_tx_ports;
    struct hfv_br_int_iface int_ifaces[HFV_BR_MAX_IFACES];
    struct hfv_br_ingress ingress[HFV_BR_MAX_IFACES];
    struct hfv_br_egress egress[HFV_BR_MAX_IFACES];
    struct hfv_br_route routes[HFV_BR_MAX_ROUTES];
    uint32_t tx_ports[HFV_BR_MAX_TXPORTS];   /* tx_port_map: ifindices a redirect may target */
};

#endif /* HFV_BR_CONFIG_H */
