/*
 * bpf_helpers.h -- TEST INFRASTRUCTURE ONLY.  Host stand-in for the BPF helper header the
 * reference router includes, written from what the names mean: a section attribute that does
 * nothing on the host, a map-attribute macro that only has to declare a member, and the three
 * helpers the router calls, handed to the driver (oracle/ref_br.c).
 */
#ifndef HFV_REFBR_BPF_HELPERS_H
#define HFV_REFBR_BPF_HELPERS_H

#define SEC(name)
#define __uint(name, val) int (*name)[val]

void *refbr_map_lookup(const void *map, const void *key);
long refbr_redirect_map(const void *map, unsigned long long key, unsigned long long flags);
long refbr_fib_lookup(void *ctx, void *params, int plen, unsigned int flags);

#define bpf_map_lookup_elem(map, key) refbr_map_lookup((map), (key))
#define bpf_redirect_map(map, key, flags) refbr_redirect_map((map), (key), (flags))
#define bpf_fib_lookup(ctx, params, plen, flags) refbr_fib_lookup((ctx), (params), (plen), (flags))

#endif
