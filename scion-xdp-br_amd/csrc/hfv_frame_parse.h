// hfv_frame_parse.h -- where the current InfoField and HopField of an Ethernet frame lie:
// parse_underlay + parse_scion + parse_scion_path of the reference (br/src/bpf/parser.h:45-204)
// and nothing else of process_packet.  One function for the host (hfv_frame_locate,
// hfv_frames_host.cpp) and the device (k_extract_records, hfv_frames_kernel.hip), templated on
// the byte reader so that each side reads the frame its own way (plain bytes on the host, the
// staged LDS row on the GPU).
//
// The status is the verdict the router records when its parse fails at the same place
// (hfv_br_process: enum verdict, common.h:56-70), 0 when the parse succeeds.  The reference's
// quirks are kept as the router kernel keeps them (hfv_br_kernel.hip, parse_*):
//   - SC_GET_DL / SC_GET_SL mask the shifted haddr with 0x2 (scion.h:50,52), so a host address
//     counts 0 or 8 further bytes, whatever its real length;
//   - an IPv4 IHL below 5 wraps the option length (size_t) past 40: NOT_SCION;
//   - the info field after the current one is bounds-checked when CurrINF + 1 < the number of
//     info fields, although only its SegID would be used;
//   - a CurrINF that points past the info fields is no error: the "info field" then lies in the
//     hop fields, and the offsets say so.
// The router's build options (HFV_BR_NO_IPV4 / _IPV6 / _SCION_PATH, hfv_br_set_build_options) do
// NOT apply here: IPv4, IPv6 and the standard SCION path type are always parsed.
//
// A reader R provides  uint32_t u8(int off), u16(int off), u32(int off): the little-endian value
// of 1, 2, 4 frame bytes at `off` (16- and 32-bit fields sit at even offsets).  The parser calls
// them only for bytes it has bounds-checked against `end` first, as the BPF code must.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HFV_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HFV_HD inline
#endif

// HFV_MUT_PATHWALK = 9 (`make pathwalk`, listed in hfv_br_kernel.hip): num_inf taken as the index of the
// last non-zero SegLen plus one, in the frame kernels' builds only.  0 (the default): the reference's count.
#ifndef HFV_MUT_PATHWALK
#define HFV_MUT_PATHWALK 0
#endif

namespace hfv {

enum : int {
    kFrameOk = 0,               // HFV_FRAME_OK
    kFrameParseError = 17,      // HFV_FRAME_PARSE_ERROR    = VERDICT_PARSE_ERROR (drop | 2 << 3)
    kFrameNotScion = 26,        // HFV_FRAME_NOT_SCION      = VERDICT_NOT_SCION (pass | 3 << 3)
    kFrameNotImplemented = 34,  // HFV_FRAME_NOT_IMPLEMENTED = VERDICT_NOT_IMPLEMENTED (pass | 4 << 3)
};

struct FrameLoc {
    int status;
    uint32_t inf, hf;   // byte offsets of the current InfoField (8 B) / HopField (12 B); valid for status 0
    // 1: the parse stopped where the next header would pass `end` (a longer `end` might go on);
    // 0: it succeeded or stopped at a value (EtherType, IHL, IP protocol, SCION version, path
    // type), which no further byte changes.  Only the windowed kernel of hfv_verify_frames_host
    // reads it (to tell a header cut by its window from a verdict).
    uint32_t bound;
};

HFV_HD FrameLoc frame_bound_stop(FrameLoc loc)
{
    loc.bound = 1u;
    return loc;
}

// end: data_end - data, i.e. min(frame length, slot)
template <class R>
HFV_HD FrameLoc frame_locate(const R &r, int end)
{
    FrameLoc loc = {kFrameNotScion, 0u, 0u, 0u};
    // parse_underlay (parser.h:45-114)
    int off = 14;
    if (off > end) return frame_bound_stop(loc);
    const uint32_t proto = r.u16(12);
    if (proto == 0x0008u) {          // ETH_P_IP, as the little-endian load of the wire bytes
        off += 20;
        if (off > end) return frame_bound_stop(loc);
        const int skip = 4 * (int)(r.u8(14) & 0x0fu) - 20;
        if (skip < 0 || skip > 40) return loc;
        off += skip;
        if (r.u8(14 + 9) != 17u) return loc;
    } else if (proto == 0xdd86u) {   // ETH_P_IPV6
        off += 40;
        if (off > end) return frame_bound_stop(loc);
        if (r.u8(14 + 6) != 17u) return loc;
    } else {
        return loc;
    }
    off += 8;                        // UDP
    if (off > end) return frame_bound_stop(loc);
    // parse_scion (parser.h:118-148)
    loc.status = kFrameParseError;
    const int sc = off;
    off += 28;                       // common header + destination and source ISD-AS
    if (off > end) return frame_bound_stop(loc);
    if ((r.u8(sc) >> 4) != 0u) {
        loc.status = kFrameNotImplemented;
        return loc;
    }
    const uint32_t haddr = r.u8(sc + 9);
    off += 8 + 4 * (int)((haddr >> 2) & 0x2u) + 4 * (int)((haddr >> 6) & 0x2u);
    if (off > end) return frame_bound_stop(loc);
    if (r.u8(sc + 8) != 1u) {        // SC_PATH_TYPE_SCION
        loc.status = kFrameNotImplemented;
        return loc;
    }
    // parse_scion_path (parser.h:153-204)
    const int meta = off;
    off += 4;
    if (off > end) return frame_bound_stop(loc);
    const uint32_t h_meta = __builtin_bswap32(r.u32(meta));
    const uint32_t seg0 = (h_meta >> 12) & 0x3fu, seg1 = (h_meta >> 6) & 0x3fu, seg2 = h_meta & 0x3fu;
    const uint32_t num_inf = HFV_MUT_PATHWALK == 9 ? (seg2 ? 3u : seg1 ? 2u : seg0 ? 1u : 0u) : (seg0 > 0) + (seg1 > 0) + (seg2 > 0);
    const uint32_t curr_inf = (h_meta >> 30) & 0x03u, curr_hf = (h_meta >> 24) & 0x3fu;
    int inf = off + (int)curr_inf * 8;
    loc.inf = (uint32_t)inf;
    if (inf + 8 > end) return frame_bound_stop(loc);
    if (curr_inf + 1 < num_inf) {
        inf += 8;
        if (inf + 8 > end) return frame_bound_stop(loc);
    }
    const int hf = off + (int)num_inf * 8 + (int)curr_hf * 12;
    loc.hf = (uint32_t)hf;
    if (hf + 12 > end) return frame_bound_stop(loc);
    loc.status = kFrameOk;
    return loc;
}

}  // namespace hfv
