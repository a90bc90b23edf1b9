// hfv_frames_host.cpp -- hfv_frame_locate and hfv_frame_extract: the frame parser
// (hfv_frame_parse.h) over one frame in host memory, the scalar counterparts of the extract
// kernels as hfv_verify_macinput is of the verify kernels.  No HIP dependency.  Despite the name,
// hfv_verify_frames_host (frames in host memory through the GPU) is not here: it is one of the
// chunked host paths of hfv_host_path.cpp.
#include <errno.h>
#include <string.h>

#include "hfv_frame_parse.h"
#include "hfv_internal.h"

namespace {

struct HostReader {
    const uint8_t *p;
    uint32_t u8(int off) const { return p[off]; }
    uint32_t u16(int off) const { return (uint32_t)p[off] | (uint32_t)p[off + 1] << 8; }
    uint32_t u32(int off) const { return u16(off) | u16(off + 2) << 16; }
};

}  // namespace

extern "C" int hfv_frame_locate(const uint8_t *frame, size_t len, uint32_t *inf_off, uint32_t *hf_off)
{
    if (!frame || !inf_off || !hf_off) return hfv::fail(-EINVAL, "null argument");
    // no header field the parser reads lies past byte 1024 (the deepest hop field ends at
    // 14 + 60 + 8 + 28 + 16 + 4 + 3 * 8 + 64 * 12), so a longer frame parses as its first 64 KiB
    const int end = len > 65536 ? 65536 : (int)len;
    const hfv::FrameLoc loc = hfv::frame_locate(HostReader{frame}, end);
    *inf_off = loc.status == hfv::kFrameOk ? loc.inf : 0u;
    *hf_off = loc.status == hfv::kFrameOk ? loc.hf : 0u;
    return loc.status;
}

// hfv_frame_extract: what the extract kernels write into a frame's record, on the host.  The two
// fields of a frame that parses; for a frame from the internal link whose InfoField has Cons = 0,
// the HopField's MAC[0:2] folded into the SegID (see hfv_extract_records_rx).
extern "C" int hfv_frame_extract(const uint8_t *frame, size_t len, int from_internal, uint8_t inf[8], uint8_t hf[12])
{
    if (!frame || !inf || !hf) return hfv::fail(-EINVAL, "null argument");
    const int end = len > 65536 ? 65536 : (int)len;   // as hfv_frame_locate
    const hfv::FrameLoc loc = hfv::frame_locate(HostReader{frame}, end);
    memset(inf, 0, 8);
    memset(hf, 0, 12);
    if (loc.status != hfv::kFrameOk) return loc.status;
    memcpy(inf, frame + loc.inf, 8);
    memcpy(hf, frame + loc.hf, 12);
    if (from_internal && !(inf[0] & 1u)) {
        inf[2] ^= hf[6];
        inf[3] ^= hf[7];
    }
    return 0;
}
