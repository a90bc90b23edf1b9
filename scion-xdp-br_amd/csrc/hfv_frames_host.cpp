// hfv_frames_host.cpp -- hfv_frame_locate: the frame parser (hfv_frame_parse.h) over one frame
// in host memory, the scalar counterpart of the extract kernel as hfv_verify_macinput is of the
// verify kernels.  No HIP dependency.
#include <errno.h>

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
