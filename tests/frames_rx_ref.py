"""Shared by test_frames_rx_host.py and test_gpu_frames_rx.py: the 4096-frame fuzz batches of
test_frames_host.py with the router oracle's verdicts, the two MAC-chaining rules of the reference
(br/src/bpf/path_processing.h) restated in Python, host-side records by hfv_frame_extract, and
the selection of the frames whose verdict is decided by the hop-field MAC.  Everything is built
once per process and left unchanged."""
import ctypes

import numpy as np

import br_fuzz as F
import br_topo as T
import orc
import scion_hfv as hfv

V = hfv.VERDICT
MAC = lambda k, m: orc.cmac(m, k)   # noqa: E731  checker-side AES for building test paths
BRS = ("br1", "br2", "br3")
CASES = [(br, v6) for br in BRS for v6 in (False, True)]
IDS = [f"{br}-{'ipv6' if v6 else 'ipv4'}" for br, v6 in CASES]

_CACHE = {}


def hop_inputs(v6):
    if ("hops", v6) not in _CACHE:
        brs = {b: T.OracleBR(T.br_config(b, v6)) for b in BRS}
        _CACHE[("hops", v6)] = F.hop_inputs(brs, v6, MAC)
    return _CACHE[("hops", v6)]


def internal_ifindices(cfg):
    return [int(cfg.int_ifaces[i].ifindex) for i in range(cfg.n_int_ifaces)]


# ---- the two rules, from the reference text -------------------------------------------------

def beta_ingress(inf: bytes, hf: bytes) -> int:
    """scion_as_ingress (path_processing.h:72-81): beta = ntohs(seg_id), and for a segment
    against construction direction beta ^= mac[1] | mac[0] << 8.  Returned in host order."""
    beta = inf[2] << 8 | inf[3]
    if not inf[0] & 1:                                   # !INF_GET_CONS
        beta ^= hf[7] | hf[6] << 8                       # hop field: flags, exp, ingress, egress, mac[6]
    return beta


def beta_egress(inf: bytes, hf: bytes) -> int:
    """scion_as_egress (path_processing.h:138-148): the hop field of a frame that came over the
    internal link (as_ing_ifid == INTERNAL_IFACE) is verified with beta = ntohs(seg_id) as it
    stands, whatever the Cons flag; the MAC goes into the SegID only afterwards."""
    return inf[2] << 8 | inf[3]


class Batch:
    """One fuzz batch (F.fuzz_batch(hops, br, v6, 4096, seed=100 + v6, payload_max=1500)) and what
    the tests compare against."""

    def __init__(self, br, v6):
        self.cfg = T.br_config(br, v6)
        self.frames, self.lens, self.ifidx = F.fuzz_batch(hop_inputs(v6), br, v6, 4096, seed=100 + v6,
                                                          payload_max=1500)
        n, slot = self.frames.shape
        _, self.verdict, _, _ = orc.br_process(self.frames.copy(), self.lens, self.ifidx, self.cfg,
                                               orc.hop_key(T.KEYS[1]))
        self.internal = np.isin(self.ifidx, internal_ifindices(self.cfg))
        # hfv_frame_locate (tests/test_frames_host.py checks it) and a gather: the frame's own fields
        L = hfv.lib()
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        base = self.frames.ctypes.data
        self.status = np.zeros(n, dtype=np.uint8)
        self.inf = np.zeros((n, 8), dtype=np.uint8)
        self.hf = np.zeros((n, 12), dtype=np.uint8)
        for i in range(n):
            self.status[i] = L.hfv_frame_locate(base + i * slot, min(int(self.lens[i]), slot), ctypes.byref(a),
                                                ctypes.byref(b))
            if self.status[i] == 0:
                self.inf[i] = self.frames[i, a.value:a.value + 8]
                self.hf[i] = self.frames[i, b.value:b.value + 12]
        # frames decided by the MAC: the router's verdict is SCION_FORWARD or INVALID_HF, and for a
        # frame from the internal link the AS-egress IFID (Cons ? ConsEgress : ConsIngress) has an
        # egress entry with fwd_external = 1 (internal to internal gets no MAC check, xdp.c:202-233)
        decided = np.isin(self.verdict, [V["SCION_FORWARD"], V["INVALID_HF"]])
        ext_ifid = {int(self.cfg.egress[i].ifid) for i in range(self.cfg.n_egress) if self.cfg.egress[i].fwd_external}
        cons = (self.inf[:, 0] & 1) == 1
        hf16 = self.hf.astype(np.uint32)
        egr_ifid = np.where(cons, hf16[:, 4] << 8 | hf16[:, 5], hf16[:, 2] << 8 | hf16[:, 3])
        self.cons = cons
        self.sel_ext = decided & ~self.internal
        self.sel_int = decided & self.internal & np.isin(egr_ifid, sorted(ext_ifid))
        self.sel = self.sel_ext | self.sel_int
        self.forward = self.verdict == V["SCION_FORWARD"]
        for x in (self.frames, self.lens, self.ifidx, self.verdict, self.internal, self.status, self.inf, self.hf,
                  self.sel, self.sel_ext, self.sel_int, self.cons, self.forward):
            x.setflags(write=False)


def batch(br, v6):
    if (br, v6) not in _CACHE:
        _CACHE[(br, v6)] = Batch(br, v6)
    return _CACHE[(br, v6)]


def frame_extract(frames, lens, internal):
    """(status u8[n], inf u8[n, 8], hf u8[n, 12]) by hfv_frame_extract per frame; `internal` is a
    bool per frame (or one for all)."""
    n, slot = frames.shape
    internal = np.broadcast_to(np.asarray(internal, dtype=bool), (n,))
    L = hfv.lib()
    status = np.zeros(n, dtype=np.uint8)
    inf = np.full((n, 8), 0xEE, dtype=np.uint8)
    hf = np.full((n, 12), 0xEE, dtype=np.uint8)
    base = frames.ctypes.data
    for i in range(n):
        rc = L.hfv_frame_extract(base + i * slot, min(int(lens[i]), slot), int(internal[i]), inf[i].ctypes.data,
                                 hf[i].ctypes.data)
        assert rc >= 0
        status[i] = rc
    return status, inf, hf


def records(inf, hf, inf_off=40, hf_off=48, stride=64):
    """Records of the given layout (the oracle's 64-byte one by default), zero elsewhere."""
    recs = np.zeros((len(inf), stride), dtype=np.uint8)
    recs[:, inf_off:inf_off + 8] = inf
    recs[:, hf_off:hf_off + 12] = hf
    return recs


def oracle_bits(status, inf, hf, hop_keys, valid, keysel):
    """orc.verify_records over the records, ANDed with status == 0: the bitmap words."""
    bits = orc.verify_records(records(inf, hf), hop_keys, valid, keysel)
    ok = np.zeros(len(bits) * 64, dtype=np.uint8)
    ok[:len(status)] = status == 0
    return bits & np.packbits(ok, bitorder="little").view(np.uint64)


def check_selection_counts(b, br):
    """The conditions of the issue that keep the router comparisons from passing vacuously."""
    if br in ("br1", "br2"):                             # br3 has the internal link only
        assert b.sel_ext.sum() >= 1000 and (b.verdict[b.sel_ext] == V["INVALID_HF"]).sum() >= 40
    if br in ("br2", "br3"):
        s = b.sel_int
        assert s.sum() >= 1000, s.sum()
        assert (s & ~b.cons).sum() >= 600, (s & ~b.cons).sum()
        assert (b.verdict[s] == V["INVALID_HF"]).sum() >= 40
