"""Frames addressed by descriptors into one buffer (hfv_verify_frames_desc): the UMEM builder, the
rule that says which descriptors are followed, the gather that defines what the call must compute,
and the corpora the tests run.  Shared by test_frames_desc.py (CPU) and test_gpu_frames_desc.py.
Plain numpy; nothing here calls the code under test.

A UMEM is a byte buffer with a GUARD-byte guard region in front of and behind the UMEM proper, which
is passed to the call as buf + umem_off.  layout() places given frames into it:

  inorder     2048-byte chunks, headroom 256 (AF_XDP's defaults): frame i at i * 2048 + 256
  permuted    the same chunks in a random order (a fill ring that recycled them)
  packed      frames back to back with no gap, so addr & 15 takes every value
  ("shift", k)   2048-byte chunks with every addr = k mod 16, k = 0..15
  ("tail", k, L) the frames packed, then the LAST frame cut to L < 128 bytes so that it starts at an
              addr = k mod 16 and ends exactly at umem_bytes (its 128-byte window would cross the end);
              the first frame lies at addr 0
  "odd"       packed, with the last frame cut by one byte where needed to make umem_bytes odd
  "one64"     a UMEM of exactly one 64-byte frame

`filler` (a byte value, or a byte pattern that is tiled) fills the guards and every gap; with
spill=True a cut frame's remaining bytes are written behind it all the same (into the gap or the back
guard), so that code which reads past len finds the whole frame there."""
import functools

import numpy as np

import br_shift as S
import br_topo as T
import frames_rx_ref as R

GUARD = 4096
CHUNK = 2048
HEADROOM = 256
MAX_LEN = 65535
BAD_DESC = 255
WIN = 128                          # the staged window of the frame kernels
DTYPE = np.dtype([("addr", "<u8"), ("len", "<u4"), ("ifindex", "<u4")])
KINDS = ("inorder", "permuted", "packed")
TAILS = ((0, 60), (1, 127), (7, 100), (8, 64), (15, 77))   # (addr & 15, cut length)


def desc_ok(addr, length, umem_bytes):
    """hfv_frame_desc_ok restated on Python integers (no wrap to think about)."""
    return 0 <= length <= MAX_LEN and 0 <= addr <= umem_bytes and length <= umem_bytes - addr


def fill(nbytes, filler):
    if isinstance(filler, (int, np.integer)):
        return np.full(nbytes, filler, dtype=np.uint8)
    pat = np.frombuffer(bytes(filler), dtype=np.uint8)
    return np.resize(pat, nbytes).copy()


def layout(frames, lens, kind, seed=0, filler=0, ifindex=None, spill=False):
    """(buf u8[GUARD + umem_bytes + GUARD], umem_off, umem_bytes, desc DTYPE[n]) for the frames
    frames[i, :min(lens[i], slot)]."""
    n, slot = frames.shape
    ln = np.minimum(np.asarray(lens, dtype=np.int64), slot)
    full = ln.copy()                                         # the bytes written with spill
    if kind in ("inorder", "permuted") or (isinstance(kind, tuple) and kind[0] == "shift"):
        assert int(ln.max()) + HEADROOM + 16 <= CHUNK
        order = np.arange(n)
        if kind == "permuted":
            order = np.random.default_rng(seed).permutation(n)
        addr = order * CHUNK + HEADROOM + (kind[1] if isinstance(kind, tuple) else 0)
        umem_bytes = n * CHUNK
    elif kind == "packed":
        addr = np.concatenate([[0], np.cumsum(ln)[:-1]])
        umem_bytes = int(ln.sum())
    elif isinstance(kind, tuple) and kind[0] == "tail":
        _, k, cut = kind
        assert cut < WIN and cut <= ln[-1] and n >= 2
        ln[-1] = cut
        addr = np.concatenate([[0], np.cumsum(ln)[:-1]])
        addr[-1] += (k - addr[-1]) % 16
        umem_bytes = int(addr[-1] + cut)
    elif kind == "odd":
        if ln.sum() % 2 == 0:
            ln[-1] -= 1
        addr = np.concatenate([[0], np.cumsum(ln)[:-1]])
        umem_bytes = int(ln.sum())
    elif kind == "one64":
        assert n == 1 and ln[0] >= 64
        ln[0] = 64
        addr = np.zeros(1, dtype=np.int64)
        umem_bytes = 64
    else:
        raise ValueError(kind)
    buf = fill(2 * GUARD + umem_bytes, filler)
    for i in range(n):
        w = int(full[i] if spill else ln[i])
        assert w <= ln[i] or w - ln[i] <= GUARD
        at = GUARD + int(addr[i])
        buf[at:at + w] = frames[i, :w]
    if spill:                                                # a spilled tail must not cover a later frame
        for i in range(n):
            at = GUARD + int(addr[i])
            buf[at:at + int(ln[i])] = frames[i, :int(ln[i])]
    desc = np.zeros(n, dtype=DTYPE)
    desc["addr"], desc["len"] = addr, ln
    desc["ifindex"] = 0 if ifindex is None else ifindex
    return buf, GUARD, umem_bytes, desc


def plant(buf, umem_off, addr, frame):
    """Write `frame` where a descriptor's addr points, taken modulo 2^64 as the device adds it to the
    pointer: into the guards for the bad addresses the tests use."""
    a = int(addr)
    if a >= 1 << 63:
        a -= 1 << 64
    at = umem_off + a
    assert 0 <= at and at + len(frame) <= len(buf), "outside the test's allocation"
    buf[at:at + len(frame)] = np.frombuffer(bytes(frame), dtype=np.uint8)


def slot_copy(buf, umem_off, umem_bytes, desc, slot=None):
    """The equivalence the call is held to, as a gather: (frames u8[n, slot], lens u16[n], ifindex
    u32[n], valid bool[n]).  Valid frames are copied to row i with lens[i] = len; the rows of invalid
    descriptors stay zero with length 0."""
    n = len(desc)
    valid = np.array([desc_ok(int(d["addr"]), int(d["len"]), umem_bytes) for d in desc], dtype=bool)
    longest = int(desc["len"][valid].max()) if valid.any() else 0
    if slot is None:
        slot = max(64, -(-longest // 8) * 8)
    assert slot % 8 == 0 and slot >= 64 and slot >= longest
    frames = np.zeros((n, slot), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint16)
    for i in np.nonzero(valid)[0]:
        a, w = umem_off + int(desc["addr"][i]), int(desc["len"][i])
        frames[i, :w] = buf[a:a + w]
        lens[i] = w
    return frames, lens, np.array(desc["ifindex"], dtype=np.uint32), valid


def placement(desc, umem_bytes):
    """What a corpus exercises, counted: (n, frames per addr & 15 over the valid descriptors, valid
    frames whose 128-byte window would cross the UMEM end, valid frames at addr 0, descriptors that
    repeat an earlier (addr, len), valid descriptors whose bytes overlap those of a descriptor at
    another addr, invalid descriptors)."""
    n = len(desc)
    addr = [int(a) for a in desc["addr"]]
    ln = [int(x) for x in desc["len"]]
    valid = [desc_ok(a, w, umem_bytes) for a, w in zip(addr, ln)]
    mod16 = [0] * 16
    cross = addr0 = 0
    for a, w, v in zip(addr, ln, valid):
        if v:
            mod16[a & 15] += 1
            cross += a + WIN > umem_bytes
            addr0 += a == 0
    seen, repeated = set(), 0
    for a, w in zip(addr, ln):
        repeated += (a, w) in seen
        seen.add((a, w))
    spans = sorted({(a, a + w) for a, w, v in zip(addr, ln, valid) if v and w})
    hit = set()
    reach, owner = -1, None
    for s in spans:
        if s[0] < reach:
            hit.add(s)
            hit.add(owner)
        if s[1] > reach:
            reach, owner = s[1], s
    overlapping = sum(1 for a, w, v in zip(addr, ln, valid) if v and w and (a, a + w) in hit)
    return (n, tuple(mod16), cross, addr0, repeated, overlapping, n - sum(valid))


# ---- sources and corpora ------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def source(name):
    """(frames u8[n, 256], lens u16[n], ifindex u32[n], br, v6) by name: "fuzz_<br>_<v6>" (the six
    4096-frame fuzz batches of frames_rx_ref), "corpus_<v6>_<br>" and "sweep_<v6>" (br_shift's
    window-edge corpus and truncation sweep)."""
    if name.startswith("fuzz_"):
        _, br, v6 = name.split("_")
        b = R.batch(br, bool(int(v6)))
        return b.frames, b.lens, b.ifidx, br, bool(int(v6))
    for leg, br, v6, frames, lens, ifidx in S.fixture_legs():
        if leg == name:
            return frames, lens, ifidx, br, v6
    raise KeyError(name)


FUZZ = tuple("fuzz_%s_%d" % (br, v6) for br, v6 in R.CASES)
SHIFT = tuple("corpus_%d_%s" % (v6, br) for v6 in (0, 1) for br in S.BRS) + ("sweep_0", "sweep_1")
SHIFT_CORPUS = SHIFT[:6]


def internal_set(name):
    _, _, _, br, v6 = source(name)
    return R.internal_ifindices(T.br_config(br, v6))


def kind_name(kind):
    return kind if isinstance(kind, str) else "_".join(str(x) for x in kind)


@functools.lru_cache(maxsize=None)
def corpus(name, kind, filler=0):
    """layout() of a source, with the source's ifindices in the descriptors; read-only."""
    frames, lens, ifidx, _, _ = source(name)
    out = layout(frames, lens, kind, seed=len(name), filler=filler, ifindex=ifidx)
    out[0].setflags(write=False)
    out[3].setflags(write=False)
    return out


# every (source, kind) the GPU module runs as a whole corpus; the tail, odd and one64 layouts are
# built from a few frames in the tests themselves (edge_cases)
CORPORA = tuple((s, k) for s in FUZZ + SHIFT for k in KINDS)
SHIFTED = tuple((s, ("shift", k)) for s in SHIFT_CORPUS for k in range(16))   # the alignment sweep


def edge_cases(frames, lens, ifidx, filler=0, spill=False):
    """[(name, buf, umem_off, umem_bytes, desc)]: the UMEM edges, from at least 8 frames of which the
    last one is the frame that gets cut."""
    out = []
    for k, cut in TAILS:
        out.append(("tail_%d_%d" % (k, cut),) + layout(frames, lens, ("tail", k, cut), filler=filler, ifindex=ifidx,
                                                       spill=spill))
    out.append(("odd",) + layout(frames, lens, "odd", filler=filler, ifindex=ifidx, spill=spill))
    out.append(("one64",) + layout(frames[-1:], lens[-1:], "one64", filler=filler, ifindex=ifidx[-1:], spill=spill))
    return out


@functools.lru_cache(maxsize=None)
def edge_source(count=9):
    """(frames, lens, ifindex) of the first `count` frames of the br1 IPv4 fuzz batch that come from
    an external interface and that the router oracle forwards: they pass the hop-field check under
    the AS key, every one is longer than 128 bytes, and the last one is the frame the tail layouts cut."""
    b = R.batch("br1", False)
    idx = np.nonzero(b.sel_ext & b.forward)[0][:count]
    assert len(idx) == count and (b.lens[idx] > WIN).all()
    return np.array(b.frames[idx]), np.array(b.lens[idx]), np.array(b.ifidx[idx])


def repeat_case(frames, lens, ifidx, other_ifindex):
    """(buf, umem_off, umem_bytes, desc): two frames A and B packed; 64 descriptors of A whose ifindex
    alternates between A's own and `other_ifindex`, then descriptors that overlap: A with B's bytes as
    its payload, B, the bytes of A from offset 7 on, and A again cut inside B."""
    buf, off, nbytes, d = layout(frames[:2], lens[:2], "packed", ifindex=ifidx[:2])
    la, lb = int(d["len"][0]), int(d["len"][1])
    desc = np.zeros(68, dtype=DTYPE)
    desc["addr"][:64], desc["len"][:64] = 0, la
    desc["ifindex"][:64] = np.where(np.arange(64) % 2 == 0, int(ifidx[0]), other_ifindex)
    desc[64] = (0, la + lb, ifidx[0])
    desc[65] = (la, lb, ifidx[1])
    desc[66] = (7, la - 7, ifidx[0])
    desc[67] = (0, la + lb // 2, ifidx[0])
    return buf, off, nbytes, desc
