"""The kernels of csrc/hfv_aux_kernels.hip -- k_macinputs behind hfv_verify_macinputs and
hfv_cmac_tags, k_count_verdicts behind hfv_verdict_counters, k_gen_records behind hfv_gen_records,
k_expand_keys behind hfv_expand_keys and hfv_key_add_batch -- on the corpora of tests/aux_edges.py:
every round of their grid-stride loops, every tail, the edges of the key validity words, the
index edges of the generator, counters that carry out of bit 31, every carry of the K1 doubling.
Everything expected comes from the CPU checker (judged on the host; nothing from the library).
Integer work: every comparison is bit-exact.

Where a wave must run many rounds the launch is capped at 1, 2 or 3 blocks with the test build's
hfv_debug_aux_grid, so those tests run in a child process on lib/libscionhfv_test.so
(conftest.rerun_on_test_build): a round then holds 512, 1024 or 1536 items and the sizes of
aux_edges.sizes(B) give a wave up to six rounds, with a partial tile in a late one
(tests/test_aux_edges.py pins the placement).  The real-grid tests need no hook: two full rounds,
three tiles and 17 items of the grid the launcher chooses for the device's CU count.

Outputs lie between guard words or rows and are pre-filled with a pattern: the guards survive, the
bits at and past n are zero, gap bytes of a stride and rows past n keep their fill.

A mutant build (make auxedge) already has the hook: run it with
HFV_LIB=lib/libscionhfv_auxedgeN.so HFV_TEST_BUILD_CHILD=1, which runs every test body in place.

What fails on which wrong-step library (make auxedge; measured on an MI355X, every failure an
assertion, the other tests of this module pass):
  1  verdict words of later rounds land on the first round's: test_capped_verify_macinputs (first
     at n = 513 under one block: the word of round 2 is missing and a bit past n is set),
     test_real_grid_macinputs[slot0, index]
  2  an invalid slot's tag is not zeroed: test_slot_edges[E, E'] (520 and 120 tag rows)
  3  `expected` masked to 48 bits: test_slot_edges[E, E'] (the entries with one of bits 48..63 set pass)
  4  the pass bit from the first round's word: test_capped_verdict_counters[default, compact] (first
     at n = 513 under one block), test_real_grid_verdict_counters[default, compact]
  5  4 * i in 32 bits: test_capped_gen_records[0, 1] (first at the window starting at 2^32 - 3),
     test_real_grid_gen_records[0, 1]
  6  rows at j * 64: test_capped_gen_records[0, 1] (gap bytes of stride 80 written),
     test_real_grid_gen_records[1] (stride 80; [0] runs at stride 64 and passes)
The older tests of these kernels -- test_gpu_parity.py::test_golden_tags_and_verdicts,
test_generator_matches_oracle and test_verdict_counters, test_gpu_hf_bits.py::test_macinputs_and_tags
and test_verdict_counters, 14 cases -- were run once on each of the six libraries and all pass on
all six: none of them reaches a second round, an invalid slot's tag, bits 48..63 of `expected`, an
index past 2^30 or a stride above 64.

Measured on an MI355X: the module's 19 cases take 26 s of wall time (pytest's figure), of which
the six capped tests, each a child process on the test build, take 3.5 to 4.4 s apiece
(test_capped_gen_records[1]: 4.4 s, the slowest; its 585 launches) and every other case under 0.3 s.
"""
import numpy as np
import pytest

import aux_edges as AE
import orc
import scion_hfv as hfv
from conftest import rerun_on_test_build

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 0x5A5A5A5A5A5A5A5A
FILL = 0xC3C3C3C3C3C3C3C3
EINVAL = -22

_DEV = {}


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def cached(key, make):
    """Read-only device copies of the corpora, uploaded once."""
    if key not in _DEV:
        _DEV[key] = make()
    return _DEV[key]


def num_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    yield c
    c.synchronize()
    c.close()


@pytest.fixture()
def cap():
    """Sets the block cap of the aux launches; the default geometry is back afterwards."""
    try:
        yield hfv.Ctx.debug_aux_grid
    finally:
        if hasattr(hfv.lib(), "hfv_debug_aux_grid"):   # (the parent process runs on the product library)
            hfv.Ctx.debug_aux_grid(0)


def install(ctx, valid=None):
    """The full table, then every slot outside `valid` removed again."""
    raw = AE.full_table()[0]
    for k in range(256):
        ctx.key_add(k, raw[16 * k:16 * k + 16])
    if valid is not None:
        for k in range(256):
            if k not in valid:
                ctx.key_remove(k)


def words_arena(nw):
    """guard, guard, nw words of fill, guard, guard"""
    a = np.full(nw + 4, GUARD, dtype=np.uint64)
    a[2:2 + nw] = FILL
    return dev(a.view(np.int64))


def check_words(t, n, want, what):
    got = host(t).view(np.uint64)
    nw = (n + 63) // 64
    assert (got[:2] == GUARD).all() and (got[2 + nw:] == GUARD).all(), ("guard written", what)
    words = got[2:2 + nw]
    if n % 64:
        assert int(words[-1]) >> (n % 64) == 0, ("a bit at or past n is set", what)
    bad = np.nonzero(words != want)[0]
    assert not len(bad), (what, "%d bad words, first %d: got %016x want %016x" % (
        len(bad), bad[0], int(words[bad[0]]), int(want[bad[0]])))


def rows_arena(n, width):
    """two guard rows, n rows of fill, two guard rows"""
    a = np.full((n + 4, width), GUARD & 0xff, dtype=np.uint8)
    a[2:2 + n] = FILL & 0xff
    return dev(a)


def check_rows(t, n, want, what):
    got = host(t)
    assert (got[:2] == GUARD & 0xff).all() and (got[2 + n:] == GUARD & 0xff).all(), ("guard row written", what)
    bad = np.nonzero((got[2:2 + n] != want).any(axis=1))[0]
    assert not len(bad), (what, "%d bad rows, first %d: got %s want %s" % (
        len(bad), bad[0], got[2 + bad[0]].tobytes().hex(), want[bad[0]].tobytes().hex()))


def mac_dev(N, use):
    mi, kidx, _, exp = AE.mac_corpus(N)[use]
    return cached(("mac", N, use), lambda: (dev(mi), dev(kidx), dev(exp.view(np.int64))))


def run_verify(ctx, N, n, use, what):
    mi, kidx, exp = mac_dev(N, use)
    arena = words_arena((n + 63) // 64)
    ctx.verify_macinputs(mi, exp, n, arena[2:], key_index=kidx if use else None)
    check_words(arena, n, AE.want_words(n), ("verify_macinputs", n, "index" if use else "slot 0") + what)


def run_tags(ctx, N, n, use, what):
    mi, kidx, _ = mac_dev(N, use)
    arena = rows_arena(n, 16)
    ctx.cmac_tags(mi, n, arena[2:], key_index=kidx if use else None)
    check_rows(arena, n, AE.mac_corpus(N)[use][2][:n], ("cmac_tags", n, "index" if use else "slot 0") + what)


# ---- k_macinputs ------------------------------------------------------------------------------

def test_capped_verify_macinputs(request, ctx, cap):
    """Every size under 1, 2 and 3 blocks, with and without a key index, under both keysels (the
    kernel ignores keysel: both give the designed bitmap)."""
    if rerun_on_test_build(request):   # uses a test hook: runs on lib/libscionhfv_test.so
        return
    install(ctx)
    for keysel in (0, 1):
        ctx.set_keysel(keysel)
        for B in AE.CAPS:
            cap(B)
            for n in AE.sizes(B):
                for use in (False, True):
                    run_verify(ctx, AE.N_CAPPED, n, use, ("B=%d" % B, "keysel %d" % keysel))


def test_capped_cmac_tags(request, ctx, cap):
    """The same launches in tag mode: every tag is the checker's."""
    if rerun_on_test_build(request):
        return
    install(ctx)
    for keysel in (0, 1):
        ctx.set_keysel(keysel)
        for B in AE.CAPS:
            cap(B)
            for n in AE.sizes(B):
                for use in (False, True):
                    run_tags(ctx, AE.N_CAPPED, n, use, ("B=%d" % B, "keysel %d" % keysel))


@pytest.mark.parametrize("use", [False, True], ids=["slot0", "index"])
def test_real_grid_macinputs(ctx, use):
    """Two full rounds, three tiles and 17 items on the launcher's own grid: the designed bitmap
    under both keysels, and every tag against the checker's bulk call (bytes 0..5 of a tag are the
    MAC the verify leg compares)."""
    n = AE.n_real("macinputs", num_cus())
    assert AE.placement("macinputs", n, num_cus()) == (3, True)
    install(ctx)
    for keysel in (0, 1):
        ctx.set_keysel(keysel)
        run_verify(ctx, n, n, use, ("real grid", "keysel %d" % keysel))
    run_tags(ctx, n, n, use, ("real grid",))
    _DEV.pop(("mac", n, use))


@pytest.mark.parametrize("name", sorted(AE.EDGE_TABLES))
def test_slot_edges(ctx, name):
    """Tables E and E': the five classes of `expected` on every slot next to an edge of a validity
    word.  Only a true MAC in a valid slot passes (a removed slot fails even a zero `expected`, and
    its old key's MAC), bits 48..63 of `expected` count, and a removed slot's tag is 16 zero bytes."""
    install(ctx, AE.EDGE_TABLES[name])
    mi, ks, exp, cls, want, tags, _ = AE.edge_corpus(name)
    n = len(mi)
    dmi, dks, dexp = dev(mi), dev(ks), dev(exp.view(np.int64))
    for keysel in (0, 1):
        ctx.set_keysel(keysel)
        arena = words_arena((n + 63) // 64)
        ctx.verify_macinputs(dmi, dexp, n, arena[2:], key_index=dks)
        torch.cuda.synchronize()
        got = np.unpackbits(host(arena).view(np.uint8)[16:16 + 8 * ((n + 63) // 64)], bitorder="little")[:n].astype(bool)
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (name, "keysel %d" % keysel, [(int(ks[i]), AE.CLASSES[cls[i]], bool(got[i])) for i in bad[:8]])
        check_words(arena, n, AE.pack(want), (name, "keysel %d" % keysel))
        rows = rows_arena(n, 16)
        ctx.cmac_tags(dmi, n, rows[2:], key_index=dks)
        check_rows(rows, n, tags, (name, "tags", "keysel %d" % keysel))


# ---- k_count_verdicts -------------------------------------------------------------------------

LAYOUTS = {"default": (40, 48, 64), "compact": (0, 8, 24)}


def count_dev(N, layout):
    recs = AE.count_records(N)
    return cached(("count", N, layout), lambda: dev(recs if layout == "default" else AE.compact(recs)))


def run_count(ctx, N, n, layout, what, twice=False):
    recs = AE.count_records(N)
    pre = AE.count_preload()
    arena = np.full((260, 2), GUARD, dtype=np.uint64)
    arena[2:258] = pre
    t = dev(arena.view(np.int64))
    bits = dev(AE.want_words(n).view(np.int64))
    want = AE.count_want(recs, n, pre)
    for call in range(2 if twice else 1):
        ctx.verdict_counters(count_dev(N, layout), n, bits, t[2:], stride=LAYOUTS[layout][2])
        got = host(t).view(np.uint64)
        assert (got[:2] == GUARD).all() and (got[258:] == GUARD).all(), ("guard written", what)
        bad = np.argwhere(got[2:258] != want)
        assert not len(bad), (what, n, "call %d" % call, "%d bad counters, first %s: got %d want %d" % (
            len(bad), tuple(bad[0]), int(got[2:258][tuple(bad[0])]), int(want[tuple(bad[0])])))
        want = AE.count_want(recs, n, want)   # a second call adds again


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_capped_verdict_counters(request, ctx, cap, layout):
    """Every size under 1, 2 and 3 blocks against np.add.at, from preloaded counters (those at
    2^32 - 3 end at exactly 2^32 - 3 + k); a second call on the largest size adds again."""
    if rerun_on_test_build(request):
        return
    ctx.set_record_layout(*LAYOUTS[layout][:2])
    for B in AE.CAPS:
        cap(B)
        for n in AE.sizes(B):
            run_count(ctx, AE.N_CAPPED, n, layout, (layout, "B=%d" % B), twice=n == AE.sizes(B)[-1])


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_real_grid_verdict_counters(ctx, layout):
    n = AE.n_real("count", num_cus())
    assert AE.placement("count", n, num_cus()) == (3, True)
    ctx.set_record_layout(*LAYOUTS[layout][:2])
    run_count(ctx, n, n, layout, (layout, "real grid"), twice=True)
    _DEV.pop(("count", n, layout))


# ---- k_gen_records ----------------------------------------------------------------------------

def gen_expect(n, first, keysel):
    if first in AE.gen_firsts(0)[:4]:                 # the fixed edges: prefixes of one run of the twin
        return AE.gen_want(AE.N_CAPPED, first, keysel)[:n]
    return AE.gen_want(n, first, keysel)


def run_gen(ctx, n, first, stride, keysel, what, want=None):
    buf = torch.full((n + 2, stride), FILL & 0xff, dtype=torch.uint8, device=DEV)
    ctx.gen_records(buf, n, AE.GEN_SEED, first_index=first, stride=stride)
    got = host(buf)
    want = gen_expect(n, first, keysel) if want is None else want
    where = what + ("n=%d" % n, "first %#x" % first, "stride %d" % stride)
    assert (got[n:] == FILL & 0xff).all(), ("a row past n was written", where)
    assert (got[:n, 64:] == FILL & 0xff).all(), ("gap bytes of the stride were written", where)
    bad = np.nonzero((got[:n, :64] != want).any(axis=1))[0]
    assert not len(bad), (where, "%d bad records, first %d: got %s want %s" % (
        len(bad), bad[0], got[bad[0], :64].tobytes().hex(), want[bad[0]].tobytes().hex()))


@pytest.mark.parametrize("keysel", [0, 1])
def test_capped_gen_records(request, ctx, cap, keysel):
    """Every size under 1, 2 and 3 blocks, from every first-index edge, at every stride: byte for
    byte the CPU twin's records."""
    if rerun_on_test_build(request):
        return
    install(ctx)
    ctx.set_keysel(keysel)
    for B in AE.CAPS:
        cap(B)
        for n in AE.sizes(B):
            for first in AE.gen_firsts(n):
                for stride in AE.GEN_STRIDES:
                    run_gen(ctx, n, first, stride, keysel, ("keysel %d" % keysel, "B=%d" % B))


@pytest.mark.parametrize("keysel", [0, 1])
def test_real_grid_gen_records(ctx, keysel):
    """Two full rounds and a ragged end on the launcher's own grid, the window crossing 2^32."""
    n = AE.n_real("gen", num_cus())
    assert AE.placement("gen", n, num_cus()) == (3, True)
    install(ctx)
    ctx.set_keysel(keysel)
    first = (1 << 32) - AE.round_items(2 * num_cus()) - 3
    want = orc.gen_records(n, AE.full_table()[1], keysel, seed=AE.GEN_SEED, first_index=first)
    run_gen(ctx, n, first, 80 if keysel else 64, keysel, ("keysel %d" % keysel, "real grid"), want=want)


# ---- k_expand_keys ----------------------------------------------------------------------------

def test_expand_keys():
    """1, 255, 256 and 257 keys (a block holds 256), the all-zero and all-ones keys and one key per
    carry class of the K1 doubling among them, on a stream of the caller's: every hop_key row is
    the checker's, between guard rows."""
    raw, hk = AE.expand_keys()
    with hfv.Ctx(0) as ctx:
        s = torch.cuda.Stream()
        for n in AE.EXPAND_N:
            with torch.cuda.stream(s):
                keys = dev(raw[:n])
                out = rows_arena(n, 192)
                ctx.expand_keys(keys, n, out[2:], stream=s)
            s.synchronize()
            check_rows(out, n, hk[:n], ("expand_keys", n))


def golden_verifies(ctx, g):
    n = len(g["records"])
    ctx.set_keysel(1)
    arena = words_arena((n + 63) // 64)
    ctx.verify_records(dev(g["records"]), n, arena[2:])
    check_words(arena, n, g["pass_bits"], ("the 256-key golden",))


@pytest.mark.parametrize("first", [0, 1, 200])
def test_key_add_batch_reaches_slot_255(first):
    """hfv_key_add_batch from `first` up to exactly slot 255: every slot reads back as the
    checker's hop_key and the 256-key golden verifies; one key more is refused and changes nothing."""
    g = orc.load_golden("hf_ifid256.npz")
    raw = g["raw_keys"].reshape(-1).tobytes()
    assert len(raw) == 256 * 16
    with hfv.Ctx(0) as ctx:
        for k in range(first):
            ctx.key_add(k, raw[16 * k:16 * k + 16])
        ctx.key_add_batch(first, raw[16 * first:])
        for k in range(256):
            assert ctx.key_get(k) == orc.hop_key(raw[16 * k:16 * k + 16]) == g["hop_keys"][k].tobytes(), k
        golden_verifies(ctx, g)
        other = AE.full_table()[0]
        for f, nk in ((first, 257 - first), (1, 256), (255, 2), (256, 1)):
            with pytest.raises(hfv.HfvError) as e:
                ctx.key_add_batch(f, other[:16 * min(nk, 256)] + other[:16 * max(0, nk - 256)])
            assert e.value.code == EINVAL, (f, nk)
        for k in range(256):
            assert ctx.key_get(k) == g["hop_keys"][k].tobytes(), k
        golden_verifies(ctx, g)


# ---- argument checks that need a ctx ------------------------------------------------------------

def refused(fn, *a, **kw):
    with pytest.raises(hfv.HfvError) as e:
        fn(*a, **kw)
    assert e.value.code == EINVAL


def test_argument_checks(ctx):
    n = 64
    mi, kidx, exp = mac_dev(AE.N_CAPPED, True)
    bits, tags = words_arena(1), rows_arena(n, 16)
    counters = torch.zeros((256, 2), dtype=torch.int64, device=DEV)
    recs = torch.full((n, 128), FILL & 0xff, dtype=torch.uint8, device=DEV)
    refused(ctx.verify_macinputs, mi.data_ptr() + 8, exp, n, bits[2:])
    refused(ctx.verify_macinputs, mi, exp.data_ptr() + 4, n, bits[2:])
    refused(ctx.verify_macinputs, mi, exp, n, bits.data_ptr() + 4)
    refused(ctx.cmac_tags, mi.data_ptr() + 8, n, tags[2:])
    refused(ctx.cmac_tags, mi, n, tags.data_ptr() + 8)
    refused(ctx.verdict_counters, recs, n, bits[2:], counters.data_ptr() + 4, stride=128)
    refused(ctx.gen_records, recs, n, 1, stride=48)
    refused(ctx.gen_records, recs, n, 1, stride=72)
    refused(ctx.gen_records, recs.data_ptr() + 8, n, 1, stride=128)
    ctx.set_record_layout(0, 8)
    refused(ctx.gen_records, recs, n, 1, stride=128)
    ctx.set_record_layout(40, 48)
    # n = 0: all six calls return 0 and write nothing
    out = rows_arena(1, 192)
    ctx.verify_macinputs(mi, exp, 0, bits[2:])
    ctx.cmac_tags(mi, 0, tags[2:])
    ctx.verdict_counters(recs, 0, bits[2:], counters, stride=128)
    ctx.gen_records(recs, 0, 1, stride=128)
    ctx.expand_keys(mi, 0, out[2:])
    ctx.key_add_batch(0, b"")
    assert (host(bits).view(np.uint64) == np.array([GUARD, GUARD, FILL, GUARD, GUARD], dtype=np.uint64)).all()
    check_rows(tags, n, np.full((n, 16), FILL & 0xff, dtype=np.uint8), ("cmac_tags", "n = 0"))
    check_rows(out, 1, np.full((1, 192), FILL & 0xff, dtype=np.uint8), ("expand_keys", "n = 0"))
    assert not host(counters).any() and (host(recs) == FILL & 0xff).all()
    with pytest.raises(hfv.HfvError):
        ctx.key_get(0)
