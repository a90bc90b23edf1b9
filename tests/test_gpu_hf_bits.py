"""The record-level hop-field verify on PASSING records with every don't-care bit set, and on
every single-bit flip of sixteen of them (the corpus and the rule of tests/hf_bits.py, which
tests/test_hf_bits.py holds to the CPU checker and to the reference's recorded bitmaps):
hfv_verify_records, hfv_verify_batches, the resident service, the host legs, the prepared-input
kernels and the verdict counters, under both key rules, three record layouts and a partial key
table.  Integer work: every comparison is bit-exact against the rule.

Every test runs the corpus once in order and once rolled by 37 records (another lane and tile
for every record).  Every bitmap lies between two guard words on either side and is pre-filled:
the guards must survive, no bit at or past n may be set, an empty batch's word stays as it was."""
import numpy as np
import pytest

import hf_bits as HB
import orc
import scion_hfv as hfv

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 0x5A5A5A5A5A5A5A5A
FILL = 0xFFFFFFFFFFFFFFFF
ROLLS = (0, 37)
KEYSELS = (0, 1)
L_DEFAULT, L_COMPACT, L_WIDE = HB.LAYOUTS
ids = lambda layouts: ["%d-%d-%d" % l for l in layouts]   # noqa: E731


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def rolled(c, roll, passes=None):
    """(records, expected verdicts) of the corpus moved on by `roll` records."""
    passes = c.passes if passes is None else passes
    return np.roll(c.recs, roll, axis=0), np.roll(passes, roll)


def check_words(words, n, want, what):
    """words: guard, guard, bitmap of n records, guard, guard (numpy u64)."""
    assert (words[:2] == GUARD).all() and (words[-2:] == GUARD).all(), ("guard words written", what)
    if n == 0:
        assert (words[2:-2] == FILL).all(), ("an empty batch was written to", what)
        return
    w = HB.bitmap(want, n)
    bad = np.nonzero(words[2:-2] != w)[0]
    assert not len(bad), (what, "n=%d" % n, "first bad word %d: got %016x want %016x" % (
        bad[0], int(words[2 + bad[0]]), int(w[bad[0]])))


class DevBits:
    """A device bitmap for n records between guard words, pre-filled with ones."""

    def __init__(self, n):
        self.n = n
        self.t = torch.full((max(1, (n + 63) // 64) + 4,), GUARD, dtype=torch.int64, device=DEV)
        self.bits = self.t[2:-2]
        self.bits.fill_(-1)

    def check(self, want, what):
        torch.cuda.synchronize()
        check_words(self.t.cpu().numpy().view(np.uint64), self.n, want, what)


class HostBits:
    """The same in host memory (pageable, or registered with the ctx)."""

    def __init__(self, n, registered=False):
        self.n = n
        words = (n + 63) // 64 + 4
        self.a = hfv.host_array((words,), np.uint64) if registered else np.zeros(words, dtype=np.uint64)
        self.a[:] = GUARD
        self.bits = self.a[2:-2]
        self.bits[:] = FILL

    def check(self, want, what):
        check_words(self.a, self.n, want, what)


def cuts_of(n):
    """Ragged batch boundaries: one record, an empty batch, the tile size and one past it, the end
    of the base records and of the first variant block's passing count."""
    return [0, 1, 1, 64, 65, 700, 2048, 2048 + 375, n]


def install(ctx, slots=range(256)):
    raw = HB.raw_keys()
    for k in slots:
        ctx.key_add(k, raw[16 * k:16 * k + 16])


@pytest.fixture()
def ctx():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = hfv.Ctx(0)
    yield c
    c.synchronize()
    c.close()


def setup(ctx, keysel, layout, slots=range(256)):
    install(ctx, slots)
    ctx.set_keysel(keysel)
    ctx.set_record_layout(layout[0], layout[1])
    return HB.corpus(keysel, layout)


def run_batches(ctx, d, stride, n, want, what):
    cuts = cuts_of(n)
    outs = [(a, b, DevBits(b - a)) for a, b in zip(cuts, cuts[1:])]
    ctx.verify_batches([(d[a:], b - a, o.bits, stride) for a, b, o in outs])
    for a, b, o in outs:
        o.check(want[a:b], (what, a, b))


@pytest.mark.parametrize("layout", HB.LAYOUTS, ids=ids(HB.LAYOUTS))
@pytest.mark.parametrize("keysel", KEYSELS)
def test_verify_records(ctx, keysel, layout):
    c = setup(ctx, keysel, layout)
    for roll in ROLLS:
        recs, want = rolled(c, roll)
        d = dev(recs)
        for n in (len(recs), 1, 63, 65):
            o = DevBits(n)
            ctx.verify_records(d, n, o.bits, stride=layout[2])
            o.check(want[:n], (keysel, layout, roll))


@pytest.mark.parametrize("layout", HB.LAYOUTS, ids=ids(HB.LAYOUTS))
@pytest.mark.parametrize("keysel", KEYSELS)
def test_verify_batches(ctx, keysel, layout):
    c = setup(ctx, keysel, layout)
    for roll in ROLLS:
        recs, want = rolled(c, roll)
        run_batches(ctx, dev(recs), layout[2], len(recs), want, (keysel, layout, roll))


@pytest.mark.parametrize("layout", [L_DEFAULT, L_COMPACT], ids=ids([L_DEFAULT, L_COMPACT]))
def test_verify_batches_no_key_in_slot_0(ctx, layout):
    """KEYSEL_ZERO with slots 1..255 installed and slot 0 empty: every verdict word is 0."""
    c = setup(ctx, 0, layout, slots=range(1, 256))
    for roll in ROLLS:
        recs, _ = rolled(c, roll)
        run_batches(ctx, dev(recs), layout[2], len(recs), np.zeros(len(recs), dtype=bool), (layout, roll))


@pytest.mark.parametrize("vector", [False, True], ids=["submit", "submitv"])
@pytest.mark.parametrize("layout", [L_DEFAULT, L_COMPACT], ids=ids([L_DEFAULT, L_COMPACT]))
@pytest.mark.parametrize("keysel", KEYSELS)
def test_service(ctx, keysel, layout, vector):
    c = setup(ctx, keysel, layout)
    try:
        for roll in ROLLS:
            recs, want = rolled(c, roll)
            d = dev(recs)
            cuts = cuts_of(len(recs))
            outs = [(a, b, DevBits(b - a)) for a, b in zip(cuts, cuts[1:])]
            batches = [(d[a:], b - a, o.bits, layout[2]) for a, b, o in outs]
            torch.cuda.synchronize()          # the service is host-ordered: buffers complete when posted
            if vector:
                tickets = ctx.service_submitv(batches)
            else:
                tickets = [ctx.service_submit(r, n, b, stride=s) for r, n, b, s in batches]
            for t in tickets:
                ctx.service_wait(t, 20000)
            ctx.service_stop()                # a device synchronize would wait for the resident grid
            for a, b, o in outs:
                o.check(want[a:b], (keysel, layout, roll, a, b))
    finally:
        ctx.service_stop()


@pytest.mark.parametrize("layout", [L_DEFAULT, L_WIDE], ids=ids([L_DEFAULT, L_WIDE]))
@pytest.mark.parametrize("keysel", KEYSELS)
def test_verify_records_host(ctx, keysel, layout):
    """Pageable records take the gather-and-stage path; records in a registered buffer the
    zero-copy kernel variant, with a pageable and with a registered bitmap."""
    c = setup(ctx, keysel, layout)
    n, stride = c.recs.shape
    ring = hfv.host_array((n, stride), np.uint8)
    reg = HostBits(n, registered=True)
    ctx.host_register(ring)
    ctx.host_register(reg.a)
    try:
        for roll in ROLLS:
            recs, want = rolled(c, roll)
            recs = np.ascontiguousarray(recs)
            for m in (n, 65):
                o = HostBits(m)
                ctx.verify_records_host(recs, m, o.bits, stride=stride)
                o.check(want[:m], ("staged", keysel, layout, roll))
            ring[:] = recs
            o = HostBits(n)
            ctx.verify_records_host(ring, n, o.bits, stride=stride)
            o.check(want, ("zero-copy", keysel, layout, roll))
            reg.bits[:] = FILL
            ctx.verify_records_host(ring, n, reg.bits, stride=stride)
            reg.check(want, ("zero-copy, registered bitmap", keysel, layout, roll))
    finally:
        ctx.host_unregister(ring)
        ctx.host_unregister(reg.a)


@pytest.mark.parametrize("layout", HB.LAYOUTS, ids=ids(HB.LAYOUTS))
def test_partial_key_table(ctx, layout):
    """KEYSEL_IFID with only the even slots installed: a record passes iff the full-table rule
    says so and its slot (the low byte of the selecting IFID) is even."""
    c = setup(ctx, 1, layout, slots=range(0, 256, 2))
    partial = HB.partial_passes(c)
    for roll in ROLLS:
        recs, want = rolled(c, roll, partial)
        d = dev(recs)
        o = DevBits(len(recs))
        ctx.verify_records(d, len(recs), o.bits, stride=layout[2])
        o.check(want, (layout, roll))
        run_batches(ctx, d, layout[2], len(recs), want, (layout, roll))


@pytest.mark.parametrize("keysel", KEYSELS)
def test_macinputs_and_tags(ctx, keysel):
    """hfv_verify_macinputs and hfv_cmac_tags on the helper's own MAC inputs, expected MACs and
    key indices: the verdicts equal the rule, the 16-byte tags the CPU checker's CMAC."""
    c = setup(ctx, keysel, L_DEFAULT)
    raw = HB.raw_keys()
    known = {}
    for roll in ROLLS:
        recs, want = rolled(c, roll)
        n = len(recs)
        mi, exp = HB.macinputs(recs, L_DEFAULT)
        slot = HB.slots(recs, L_DEFAULT) if keysel else np.zeros(n, dtype=np.uint8)
        kidx = dev(slot) if keysel else None
        dmi = dev(mi)
        o = DevBits(n)
        ctx.verify_macinputs(dmi, dev(exp.view(np.int64)), n, o.bits, key_index=kidx)
        o.check(want, (keysel, roll))
        tags = torch.zeros((n, 16), dtype=torch.uint8, device=DEV)
        ctx.cmac_tags(dmi, n, tags, key_index=kidx)
        torch.cuda.synchronize()
        got = tags.cpu().numpy()
        for i in range(n):
            k = (mi[i].tobytes(), int(slot[i]))
            if k not in known:
                known[k] = orc.cmac(k[0], raw[16 * k[1]:16 * k[1] + 16])
            assert got[i].tobytes() == known[k], (keysel, roll, i)


@pytest.mark.parametrize("layout", HB.LAYOUTS, ids=ids(HB.LAYOUTS))
@pytest.mark.parametrize("keysel", KEYSELS)
def test_verdict_counters(ctx, keysel, layout):
    """counters[2 * slot + fail] over the corpus with the rule's bitmap, against a bincount from
    the helper's own slot rule: IFIDs above 255 and of 0, garbage in inf[0] bits 1..7 and inf[1]."""
    c = setup(ctx, keysel, layout)
    total = np.zeros(512, dtype=np.uint64)
    counters = torch.zeros((256, 2), dtype=torch.int64, device=DEV)
    for roll in ROLLS:
        recs, want = rolled(c, roll)
        n = len(recs)
        bits = dev(HB.bitmap(want).view(np.int64))
        ctx.verdict_counters(dev(recs), n, bits, counters, stride=layout[2])
        torch.cuda.synchronize()
        total += np.bincount(2 * HB.slots(recs, layout).astype(np.int64) + (~want).astype(np.int64),
                             minlength=512).astype(np.uint64)
        assert np.array_equal(counters.cpu().numpy().view(np.uint64).reshape(-1), total), (keysel, layout, roll)
    assert int(total.sum()) == 2 * n and int(total[1::2].sum()) == 2 * int((~c.passes).sum())
