"""The corpus of tests/hf_bits.py (passing records with every don't-care bit set, and every
single-bit flip of sixteen of them) and its rule, held to the CPU checker, to the reference's
aes.c where it is built, to the reference's recorded bitmaps (tests/golden/hf_bits.npz) and to
the host C ABI's hfv_verify_macinput.  CPU only; tests/test_gpu_hf_bits.py holds the kernels to
the same rule."""
import numpy as np
import pytest

import hf_bits as HB
import orc
import scion_hfv as hfv

KEYSELS = (0, 1)
LAYOUT_IDS = ["%d-%d-%d" % l for l in HB.LAYOUTS]


@pytest.fixture(scope="module")
def table():
    raw = HB.raw_keys()
    hk, valid = orc.key_table(raw)
    return raw, hk, valid


def test_splitmix_is_the_oracles():
    L = orc.oracle()
    got = HB.splitmix(HB.SEED, 5, start=123456789)
    assert [int(x) for x in got] == [L.orc_splitmix_at(HB.SEED, 123456789 + j) for j in range(5)]


@pytest.mark.parametrize("keysel", KEYSELS)
def test_corpus_conditions(keysel):
    """What the base records hold by construction."""
    L0 = HB.LAYOUTS[0]
    c = HB.corpus(keysel)
    base = c.recs[:c.nbase]
    assert base.shape == (2048, 64) and c.recs.shape == (2048 + 8 * 512, 64)
    inf, hf = HB.fields(base, L0)
    cons = (inf[:, 0] & 1).astype(bool)
    sel, oth, slot = HB.selecting_ifid(base, L0), HB.other_ifid(base, L0), HB.slots(base, L0)
    # every slot is selected by a Cons and by a non-Cons record (the slot is the key only under
    # KEYSEL_IFID, but the counters use it under both rules)
    assert len(np.unique(slot[cons])) == 256 and len(np.unique(slot[~cons])) == 256
    assert int((sel > 255).sum()) >= 256
    assert int((sel == 0).sum()) >= 16
    assert int((oth == 0).sum()) >= 16
    for byte, bits in ((hf[:, 0], range(8)), (inf[:, 1], range(8)), (inf[:, 0], range(1, 8))):
        for b in bits:
            assert int(((byte >> b) & 1).sum()) >= len(base) // 4, b
    assert ((hf[:, 6] != 0) | (hf[:, 7] != 0)).all()
    # the header and the payload are random bytes too: every bit outside INF/HF is set somewhere
    outside = np.concatenate([base[:, :40], base[:, 60:]], axis=1)
    assert (np.bitwise_or.reduce(outside, axis=0) == 0xff).all()
    # the variants: 4 Cons and 4 non-Cons bases, each of their 512 records one bit away
    vb = list(HB.VAR_BASES)
    assert int(cons[vb].sum()) == 4 and len(vb) == 8
    for j, r in enumerate(vb):
        blk = c.recs[c.nbase + 512 * j:c.nbase + 512 * (j + 1)]
        diff = np.unpackbits(blk ^ base[r], axis=1, bitorder="little")
        assert np.array_equal(diff, np.eye(512, dtype=np.uint8))
        assert int(c.passes[c.nbase + 512 * j:c.nbase + 512 * (j + 1)].sum()) == 512 - HB.SENS_BITS == 375
    assert int(HB.sens(L0).sum()) == HB.SENS_BITS
    assert c.passes[:c.nbase].all()


@pytest.mark.parametrize("keysel", KEYSELS)
def test_layouts_hold_the_same_fields(keysel):
    c0 = HB.corpus(keysel)
    inf0, hf0 = HB.fields(c0.recs[:c0.nbase], c0.layout)
    for layout in HB.LAYOUTS[1:]:
        c = HB.corpus(keysel, layout)
        stride = layout[2]
        assert c.recs.shape == (2048 + 8 * 8 * stride, stride)
        inf, hf = HB.fields(c.recs[:c.nbase], layout)
        assert np.array_equal(inf, inf0) and np.array_equal(hf, hf0)
        assert int(HB.sens(layout).sum()) == HB.SENS_BITS
        assert int(c.passes.sum()) == 2048 + 8 * (8 * stride - HB.SENS_BITS)


def _oracle_bits(c, hk, valid):
    return orc.verify_records(HB.at_default_offsets(c.recs, c.layout), hk, valid, c.keysel, stride=c.layout[2],
                              n=len(c.recs))


@pytest.mark.parametrize("layout", HB.LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("keysel", KEYSELS)
def test_oracle_equals_the_rule(table, keysel, layout):
    raw, hk, valid = table
    c = HB.corpus(keysel, layout)
    assert np.array_equal(_oracle_bits(c, hk, valid), HB.bitmap(c.passes))
    if keysel == 1:
        want = HB.partial_passes(c)
        assert 0 < int(want.sum()) < int(c.passes.sum())
        assert np.array_equal(_oracle_bits(c, hk, HB.partial_valid()), HB.bitmap(want))


@pytest.mark.parametrize("layout", HB.LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("keysel", KEYSELS)
def test_reference_build_equals_the_rule(table, keysel, layout):
    if orc.reference() is None:
        pytest.skip("the reference aes.c is not built here")
    raw, hk, valid = table
    c = HB.corpus(keysel, layout)
    view = HB.at_default_offsets(c.recs, layout)
    for aesni in (0, 1):
        got = orc.ref_verify_records(view, raw, hk, valid, keysel, aesni=aesni, stride=layout[2], n=len(c.recs))
        assert np.array_equal(got, HB.bitmap(c.passes)), aesni
        if keysel == 1:
            got = orc.ref_verify_records(view, raw, hk, HB.partial_valid(), 1, aesni=aesni, stride=layout[2],
                                         n=len(c.recs))
            assert np.array_equal(got, HB.bitmap(HB.partial_passes(c))), aesni


@pytest.mark.parametrize("keysel", KEYSELS)
def test_reference_fixture_equals_the_rule(keysel):
    """tests/golden/hf_bits.npz: the bitmaps the reference's aes.c gave on this corpus (soft and
    AES-NI path), and the SHA-256 of the corpus bytes they were computed from."""
    g = orc.load_golden("hf_bits.npz")
    for j, layout in enumerate(HB.LAYOUTS):
        c = HB.corpus(keysel, layout)
        assert g["sha256"][keysel, j].tobytes() == HB.sha256(c), layout
        assert np.array_equal(g["bits_%d_%d" % (keysel, j)], HB.bitmap(c.passes)), layout
        if keysel == 1:
            assert np.array_equal(g["partial_%d" % j], HB.bitmap(HB.partial_passes(c))), layout


@pytest.mark.parametrize("keysel", KEYSELS)
def test_host_verify_macinput_equals_the_rule(keysel):
    """hfv_verify_macinput (the host C ABI) over the helper's MAC inputs and expected MACs with
    the key of each record's slot; a missing key (the odd slots of the partial table) fails."""
    c = HB.corpus(keysel)
    mi, exp = HB.macinputs(c.recs, c.layout)
    slot = HB.slots(c.recs, c.layout) if keysel else np.zeros(len(c.recs), dtype=np.uint8)
    raw = HB.raw_keys()
    hks = [orc.hop_key(raw[16 * k:16 * k + 16]) for k in range(256)]
    got = np.array([hfv.verify_macinput(mi[i].tobytes(), int(exp[i]), hks[slot[i]]) for i in range(len(c.recs))])
    assert np.array_equal(got, c.passes)
    if keysel == 1:
        got = np.array([hfv.verify_macinput(mi[i].tobytes(), int(exp[i]), None if slot[i] & 1 else hks[slot[i]])
                        for i in range(len(c.recs))])
        assert np.array_equal(got, HB.partial_passes(c))
