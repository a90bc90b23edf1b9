"""The three-table corpus of tests/key_tables.py really tells the tables apart (CPU checker only):
otherwise the key-publication tests on the GPU, which compare a launch's verdicts with the
verdicts under the table it was launched with, could pass under any table."""
import itertools

import numpy as np

import key_tables as KT


def test_each_table_passes_only_its_own_records():
    _, origin = KT.corpus()
    wb = KT.want_bool()
    slots = KT.slots()
    for i, name in enumerate(KT.NAMES):
        passing = wb[name]
        assert passing.sum() >= 1000, name
        assert (origin[passing] == i).all(), name          # only records generated for this table
        assert len(np.unique(slots[passing])) >= 200, name   # spread over the key slots, not one row
    for x, y in itertools.combinations(KT.NAMES, 2):
        assert not (wb[x] & wb[y]).any(), (x, y)
        assert (KT.want()[x] != KT.want()[y]).sum() >= 60     # of 71 bitmap words


def test_tables_differ_in_every_slot():
    t = KT.tables()
    for x, y in itertools.combinations(KT.NAMES, 2):
        a = np.frombuffer(t[x][0], dtype=np.uint8).reshape(256, 16)
        b = np.frombuffer(t[y][0], dtype=np.uint8).reshape(256, 16)
        assert (a != b).any(axis=1).all(), (x, y)
        assert (t[x][2] == 0xFFFFFFFF).all()


def test_batches_cover_the_corpus():
    assert KT.CUTS[0] == 0 and KT.CUTS[-1] == KT.N == 4500
    for name in KT.NAMES:
        parts = KT.want_batches()[name]
        assert len(parts) == len(KT.CUTS) - 1
        joined = np.concatenate([np.unpackbits(p.view(np.uint8), bitorder="little")[:b - a]
                                 for p, a, b in zip(parts, KT.CUTS[:-1], KT.CUTS[1:])]).astype(bool)
        assert np.array_equal(joined, KT.want_bool()[name])
        assert np.array_equal(KT.pack_bits(KT.want_bool()[name]), KT.want()[name])


def test_macinputs_and_tags_agree_with_the_verdicts():
    """The macinput form of the corpus gives the record form's verdicts: a sampled record passes
    under table X exactly when the first six bytes of its tag under X's key equal its MAC."""
    _, expected, kidx = KT.macinputs()
    assert np.array_equal(kidx, KT.slots())
    idx = KT.tag_sample()
    assert idx[0] == 0 and idx[-1] == KT.N - 1 and all(((idx >= lo) & (idx < lo + 1500)).sum() >= 80 for lo in (0, 1500, 3000))
    exp6 = expected[idx].view(np.uint8).reshape(-1, 8)[:, :6]
    for name in KT.NAMES:
        match = (KT.want_tags()[name][:, :6] == exp6).all(axis=1)
        assert np.array_equal(match, KT.want_bool()[name][idx]), name
        assert match.sum() >= 50


def test_generated_records_differ_per_table():
    g = KT.want_gen()
    for x, y in itertools.combinations(KT.NAMES, 2):
        assert (g[x] != g[y]).any(axis=1).sum() >= KT.GEN_N * 9 // 10
