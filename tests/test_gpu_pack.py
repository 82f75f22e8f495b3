"""GPU: the three producers of the exchange's receive layout -- the host packer
of mox_reduce_pairs, the accumulator's packer (mox_accum.hip) and the re-keying
packer (mox_rekey.hip) -- agree on one word list, pack_cases.table(), made of
the shapes at which the pieces the two device packers share (mox_pack.h) can go
wrong.  Every comparison is exact (words, counts, tokens), against
accum_cases.oracle_sum and rekey_cases.expected.  The reduce-only pass behind
all three merges by the hash and the bytes a packer wrote, so a wrong hash of a
form (one lane, a whole wave, the host) or a wrong byte splits or loses a word."""
import pytest

import accum_cases as A
import mox
import pack_cases as C
import rekey_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    e = mox.Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def table():
    return C.table()


def resident(e):
    """(items, tokens, start phases mod 8 of the short rows, of the long rows) of the resident result."""
    t = e.fetch()
    try:
        _, offs, _ = t.arrays()
        items, tok = list(t.items()), t.tokens
    finally:
        t.close()
    s, l = set(), set()
    for i, (w, _) in enumerate(items):
        (s if A.is_short(w) else l).add(int(offs[i]) % 8)
    return items, tok, s, l


def test_reduce_pairs(eng, table):
    words, ca, cb = table
    again = words[::3]  # every third word a second time: the pass merges, too
    t = eng.reduce_pairs(words + again, ca + cb[:len(again)])
    try:
        got, tok = sorted(t.items()), t.tokens
    finally:
        t.close()
    want, wtok = A.oracle_sum((words, ca), (again, cb[:len(again)]))
    assert got == want and tok == wtok
    assert C.kinds([w for w, _ in got]) == C.kinds(words) and min(C.kinds(words)) >= 90


def test_accumulate_twice(eng, table):
    words, ca, cb = table
    for counts in (ca, cb):
        A.load(eng, (words, counts))
        _, _, s, l = resident(eng)
        assert l == set(range(8)) and s == set(range(8))  # the table the packer reads: rows at every phase of an 8-byte word
        eng.accumulate()
    _, _, s, l = resident(eng)  # the total, which was source 0 of the second fold
    assert l == set(range(8))
    got, tok = A.fetched(eng)
    want, wtok = A.oracle_sum((words, ca), (words, cb))
    assert sorted(got) == want and tok == wtok
    assert dict(got)[C.word(8, 0)] == 0 and dict(got)[C.word(C.COOP + 1, 0)] == 0  # zero counts stay rows


def test_rekey_wrapped(eng, table):
    words, ca, _ = table
    A.load(eng, (C.wrapped(words), ca))
    items, tok, _, l = resident(eng)
    assert l == set(range(8))  # and every window starts one byte further on
    assert sum(A.is_short(w) for w, _ in items) == sum(len(w) <= 14 and b"\x00" not in w for w in words)
    want, _, winfo = R.expected(items, trim=b"()", tokens=tok)
    info = eng.rekey_result(trim=b"()")
    got, tokens = A.fetched(eng)
    assert sorted(got) == sorted(want) == sorted(zip(words, ca))
    assert tokens == winfo["tokens_out"] == sum(ca)
    assert {k: info[k] for k in R.INFO_KEYS} == winfo and info["words_changed"] == len(words)
