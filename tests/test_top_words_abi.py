"""CPU: the surface of the device top-k (include/mox.h mox_top_words, the
Python mirror, dist.merge_top) and the case tables of test_gpu_top_words.py.
No GPU code runs here."""
import ctypes
import os
import re

import pytest

import mox
from mox import dist as mdist
from conftest import ROOT
from srcpins import _read
import top_cases as C


def test_header_declares_top_words():
    src = _read("include", "mox.h")
    assert re.search(r"^#define MOX_TOP_MAX 4096\s*$", src, re.M)
    assert re.search(r"\bint mox_top_words\(mox_engine\* e, size_t k, mox_table\*\* out\);", src)
    assert re.search(r"^#define MOX_ABI_VERSION 4\s*$", src, re.M)  # additive: the version stays
    assert mox.TOP_MAX == 4096 == C.TOP_MAX


def test_library_exports_top_words_with_its_signature():
    raw = ctypes.CDLL(mox.LIB_PATH)
    assert hasattr(raw, "mox_top_words")
    f = mox.lib().mox_top_words
    assert f.restype is ctypes.c_int
    assert list(f.argtypes) == [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.POINTER(mox._Table))]
    for path in (mox.CHECK_LIB_PATH, mox.HC_LIB_PATH):  # the check builds link the same kernels
        assert hasattr(ctypes.CDLL(path), "mox_top_words")
    assert callable(mox.Engine.top_words)


def test_null_arguments_are_einval():
    L = mox.lib()
    t = ctypes.POINTER(mox._Table)()
    assert L.mox_top_words(None, 10, ctypes.byref(t)) == mox.MOX_EINVAL
    assert not t


def test_tile_matches_the_source():
    src = _read("map-oxidize_amd", "csrc", "mox_topk.hip")
    m = re.search(r"^constexpr uint64_t TK_TILE = (\d+);", src, re.M)
    assert m and int(m.group(1)) == C.TILE
    per = int(re.search(r"^constexpr int TK_PER = (\d+);", src, re.M).group(1))
    assert 64 * per == C.TILE  # one wave per tile
    assert re.search(r"^constexpr uint32_t TK_MAX = MOX_TOP_MAX;", src, re.M)
    assert C.EDGE_NS == (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)


def test_merge_top_orders_ties_by_rank_then_position():
    parts = [[(b"a", 9), (b"b", 5), (b"c", 5)],
             [(b"d", 9), (b"e", 7), (b"f", 5)],
             [(b"g", 5)]]
    want = [(b"a", 9), (b"d", 9), (b"e", 7), (b"b", 5), (b"c", 5), (b"f", 5), (b"g", 5)]
    for k in range(9):
        assert mdist.merge_top(parts, k) == want[:k]
    assert mdist.merge_top(parts, 100) == want  # k larger than the union
    # position, not the word's bytes, breaks a tie inside a rank
    assert mdist.merge_top([[(b"z", 3), (b"a", 3)]], 2) == [(b"z", 3), (b"a", 3)]
    # a later rank's higher count goes first whatever the rank
    assert mdist.merge_top([[(b"x", 1)], [(b"y", 2)]], 1) == [(b"y", 2)]


def test_merge_top_empty_parts():
    assert mdist.merge_top([], 10) == []
    assert mdist.merge_top([[], []], 10) == []
    assert mdist.merge_top([[], [(b"a", 1)], []], 10) == [(b"a", 1)]
    assert mdist.merge_top([[(b"a", 1)]], 0) == []


def test_merge_top_duplicate_word_raises():
    with pytest.raises(ValueError):
        mdist.merge_top([[(b"a", 2)], [(b"b", 1), (b"a", 1)]], 5)
    with pytest.raises(ValueError):
        mdist.merge_top([[(b"a", 2), (b"a", 1)]], 5)


def test_merge_top_is_the_top_of_the_rank_order_concatenation():
    """The claim merge_top rests on: per-rank top-k lists merged by (count, rank,
    position) are the top-k of the ranks' tables laid end to end."""
    import random
    rng = random.Random(3)
    for trial in range(50):
        tables, seq = [], 0
        for r in range(rng.randint(1, 4)):
            tab = []
            for _ in range(rng.randint(0, 30)):
                tab.append((b"w%d" % seq, rng.randint(1, 4)))
                seq += 1
            tables.append(tab)
        k = rng.randint(0, 20)
        gathered = [x for tab in tables for x in tab]
        assert mdist.merge_top([C.expected(tab, k) for tab in tables], k) == C.expected(gathered, k)


def test_expected_is_print_top_words_rule():
    items = [(b"a", 2), (b"b", 5), (b"c", 2), (b"d", 5), (b"e", 1)]
    assert C.expected(items, 3) == [(b"b", 5), (b"d", 5), (b"a", 2)]
    assert C.expected(items, 0) == [] and C.expected(items, 9) == [(b"b", 5), (b"d", 5), (b"a", 2), (b"c", 2), (b"e", 1)]


def test_case_tables_have_their_shapes():
    w, c = C.distinct(5000, 1)
    assert len(set(w)) == 5000 and sorted(c) == list(range(1, 5001)) and c != sorted(c)
    w, c = C.sparse_ties()
    assert len(set(w)) == 40000 and c.count(7) == 1000 and c.count(1) == 40000 - 1003 and sum(x > 7 for x in c) == 3
    w, c = C.every_bit()
    assert len(w) == 128 and len(set(c)) == 128 and {1 << 63, C.U64, 1, (1 << 63) + 1} <= set(c)
    assert all((1 << b) in c for b in range(64)) and all((1 << b) + 1 in c for b in range(1, 64))
    w, c = C.last_digit()
    assert len(c) == 256 and {x >> 8 for x in c} == {0xFFFFFFFFFFFFFF} and max(c) == C.U64
    w, c = C.first_digit()
    assert len(c) == 255 and all(x & ((1 << 56) - 1) == 0 for x in c) and len(set(c)) == 255
    w, c, winners = C.word_shapes()
    assert len(set(w)) == len(w) == 3000
    top = C.expected(list(zip(w, c)), 64)
    assert [x for x, _ in top] == winners
    lens = [len(x) for x in winners]
    assert set(range(1, 41)) <= set(lens) and max(lens) == 100000 and sum(L > 16 for L in lens) > 20
    i = lens.index(100000)
    assert lens[i + 1] == 1
    assert sum(any(b > 127 for b in x) for x in winners) >= 5
    w, c = C.many_equal()
    assert len(set(w)) == 6000 and set(c) == {1, 2, 3, 4, 5} and all(1 <= len(x) <= 12 for x in w)
