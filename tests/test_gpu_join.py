"""GPU: the device join (mox_join_total, map-oxidize_amd/csrc/mox_join.hip and
the compaction in mox_filter.hip) against a plain Python dict join.  Every
comparison is exact.  The total T is loaded by reduce_pairs + accumulate and
the result R by a second reduce_pairs, unless the case says otherwise; the
expectation is join_cases.expected over a fetch() of R taken immediately
before the call (the engine order of words longer than 16 bytes can differ
from run to run) and T's items from a fetch made while T was the result.
After the call three things are compared: the fetched table, in order; its
tokens; every info key that is a function of the tables.  The case tables and
the CPU checks of their shapes: join_cases.py, test_join_abi.py."""
import os
import subprocess

import pytest

import coracle
import join_cases as C
import mox

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    e = mox.Engine(device=0)
    yield e
    e.close()


def fetched(e):
    """The engine's resident result as ((word, count) items in table order, tokens)."""
    t = e.fetch()
    try:
        return list(t.items()), t.tokens
    finally:
        t.close()


def load(e, table):
    e.reduce_pairs(*table).close()


def load_total(e, table):
    """table becomes the accumulator's total; returns its items as fetched while it was the result."""
    load(e, table)
    items, _ = fetched(e)
    e.accumulate()
    return items


def assert_join(e, t_items, mode="semi", counts="result"):
    """join_total on e's resident result: table, tokens and info equal the Python
    join over the fetch taken just before.  Returns (R's items, kept items, info)."""
    items, _ = fetched(e)
    want, winfo = C.expected(items, t_items, mode, counts)
    info = e.join_total(mode, counts)
    got, tokens = fetched(e)
    assert got == want
    assert tokens == winfo["tokens_kept"]
    assert {k: info[k] for k in C.INFO_KEYS} == winfo
    assert info["device_bytes"] > 0 and info["ms"] > 0
    return items, want, info


def assert_both_modes(e, r, t_items):
    """SEMI and ANTI on the same R: each as expected, and together they partition R."""
    load(e, r)
    items, semi, _ = assert_join(e, t_items, "semi")
    load(e, r)
    _, anti, _ = assert_join(e, t_items, "anti")
    assert sorted(semi + anti) == sorted(items) and len(semi) + len(anti) == len(items)
    return semi, anti


def assert_empty(e):
    """An empty result is a valid result for every reader."""
    assert fetched(e) == ([], 0)
    t = e.top_words(5)
    assert list(t.items()) == []
    t.close()
    assert e.result_text() == b""
    assert e.lookup([b"a"]).tolist() == [0]


# ---- 1. size edges
@pytest.mark.parametrize("n", C.TABLE_NS)
def test_result_size_edges(eng, n):
    r, t = C.pair(n, 300, 100 + n)
    t_items = load_total(eng, t)
    semi, anti = assert_both_modes(eng, r, t_items)
    assert len(semi) == max(1, min(n, 300) // 3) and len(semi) + len(anti) == n


@pytest.mark.parametrize("n", C.TABLE_NS)
def test_total_size_edges(eng, n):
    r, t = C.pair(300, n, 200 + n)
    t_items = load_total(eng, t)
    assert len(t_items) == n
    semi, anti = assert_both_modes(eng, r, t_items)
    assert len(semi) == max(1, min(n, 300) // 3) and len(anti) == 300 - len(semi)


# ---- 2. grid strides
def test_three_strides(eng, monkeypatch):
    r, t = C.pair(C.STRIDE_N, C.STRIDE_N, 5)
    t_items = load_total(eng, t)
    load(eng, r)
    items, free, _ = assert_join(eng, t_items, "semi", "min")
    assert len(items) == C.STRIDE_N and len(free) == C.STRIDE_N // 3
    monkeypatch.setenv("MOX_JOIN_GRID", str(C.STRIDE_GRID))
    load(eng, r)
    _, capped, _ = assert_join(eng, t_items, "semi", "min")
    assert dict(capped) == dict(free) and len(capped) == len(free)  # the grid does not matter
    load(eng, r)
    _, anti, _ = assert_join(eng, t_items, "anti")
    assert len(anti) == C.STRIDE_N - len(free)


# ---- 3. word shapes
@pytest.fixture(scope="module")
def shapes():
    return C.shape_table()


def test_word_shapes_on_both_sides(eng, shapes):
    """Lengths 15..17 and 63..65, the 100,000-byte word, words with NUL bytes and the prefix chain, in both tables."""
    words, counts = shapes
    long_word = max(words, key=len)
    assert len(long_word) == 100000
    edges = {15, 16, 17, 63, 64, 65, 100000}
    t_words = words[::2] + [w for w in words[1::2] if len(w) in edges]
    t_items = load_total(eng, (t_words, list(range(1, len(t_words) + 1))))
    semi, anti = assert_both_modes(eng, (words, counts), t_items)
    assert long_word in dict(semi) and len(semi) == len(t_words) and len(anti) == len(words) - len(semi) > 1000
    assert {len(w) for w, _ in semi} >= edges


def test_long_word_against_one_that_differs_in_its_last_byte(eng, shapes):
    words, counts = shapes
    long_word = max(words, key=len)
    twin = long_word[:-1] + bytes([long_word[-1] ^ 1])
    t_words = [w for w in words if w != long_word][::3] + [twin]
    t_items = load_total(eng, (t_words, list(range(1, len(t_words) + 1))))
    semi, anti = assert_both_modes(eng, (words, counts), t_items)
    assert long_word in dict(anti) and long_word not in dict(semi) and len(semi) == len(t_words) - 1
    assert {len(w) for w, _ in anti} >= {15, 16, 17, 63, 64, 65, 100000}


def test_near_misses_nul_words_and_the_prefix_chain(eng):
    base = C.NUL_WORDS + C.PREFIX_CHAIN[::2] + [b"ab", b"word", b"x" * 17, b"y" * 64]
    misses = sorted({m for w in base for m in C.near_misses(w) if m} - set(base))
    # T holds the near misses (and a few of the words themselves): only exact equals match
    t_words = misses + base[::5]
    t_items = load_total(eng, (t_words, list(range(1, len(t_words) + 1))))
    semi, anti = assert_both_modes(eng, (base, list(range(10, 10 + len(base)))), t_items)
    assert {w for w, _ in semi} == set(base[::5]) and b"ab\x00" in dict(anti) and b"ab" in {w for w, _ in semi + anti}
    # ... and the other way round: R holds "ab\0", T holds "ab"
    eng.accumulate_reset()
    t_items = load_total(eng, ([b"ab", b"\x00", b"a" * 16], [1, 2, 3]))
    load(eng, ([b"ab\x00", b"\x00\x00", b"a" * 15, b"a" * 17, b"\x00"], [5, 6, 7, 8, 9]))
    _, kept, _ = assert_join(eng, t_items, "semi", "total")
    assert kept == [(b"\x00", 2)]


def test_one_byte_word_last_in_the_bytes_buffer(eng):
    """The 16-byte load of a 1-byte last word reads the slack, on either side."""
    words, counts = C.last_is_one_byte()
    load(eng, (words, counts))
    eng.sort_result()
    t_items, _ = fetched(eng)
    assert t_items[-1][0] == b"~"
    eng.accumulate()  # T: "~" is the last byte of its bytes buffer
    load(eng, ([b"~", b"w7", b"none"], [4, 5, 6]))
    _, kept, _ = assert_join(eng, t_items, "semi", "total")
    assert sorted(kept) == [(b"w7", 8), (b"~", 301)]
    load(eng, (words[:50] + [b"~"], counts[:50] + [9]))
    eng.sort_result()  # R: the same
    items, kept, _ = assert_join(eng, t_items, "semi", "min")
    assert items[-1][0] == b"~" and kept[-1] == (b"~", 9) and len(kept) == 51


# ---- 4. counts modes
@pytest.mark.parametrize("counts", ["total", "min"])
def test_counts_modes(eng, counts):
    r, t = C.pair(3000, 2500, 41)
    t_items = load_total(eng, t)
    load(eng, r)
    items, kept, info = assert_join(eng, t_items, "semi", counts)
    tot = dict(t_items)
    assert len(kept) == 2500 // 3 and kept != [(w, c) for w, c in items if w in tot]  # the counts were substituted
    assert info["tokens_min"] < min(info["tokens_matched_result"], info["tokens_matched_total"])


def test_zero_count_total_word_is_held(eng):
    t_items = load_total(eng, ([b"zero", b"one", b"a_long_word_with_count_zero"], [0, 1, 0]))
    assert sorted(t_items) == [(b"a_long_word_with_count_zero", 0), (b"one", 1), (b"zero", 0)]
    r = ([b"zero", b"a_long_word_with_count_zero", b"two"], [5, 6, 7])
    load(eng, r)
    _, kept, info = assert_join(eng, t_items, "semi", "total")
    assert sorted(kept) == [(b"a_long_word_with_count_zero", 0), (b"zero", 0)] and info["tokens_kept"] == 0
    load(eng, r)
    _, kept, _ = assert_join(eng, t_items, "anti")
    assert kept == [(b"two", 7)]


def test_counts_of_2_to_the_64_minus_1(eng):
    U = C.U64
    t_items = load_total(eng, ([b"a", b"b", b"c", b"a_word_of_more_than_16_bytes"], [U, 3, U, U]))
    r = ([b"a", b"b", b"c", b"a_word_of_more_than_16_bytes", b"d"], [2, U, U, 9, U])
    load(eng, r)
    _, kept, info = assert_join(eng, t_items, "semi", "min")
    assert dict(kept) == {b"a": 2, b"b": 3, b"c": U, b"a_word_of_more_than_16_bytes": 9}
    assert info["tokens_kept"] == info["tokens_min"] == (U + 14) & U == 13  # the sums wrap
    load(eng, r)
    _, kept, info = assert_join(eng, t_items, "semi", "total")
    assert info["tokens_kept"] == (3 * U + 3) & U == 0 and dict(kept)[b"b"] == 3


def test_anti_with_substituted_counts_is_einval(eng):
    r, t = C.pair(100, 100, 43)
    load_total(eng, t)
    load(eng, r)
    before = fetched(eng)
    L = eng._L
    import ctypes
    info = mox.JoinInfo(words_in=77)
    for counts in (mox.JOIN_COUNTS_TOTAL, mox.JOIN_COUNTS_MIN):
        j = mox.Join(mode=mox.JOIN_ANTI, counts=counts)
        assert L.mox_join_total(eng._h, ctypes.byref(j), ctypes.byref(info)) == mox.MOX_EINVAL
    with pytest.raises(mox.MoxError) as ei:
        eng.join_total("anti", "total")
    assert ei.value.code == mox.MOX_EINVAL
    assert info.words_in == 77 and fetched(eng) == before
    assert L.mox_join_total(eng._h, ctypes.byref(mox.Join(mode=mox.JOIN_ANTI)), None) == mox.MOX_OK  # info may be NULL


# ---- 5. empty operands
def test_accumulator_never_folded_and_after_reset(eng):
    r, t = C.pair(700, 300, 51)
    load(eng, r)
    items, kept, info = assert_join(eng, [], "anti")  # no fold since create: an empty T
    assert kept == items and info["words_total"] == 0 == info["words_matched"]
    _, kept, _ = assert_join(eng, [], "semi", "total")
    assert kept == []
    assert_empty(eng)
    load_total(eng, t)
    eng.accumulate_reset()
    load(eng, r)
    items, kept, info = assert_join(eng, [], "anti")
    assert kept == items and info["tokens_total"] == 0
    _, kept, _ = assert_join(eng, [], "semi")
    assert kept == []
    assert_empty(eng)
    assert eng.accumulate_info()["passes"] == 0


def test_accumulator_holding_the_empty_table_and_an_empty_result(eng):
    r, t = C.pair(300, 300, 53)
    eng.count(b"").close()
    eng.accumulate()
    assert eng.accumulate_info()["passes"] == 1 and eng.accumulate_info()["words"] == 0
    semi, anti = assert_both_modes(eng, r, [])
    assert semi == [] and len(anti) == 300
    eng.accumulate_reset()
    t_items = load_total(eng, t)
    for mode, counts in (("semi", "result"), ("anti", "result"), ("semi", "min")):
        eng.count(b"").close()  # an empty R
        _, kept, info = assert_join(eng, t_items, mode, counts)
        assert kept == [] and info["words_total"] == 300 and info["words_in"] == 0
        assert_empty(eng)


# ---- 6. forms of R and of T
def test_sorted_result_stays_sorted(eng):
    r, t = C.pair(3000, 3000, 61)
    t_items = load_total(eng, t)
    load(eng, r)
    eng.sort_result()
    items, kept, _ = assert_join(eng, t_items, "semi", "total")
    assert [w for w, _ in items] == sorted(r[0]) and [w for w, _ in kept] == sorted(w for w, _ in kept) and len(kept) == 1000
    w, c = kept[417]
    first, last, sums = eng.find([w], mode="exact")  # find takes a sorted result only
    assert (int(first[0]), int(last[0]), int(sums[0])) == (417, 418, c)


def test_ranked_result_stays_ranked_with_its_own_counts_only(eng):
    r, t = C.pair(2000, 2000, 63)
    t_items = load_total(eng, t)
    load(eng, r)
    eng.rank_result()
    items, kept, _ = assert_join(eng, t_items, "semi", "result")
    assert [c for _, c in kept] == sorted((c for _, c in kept), reverse=True) and [w for w, _ in kept] != sorted(w for w, _ in kept)
    eng.set_flags(mox.MOX_F_SORT_BYTES)
    assert fetched(eng)[0] == kept  # still ranked: the implicit sort leaves it alone
    eng.set_flags(0)
    load(eng, r)
    eng.rank_result()
    _, kept, _ = assert_join(eng, t_items, "semi", "total")
    assert [c for _, c in kept] != sorted((c for _, c in kept), reverse=True)
    eng.set_flags(mox.MOX_F_SORT_BYTES)
    assert fetched(eng)[0] == sorted(kept)  # no longer ranked: the fetch sorts bytewise


def test_filtered_and_rekeyed_results(eng):
    r, t = C.pair(3000, 3000, 65)
    t_items = load_total(eng, t)
    load(eng, r)
    eng.filter_result(min_count=300)
    items, kept, _ = assert_join(eng, t_items, "semi", "min")  # from one filter set into the other
    assert 100 < len(kept) < len(items) < 3000
    _, kept2, _ = assert_join(eng, t_items, "anti")  # a joined result joins again
    assert kept2 == []
    punct = ([b"(" + w + b")," for w in r[0]], r[1])
    load(eng, punct)
    eng.rekey_result(trim=b"(),")
    items, kept, _ = assert_join(eng, t_items, "semi")
    assert dict(items) == dict(zip(*r)) and len(kept) == 1000


def test_result_is_the_total_itself(eng):
    _, t = C.pair(10, 2000, 67)
    t_items = load_total(eng, t)  # the result is still the table just folded
    items, kept, info = assert_join(eng, t_items, "semi", "min")
    assert kept == items == t_items and info["tokens_min"] == info["tokens_in"]
    with pytest.raises(mox.MoxError) as ei:
        eng.accumulate()  # folded state is R's
    assert ei.value.code == mox.MOX_ESTATE
    _, kept, _ = assert_join(eng, t_items, "anti")
    assert kept == []


def test_total_from_a_sorted_result_and_from_a_merge(eng):
    r, t = C.pair(1500, 1500, 69)
    load(eng, t)
    eng.sort_result()
    t_items, _ = fetched(eng)
    eng.accumulate()  # first fold: T is the saved sorted table
    semi, _ = assert_both_modes(eng, r, t_items)
    assert len(semi) == 500
    _, t2 = C.pair(1500, 2500, 70)  # shares the "s" words with t, under other counts
    load(eng, t2)
    eng.accumulate()  # second fold: T is a merge, in the engine's order
    t_items, _ = fetched(eng)
    assert len(t_items) == len(set(t[0]) | set(t2[0])) > 1500 and eng.accumulate_info()["passes"] == 2
    load(eng, r)
    _, kept, _ = assert_join(eng, t_items, "semi", "total")
    assert len(kept) == 500


# ---- 7. state
def test_count_only_changes_nothing(eng):
    r, t = C.pair(3000, 3000, 71)
    t_items = load_total(eng, t)
    load(eng, r)
    eng.sort_result()
    before = fetched(eng)
    text = eng.result_text()
    for mode, counts in (("semi", "total"), ("anti", "result")):
        dry = eng.join_total(mode, counts, count_only=True)
        assert {k: dry[k] for k in C.INFO_KEYS} == C.expected(before[0], t_items, mode, counts)[1]
        assert fetched(eng) == before and eng.result_text() == text
    assert int(eng.find([before[0][5][0]], mode="exact")[0][0]) == 5  # still sorted
    real = eng.join_total("anti")
    assert {k: real[k] for k in C.INFO_KEYS} == {k: dry[k] for k in C.INFO_KEYS}
    eng.accumulate()  # still an unfolded result: it folds, once
    with pytest.raises(mox.MoxError) as ei:
        eng.accumulate()
    assert ei.value.code == mox.MOX_ESTATE


def test_the_accumulator_is_untouched(eng):
    r, t = C.pair(2000, 2000, 73)
    t_items = load_total(eng, t)
    acc = eng.accumulate_info()
    load(eng, r)
    for mode, counts in (("semi", "total"), ("semi", "min"), ("anti", "result")):
        load(eng, r)
        eng.join_total(mode, counts)
        assert eng.accumulate_info() == acc
    eng.count(b"").close()
    eng.accumulate()  # a fresh fold of nothing: the result is the total
    got, tokens = fetched(eng)
    assert dict(got) == dict(t_items) and len(got) == len(t_items) and tokens == acc["tokens"]


def test_exchange_after_a_join_is_estate(eng):
    eng.count(b"one two two").close()
    eng.accumulate()
    eng.count(b"two three").close()
    eng.join_total("semi")
    before = fetched(eng)
    assert before == ([(b"two", 1)], 1)

    def never(*a):
        raise AssertionError("the transport is not reached")

    with pytest.raises(mox.MoxError) as ei:
        eng.exchange_host(1, 0, never)
    assert ei.value.code == mox.MOX_ESTATE
    assert fetched(eng) == before


def test_injected_failure_leaves_the_result(eng, monkeypatch):
    r, t = C.pair(3000, 3000, 75)
    t_items = load_total(eng, t)
    load(eng, r)
    before = fetched(eng)
    monkeypatch.setenv("MOX_TEST_FAIL_JOIN", "1")
    with pytest.raises(mox.MoxError) as ei:
        eng.join_total("semi", "total")
    assert ei.value.code == mox.MOX_ENOMEM
    assert fetched(eng) == before
    monkeypatch.delenv("MOX_TEST_FAIL_JOIN")
    assert_join(eng, t_items, "semi", "total")


def test_fresh_engine_is_estate(eng):
    with pytest.raises(mox.MoxError) as ei:
        eng.join_total()
    assert ei.value.code == mox.MOX_ESTATE


# ---- 8. cross-check against the filter's list term
def test_equals_the_filter_with_the_totals_words(eng):
    r, t = C.pair(4000, 2000, 81)
    t_items = load_total(eng, t)
    t_words = [w for w, _ in t_items]
    for mode, kw in (("semi", "keep"), ("anti", "drop")):
        load(eng, r)
        items, _ = fetched(eng)
        eng.filter_result(**{kw: t_words})
        by_filter = fetched(eng)
        eng.reduce_pairs([w for w, _ in items], [c for _, c in items]).close()
        assert sorted(fetched(eng)[0]) == sorted(items)
        _, kept, _ = assert_join(eng, t_items, mode)
        assert sorted(kept) == sorted(by_filter[0]) and len(kept) == len(by_filter[0]) > 600


# ---- 9. the streaming use
def test_new_words_per_window(eng):
    windows = [b"the cat and the dog and a bird", b"the end of the cat and a beta beta", "ΟΔΟΣ οδος the gamma beta of".encode()]
    seen, total = set(), {}
    for text in windows:
        counts = dict(coracle.count(text)[0])
        eng.count(text).close()
        info = eng.join_total("anti", count_only=True)
        assert info["words_kept"] == len(set(counts) - seen) > 0  # the words the stream has not shown before
        assert info["words_matched"] == len(set(counts) & seen) and info["words_total"] == len(seen)
        eng.accumulate()
        seen |= set(counts)
        for w, c in counts.items():
            total[w] = total.get(w, 0) + c
    got, tokens = fetched(eng)
    assert dict(got) == total == dict(coracle.count(b" ".join(windows))[0]) and tokens == sum(total.values())


# ---- 10. forced collisions
def test_forced_collisions():
    r, t = C.pair(600, 700, 91)
    long_words = [b"L%d-" % i + bytes(97 + (i * j) % 26 for j in range(70 + i)) for i in range(12)]
    r = (r[0] + long_words, r[1] + [5] * 12)
    t = (t[0] + long_words[::2], t[1] + [9] * 6)
    got = {}
    for path in (mox.LIB_PATH, mox.HC_LIB_PATH):
        e = mox.Engine(device=0, lib_path=path)
        try:
            t_items = load_total(e, t)
            load(e, r)
            _, kept, info = assert_join(e, t_items, "semi", "min")
            load(e, r)
            _, anti, _ = assert_join(e, t_items, "anti")
            got[path] = (sorted(kept), sorted(anti), info["tag_mismatch"])
        finally:
            e.close()
    plain, hc = got[mox.LIB_PATH], got[mox.HC_LIB_PATH]
    assert plain[:2] == hc[:2] and len(plain[0]) == 200 + 6
    assert hc[2] > 0 and plain[2] == 0  # every exact compare behind an equal tag ran


# ---- 10b. the lookup and the join are two policies over one word set (mox_wordset.h)
def cross_tables():
    """R of 1,025 rows and T of 2,049 (a tile and one row; two tiles and one row).  They share 512 short
    words, 6 of each side's 12 words over 64 bytes, a word T counts 0 times and b"ab" of R's b"ab" / b"ab\\0"."""
    short = [b"w%d" % i + b"x" * (i % 20) for i in range(1006 + 1519)]
    r_long = [b"L%d-" % i + bytes(97 + (i * j) % 26 for j in range(70 + i)) for i in range(12)]
    t_long = r_long[::2] + [b"M%d-" % i + b"z" * (65 + 3 * i) for i in range(6)]
    r_words = short[:1006] + r_long + [b"ab", b"ab\x00"] + [b"zero", b"a", b"r-only", b"q" * 64, b"q" * 63]
    t_words = short[494:1006] + short[1006:] + t_long + [b"ab"] + [b"zero", b"a", b"t-only", b"q" * 64, b"Q" * 63]
    t_counts = [0 if w == b"zero" else 3 + 2 * i for i, w in enumerate(t_words)]
    assert len(r_words) == len(set(r_words)) == 1025 and len(t_words) == len(set(t_words)) == 2049
    assert len(set(r_words) & set(t_words)) == 512 + 6 + 4 and len(set(r_long) & set(t_long)) == 6
    return (r_words, list(range(1, 1026))), (t_words, t_counts)


@pytest.mark.parametrize("path", [mox.LIB_PATH, mox.HC_LIB_PATH], ids=["plain", "hc"])
def test_lookup_and_join_agree_on_one_pair_of_tables(path):
    """With T as the result, the lookup of R's words finds exactly the rows that the SEMI join of R against T
    keeps, with the kept row's count and the row's position in T.  Each library truncates the tag differently."""
    from mox import spill

    r, t = cross_tables()
    data, offs, _ = spill.pack_pairs(r[0], [])
    e = mox.Engine(device=0, lib_path=path)
    try:
        load(e, t)
        t_items, _ = fetched(e)
        counts, index = e.lookup_packed(data, offs, with_index=True)
        e.accumulate()
        load(e, r)
        info = e.join_total("semi", "total")
        kept, _ = fetched(e)
    finally:
        e.close()
    assert len(t_items) == 2049 and info["words_in"] == 1025 and info["words_matched"] == len(kept) == 522
    kept_count = dict(kept)
    assert len(kept_count) == len(kept)
    for w, c, i in zip(r[0], counts.tolist(), index.tolist()):
        assert (i != mox.LOOKUP_NONE) == (w in kept_count), w  # found exactly where the join keeps the row
        if w in kept_count:
            assert c == kept_count[w] and t_items[i] == (w, c), w  # the kept row's count; the row's position in T
        else:
            assert c == 0, w
    assert kept_count[b"zero"] == 0 and b"ab" in kept_count and b"ab\x00" not in kept_count


# ---- 11. an engine group
def test_engine_group_joins_on_member_0():
    a = b"the cat and the dog and the bird " * 3 + b"alpha a_word_of_more_than_16_bytes"
    b = b"the end of the cat and a beta beta a_word_of_more_than_16_bytes"
    g = mox.Engine(device=0, n_gpus=2, transport=mox.XPORT_COPY, devices=[0, 0])
    try:
        g.count(a).close()
        t_items, _ = fetched(g)
        g.accumulate()
        g.count(b).close()
        items, kept, _ = assert_join(g, t_items, "semi", "total")
        wa, wb = dict(coracle.count(a)[0]), dict(coracle.count(b)[0])
        assert dict(items) == wb and dict(kept) == {w: wa[w] for w in wb if w in wa} and len(kept) == 4
        g.count(b).close()
        _, kept, _ = assert_join(g, t_items, "anti")
        assert dict(kept) == {w: c for w, c in wb.items() if w not in wa}
    finally:
        g.close()


# ---- 12. the command-line tool
def test_cli_not_in_and_also_in(tmp_path):
    from conftest import ROOT
    base = b"The cat and the dog.\nA bird, a cat\n"
    data = b"the cat saw (the) third cat; a fish and a FISH\n" + "ΟΔΟΣ οδος\n".encode()
    (tmp_path / "base.txt").write_bytes(base)
    (tmp_path / "shakes.txt").write_bytes(data)
    cli = os.path.join(ROOT, "map-oxidize_amd", "mox", "meduce-gpu")
    cb, cd = dict(coracle.count(base)[0]), dict(coracle.count(data)[0])
    for opt, keep in (("--not-in", lambda w: w not in cb), ("--also-in", lambda w: w in cb)):
        r = subprocess.run([cli, opt, "base.txt"], cwd=tmp_path, capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr
        want = {w: c for w, c in cd.items() if keep(w)}
        lines = (tmp_path / "final_result.txt").read_bytes().splitlines()
        assert sorted(lines) == sorted(w + b" %d" % c for w, c in want.items()) and 0 < len(lines) < len(cd)
    # with --trim-punct both sides are re-keyed before they meet, and --min-count applies to what the join kept
    r = subprocess.run([cli, "--also-in", "base.txt", "--trim-punct", "--min-count", "2"], cwd=tmp_path, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted((tmp_path / "final_result.txt").read_bytes().splitlines()) == [b"a 2", b"cat 2", b"the 2"]
