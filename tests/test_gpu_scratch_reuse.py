"""GPU: every call over the device-resident result on one engine whose scratch
buffers are reused across table sizes (mox_carve.h, mox_result.hip).  The sizes
are odd, so 4 n and 8 n bytes fall off every boundary an array behind them
needs; they cross the 1024-row and the 4096-row tiles; and they go large, small,
large, small, so a call lays its arrays out again in a buffer an earlier,
larger call grew.  Every answer is compared with what the *_cases.py models
give for the word list: no expectation comes from the library.  The table is
sorted first, so its order is known (bytewise) for every call that follows."""
import pytest

import filter_cases
import find_cases
import hist_cases
import join_cases
import lookup_cases
import mox
import rank_cases
import rekey_cases
import text_cases
import top_cases

pytestmark = pytest.mark.gpu

SIZES = (4097, 1, 1025, 3)
LONG = 300


def table(n, tag):
    """n distinct words with counts (ties and zeros among them): word n // 2 is
    LONG bytes long, every tenth word is its predecessor with a trailing comma."""
    words = [tag + b"%d" % i + b"q" * (i % 23) for i in range(n)]
    words[n // 2] = tag.upper() * LONG
    for i in range(9, n, 10):
        words[i] = words[i - 1] + b","
    assert len(set(words)) == n and len(words[n // 2]) == LONG
    return words, [(i * 37) % 101 for i in range(n)]


def fetched(e):
    t = e.fetch()
    try:
        return list(t.items()), t.tokens
    finally:
        t.close()


def check_size(e, n):
    words, counts = table(n, b"w")
    # the total: two of every three words of the table with another count, and three words the table lacks
    t_words = [w for i, w in enumerate(words) if i % 3 != 1] + [b"absent%d" % i for i in range(3)]
    t_items = [(w, (i * 53) % 97) for i, w in enumerate(t_words)]
    e.accumulate_reset()
    e.reduce_pairs(t_words, [c for _, c in t_items]).close()
    e.accumulate()
    assert e.accumulate_info()["words"] == len(t_items)

    e.reduce_pairs(words, counts).close()
    tokens = sum(counts)

    # sort: the order of everything below
    e.sort_result()
    items = sorted(zip(words, counts))
    assert fetched(e) == (items, tokens)

    # result text
    assert e.result_text() == text_cases.expected(items)

    # lookup, an odd number of query words: present and absent ones, the long word and a near miss of it
    queries = words[::3] + [b"none%d" % i for i in range(4)] + [words[n // 2], words[n // 2][:-1]]
    queries += [b"odd"] * (1 - len(queries) % 2)
    assert len(queries) % 2 == 1
    got_c, got_i = e.lookup(queries, with_index=True)
    want_c, want_i = lookup_cases.expected(items, queries)
    assert got_c.tolist() == want_c and got_i.tolist() == want_i

    # find: prefixes with many rows, one row and none; exact words
    keys = [b"", b"w", b"w1", b"w10", b"W", b"W" * LONG, b"W" * (LONG + 1), b"x", b"a"] + words[::97]
    for mode_name, mode in (("prefix", find_cases.PREFIX), ("exact", find_cases.EXACT)):
        first, last, sums = e.find(keys, mode_name)
        want = find_cases.expected(items, keys, mode)
        assert (first.tolist(), last.tolist(), sums.tolist()) == want, mode_name

    # histograms on count and on first
    for key in ("count", "first"):
        hk, hw, ht, hr, h_words, h_tokens = e.histogram(key)
        want = hist_cases.expected(items, key)
        assert list(zip(hk.tolist(), hw.tolist(), ht.tolist(), hr.tolist())) == want, key
        assert (h_words, h_tokens) == (n, tokens)

    # top-k
    t = e.top_words(10)
    try:
        assert list(t.items()) == top_cases.expected(items, 10)
    finally:
        t.close()

    # rank: stable over the bytewise order
    info = e.rank_result()
    items = rank_cases.expected(items)
    assert fetched(e) == (items, tokens)
    assert {k: info[k] for k in rank_cases.INFO_KEYS} == dict(rank_cases.info_of(items), tokens=tokens)

    # join against the total, the smaller count of both
    info = e.join_total("semi", "min")
    items, want = join_cases.expected(items, t_items, "semi", "min")
    assert {k: info[k] for k in join_cases.INFO_KEYS} == want
    assert fetched(e) == (items, want["tokens_kept"])

    # filter with a word list: kept words, dropped words and words the result does not hold
    drop = [w for w, _ in items[1::3]] + words[1::2][:5] + [b"nowhere"]
    info = e.filter_result(drop=drop)
    items, want = filter_cases.expected(items, drop=drop)
    assert {k: info[k] for k in filter_cases.INFO_KEYS} == want
    assert fetched(e) == (items, want["tokens_kept"])

    # re-key: the commas go, the rows that became equal are summed (the merged table is in the engine's order)
    info = e.rekey_result(punct=True)
    want_table, _, want = rekey_cases.expected(items, punct=True)
    assert {k: info[k] for k in want} == want
    got, got_tokens = fetched(e)
    assert sorted(got) == sorted(want_table) and got_tokens == want["tokens_out"]


def test_every_call_over_the_result_across_reused_buffers():
    e = mox.Engine(device=0)
    try:
        for n in SIZES:
            check_size(e, n)
    finally:
        e.close()
