"""GPU: the device ranking (mox_rank_result, map-oxidize_amd/csrc/mox_rank.hip)
and the row fetch (mox_fetch_rows) against Python's stable sorted() over the
fetched table.  Every comparison is exact: the expectation is
rank_cases.expected over a fetch() of the same device-resident result taken
immediately before the call, with no run in between (the engine order of words
longer than 16 bytes can differ from run to run).  Tables come from
Engine.reduce_pairs unless the case says otherwise.  The case tables and the
CPU checks of their shapes: rank_cases.py, test_rank_abi.py."""
import ctypes
import os
import subprocess

import pytest

import coracle
import filter_cases
import lookup_cases
import mox
import rank_cases as C
import top_cases
from mox import corpus

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


def load(e, words, counts):
    e.reduce_pairs(words, counts).close()


def text_of(items):
    return b"".join(w + b" %d\n" % c for w, c in items)


def rows(e, first, n):
    t = e.fetch_rows(first, n)
    try:
        return list(t.items()), t.tokens
    finally:
        t.close()


def assert_rank(e, ascending=False):
    """rank_result on e's resident result: table, tokens and info equal the
    stable Python sort of the fetch taken just before.  Returns (source items, ranked items, info)."""
    items, tokens = fetched(e)
    want = C.expected(items, ascending)
    info = e.rank_result(ascending=ascending)
    got, tokens2 = fetched(e)
    assert got == want
    assert tokens2 == tokens
    assert {k: info[k] for k in C.INFO_KEYS} == dict(C.info_of(items), tokens=tokens)
    assert info["ms"] > 0
    return items, want, info


# ---- 1. table-size edges
@pytest.mark.parametrize("ascending", [False, True])
@pytest.mark.parametrize("n", C.TABLE_NS)
def test_table_size_edges(eng, n, ascending):
    words, counts = lookup_cases.table_words(n, 300 + n)
    counts = [c % 300 for c in counts]  # ties at the larger sizes, a zero among them
    load(eng, words, counts)
    items, ranked, info = assert_rank(eng, ascending)
    assert len(items) == n == len(ranked)
    if n > 1:
        assert info["device_bytes"] > 0 and info["digit_passes"] == (2 if n > 255 else 1)


# ---- 2. grid strides
def test_four_strides_equal_the_uncapped_call(eng, monkeypatch):
    words = top_cases.names(C.STRIDE_N)
    counts = C.zipf_counts(C.STRIDE_N, 21, top=70000)
    load(eng, words, counts)
    items, free, info = assert_rank(eng)
    assert len(items) == C.STRIDE_N and info["digit_passes"] == 3
    monkeypatch.setenv("MOX_RANK_GRID", str(C.STRIDE_GRID))
    load(eng, words, counts)
    items2, capped, _ = assert_rank(eng)
    assert items2 == items  # (short words: the engine order is the same in both loads)
    assert capped == free  # the grid does not matter


def test_zipf_table_of_200000_rows(eng):
    counts = C.zipf_counts(C.ZIPF_N, 5)
    load(eng, top_cases.names(C.ZIPF_N), counts)
    _, ranked, info = assert_rank(eng)
    assert info["digit_passes"] == 3 and info["max_count"] == max(counts)
    assert [c for _, c in ranked] == sorted(counts, reverse=True)


def test_a_table_past_one_step_of_the_scans(eng):
    """More than TOP_STEP tiles: the one-workgroup scan of the tile bytes runs with its carry, the scan
    of the digit counts over many chunks, and every pass over rows strides its full grid.  Compared as arrays."""
    import numpy as np
    data = corpus.fill(corpus.HICARD, 17, 0, C.BIG_CORPUS).tobytes()
    t = eng.count(data)
    counts, offs, text = t.arrays()
    n, tokens = t.n, t.tokens
    t.close()
    assert n > C.TOP_STEP * C.TILE
    want_c, want_o, want_b = C.ranked_arrays(counts, offs, text)
    info = eng.rank_result()
    assert (info["words"], info["tokens"], info["max_count"]) == (n, tokens, int(counts.max()))
    t = eng.fetch()
    got_c, got_o, got_b = t.arrays()
    t.close()
    assert np.array_equal(got_c, want_c) and np.array_equal(got_o, want_o) and got_b == want_b


# ---- 3. stability
def test_all_counts_equal_is_the_identity(eng):
    n = 2 * C.TILE + 77
    load(eng, top_cases.names(n), [7] * n)
    items, ranked, info = assert_rank(eng)
    assert ranked == items and info["digit_passes"] == 1 and info["max_count"] == 7
    _, again, _ = assert_rank(eng, ascending=True)
    assert again == items


@pytest.mark.parametrize("ascending", [False, True])
@pytest.mark.parametrize("values", [(7, 300), (1, 2, 70000)])
def test_ties_straddle_every_boundary(eng, values, ascending):
    n = 3 * C.TILE + 100
    load(eng, top_cases.names(n), C.spread_counts(n, values, 9))
    items, ranked, _ = assert_rank(eng, ascending)
    assert C.straddles(items, values)
    # the order of the ties themselves: each value's words, in the order they had
    order = sorted(values, reverse=not ascending)
    assert [w for w, _ in ranked] == [w for v in order for w, c in items if c == v]


# ---- 4. digit edges
@pytest.mark.parametrize("ascending", [False, True])
@pytest.mark.parametrize("max_count,passes", C.DIGIT_EDGES)
def test_digit_edges(eng, max_count, passes, ascending):
    counts = C.digit_edge_counts(max_count)
    load(eng, top_cases.names(len(counts)), counts)
    items, ranked, info = assert_rank(eng, ascending)
    assert info["max_count"] == max_count and info["digit_passes"] == passes
    if max_count == 0:
        assert ranked == items  # no pass: the identity
    else:
        assert 0 in dict(ranked).values()  # zeros mixed in


@pytest.mark.parametrize("ascending", [False, True])
@pytest.mark.parametrize("case,passes", [("byte7_only", 8), ("byte0_only", 4)])
def test_counts_that_differ_in_one_byte(eng, case, passes, ascending):
    counts = getattr(C, case)()
    load(eng, top_cases.names(len(counts)), counts)
    _, _, info = assert_rank(eng, ascending)
    assert info["digit_passes"] == passes


# ---- 5. word shapes
@pytest.fixture(scope="module")
def shapes():
    return filter_cases.shape_table()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_word_shapes(eng, shapes, where):
    """Lengths 1, 7, 8, 9, 15, 16, 17, 63, 64, 65 and 100,000 bytes, the long word
    placed at either end of the ranking and in its middle; bytes compared exactly."""
    words, counts = shapes
    counts = [c % 1000 + 1 for c in counts]
    big = [i for i, w in enumerate(words) if len(w) == 100000][0]
    counts[big] = {"first": 5000, "middle": 500, "last": 0}[where]
    load(eng, words, counts)
    items, ranked, _ = assert_rank(eng)
    assert {len(w) for w, _ in items} >= {1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 100000}
    pos = [i for i, (w, _) in enumerate(ranked) if len(w) == 100000][0]
    assert {"first": pos == 0, "middle": 0 < pos < len(ranked) - 1, "last": pos == len(ranked) - 1}[where]
    _, back, _ = assert_rank(eng, ascending=True)
    assert len(back[-1 - pos][0]) == 100000 or where == "middle"


# ---- 6. a run's table
def test_a_real_run(eng):
    data = corpus.fill(corpus.UNICODE, 3, 0, 1 << 19).tobytes().decode("utf-8", "ignore").encode()
    data += b" " + b"x" * 300 + b" " + "ΣΊΣΥΦΟΣ".encode() * 9 + b" the the the"
    want = dict(coracle.count(data)[0])
    eng.count(data).close()
    items, ranked, info = assert_rank(eng)
    assert dict(ranked) == want and len(ranked) == len(want) > 100
    assert max(len(w) for w, _ in ranked) >= 300 and info["tokens"] == sum(want.values())


# ---- 7. every reader after a ranking
def test_readers_see_the_ranked_table(eng, tmp_path):
    words, counts = top_cases.many_equal()
    load(eng, words, counts)
    tops = {}
    for k in (1, 10, 4096):
        t = eng.top_words(k)
        tops[k] = list(t.items())
        t.close()
    items, ranked, _ = assert_rank(eng)
    for k, top in tops.items():
        assert top == ranked[:k] == top_cases.expected(items, k)
    assert eng.result_text() == text_of(ranked)
    eng.write_result(str(tmp_path / "out.txt"))
    assert (tmp_path / "out.txt").read_bytes() == text_of(ranked)
    queries = [w for w, _ in ranked[:300]] + [b"absent"]
    got_c, got_i = eng.lookup(queries, with_index=True)
    assert got_i.tolist() == list(range(300)) + [mox.LOOKUP_NONE]  # ranked positions
    assert got_c.tolist() == [c for _, c in ranked[:300]] + [0]


def test_filter_keeps_a_prefix_and_stays_ranked(eng):
    words, counts = top_cases.many_equal()
    load(eng, words, counts)
    _, ranked, _ = assert_rank(eng)
    eng.filter_result(min_count=4)
    kept = [wc for wc in ranked if wc[1] >= 4]
    assert fetched(eng)[0] == kept == ranked[:len(kept)] and 0 < len(kept) < len(ranked)
    eng.set_flags(mox.MOX_F_SORT_BYTES)  # still ranked: the flag's sort leaves it alone
    assert fetched(eng)[0] == kept


def test_accumulate_and_sort_after_a_ranking(eng):
    words, counts = top_cases.many_equal()
    load(eng, words, counts)
    items, ranked, _ = assert_rank(eng)
    eng.accumulate()  # the first fold: the result stays the (ranked) table it was
    assert fetched(eng)[0] == ranked
    load(eng, words[:100], [3] * 100)
    eng.rank_result()
    eng.accumulate()  # a merge of a ranked result: the same dict as ever
    want = dict(items)
    for w in words[:100]:
        want[w] += 3
    total = fetched(eng)[0]
    assert dict(total) == want and len(total) == len(want)
    eng.sort_result()
    assert fetched(eng)[0] == sorted(total)
    _, both, _ = assert_rank(eng)
    assert both == sorted(total, key=lambda wc: (-wc[1], wc[0]))


def test_ascending_after_descending(eng):
    """With distinct counts ascending after descending is ascending on the
    original, and the descending table reversed.  With ties only the first
    holds: both rankings are stable, so equal counts keep the original's order
    through both calls, and the ascending table is not the descending one
    reversed -- reversing would reverse the ties too."""
    words, counts = top_cases.distinct(3000, 8)
    load(eng, words, counts)
    items, _, _ = assert_rank(eng)
    _, up, _ = assert_rank(eng, ascending=True)
    assert up == C.expected(items, ascending=True) == sorted(items, key=lambda wc: wc[1])
    _, down, _ = assert_rank(eng)  # and ranking twice is legal, through both sets of output buffers
    assert down == up[::-1]
    words, counts = top_cases.many_equal()
    load(eng, words, counts)
    items, down, _ = assert_rank(eng)
    _, up, _ = assert_rank(eng, ascending=True)
    assert up == C.expected(items, ascending=True) and up != down[::-1]


# ---- 8. state
def test_sort_bytes_flag_leaves_a_ranking_alone():
    e = mox.Engine(device=0, flags=mox.MOX_F_SORT_BYTES)
    try:
        words, counts = top_cases.many_equal()
        load(e, words, counts)
        bytewise = fetched(e)[0]
        assert bytewise == sorted(zip(words, counts))
        want = C.expected(bytewise)
        e.rank_result()
        assert fetched(e)[0] == want and e.result_text() == text_of(want) and rows(e, 0, 50)[0] == want[:50]
        # whatever replaces the result ends the ranking: the table fetches bytewise again
        load(e, words[:500], counts[:500])
        assert fetched(e)[0] == sorted(zip(words[:500], counts[:500]))
        e.rank_result()
        e.count(b"b a c a").close()
        assert fetched(e)[0] == [(b"a", 2), (b"b", 1), (b"c", 1)]
        e.rank_result()
        e.accumulate()  # the first fold keeps the ranked table ...
        assert fetched(e)[0] == [(b"a", 2), (b"b", 1), (b"c", 1)]
        e.count(b"c c c").close()
        e.rank_result()
        e.accumulate()  # ... a merge replaces it
        assert fetched(e)[0] == [(b"a", 2), (b"b", 1), (b"c", 4)]
        e.rank_result()
        assert fetched(e)[0] == [(b"c", 4), (b"a", 2), (b"b", 1)]
        e.sort_result()  # an explicit sort ends the ranking too
        assert fetched(e)[0] == [(b"a", 2), (b"b", 1), (b"c", 4)]
    finally:
        e.close()


def test_exchange_after_a_ranking_is_estate(eng):
    eng.count(b"one two two").close()
    eng.rank_result()
    before = fetched(eng)

    def never(send, ss, rs):
        raise AssertionError("the transport is not reached")

    with pytest.raises(mox.MoxError) as ei:
        eng.exchange_host(1, 0, never)
    assert ei.value.code == mox.MOX_ESTATE
    assert fetched(eng) == before == ([(b"two", 2), (b"one", 1)], 3)


def test_errors_leave_the_result(eng, monkeypatch):
    with pytest.raises(mox.MoxError) as ei:
        eng.rank_result()
    assert ei.value.code == mox.MOX_ESTATE  # no result yet
    with pytest.raises(mox.MoxError) as ei:
        eng.fetch_rows(0, 1)
    assert ei.value.code == mox.MOX_ESTATE
    words, counts = top_cases.many_equal()
    load(eng, words, counts)
    before = fetched(eng)
    info = mox.RankInfo(words=77)
    assert eng._L.mox_rank_result(eng._h, 2, ctypes.byref(info)) == mox.MOX_EINVAL  # unknown flag bits
    assert eng._L.mox_rank_result(eng._h, 0x80000001, ctypes.byref(info)) == mox.MOX_EINVAL
    assert info.words == 77 and fetched(eng) == before
    monkeypatch.setenv("MOX_TEST_FAIL_RANK", "1")
    assert eng._L.mox_rank_result(eng._h, 0, ctypes.byref(info)) == mox.MOX_ENOMEM
    assert info.words == 77 and fetched(eng) == before
    eng.accumulate()  # still an unfolded result
    eng.accumulate_reset()
    monkeypatch.delenv("MOX_TEST_FAIL_RANK")
    assert eng._L.mox_rank_result(eng._h, 0, None) == mox.MOX_OK  # info may be NULL
    assert fetched(eng)[0] == C.expected(before[0])
    assert_rank(eng, ascending=True)


# ---- 9. fetch_rows
def pages(e, size, n):
    out = []
    for first in range(0, n + size, size):
        got, _ = rows(e, first, size)
        out += got
    return out


@pytest.mark.parametrize("order", ["engine", "sorted", "ranked"])
def test_pages_laid_end_to_end_are_the_table(eng, order):
    n = C.TILE + 37
    words, counts = lookup_cases.table_words(n, 77)
    load(eng, words, [c % 50 for c in counts])
    if order == "sorted":
        eng.sort_result()
    elif order == "ranked":
        eng.rank_result()
    items, tokens = fetched(eng)
    assert len(items) == n
    for size in (1, 7, C.TILE, n + 5):
        assert pages(eng, size, n) == items, size
    for first in (0, n - 1, n, n + 1):
        assert rows(eng, first, 3) == (items[first:first + 3], tokens), first  # tokens: the whole result's
    assert rows(eng, 5, 0) == ([], tokens) and rows(eng, 0, C.U64)[0] == items
    assert fetched(eng) == (items, tokens)  # the result stays where it is


def test_pages_of_the_shape_table(eng, shapes):
    words, counts = shapes
    load(eng, words, counts)
    items, _ = fetched(eng)
    assert pages(eng, 7, len(items)) == items  # the 100,000-byte word among them


def test_pages_are_bytewise_under_the_flag():
    e = mox.Engine(device=0)
    try:
        words, counts = filter_cases.random_words(3000, 5)
        load(e, words, counts)
        assert fetched(e)[0] != sorted(zip(words, counts))
        e.set_flags(mox.MOX_F_SORT_BYTES)
        assert pages(e, 1000, 3000) == sorted(zip(words, counts))  # the first page sorts, as fetch() would
    finally:
        e.close()


def test_rows_past_top_max_after_a_ranking(eng):
    n = 6000
    load(eng, top_cases.names(n), C.zipf_counts(n, 31, top=100000))
    items, ranked, _ = assert_rank(eng)
    got, tokens = rows(eng, 0, 5000)
    assert got == ranked[:5000] and len(got) == 5000 > C.TOP_MAX and tokens == sum(c for _, c in items)
    least, _ = rows(eng, n - 10, 10)
    assert least == ranked[-10:]


# ---- 10. an engine group
def test_engine_group_ranks_member_zeros_table():
    g = mox.Engine(device=0, n_gpus=2, transport=mox.XPORT_COPY, devices=[0, 0])
    try:
        data = corpus.fill(corpus.ZIPF, 9, 0, 1 << 18).tobytes()
        want = dict(coracle.count(data)[0])
        g.count(data).close()
        items, ranked, _ = assert_rank(g)
        assert dict(ranked) == want and len(ranked) == len(want)
        assert rows(g, 0, 20)[0] == ranked[:20]
        t = g.top_words(20)
        assert list(t.items()) == ranked[:20]
        t.close()
    finally:
        g.close()


# ---- 11. the other builds
@pytest.mark.parametrize("lib_path", [mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_other_builds(lib_path, shapes):
    e = mox.Engine(device=0, lib_path=lib_path)
    try:
        words, counts = shapes  # (forced collisions in reduce_pairs behind it)
        load(e, words, counts)
        _, ranked, _ = assert_rank(e)
        assert rows(e, 3, 40)[0] == ranked[3:43]
        assert_rank(e, ascending=True)
    finally:
        e.close()


# ---- 12. the command-line tool
def test_cli_by_count(tmp_path):
    from conftest import ROOT
    data = b"The cat and the other cat saw THE third cat\n" * 3 + b"a dog and a bird\n" + "ΟΔΟΣ οδος\n".encode() + b"x" * 40 + b"\n"
    (tmp_path / "shakes.txt").write_bytes(data)
    cli = os.path.join(ROOT, "map-oxidize_amd", "mox", "meduce-gpu")
    plain = subprocess.run([cli], cwd=tmp_path, capture_output=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    plain_file = (tmp_path / "final_result.txt").read_bytes()
    counts = dict(coracle.count(data)[0])
    assert sorted(plain_file.splitlines()) == sorted(w + b" %d" % c for w, c in counts.items())  # today's output
    order = [ln.rsplit(b" ", 1)[0] for ln in plain_file.splitlines()]
    top = sorted(order, key=lambda w: (-counts[w], order.index(w)))[:10]
    assert plain.stdout == b"Top 10 words:\n" + b"".join(w + b": %d\n" % counts[w] for w in top)
    r = subprocess.run([cli, "--by-count"], cwd=tmp_path, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = sorted(counts.items(), key=lambda wc: (-wc[1], wc[0]))
    assert (tmp_path / "final_result.txt").read_bytes() == text_of(want)
    assert r.stdout == b"Top 10 words:\n" + b"".join(w + b": %d\n" % c for w, c in want[:10])  # the file's first ten
    again = subprocess.run([cli], cwd=tmp_path, capture_output=True, timeout=120)
    assert again.stdout == plain.stdout and (tmp_path / "final_result.txt").read_bytes() == plain_file  # one long word: no slot race
