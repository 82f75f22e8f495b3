"""GPU: the device filter (mox_filter_result, map-oxidize_amd/csrc/mox_filter.hip)
against a plain Python filter over the fetched table.  Every comparison is
exact: the expectation is filter_cases.expected over a fetch() of the same
device-resident result taken immediately before the filter, with no run in
between (the engine order of words longer than 16 bytes can differ from run to
run).  After the call three things are compared: the fetched table, in order;
its tokens; the info.  Tables come from Engine.reduce_pairs unless the case
says otherwise.  The case tables and the CPU checks of their shapes:
filter_cases.py, test_filter_abi.py."""
import os
import subprocess

import pytest

import coracle
import filter_cases as C
import lookup_cases
import mox
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


def assert_filter(e, **pred):
    """filter_result(**pred) on e's resident result: table, tokens and info equal
    the Python filter over the fetch taken just before.  Returns (source items, kept items)."""
    items, _ = fetched(e)
    want, winfo = C.expected(items, **pred)
    info = e.filter_result(**pred)
    got, tokens = fetched(e)
    assert got == want
    assert tokens == winfo["tokens_kept"]
    assert {k: info[k] for k in C.INFO_KEYS} == winfo
    assert info["device_bytes"] > 0 and info["ms"] > 0
    return items, want


def assert_empty(e):
    """An empty result is a valid result for every reader."""
    assert fetched(e) == ([], 0)
    t = e.top_words(5)
    assert list(t.items()) == []
    t.close()
    assert e.result_text() == b""
    assert e.lookup([b"a"]).tolist() == [0]


# ---- 1. table-size edges
@pytest.mark.parametrize("n", C.TABLE_NS)
def test_table_size_edges(eng, n):
    words, counts = C.table_words(n, 200 + n)
    load(eng, words, counts)
    items, kept = assert_filter(eng, min_count=n // 2)
    assert len(items) == n and len(kept) == n - max(0, n // 2 - 1)
    load(eng, words, counts)
    items, kept = assert_filter(eng)  # the zeroed filter keeps everything
    assert kept == items and len(kept) == n
    _, kept = assert_filter(eng, min_count=n + 1)  # ... and this one nothing
    assert kept == []
    assert_empty(eng)


# ---- 2. grid strides
def test_three_strides(eng, monkeypatch):
    words, counts = C.table_words(C.STRIDE_N, 5)
    pred = dict(min_count=C.STRIDE_N // 3, drop=words[::7], max_len=20)
    load(eng, words, counts)
    items, free = assert_filter(eng, **pred)
    assert len(items) == C.STRIDE_N and 1000 < len(free) < len(items)
    monkeypatch.setenv("MOX_FILTER_GRID", str(C.STRIDE_GRID))
    load(eng, words, counts)
    _, capped = assert_filter(eng, **pred)
    assert dict(capped) == dict(free) and len(capped) == len(free)  # the grid does not matter


# ---- 3. each term's edges
def test_count_term_edges(eng):
    words, counts = C.table_words(300, 31)
    load(eng, words, counts)
    _, kept = assert_filter(eng, min_count=counts[17], max_count=counts[17])
    assert kept == [(words[17], counts[17])]
    load(eng, words, counts)
    _, kept = assert_filter(eng, min_count=200, max_count=100)  # min > max: nothing
    assert kept == []


def test_zero_count_words(eng):
    zw = [b"zero", b"one", b"a_long_word_with_count_zero"]
    load(eng, zw, [0, 1, 0])
    _, kept = assert_filter(eng)
    assert sorted(kept) == sorted(zip(zw, [0, 1, 0]))  # {0, 0} is "any count"
    _, kept = assert_filter(eng, min_count=1)
    assert kept == [(b"one", 1)]


@pytest.fixture(scope="module")
def shapes():
    return C.shape_table()


@pytest.mark.parametrize("term", ["max_len", "min_len"])
@pytest.mark.parametrize("edge", [15, 16, 17, 63, 64, 65, 100000])
def test_length_term_edges(eng, shapes, term, edge):
    words, counts = shapes
    load(eng, words, counts)
    # max_len = edge - 1 / edge and min_len = edge / edge + 1: the words of `edge` bytes on both sides
    first = edge - 1 if term == "max_len" else edge
    items, a = assert_filter(eng, **{term: first})
    load(eng, words, counts)
    _, b = assert_filter(eng, **{term: first + 1})
    n_edge = sum(len(w) == edge for w, _ in items)
    assert n_edge >= 1 and abs(len(a) - len(b)) == n_edge
    if term == "min_len":
        assert max(len(w) for w, _ in a) == 100000  # the long word is copied by a wave, next to lane-copied ones


PREFIXES = [b"a", b"a" * 8, b"a" * 9, b"a" * 16,  # 1, 8, 9, 16 bytes; "a" * 16 is a whole word, and longer than "a" * 15
            b"Q", "ΣΊΣΥ".encode(), b"L" * 16, b"a\x00", b"\x00", b"\x00\x00", b"n" * 16, b"x" * 16, b"zz-none"]


@pytest.mark.parametrize("prefix", PREFIXES)
def test_prefix_term_edges(eng, shapes, prefix):
    words, counts = shapes
    load(eng, words, counts)
    items, kept = assert_filter(eng, prefix=prefix)
    assert [w for w, _ in kept] == [w for w, _ in items if w[:len(prefix)] == prefix]
    if prefix == b"a" * 16:
        got = {w for w, _ in kept}
        assert b"a" * 16 in got and b"a" * 15 not in got and b"a" * 70 in got
    if prefix == b"\x00":
        assert {w for w, _ in kept} == {b"\x00", b"\x00\x00"}
    assert bool(kept) == (prefix != b"zz-none")


def test_prefix_of_17_bytes_is_einval(eng, shapes):
    load(eng, *shapes)
    before = fetched(eng)
    with pytest.raises(mox.MoxError) as ei:
        eng.filter_result(prefix=b"a" * 17)
    assert ei.value.code == mox.MOX_EINVAL
    assert fetched(eng) == before


def test_prefix_matches_only_a_one_byte_last_word(eng):
    words, counts = C.last_is_one_byte()
    load(eng, words, counts)
    eng.sort_result()
    items, _ = fetched(eng)
    assert items[-1][0] == b"~"
    _, kept = assert_filter(eng, prefix=b"~")
    assert kept == [items[-1]]


# ---- 4. the list term
@pytest.fixture(scope="module")
def rand3000():
    return C.random_words(3000, 41)


@pytest.mark.parametrize("mode", ["drop", "keep"])
@pytest.mark.parametrize("n", C.LIST_NS)
def test_list_sizes(eng, rand3000, mode, n):
    words, counts = rand3000
    load(eng, words, counts)
    lw = C.list_words(words, n, 42 + n)
    items, kept = assert_filter(eng, **{mode: lw})
    hit = len(set(lw) & set(words))
    assert hit >= 1 and len(kept) == (len(items) - hit if mode == "drop" else hit)


def test_near_misses_do_not_match(eng, shapes):
    words, counts = shapes
    load(eng, words, counts)
    probe = [w for w in words if 1 < len(w) <= 70][:40]
    lw = [m for w in probe for m in C.near_misses(w)]
    table = set(words)
    items, kept = assert_filter(eng, keep=lw)
    assert {w for w, _ in kept} == set(lw) & table and len(kept) < len(lw) // 2
    load(eng, words, counts)
    _, kept = assert_filter(eng, drop=[m for m in lw if m not in table])  # only near misses: nothing goes
    assert len(kept) == len(words)


def test_keep_nothing_and_drop_nothing(eng, rand3000):
    load(eng, *rand3000)
    items, kept = assert_filter(eng, drop=[])
    assert kept == items
    _, kept = assert_filter(eng, keep=[])
    assert kept == []
    assert_empty(eng)


def test_list_of_lookup_max_plus_one_is_einval(eng, rand3000):
    load(eng, *rand3000)
    before = fetched(eng)
    mat, offs = lookup_cases.fixed_width_queries(C.LOOKUP_MAX + 1)
    with pytest.raises(mox.MoxError) as ei:
        eng.filter_result_packed(mat.reshape(-1), offs)
    assert ei.value.code == mox.MOX_EINVAL
    assert fetched(eng) == before
    n = 5000
    info = eng.filter_result_packed(mat[:n].reshape(-1), offs[:n + 1], keep=True, count_only=True)  # the packed form works
    assert info["words_kept"] == 0 == info["list_found"]


# ---- 5. all terms together
ALL_TERMS = dict(min_count=2, max_count=10 ** 9, min_len=2, max_len=100, prefix=b"a")


def test_all_terms_on_the_shape_table(eng, shapes):
    words, counts = shapes
    load(eng, words, counts)
    items, kept = assert_filter(eng, drop=[b"a" * 5, b"a" * 64, b"nope", b"a" * 5], **ALL_TERMS)
    assert 50 < len(kept) < 100 and (b"a" * 5) not in dict(kept) and (b"a" * 65) in dict(kept)


def test_all_terms_and_filtering_twice(eng):
    words, counts = C.random_words(5000, 51)
    stop = C.list_words(words, 300, 52)
    load(eng, words, counts)
    items, once = assert_filter(eng, min_count=5, max_count=30, min_len=3, max_len=20, prefix=b"un", drop=stop)
    assert 10 < len(once) < 500
    # the same in three calls: the conjunction, through both sets of output buffers
    eng.reduce_pairs([w for w, _ in items], [c for _, c in items]).close()
    src, _ = fetched(eng)
    assert_filter(eng, min_count=5, max_count=30)
    assert_filter(eng, min_len=3, max_len=20, drop=stop)
    _, thrice = assert_filter(eng, prefix=b"un")
    assert thrice == C.expected(src, min_count=5, max_count=30, min_len=3, max_len=20, prefix=b"un", drop=stop)[0]
    assert dict(thrice) == dict(once)


# ---- 6. order and flags
def test_order_is_the_sources(eng):
    words, counts = C.random_words(4000, 61)
    load(eng, words, counts)
    items, kept = assert_filter(eng, min_count=10)  # engine order
    assert [w for w, _ in items] != sorted(words) and len(kept) > 1000
    load(eng, words, counts)
    eng.sort_result()
    items, kept = assert_filter(eng, min_count=10, prefix=b"b")
    assert [w for w, _ in kept] == sorted(w for w, _ in kept) and len(kept) > 100
    eng.set_flags(mox.MOX_F_SORT_BYTES)  # a sorted result's subset is sorted: the fetch has nothing to do
    assert fetched(eng)[0] == kept


def test_on_an_accumulated_total(eng):
    a = corpus.fill(corpus.ZIPF, 7, 0, 1 << 19).tobytes()
    b = corpus.fill(corpus.ZIPF, 8, 0, 1 << 19).tobytes()
    eng.count(a).close()
    eng.accumulate()
    eng.count(b).close()
    eng.accumulate()
    items, kept = assert_filter(eng, min_count=3, min_len=3)
    wa, wb = dict(coracle.count(a)[0]), dict(coracle.count(b)[0])
    total = {w: wa.get(w, 0) + wb.get(w, 0) for w in set(wa) | set(wb)}
    assert dict(items) == total and dict(kept) == {w: c for w, c in total.items() if c >= 3 and len(w) >= 3}
    info = eng.accumulate_info()
    assert info["passes"] == 2 and info["words"] == len(total)  # the accumulator is untouched
    with pytest.raises(mox.MoxError) as ei:
        eng.accumulate()  # a subset of a folded total is folded
    assert ei.value.code == mox.MOX_ESTATE


# ---- 7. composition
def test_readers_see_the_subset(eng, shapes):
    words, counts = shapes
    load(eng, words, counts)
    _, kept = assert_filter(eng, min_count=20, drop=[b"Q", b"x" * 17])
    for k in (1, 10, 64, 200):
        t = eng.top_words(k)
        assert list(t.items()) == top_cases.expected(kept, k) and t.tokens == sum(c for _, c in kept)
        t.close()
    assert eng.result_text() == text_of(kept)
    queries = [w for w in words[:500]] + [b"Q", b"absent"]
    got_c, got_i = eng.lookup(queries, with_index=True)
    want_c, want_i = lookup_cases.expected(kept, queries)
    assert got_c.tolist() == want_c and got_i.tolist() == want_i
    eng.sort_result()
    assert fetched(eng)[0] == sorted(kept)


def test_run_filter_accumulate(eng):
    a = b"the cat and the dog and the bird " * 3 + b"alpha"
    b = b"the end of the cat and a beta beta"
    stop = [b"the", b"and", b"a", b"of", b"The"]
    for text in (a, b):
        eng.count(text).close()
        eng.filter_result(drop=stop)
        eng.accumulate()
    wa, wb = dict(coracle.count(a)[0]), dict(coracle.count(b)[0])
    total = {w: wa.get(w, 0) + wb.get(w, 0) for w in set(wa) | set(wb) if w not in stop}
    items, tokens = fetched(eng)
    assert dict(items) == total and tokens == sum(total.values())
    assert eng.accumulate_info()["tokens"] == tokens
    # prune the running total: the pruned table becomes the new total
    _, kept = assert_filter(eng, min_count=2)
    assert dict(kept) == {w: c for w, c in total.items() if c >= 2} and len(kept) < len(total)
    with pytest.raises(mox.MoxError) as ei:
        eng.accumulate()
    assert ei.value.code == mox.MOX_ESTATE
    eng.accumulate_reset()
    eng.accumulate()
    info = eng.accumulate_info()
    assert info["passes"] == 1 and info["words"] == len(kept) and info["tokens"] == sum(c for _, c in kept)
    eng.count(b"cat gamma").close()
    eng.accumulate()
    want = dict(kept)
    want[b"cat"] = want.get(b"cat", 0) + 1
    want[b"gamma"] = 1
    assert dict(fetched(eng)[0]) == want


# ---- 8. a real run
def test_a_real_run_against_the_oracle(eng):
    data = corpus.fill(corpus.UNICODE, 3, 0, 1 << 20).tobytes().decode("utf-8", "ignore").encode()
    want, _ = coracle.count(data)
    top10 = [w for w, _ in sorted(want, key=lambda x: -x[1])[:10]]
    eng.count(data).close()
    info = eng.filter_result(min_count=3, min_len=4, drop=top10)
    kept, winfo = C.expected(want, min_count=3, min_len=4, drop=top10)
    got, tokens = fetched(eng)
    assert dict(got) == dict(kept) and len(got) == len(kept) > 100
    assert tokens == winfo["tokens_kept"] and {k: info[k] for k in C.INFO_KEYS} == winfo
    assert info["list_found"] == 10


# ---- 9. read-only and failure paths
def test_count_only_changes_nothing(eng, shapes):
    words, counts = shapes
    pred = dict(min_count=50, prefix=b"r", drop=[b"r17", b"r18"])
    load(eng, words, counts)
    before = fetched(eng)
    text, top = eng.result_text(), list(eng.top_words(20).items())
    dry = eng.filter_result(count_only=True, **pred)
    assert {k: dry[k] for k in C.INFO_KEYS} == C.expected(before[0], **pred)[1]
    assert fetched(eng) == before and eng.result_text() == text and list(eng.top_words(20).items()) == top
    eng.accumulate()  # the result is still the run's: it folds, once
    with pytest.raises(mox.MoxError) as ei:
        eng.accumulate()
    assert ei.value.code == mox.MOX_ESTATE
    assert fetched(eng) == before
    real = eng.filter_result(**pred)
    assert {k: real[k] for k in C.INFO_KEYS} == {k: dry[k] for k in C.INFO_KEYS}


def test_injected_failure_leaves_the_result(eng, rand3000, monkeypatch):
    load(eng, *rand3000)
    before = fetched(eng)
    monkeypatch.setenv("MOX_TEST_FAIL_FILTER", "1")
    with pytest.raises(mox.MoxError) as ei:
        eng.filter_result(min_count=10)
    assert ei.value.code == mox.MOX_ENOMEM
    assert fetched(eng) == before
    eng.accumulate()  # still an unfolded result
    monkeypatch.delenv("MOX_TEST_FAIL_FILTER")
    assert_filter(eng, min_count=10)


def test_fresh_engine_is_estate(eng):
    with pytest.raises(mox.MoxError) as ei:
        eng.filter_result(min_count=1)
    assert ei.value.code == mox.MOX_ESTATE


def test_bad_arguments_are_einval(eng):
    import ctypes
    load(eng, [b"a", b"b"], [1, 2])
    before = fetched(eng)
    L = eng._L
    info = mox.FilterInfo(words_in=77)

    def call(**kw):
        f = mox.Filter()
        for k, v in kw.items():
            setattr(f, k, v)
        return L.mox_filter_result(eng._h, ctypes.byref(f), ctypes.byref(info))

    down = (ctypes.c_uint64 * 3)(0, 2, 1)
    ok = (ctypes.c_uint64 * 3)(0, 1, 2)
    buf = ctypes.create_string_buffer(b"ab")
    assert call(words=ctypes.addressof(buf), word_offs=down, n_words=2) == mox.MOX_EINVAL
    assert call(word_offs=ok, n_words=2) == mox.MOX_EINVAL  # words is needed
    assert call(words=ctypes.addressof(buf), n_words=2) == mox.MOX_EINVAL  # word_offs is needed
    assert call(prefix_len=1) == mox.MOX_EINVAL  # prefix is needed
    assert call(words_mode=2) == mox.MOX_EINVAL and call(flags=2) == mox.MOX_EINVAL
    bad = mox.Filter()
    bad.reserved[3] = 1
    assert L.mox_filter_result(eng._h, ctypes.byref(bad), ctypes.byref(info)) == mox.MOX_EINVAL
    assert info.words_in == 77 and fetched(eng) == before
    assert call(words=ctypes.addressof(buf), word_offs=ok, n_words=2, words_mode=mox.FILTER_WORDS_KEEP) == mox.MOX_OK
    assert info.words_in == 2 and info.words_kept == 2 and info.list_found == 2
    assert L.mox_filter_result(eng._h, ctypes.byref(mox.Filter()), None) == mox.MOX_OK  # info may be NULL


# ---- 10. the other builds
@pytest.mark.parametrize("lib_path", [mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_other_builds(lib_path, shapes):
    e = mox.Engine(device=0, lib_path=lib_path)
    try:
        words, counts = shapes
        load(e, words, counts)
        assert_filter(e, prefix=b"a" * 9)  # item 3
        load(e, words, counts)
        lw = C.list_words(words, 65, 101) + [w for w in words if len(w) > 64][:5]
        _, kept = assert_filter(e, keep=lw)  # item 4 (the forced-collision lookup behind it)
        assert len(kept) == len(set(lw) & set(words))
        load(e, words, counts)
        assert_filter(e, drop=[b"a" * 5, b"a" * 64, b"nope"], **ALL_TERMS)  # item 5
    finally:
        e.close()


# ---- 11. the command-line tool
def test_cli_min_count_and_stop(tmp_path):
    from conftest import ROOT
    data = b"The cat and the other cat saw THE third cat\n" * 3 + b"a dog and a bird\n" + "ΟΔΟΣ οδος\n".encode()
    (tmp_path / "shakes.txt").write_bytes(data)
    (tmp_path / "stop.txt").write_bytes(b"the and\ta\n\nThe  nosuchword \n")
    cli = os.path.join(ROOT, "map-oxidize_amd", "mox", "meduce-gpu")
    plain = subprocess.run([cli], cwd=tmp_path, capture_output=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    plain_file = (tmp_path / "final_result.txt").read_bytes()
    counts = dict(coracle.count(data)[0])
    assert sorted(plain_file.splitlines()) == sorted(w + b" %d" % c for w, c in counts.items())  # today's output
    r = subprocess.run([cli, "--min-count", "2", "--stop", "stop.txt"], cwd=tmp_path, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = {w: c for w, c in counts.items() if c >= 2 and w not in (b"the", b"and", b"a", b"The", b"nosuchword")}
    assert want == {b"cat": 9, b"other": 3, b"saw": 3, b"third": 3, "οδος".encode(): 2}
    lines = (tmp_path / "final_result.txt").read_bytes().splitlines()
    assert sorted(lines) == sorted(w + b" %d" % c for w, c in want.items()) and len(lines) == len(want)
    # the top ten: count descending, ties in the file's (table) order
    order = [ln.rsplit(b" ", 1)[0] for ln in lines]
    top = sorted(order, key=lambda w: (-want[w], order.index(w)))
    assert r.stdout == b"Top 10 words:\n" + b"".join(w + b": %d\n" % want[w] for w in top)
    again = subprocess.run([cli], cwd=tmp_path, capture_output=True, timeout=120)
    assert again.stdout == plain.stdout and sorted((tmp_path / "final_result.txt").read_bytes().splitlines()) == sorted(plain_file.splitlines())
    assert len(plain_file.splitlines()) == len(counts)
