"""GPU: the device search of the sorted result (mox_find_ranges,
map-oxidize_amd/csrc/mox_find.hip) and the top-k of a row range (mox_top_rows)
against Python's bytes order and bisect over the fetched table.  Every
comparison is exact: the expectation is find_cases.expected over a fetch() of
the same device-resident result, with no run in between.  Tables come from
Engine.reduce_pairs + sort_result() unless the case says otherwise (reduce_pairs
takes no empty word, so a word of length 0 appears as a key only).  The model,
the case tables and the CPU checks of both: find_cases.py, test_find_abi.py."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import coracle
import find_cases as C
import mox
from conftest import ROOT
from mox import corpus

pytestmark = pytest.mark.gpu

U64P = ctypes.POINTER(ctypes.c_uint64)


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


def load_sorted(e, words, counts):
    """words / counts as the engine's result, in bytewise order; the fetched items."""
    e.reduce_pairs(words, counts).close()
    e.sort_result()
    items, _ = fetched(e)
    assert [w for w, _ in items] == sorted(words)
    return items


def table_of(t):
    """A Table as comparable values, closed."""
    try:
        counts, offs, data = t.arrays()
        return counts.tolist(), offs.tolist(), data, t.tokens
    finally:
        t.close()


def assert_find(e, items, keys, mode_name, mode):
    """find on e's resident result equals the model, in first, last, sums and info; without sums the same ranges."""
    want = C.expected(items, keys, mode)
    first, last, sums, info = e.find(keys, mode_name, with_info=True)
    assert first.tolist() == want[0]
    assert last.tolist() == want[1]
    assert sums.tolist() == want[2]
    assert {k: info[k] for k in ("queries", "matched", "rows")} == C.info_of(want[0], want[1])
    assert info["tile_pass"] == int(any(C.holds_tile(a, b) for a, b in zip(want[0], want[1])))
    assert info["ms"] > 0 and (info["device_bytes"] > 0 or not keys)
    f2, l2, info2 = e.find(keys, mode_name, with_sums=False, with_info=True)
    assert f2.tolist() == want[0] and l2.tolist() == want[1] and info2["tile_pass"] == 0
    return first, last, sums, info


def raw_find(e, keys, mode, fill=(11, 12, 13)):
    """mox_find_ranges through ctypes with prefilled outputs: (rc, first, last, sums, info)."""
    data = b"".join(keys)
    offs = np.zeros(len(keys) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(k) for k in keys])
    first, last, sums = (np.full(len(keys), v, dtype=np.uint64) for v in fill)
    info = mox.FindInfo(queries=5, matched=6, rows=7, tile_pass=8, device_bytes=9)
    rc = e._L.mox_find_ranges(e._h, ctypes.c_char_p(data), offs.ctypes.data_as(U64P), len(keys), mode, first.ctypes.data_as(U64P),
                              last.ctypes.data_as(U64P), sums.ctypes.data_as(U64P), ctypes.byref(info))
    return rc, first.tolist(), last.tolist(), sums.tolist(), (info.queries, info.matched, info.rows, info.tile_pass, info.device_bytes)


UNTOUCHED = (5, 6, 7, 8, 9)


# ---- 1. table sizes
@pytest.mark.parametrize("n", C.TABLE_NS)
def test_table_size_edges(eng, n):
    words, counts = C.table_words(n, 40 + n)
    items = load_sorted(eng, words, counts)
    assert len(items) == n
    keys = C.keys_around(words, seed=n)
    for name, mode in C.MODES:
        assert_find(eng, items, keys, name, mode)


# ---- 2. grid strides
def test_three_strides_equal_the_uncapped_call(eng, monkeypatch):
    words, counts = C.table_words(C.STRIDE_N, 7)
    items = load_sorted(eng, words, counts)
    keys = C.keys_around(words, seed=8)
    free = {name: assert_find(eng, items, keys, name, mode) for name, mode in C.MODES}
    assert free["prefix"][3]["tile_pass"] == 1  # the empty key is every row: k_fd_tiles strides too
    monkeypatch.setenv("MOX_FIND_GRID", str(C.STRIDE_GRID))
    for name, mode in C.MODES:
        capped = assert_find(eng, items, keys, name, mode)
        for a, b in zip(free[name][:3], capped[:3]):
            assert np.array_equal(a, b)  # the grid does not matter


# ---- 3. compare edges
def test_compare_edges(eng):
    words, counts = C.edge_table()
    items = load_sorted(eng, words, counts)
    keys = C.edge_keys(words)
    for name, mode in C.MODES:
        assert_find(eng, items, keys, name, mode)
    # spelled out: "ab" against "ab\0", a key that is a proper prefix of a word and the reverse, unsigned bytes
    pos = {w: i for i, (w, _) in enumerate(items)}
    first, last = eng.find([b"ab", b"ab\x00", b"m" * 10, b"m" * 19, b"q" * 11 + b"\x80"], "exact", with_sums=False)
    assert pos[b"ab\x00"] == pos[b"ab"] + 1
    assert first.tolist()[:3] == [pos[b"ab"], pos[b"ab\x00"], pos[b"m" * 10]] and (last - first).tolist() == [1, 1, 1, 0, 1]
    assert pos[b"q" * 11 + b"\x7f"] < pos[b"q" * 11 + b"\x80"] < pos[b"q" * 11 + b"\xff"]
    first, last = eng.find([b"m" * 18, b"m" * 66, b"z" * 199], "prefix", with_sums=False)
    assert (last - first).tolist() == [5, 1, 7]  # m x 18, 63, 64, 65, 300; m x 300; the seven 200-byte words


# ---- 4. sums across the tile logic
@pytest.mark.parametrize("groups,ranges", [(C.TILE_GROUPS_A, C.TILE_RANGES_A), (C.TILE_GROUPS_B, C.TILE_RANGES_B)])
def test_sums_across_the_tile_logic(eng, groups, ranges):
    words, counts = C.group_table(groups, 31)
    items = load_sorted(eng, words, counts)
    keys = [k for k, _, _ in ranges]
    first, last, sums, info = assert_find(eng, items, keys, "prefix", C.PREFIX)
    assert list(zip(first.tolist(), last.tolist())) == [(a, b) for _, a, b in ranges]
    # one key per call: the pass over the counts runs exactly when the range holds an aligned whole tile
    for k, a, b in ranges:
        _, _, s1, i1 = assert_find(eng, items, [k], "prefix", C.PREFIX)
        assert i1["tile_pass"] == int(C.holds_tile(a, b)), k
        assert s1.tolist() == [sum(c for _, c in items[a:b]) & C.U64]
    small = [k for k, a, b in ranges if not C.holds_tile(a, b)]
    assert small and assert_find(eng, items, small, "prefix", C.PREFIX)[3]["tile_pass"] == 0


# ---- 5. wrapping sums
def test_sums_wrap_as_the_models(eng):
    words = [b"w%02d" % i for i in range(len(C.WRAP_COUNTS))] + [b"a", b"x"]
    counts = list(C.WRAP_COUNTS) + [7, 9]
    items = load_sorted(eng, words, counts)
    first, last, sums, _ = assert_find(eng, items, [b"w", b"w0", b"", b"w01", b"w02"], "prefix", C.PREFIX)
    assert sums.tolist()[0] == sum(C.WRAP_COUNTS) & C.U64 == 2 and (last - first).tolist()[0] == len(C.WRAP_COUNTS)
    assert sums.tolist()[2] == (sum(C.WRAP_COUNTS) + 16) & C.U64
    _, _, sums, _ = assert_find(eng, items, [b"w00", b"w01", b"w02", b"nope"], "exact", C.EXACT)
    assert sums.tolist() == [0, 1, C.U64, 0]
    got = eng.find([b"w", b"a"], "prefix", with_sums=False)
    assert len(got) == 2 and got[0].tolist() == [1, 0] and got[1].tolist() == [1 + len(C.WRAP_COUNTS), 1]


# ---- 6. cross-checks against what exists
def test_exact_equals_the_lookup_and_prefix_the_filter(eng):
    words, counts = C.table_words(3000, 19)
    items = load_sorted(eng, words, counts)
    keys = C.keys_around(words[::7], seed=20)
    first, last, sums = eng.find(keys, "exact")
    lk_counts, lk_index = eng.lookup(keys, with_index=True)
    found = last > first
    assert np.array_equal(sums, lk_counts)
    assert np.array_equal(lk_index[found], first[found]) and (lk_index[~found] == mox.LOOKUP_NONE).all()
    assert found.sum() >= len(words[::7])
    prefixes = [b"t1", b"t29", b"\xc3", b"\xc31", b"t", b"", b"zz", b"t2999" + b"_" * 11]
    first, last, sums = eng.find(prefixes, "prefix")
    for p, a, b, s in zip(prefixes, first.tolist(), last.tolist(), sums.tolist()):
        assert len(p) <= mox.FILTER_PREFIX_MAX
        info = eng.filter_result(prefix=p, count_only=True)
        assert (info["words_kept"], info["tokens_kept"]) == (b - a, s), p
        t = eng.fetch_rows(a, b - a)
        assert list(t.items()) == [it for it in items if it[0].startswith(p)], p
        t.close()


# ---- 7. state
def test_unsorted_and_ranked_results_are_estate(eng):
    words, counts = C.table_words(500, 23)
    eng.reduce_pairs(words, counts).close()
    for step in ("engine order", "ranked"):
        if step == "ranked":
            eng.sort_result()
            eng.rank_result()
        before = fetched(eng)
        rc, first, last, sums, info = raw_find(eng, [b"t1", b""], mox.FIND_PREFIX)
        assert rc == mox.MOX_ESTATE and b"mox_sort_result" in eng._L.mox_last_error(), step
        assert (first, last, sums, info) == ([11, 11], [12, 12], [13, 13], UNTOUCHED), step
        with pytest.raises(mox.MoxError) as ex:
            eng.complete(b"t1")  # does not sort behind the caller's back
        assert ex.value.code == mox.MOX_ESTATE
        assert fetched(eng) == before
    eng.sort_result()  # ends the ranking: the search works again
    items, _ = fetched(eng)
    assert_find(eng, items, [b"t1", b""], "prefix", C.PREFIX)


def test_no_result_and_bad_arguments():
    e = mox.Engine(device=0)
    try:
        rc, first, last, sums, info = raw_find(e, [b"a"], mox.FIND_EXACT)
        assert rc == mox.MOX_ESTATE and (first, last, sums, info) == ([11], [12], [13], UNTOUCHED)
        items = load_sorted(e, [b"a", b"b"], [1, 2])
        rc, first, last, sums, info = raw_find(e, [b"a"], 3)
        assert rc == mox.MOX_EINVAL and b"mode" in e._L.mox_last_error() and (first, last, sums, info) == ([11], [12], [13], UNTOUCHED)
        offs = np.array([0, 2, 1], dtype=np.uint64)
        out = [np.full(2, 11, dtype=np.uint64) for _ in range(3)]
        rc = e._L.mox_find_ranges(e._h, ctypes.c_char_p(b"ab"), offs.ctypes.data_as(U64P), 2, 0, *(o.ctypes.data_as(U64P) for o in out), None)
        assert rc == mox.MOX_EINVAL and b"decrease" in e._L.mox_last_error() and all(o.tolist() == [11, 11] for o in out)
        n = mox.FIND_MAX + 1
        offs = np.zeros(n + 1, dtype=np.uint64)
        out = [np.full(n, 11, dtype=np.uint64) for _ in range(3)]
        rc = e._L.mox_find_ranges(e._h, None, offs.ctypes.data_as(U64P), n, 0, *(o.ctypes.data_as(U64P) for o in out), None)
        assert rc == mox.MOX_EINVAL and b"MOX_FIND_MAX" in e._L.mox_last_error() and all((o == 11).all() for o in out)
        rc = e._L.mox_find_ranges(e._h, None, np.zeros(2, np.uint64).ctypes.data_as(U64P), 1, 0, None, None, None, None)
        assert rc == mox.MOX_EINVAL
        # n == 0: nothing runs, the data pointers may be NULL
        info = mox.FindInfo(queries=5)
        assert e._L.mox_find_ranges(e._h, None, None, 0, 0, None, None, None, ctypes.byref(info)) == mox.MOX_OK and info.queries == 0
        first, last, sums = e.find([])
        assert first.size == last.size == sums.size == 0
        assert_find(e, items, [b"a", b"b", b"c"], "exact", C.EXACT)  # the engine is usable after the errors
    finally:
        e.close()


def test_sort_bytes_flag_sorts_implicitly():
    e = mox.Engine(device=0)
    try:
        words, counts = C.table_words(2000, 29)
        e.reduce_pairs(words, counts).close()  # (fetched without the flag: the result stays in engine order)
        e.set_flags(mox.MOX_F_SORT_BYTES)
        keys = C.keys_around(words[::9], seed=30)
        want = C.expected(sorted(zip(words, counts)), keys, C.PREFIX)
        first, last, sums = e.find(keys, "prefix")
        assert (first.tolist(), last.tolist(), sums.tolist()) == want
        items, _ = fetched(e)
        assert items == sorted(zip(words, counts))
        # ... but an explicit ranking wins over the flag
        e.rank_result()
        assert raw_find(e, [b"t1"], mox.FIND_PREFIX)[0] == mox.MOX_ESTATE
    finally:
        e.close()


def test_the_call_only_reads(eng):
    words, counts = C.table_words(2500, 33)
    eng.reduce_pairs(words[:1000], counts[:1000]).close()
    eng.accumulate()
    eng.reduce_pairs(words[1000:], counts[1000:]).close()
    eng.sort_result()
    before = (fetched(eng), table_of(eng.top_words(20)), eng.accumulate_info())
    keys = C.keys_around(words[::11], seed=34)
    a = [x.tolist() for x in eng.find(keys, "prefix")]
    assert (fetched(eng), table_of(eng.top_words(20)), eng.accumulate_info()) == before
    assert [x.tolist() for x in eng.find(keys, "prefix")] == a
    assert a == list(C.expected(before[0][0], keys, C.PREFIX))
    eng.accumulate()  # the result is still unfolded: the state flags are what they were
    assert eng.accumulate_info()["passes"] == 2


# ---- 8. top_rows and complete
@pytest.mark.parametrize("sort", [False, True])
def test_top_rows_over_everything_is_top_words(eng, sort):
    rng = random.Random(37)
    words = [b"w%d" % i + b"-" * (i % 29) for i in range(3000)]
    counts = [rng.randint(0, 40) for _ in words]  # many ties
    eng.reduce_pairs(words, counts).close()
    if sort:
        eng.sort_result()
    items, tokens = fetched(eng)
    n = len(items)
    for k in (1, 10, 257):
        want = table_of(eng.top_words(k))
        assert table_of(eng.top_rows(0, n, k)) == want
        assert table_of(eng.top_rows(0, n + 5, k)) == want
        assert [(want[2][a:b], c) for a, b, c in zip(want[1], want[1][1:], want[0])] == C.top_of(items, 0, n, k)
    # a range that starts at an odd row, equal counts inside: ties by table index
    for first, rows, k in ((1001, 777, 50), (7, 1, 3), (2999, 10, 4), (1, 2998, 4096)):
        t = eng.top_rows(first, rows, k)
        assert t.tokens == tokens
        assert list(t.items()) == C.top_of(items, first, min(first + rows, n), k)
        t.close()
    for first, rows, k in ((n, 5, 3), (n + 9, 5, 3), (5, 0, 3), (5, 5, 0)):
        t = eng.top_rows(first, rows, k)
        assert (t.n, t.tokens, list(t.items())) == (0, tokens, [])
        t.close()
    with pytest.raises(mox.MoxError) as ex:
        eng.top_rows(0, n, mox.TOP_MAX + 1)
    assert ex.value.code == mox.MOX_EINVAL


def test_complete_is_the_top_k_of_the_prefix_rows(eng):
    rng = random.Random(41)
    words = [p + b"%d" % i for p in (b"un", b"under", b"up", b"u", b"v") for i in range(400)] + [b"un", b"u"]
    counts = [rng.randint(1, 30) for _ in words]
    items = load_sorted(eng, words, counts)
    tokens = sum(counts)
    for prefix, k in ((b"un", 10), (b"under1", 5), (b"u", 300), (b"", 10), (b"w", 10), (b"un399", 10)):
        first, last, _ = C.expected(items, [prefix], C.PREFIX)
        t = eng.complete(prefix, k)
        assert t.tokens == tokens
        assert list(t.items()) == C.top_of(items, first[0], last[0], k), prefix
        t.close()
    t = eng.complete("un")  # str is encoded; k defaults to 10
    assert t.n == 10 and all(w.startswith(b"un") for w, _ in t.items())
    t.close()


# ---- 9. a real pass
def test_a_real_pass_with_unicode_words(eng):
    rng = random.Random(43)
    vocab = "a an and ant apple Étoile étoile éclair école été über uber zebra the a.m. añejo ábaco ǅungla İstanbul".split()
    text = " ".join(rng.choice(vocab) for _ in range(900)).encode()
    assert 2048 < len(text) < 16384
    eng.count(text).close()
    eng.sort_result()
    items, tokens = fetched(eng)
    assert items == coracle.count(text)[0]
    prefixes = ["a".encode(), "é".encode(), b""]
    first, last, sums, _ = assert_find(eng, items, prefixes, "prefix", C.PREFIX)
    assert (last - first).tolist() == [sum(1 for w, _ in items if w.startswith(p)) for p in prefixes]
    assert sums.tolist()[2] == tokens == 900 and last.tolist()[2] == len(items)
    assert [w.decode() for w, _ in items[first[1]:last[1]]] == ["éclair", "école", "étoile", "été"]  # (bytes: "o" < 0xC3)
    for p in prefixes:
        t = eng.complete(p, 3)
        a, b, _ = C.expected(items, [p], C.PREFIX)
        assert list(t.items()) == C.top_of(items, a[0], b[0], 3)
        t.close()
    assert_find(eng, items, [w for w, _ in items] + [b"zz"], "exact", C.EXACT)


# ---- 10. an engine group
def test_engine_group_searches_the_gathered_result():
    data = corpus.fill(corpus.UNICODE, 5, 0, 256 << 10).tobytes().decode("utf-8", "ignore").encode()  # (the cut can split a character)
    g = mox.Engine(device=0, n_gpus=2, transport=mox.XPORT_COPY, devices=[0, 0], flags=mox.MOX_F_SORT_BYTES)
    try:
        g.count(data).close()
        items, tokens = fetched(g)
        assert items == coracle.count(data)[0]
        words = [w for w, _ in items]
        keys = C.keys_around(words[::5], seed=47) + [w[:2] for w in words[::50]]
        for name, mode in C.MODES:
            assert_find(g, items, keys, name, mode)
        assert g.find([b""])[2].tolist() == [tokens]
    finally:
        g.close()


# ---- 11. the command line
def test_cli_prefix(tmp_path):
    rng = random.Random(53)
    vocab = ("the that this then there thin thick thy th other a an and to of in it is was he for with as his "
             "be at thee thou three throne thus").split()
    words = [rng.choice(vocab) for _ in range(1500)] + ["the"] * 40 + ["that"] * 7 + ["this"] * 7
    rng.shuffle(words)
    data = "\n".join(" ".join(words[i:i + 12]) for i in range(0, len(words), 12)).encode()
    (tmp_path / "shakes.txt").write_bytes(data)
    cli = os.path.join(ROOT, "map-oxidize_amd", "mox", "meduce-gpu")
    plain = subprocess.run([cli], cwd=tmp_path, capture_output=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    plain_file = (tmp_path / "final_result.txt").read_bytes()
    items = coracle.count(data)[0]
    counts = dict(items)
    assert sorted(plain_file.splitlines()) == sorted(w + b" %d" % c for w, c in items)  # today's output
    order = [ln.rsplit(b" ", 1)[0] for ln in plain_file.splitlines()]
    top = sorted(order, key=lambda w: (-counts[w], order.index(w)))[:10]
    assert plain.stdout == b"Top 10 words:\n" + b"".join(w + b": %d\n" % counts[w] for w in top)

    def block(p):
        a, b, s = C.expected(items, [p], C.PREFIX)
        return b"Prefix %s: %d words, %d tokens\n" % (p, b[0] - a[0], s[0]) + b"".join(
            w + b": %d\n" % c for w, c in C.top_of(items, a[0], b[0], 10))

    r = subprocess.run([cli, "--prefix", "th", "--prefix", "zz", "--prefix", "thee"], cwd=tmp_path, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    head = b"Top 10 words:\n" + b"".join(w + b": %d\n" % c for w, c in C.top_of(items, 0, len(items), 10))
    assert r.stdout == head + block(b"th") + block(b"zz") + block(b"thee")
    assert block(b"th").count(b"\n") == 11 and block(b"zz") == b"Prefix zz: 0 words, 0 tokens\n"
    assert (tmp_path / "final_result.txt").read_bytes() == b"".join(w + b" %d\n" % c for w, c in items)  # sorted for the search
    # the queries run before a --by-count ranking
    r2 = subprocess.run([cli, "--by-count", "--prefix", "th"], cwd=tmp_path, capture_output=True, timeout=120)
    assert r2.returncode == 0, r2.stderr
    ranked = sorted(items, key=lambda wc: (-wc[1], wc[0]))
    assert r2.stdout == b"Top 10 words:\n" + b"".join(w + b": %d\n" % c for w, c in ranked[:10]) + block(b"th")
    again = subprocess.run([cli], cwd=tmp_path, capture_output=True, timeout=120)
    assert again.stdout == plain.stdout and (tmp_path / "final_result.txt").read_bytes() == plain_file  # unchanged without the option
