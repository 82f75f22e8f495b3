"""GPU: the device lookup (mox_lookup_words, map-oxidize_amd/csrc/mox_lookup.hip)
against the fetched table.  Every comparison is exact: the expectation is a
dictionary over a fetch() of the same device-resident result, with no run in
between (the engine order of words longer than 16 bytes can differ from run to
run).  Tables come from Engine.reduce_pairs unless the case says otherwise.
The case tables and the CPU checks of their shapes: lookup_cases.py,
test_lookup_abi.py."""
import ctypes
import random
import threading

import numpy as np
import pytest

import coracle
import lookup_cases as C
import mox
import top_cases
from mox import corpus
from mox import dist as mdist

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    e = mox.Engine(device=0)
    yield e
    e.close()


def fetched(e):
    """The engine's resident result as (word, count) items in table order."""
    t = e.fetch()
    try:
        return list(t.items())
    finally:
        t.close()


def load(e, words, counts):
    """reduce_pairs(words, counts) on e; the fetched items."""
    e.reduce_pairs(words, counts).close()
    return fetched(e)


def assert_lookup(e, items, queries):
    """lookup(queries) equals the dictionary over items at every position; returns the info."""
    counts, index, info = e.lookup(queries, with_index=True, with_info=True)
    want_c, want_i = C.expected(items, queries)
    assert counts.dtype == np.uint64 and index.dtype == np.uint64
    assert counts.tolist() == want_c
    assert index.tolist() == want_i
    assert info["queries"] == len(queries) and info["distinct"] == len(set(queries))
    assert info["found"] == sum(i != C.NONE for i in want_i)
    assert np.array_equal(e.lookup(queries), counts)  # without the index: the same counts
    return info


# ---- 1. table-size edges
@pytest.mark.parametrize("n", C.TABLE_NS)
def test_table_size_edges(eng, n):
    words, counts = C.table_words(n, 100 + n)
    items = load(eng, words, counts)
    assert len(items) == n
    assert_lookup(eng, items, C.present_and_absent(words, n))


def test_three_strides(eng, monkeypatch):
    words, counts = C.table_words(C.STRIDE_N, 5)
    items = load(eng, words, counts)
    assert len(items) == C.STRIDE_N
    queries = C.present_and_absent(words, 6)
    want = eng.lookup(queries, with_index=True)
    monkeypatch.setenv("MOX_LOOKUP_GRID", str(C.STRIDE_GRID))
    assert_lookup(eng, items, queries)
    got = eng.lookup(queries, with_index=True)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])  # the grid does not matter


# ---- 2. query-count edges
@pytest.fixture(scope="module")
def table5000():
    return C.table_words(5000, 21)


@pytest.mark.parametrize("q", C.QUERY_NS)
def test_query_count_edges(eng, table5000, q):
    words, counts = table5000
    items = load(eng, words, counts)
    pool = C.present_and_absent(words, 22)
    assert_lookup(eng, items, pool[:q])


def test_lookup_max_is_accepted_and_one_more_is_not(eng):
    n = C.LOOKUP_MAX
    mat, offs = C.fixed_width_queries(n + 1)
    rng = random.Random(23)
    nums = rng.sample(range(n), 5000)
    words = [mat[i].tobytes() for i in nums]
    items = load(eng, words, [i + 1 for i in nums])  # word number i has count i + 1
    want_c, want_i = np.zeros(n, np.uint64), np.full(n, C.NONE, np.uint64)
    for pos, (w, c) in enumerate(items):
        i = C.fixed_width_number(w)
        assert c == i + 1
        want_c[i], want_i[i] = c, pos
    counts, index, info = eng.lookup_packed(mat[:n].reshape(-1), offs[:n + 1], with_index=True, with_info=True)
    assert np.array_equal(counts, want_c) and np.array_equal(index, want_i)
    assert info == {"queries": n, "distinct": n, "found": 5000, "tag_mismatch": info["tag_mismatch"]}
    with pytest.raises(mox.MoxError) as ei:
        eng.lookup_packed(mat.reshape(-1), offs)
    assert ei.value.code == mox.MOX_EINVAL
    assert_lookup(eng, items, words[:10] + [b"absent"])  # the refused call left the engine usable


# ---- 3. word shapes
def test_word_shapes_and_near_misses(eng):
    words, counts = C.shape_table()
    items = load(eng, words, counts)
    assert sorted(w for w, _ in items) == sorted(words)
    info = assert_lookup(eng, items, C.shape_queries(words))
    assert info["found"] >= len(words)


def test_last_word_of_the_table_has_one_byte(eng):
    words, counts = C.last_is_one_byte()
    eng.reduce_pairs(words, counts).close()
    eng.sort_result()
    items = fetched(eng)
    assert items[-1][0] == b"~" and [w for w, _ in items] == sorted(words)
    assert_lookup(eng, items, [b"~", b"~~", b"}", b"~\x00", b""] + words)


# ---- 4. duplicates
def test_duplicates(eng, table5000):
    words, counts = table5000
    items = load(eng, words, counts)
    base = C.present_and_absent(words[:400], 31)
    queries = base * 3
    random.Random(32).shuffle(queries)
    info = assert_lookup(eng, items, queries)
    assert info["distinct"] == 800 and info["found"] == 1200
    w = words[17]
    counts_w, index_w, info = eng.lookup([w] * 1000, with_index=True, with_info=True)
    c, i = C.expected(items, [w])
    assert counts_w.tolist() == c * 1000 and index_w.tolist() == i * 1000 and c[0] > 0
    assert info["distinct"] == 1 and info["found"] == 1000
    counts_a, index_a, info = eng.lookup([b"no such word"] * 1000, with_index=True, with_info=True)
    assert not counts_a.any() and (index_a == C.NONE).all()
    assert info["distinct"] == 1 and info["found"] == 0
    long_w = b"d" * 300  # a wave-path query repeated
    assert_lookup(eng, items, [long_w] * 70 + [words[3]] * 5)


# ---- 5. counts
def test_counts_bit_exact(eng):
    words, counts = top_cases.every_bit()
    items = load(eng, words, counts)
    got = eng.lookup(words)
    assert got.tolist() == counts  # every bit of the 64, 2**64 - 1 among them
    assert_lookup(eng, items, words + [b"nope"])


def test_zero_count_word_has_an_index(eng):
    items = load(eng, [b"zero", b"one", b"a_long_word_with_count_zero"], [0, 1, 0])
    counts, index = eng.lookup([b"zero", b"absent", b"a_long_word_with_count_zero", b"one"], with_index=True)
    assert counts.tolist() == [0, 0, 0, 1]
    assert index[1] == C.NONE and C.NONE not in (index[0], index[2], index[3])
    assert items[int(index[0])] == (b"zero", 0) and items[int(index[2])] == (b"a_long_word_with_count_zero", 0)


# ---- 6. against the oracle, not the engine's own fetch
def test_count_against_the_oracle(eng):
    data = corpus.fill(corpus.UNICODE, 3, 0, 2 << 20).tobytes().decode("utf-8", "ignore").encode()
    eng.count(data).close()
    want, _ = coracle.count(data)
    tw = {w for w, _ in want}
    absent = [w + b"\xc3\xa9" for w, _ in want[:500] if w + b"\xc3\xa9" not in tw] + [w for w in C.absent_words(500) if w not in tw]
    queries = [w for w, _ in want] + absent
    random.Random(61).shuffle(queries)
    wd = dict(want)
    got = eng.lookup(queries)
    assert got.tolist() == [wd.get(w, 0) for w in queries]
    assert eng.lookup(["ΟΔΟΣ".lower(), "ΟΔΟΣ"]).tolist() == [wd.get("ΟΔΟΣ".lower().encode(), 0), wd.get("ΟΔΟΣ".encode(), 0)]  # str: UTF-8


# ---- 7. result forms
def test_after_sort_result(eng, table5000):
    words, counts = table5000
    items = load(eng, words, counts)
    queries = C.present_and_absent(words, 71)[:3000]
    before = eng.lookup(queries, with_index=True)
    eng.sort_result()
    sitems = fetched(eng)
    assert sitems == sorted(items)
    assert_lookup(eng, sitems, queries)
    after = eng.lookup(queries, with_index=True)
    assert np.array_equal(before[0], after[0]) and not np.array_equal(before[1], after[1])  # the same counts at new positions


def test_after_accumulate(eng):
    a = corpus.fill(corpus.ZIPF, 7, 0, 1 << 20).tobytes()
    b = corpus.fill(corpus.ZIPF, 8, 0, 1 << 20).tobytes() + b" only_in_the_second_run"
    eng.count(a).close()
    eng.accumulate()
    eng.count(b).close()
    first_only = eng.lookup([b"only_in_the_second_run"])
    eng.accumulate()
    items = fetched(eng)  # the running total
    wa, wb = dict(coracle.count(a)[0]), dict(coracle.count(b)[0])
    total = {w: wa.get(w, 0) + wb.get(w, 0) for w in set(wa) | set(wb)}
    assert dict(items) == total
    queries = C.present_and_absent(sorted(total), 72)
    assert_lookup(eng, items, queries)
    assert eng.lookup(queries).tolist() == [total.get(w, 0) for w in queries]  # the totals, not the last run
    assert first_only.tolist() == [1]
    assert eng.accumulate_info()["passes"] == 2


def test_after_a_sort_bytes_fetch(table5000):
    words, counts = table5000
    e = mox.Engine(device=0, flags=mox.MOX_F_SORT_BYTES)
    try:
        items = load(e, words, counts)  # (the fetch sorts the resident result)
        assert [w for w, _ in items] == sorted(words)
        assert_lookup(e, items, C.present_and_absent(words, 73)[:3000])
    finally:
        e.close()


def test_ranks_sum_equals_the_gathered_lookup():
    """Two ranks on device 0 (host transport): each rank's lookup after the
    exchange, summed by dist.sum_lookups, is the root's lookup after the gather."""
    import test_gpu_exchange as X
    data = X.mixed_corpus(2 << 20, 34)
    world = 2
    x = mdist.ThreadAlltoall(world)
    vocab = [None, None]  # the queried words of rank 0's and of rank 1's table
    parts, gathered, errs = [None] * world, [None], []
    vocab_ready = threading.Barrier(world)

    def rank_main(r):
        try:
            lo, hi, ob, oe, at_end = mdist.shard_range(len(data), world, r)
            e = mox.Engine(device=0)
            try:
                buf = data[lo:hi]
                d = e.alloc(max(1, len(buf)))
                try:
                    e.h2d(d, buf)
                    e.run_range(d, len(buf), ob, oe, at_end)
                    e.exchange_host(world, r, x.fn(r))
                    mine = fetched(e)
                    vocab[r] = [w for w, _ in mine[:2000]]
                    vocab_ready.wait()
                    q = vocab[1] + C.absent_words(500) + vocab[0]  # rank 1's words, absent words, rank 0's
                    parts[r] = (assert_pair(e, mine, q), mine)
                    e.gather_host(world, r, x.fn(r), root=0)
                    if r == 0:
                        items = fetched(e)
                        gathered[0] = (items, assert_pair(e, items, q))
                finally:
                    e.free(d)
            finally:
                e.close()
        except BaseException as ex:  # noqa: BLE001
            errs.append(ex)
            x.barrier.abort()
            vocab_ready.abort()

    def assert_pair(e, items, q):
        counts, index = e.lookup(q, with_index=True)
        wc, wi = C.expected(items, q)
        assert counts.tolist() == wc and index.tolist() == wi
        return counts, index

    ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join(300) for t in ts]
    if errs:
        raise errs[0]
    items, (gcounts, gindex) = gathered[0]
    total = mdist.sum_lookups([p[0][0] for p in parts], found=[p[0][1] != C.NONE for p in parts])
    assert np.array_equal(total, gcounts)
    n1 = len(vocab[1])
    assert n1 > 100 and len(vocab[0]) > 100
    assert gcounts[:n1].all() and not gcounts[n1:n1 + 500].any() and gcounts[n1 + 500:].all()
    # rank order: rank 0's words keep their positions, rank 1's follow them
    n0 = len(parts[0][1])
    i0, i1 = parts[0][0][1], parts[1][0][1]
    assert np.array_equal(gindex[i0 != C.NONE], i0[i0 != C.NONE])
    assert np.array_equal(gindex[i1 != C.NONE], i1[i1 != C.NONE] + np.uint64(n0))


def test_engine_group():
    import test_gpu_group as G
    data = G.mixed(2 << 20, 91)
    g = G.group(2)
    try:
        g.count(data).close()
        items = fetched(g)
        queries = C.present_and_absent([w for w, _ in items[:3000]], 74)
        assert_lookup(g, items, queries)
    finally:
        g.close()
    assert sorted(items) == coracle.count(data)[0]


# ---- 8. read-only
def test_lookup_only_reads(eng):
    words, counts = C.shape_table()
    eng.reduce_pairs(words, counts).close()
    t = eng.fetch()
    before, items = t.arrays(), list(t.items())
    t.close()
    text = eng.result_text()
    top = [x for x in eng.top_words(50).items()]
    assert_lookup(eng, items, C.shape_queries(words)[:4000])
    assert_lookup(eng, items, [b"x"])  # a small call after a big one: nothing stale in the scratch
    t = eng.fetch()
    after = t.arrays()
    t.close()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    assert eng.result_text() == text and [x for x in eng.top_words(50).items()] == top


def test_unfolded_result_folds_exactly_once_after_a_lookup(eng):
    eng.count(b"a b b c c c").close()
    assert eng.lookup([b"c", b"b", b"a", b"d"]).tolist() == [3, 2, 1, 0]
    eng.accumulate()  # the lookup did not fold it ...
    assert eng.lookup([b"c"]).tolist() == [3]
    with pytest.raises(mox.MoxError) as ei:
        eng.accumulate()  # ... and it folds once
    assert ei.value.code == mox.MOX_ESTATE
    eng.count(b"c d").close()
    assert eng.lookup([b"c", b"d"]).tolist() == [1, 1]  # the run's result, the total untouched
    eng.accumulate()
    assert eng.lookup([b"c", b"b", b"a", b"d"]).tolist() == [4, 2, 1, 1]
    assert eng.accumulate_info()["passes"] == 2


# ---- 9. order and errors
def test_fresh_engine_is_estate(eng):
    with pytest.raises(mox.MoxError) as ei:
        eng.lookup([b"a"])
    assert ei.value.code == mox.MOX_ESTATE
    with pytest.raises(mox.MoxError) as ei:
        eng.lookup([])
    assert ei.value.code == mox.MOX_ESTATE


def test_bad_arguments_are_einval_and_leave_the_outputs(eng):
    items = load(eng, [b"a", b"b"], [1, 2])
    L, U64P = eng._L, ctypes.POINTER(ctypes.c_uint64)
    counts, index = (ctypes.c_uint64 * 2)(7, 8), (ctypes.c_uint64 * 2)(9, 10)
    down = (ctypes.c_uint64 * 3)(0, 2, 1)
    assert L.mox_lookup_words(eng._h, b"ab", down, 2, counts, index, None) == mox.MOX_EINVAL
    ok = (ctypes.c_uint64 * 3)(0, 1, 2)
    assert L.mox_lookup_words(eng._h, b"ab", ok, 2, None, index, None) == mox.MOX_EINVAL  # counts is required
    assert L.mox_lookup_words(eng._h, None, ok, 2, counts, index, None) == mox.MOX_EINVAL  # bytes, with bytes to read
    assert L.mox_lookup_words(eng._h, b"ab", ctypes.cast(None, U64P), 2, counts, index, None) == mox.MOX_EINVAL
    huge = (ctypes.c_uint64 * 2)(0, 1 << 32)
    assert L.mox_lookup_words(eng._h, b"a", huge, 1, counts, index, None) == mox.MOX_EINVAL  # 2^32 query bytes
    assert list(counts) == [7, 8] and list(index) == [9, 10]
    assert L.mox_lookup_words(eng._h, None, None, 0, None, None, None) == mox.MOX_OK  # n == 0: nothing is required
    nz = (ctypes.c_uint64 * 3)(5, 6, 7)  # offsets need not start at 0
    assert L.mox_lookup_words(eng._h, b"xxxxxab", nz, 2, counts, None, None) == mox.MOX_OK
    assert list(counts) == [1, 2] and list(index) == [9, 10]
    assert_lookup(eng, items, [b"b", b"a", b"c"])


def test_completes_a_pending_async_pass(eng):
    data = corpus.fill(corpus.ZIPF, 5, 0, 2 << 20).tobytes()
    d = eng.alloc(len(data))
    try:
        eng.h2d(d, data)
        eng.run_range(d, len(data), 0, len(data), True)  # sizes the buffers
        half = len(data) // 2  # (ASCII text: any cut is a valid corpus end)
        eng.run_range_async(d, half, 0, half, True)
        want = coracle.count(data[:half])[0]
        queries = [w for w, _ in want] + C.absent_words(100)
        got = eng.lookup(queries)  # no run_wait: the lookup completes the pass
        assert got.tolist() == [c for _, c in want] + [0] * 100
        assert_lookup(eng, fetched(eng), queries)
    finally:
        eng.free(d)


# ---- 10. forced collisions
def test_forced_collisions():
    words, counts, queries = C.collide_table()
    e = mox.Engine(device=0, lib_path=mox.HC_LIB_PATH)
    try:
        items = load(e, words, counts)
        assert len(items) == 4000
        info = assert_lookup(e, items, queries)
        assert info["found"] == 1000
        assert info["tag_mismatch"] > 0  # the byte compare behind an equal tag ran
        # the build step alone meets equal tags too: no table word has these lengths
        e.reduce_pairs([b"x"], [1]).close()
        _, info = e.lookup(queries, with_info=True)
        assert info["tag_mismatch"] > 0 and info["found"] == 0
    finally:
        e.close()


# ---- 11. the command-line tool
def test_cli_word_flag(tmp_path):
    """meduce-gpu --word W ...: "Counts:" and one "{word}: {count}" line per W in
    argument order behind the top-10 block; without --word the output is unchanged."""
    import os
    import subprocess
    from conftest import ROOT
    data = b"The cat and the other cat saw THE third cat\n" * 3 + "ΟΔΟΣ οδος\n".encode()
    (tmp_path / "shakes.txt").write_bytes(data)
    cli = os.path.join(ROOT, "map-oxidize_amd", "mox", "meduce-gpu")
    plain = subprocess.run([cli], cwd=tmp_path, capture_output=True, timeout=120)
    assert plain.returncode == 0, plain.stderr
    assert b"Counts:" not in plain.stdout
    result = (tmp_path / "final_result.txt").read_bytes()
    args = ["--word", "cat", "--word", "The", "--word", "the", "--word", "οδος", "--word", "dog", "--word", "cat"]
    r = subprocess.run([cli] + args, cwd=tmp_path, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith(plain.stdout)  # byte for byte what it printed before, then the counts
    want = "Counts:\ncat: 9\nThe: 0\nthe: 9\nοδος: 2\ndog: 0\ncat: 9\n".encode()  # verbatim: "The" is not in the table
    assert r.stdout[len(plain.stdout):] == want
    assert (tmp_path / "final_result.txt").read_bytes() == result
