"""GPU: the device histograms (mox_hist_result, map-oxidize_amd/csrc/mox_hist.hip)
against a Python model over the fetched table.  Every comparison is exact:
the expectation is hist_cases.expected over a fetch() of the same
device-resident result taken immediately before the call, with no run in
between (the engine order of words longer than 16 bytes can differ from run to
run).  Tables come from Engine.reduce_pairs unless the case says otherwise.
The model, the case tables and the CPU checks of both: hist_cases.py,
test_hist_abi.py."""
import collections
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

import coracle
import filter_cases
import hist_cases as C
import lookup_cases
import mox
import rank_cases
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
    """The engine's resident result as ((word, count) items in table order, tokens)."""
    t = e.fetch()
    try:
        return list(t.items()), t.tokens
    finally:
        t.close()


def load(e, words, counts):
    e.reduce_pairs(words, counts).close()


def bins_of(h):
    return list(zip(*(a.tolist() for a in h[:4])))


def assert_hist(e, key, first=None, n=None, table=None):
    """histogram(key) on e's resident result: bins, totals and info equal the
    model over the fetch taken just before (or ``table``, a fetch the caller
    took with nothing in between).  Returns (items, bins, info)."""
    items, tokens = table or fetched(e)
    want = C.expected(items, key, first, n)
    h = e.histogram(key, first, n, with_info=True)
    info = h[6]
    assert bins_of(h) == want
    assert all(a.dtype == np.uint64 for a in h[:4])
    assert (h[4], h[5]) == (sum(b[1] for b in want), sum(b[2] for b in want) & C.U64)
    if first is None and n is None:
        assert (h[4], h[5]) == (len(items), tokens)
    assert {k: info[k] for k in C.INFO_KEYS} == C.info_of(want)
    assert info["ms"] > 0
    return items, want, info


# ---- 1. table-size edges
@pytest.mark.parametrize("n", C.TABLE_NS)
def test_table_size_edges(eng, n):
    words, counts = lookup_cases.table_words(n, 300 + n)
    load(eng, words, [c % 300 for c in counts])  # ties at the larger sizes, a zero among them
    table = fetched(eng)
    assert len(table[0]) == n
    for key in C.KEYS:
        _, want, info = assert_hist(eng, key, table=table)
        assert (len(want) > 0) == (n > 0)
        if n:
            assert info["device_bytes"] > 0
    assert fetched(eng) == table


# ---- 2. grid strides
def test_four_strides_equal_the_uncapped_call(eng, monkeypatch):
    words, counts = lookup_cases.table_words(C.STRIDE_N, 21)
    load(eng, words, rank_cases.zipf_counts(C.STRIDE_N, 21, top=70000))
    table = fetched(eng)
    free = {key: assert_hist(eng, key, table=table)[1] for key in C.KEYS}
    assert len(free["count"]) > 300 and len(free["bytes"]) > 20
    monkeypatch.setenv("MOX_HIST_GRID", str(C.STRIDE_GRID))
    for key in C.KEYS:
        assert assert_hist(eng, key, table=table)[1] == free[key]  # the grid does not matter


# ---- 3. every position a head, and one bin
def test_every_position_a_head(eng):
    n = 3 * C.TILE + 100
    words, counts = top_cases.distinct(n, 8)
    load(eng, words, counts)
    _, want, info = assert_hist(eng, "count")
    assert info["bins"] == n == len(want) and sorted(b[3] for b in want) == list(range(n))
    assert [b[:3] for b in want] == [(c, 1, c) for c in range(1, n + 1)]


def test_one_bin(eng):
    n = 2 * C.TILE + 77
    load(eng, top_cases.names(n), [7] * n)
    _, want, info = assert_hist(eng, "count")
    assert want == [(7, n, 7 * n, 0)] and info["digit_passes"] == 1
    load(eng, top_cases.names(n), [0] * n)
    _, want, info = assert_hist(eng, "count")
    assert want == [(0, n, 0, 0)] and info["digit_passes"] == 0 and info["max_key"] == 0  # no radix pass
    load(eng, [b"only"], [300])
    assert assert_hist(eng, "count")[1] == [(300, 1, 300, 0)]
    assert assert_hist(eng, "first")[1] == [(C.key_first(b"o", 0), 1, 300, 0)]


@pytest.mark.parametrize("values", [(7, 300), (1, 2, 70000)])
def test_bins_straddle_every_boundary(eng, values):
    n = 3 * C.TILE + 100
    load(eng, top_cases.names(n), rank_cases.spread_counts(n, values, 9))
    items, want, _ = assert_hist(eng, "count")
    assert rank_cases.straddles(items, values) and [b[0] for b in want] == sorted(values)


# ---- 4. digit edges
@pytest.mark.parametrize("max_count,passes", rank_cases.DIGIT_EDGES)
def test_digit_edges(eng, max_count, passes):
    counts = rank_cases.digit_edge_counts(max_count)
    load(eng, top_cases.names(len(counts)), counts)
    _, want, info = assert_hist(eng, "count")
    assert info["max_key"] == max_count and info["digit_passes"] == passes
    assert want[0][0] == 0 and want[-1][0] == max_count


@pytest.mark.parametrize("case,passes", [("byte7_only", 8), ("byte0_only", 4)])
def test_counts_that_differ_in_one_byte(eng, case, passes):
    counts = getattr(rank_cases, case)()
    load(eng, top_cases.names(len(counts)), counts)
    _, want, info = assert_hist(eng, "count")
    assert info["digit_passes"] == passes and len(want) == len(set(counts))


def test_sums_wrap(eng):
    load(eng, [b"a", b"bb", b"c", b"dd"], [C.U64, C.U64, C.U64, 5])
    _, want, _ = assert_hist(eng, "count")
    assert sorted(want) == [(5, 1, 5, want[0][3]), (C.U64, 3, (3 * C.U64) & C.U64, want[1][3])]
    assert want[1][2] == C.U64 - 2
    _, by_len, _ = assert_hist(eng, "bytes")
    assert [b[:3] for b in by_len] == [(1, 2, C.U64 - 1), (2, 2, 4)]


# ---- 5. word shapes
@pytest.fixture(scope="module")
def shapes():
    return filter_cases.shape_table()


@pytest.mark.parametrize("key", ["bytes", "chars", "first"])
def test_word_shapes(eng, shapes, key):
    words, counts = shapes
    load(eng, words, counts)
    items, want, _ = assert_hist(eng, key)
    assert {len(w) for w, _ in items} >= {1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 100000} and any(0 in w for w, _ in items)
    if key == "bytes":
        assert want[-1][0] == 100000


@pytest.mark.parametrize("key", ["bytes", "chars", "first"])
def test_utf8_words(eng, key):
    """First characters of 1, 2, 3 and 4 bytes, words that open with continuation bytes, a NUL inside, characters across
    the 8-byte steps and the lane / wave edge, and 50,000 two-byte characters through the wave path."""
    words, counts = C.utf8_words()
    load(eng, words, counts)
    items, want, info = assert_hist(eng, key)
    assert len(items) == len(words)
    if key == "chars":
        assert info["max_key"] == 50000 and want[0][0] == 0
    if key == "first":
        assert {k & 0xFF for k, _, _, _ in want} == {1, 2, 3, 4}
        assert {mox.hist_first_bytes(k) for k, _, _, _ in want} == {C.first_window(w) for w in words}


def test_one_byte_word_as_the_last_row(eng):
    words, counts = lookup_cases.last_is_one_byte()
    load(eng, words, counts)
    eng.sort_result()
    items, _ = fetched(eng)
    assert items[-1][0] == b"~"  # the 4-byte load of FIRST runs into the slack behind the table
    for key in ("first", "chars", "bytes"):
        assert_hist(eng, key)
    n = len(items)
    assert assert_hist(eng, "first", n - 1, 1)[1] == [(C.key_first(b"~", 0), 1, items[-1][1], n - 1)]


# ---- 6. ranges
def test_ranges(eng):
    words, counts = filter_cases.random_words(3000, 5)
    load(eng, words, counts)
    table = fetched(eng)
    n = len(table[0])
    for first, rows in ((0, 0), (n - 1, 1), (n, 5), (n + 7, 5), (5, C.U64), (0, n), (77, 1001), (1, 64), (63, 129), (None, 10), (2990, None)):
        for key in C.KEYS:
            _, want, _ = assert_hist(eng, key, first, rows, table=table)
            assert all(b[3] >= (first or 0) for b in want)  # first_row is absolute
    assert assert_hist(eng, "count", n, 5, table=table)[1] == [] == assert_hist(eng, "count", 0, 0, table=table)[1]
    assert fetched(eng) == table


def test_histogram_under_a_prefix(eng):
    words, counts = filter_cases.random_words(3000, 6)
    load(eng, words, counts)
    eng.sort_result()
    table = fetched(eng)
    for prefix in (b"ab", b"u", b"nun", b"zz", b""):
        first, last = eng.find([prefix], "prefix", with_sums=False)
        lo, hi = int(first[0]), int(last[0])
        under = [(w, c) for w, c in table[0] if w.startswith(prefix)]
        assert under == table[0][lo:hi]
        for key in ("count", "bytes"):
            _, want, _ = assert_hist(eng, key, lo, hi - lo, table=table)
            assert [b[:3] for b in want] == [b[:3] for b in C.expected(under, key)]


# ---- 7. first_row on a ranked table
def test_count_bins_of_a_ranked_table_are_row_ranges(eng):
    words, counts = top_cases.many_equal()
    load(eng, words[:5000], counts[:5000])
    eng.rank_result()
    items, want, _ = assert_hist(eng, "count")
    at = 0
    for key, bin_words, _, first_row in reversed(want):  # most frequent first: the bins tile [0, N)
        assert first_row == at
        t = eng.fetch_rows(first_row, bin_words)
        got = list(t.items())
        t.close()
        assert len(got) == bin_words and {c for _, c in got} == {key}
        at += bin_words
    assert at == len(items)


# ---- 8. larger tables
def test_zipf_table_of_200000_rows(eng):
    counts = rank_cases.zipf_counts(rank_cases.ZIPF_N, 5)
    load(eng, top_cases.names(rank_cases.ZIPF_N), counts)
    keys, bin_words, bin_tokens, first_row, words, tokens, info = eng.histogram("count", with_info=True)
    spectrum = collections.Counter(counts)
    assert dict(zip(keys.tolist(), bin_words.tolist())) == spectrum and keys.tolist() == sorted(spectrum)
    assert bin_tokens.tolist() == [k * spectrum[k] for k in sorted(spectrum)]
    assert info["digit_passes"] == 3 and info["max_key"] == max(counts) and (words, tokens) == (len(counts), sum(counts))
    t = eng.fetch()
    table_counts = t.arrays()[0]
    t.close()
    assert table_counts[first_row.astype(np.int64)].tolist() == keys.tolist()
    assert all(int(np.flatnonzero(table_counts == k)[0]) == r for k, r in list(zip(keys.tolist(), first_row.tolist()))[::50])


def test_a_table_past_one_step_of_the_scan(eng):
    """More than TOP_STEP tiles: the one-workgroup scan of the tile heads and sums runs with its carry, and
    every pass over rows strides its full grid.  Compared as arrays."""
    data = corpus.fill(corpus.HICARD, 17, 0, rank_cases.BIG_CORPUS).tobytes()
    t = eng.count(data)
    counts, offs, _ = t.arrays()
    n, tokens = t.n, t.tokens
    t.close()
    assert n > C.TOP_STEP * C.TILE
    for key, col in (("count", counts), ("bytes", np.diff(offs))):
        want_k, want_first, want_w = np.unique(col, return_index=True, return_counts=True)
        want_t = np.zeros(want_k.size, dtype=np.uint64)
        np.add.at(want_t, np.searchsorted(want_k, col), counts)
        keys, bin_words, bin_tokens, first_row, words, toks, info = eng.histogram(key, with_info=True)
        assert np.array_equal(keys, want_k) and np.array_equal(bin_words, want_w.astype(np.uint64))
        assert np.array_equal(bin_tokens, want_t) and np.array_equal(first_row, want_first.astype(np.uint64))
        assert (words, toks, info["bins"]) == (n, tokens, want_k.size)


def test_a_real_run(eng):
    data = corpus.fill(corpus.UNICODE, 3, 0, 1 << 19).tobytes().decode("utf-8", "ignore").encode()
    data += b" " + b"x" * 300 + b" " + "ΣΊΣΥΦΟΣ".encode() * 9 + b" the the the"
    want = dict(coracle.count(data)[0])
    eng.count(data).close()
    table = fetched(eng)
    assert dict(table[0]) == want and len(table[0]) == len(want) > 100
    for key in C.KEYS:
        _, bins, _ = assert_hist(eng, key, table=table)  # first_row: against the fetched order
        model = C.expected(sorted(want.items()), key)
        assert [b[:3] for b in bins] == [b[:3] for b in model]
    assert fetched(eng) == table


# ---- 9. the call only reads
@pytest.mark.parametrize("form", ["pass", "sorted", "ranked", "filtered"])
def test_the_call_only_reads(eng, form):
    words, counts = top_cases.many_equal()
    if form == "pass":  # a run's own table
        eng.count(b" ".join(w for w, c in zip(words, counts) for _ in range(c))).close()
    else:
        load(eng, words, counts)
    if form == "sorted":
        eng.sort_result()
    elif form == "ranked":
        eng.rank_result()
    elif form == "filtered":
        eng.filter_result(min_count=3)
    before = fetched(eng)
    for key in C.KEYS:
        assert_hist(eng, key, table=before)
    assert fetched(eng) == before
    if form == "sorted":
        first, last = eng.find([b"ab"], "prefix", with_sums=False)  # still sorted
        assert before[0][int(first[0]):int(last[0])] == [wc for wc in before[0] if wc[0].startswith(b"ab")]
    if form == "pass":
        x = mdist.ThreadAlltoall(1)
        eng.exchange_host(1, 0, x.fn(0))  # still a pass result: an exchange starts from it
        assert sorted(fetched(eng)[0]) == sorted(before[0])
        for key in C.KEYS:
            assert_hist(eng, key)
    else:
        eng.accumulate()  # still unfolded: one fold, then ESTATE
        with pytest.raises(mox.MoxError) as ei:
            eng.accumulate()
        assert ei.value.code == mox.MOX_ESTATE
        assert fetched(eng) == before


def test_sort_bytes_flag_does_not_sort():
    e = mox.Engine(device=0)
    try:
        words, counts = filter_cases.random_words(3000, 5)
        load(e, words, counts)
        engine_order = fetched(e)
        assert engine_order[0] != sorted(engine_order[0])
        e.set_flags(mox.MOX_F_SORT_BYTES)
        _, want, _ = assert_hist(e, "first", table=engine_order)  # first_row: rows of the table as it lies, unsorted
        assert fetched(e)[0] == sorted(engine_order[0])  # ... the fetch sorts, as ever
    finally:
        e.close()


def test_interleaved_with_the_ranking(eng):
    """rank_result and histogram share r_tmp: each call's answer is right whatever ran before."""
    words, counts = top_cases.distinct(3000, 8)
    load(eng, words, [c % 97 for c in counts])
    items = fetched(eng)[0]
    eng.rank_result()
    assert fetched(eng)[0] == rank_cases.expected(items)
    assert_hist(eng, "count")
    assert_hist(eng, "bytes")
    eng.rank_result(ascending=True)
    assert fetched(eng)[0] == rank_cases.expected(rank_cases.expected(items), ascending=True)
    _, want, _ = assert_hist(eng, "count")
    assert [b[3] for b in want] == [sum(b2[1] for b2 in want[:i]) for i in range(len(want))]  # ascending: bins in row order


# ---- 10. the accumulator's total, an engine group, ranks after an exchange
def test_the_accumulators_total(eng):
    words, counts = top_cases.many_equal()
    load(eng, words, counts)
    eng.accumulate()
    load(eng, words[:100] + [b"fresh", "été".encode()], [3] * 102)
    eng.accumulate()  # a merge: the result is the total
    items, want, _ = assert_hist(eng, "count")
    assert len(items) == len(words) + 2
    for key in ("bytes", "chars", "first"):
        assert_hist(eng, key)
    assert eng.accumulate_info()["passes"] == 2


def test_engine_group_histograms_member_zeros_table():
    g = mox.Engine(device=0, n_gpus=2, transport=mox.XPORT_COPY, devices=[0, 0])
    try:
        data = corpus.fill(corpus.ZIPF, 9, 0, 1 << 18).tobytes()
        want = dict(coracle.count(data)[0])
        g.count(data).close()
        table = fetched(g)
        assert dict(table[0]) == want
        for key in C.KEYS:
            assert_hist(g, key, table=table)
    finally:
        g.close()


def test_ranks_bins_add_up_after_an_exchange():
    data = corpus.fill(corpus.ZIPF, 29, 0, 512 << 10).tobytes()
    world = 2
    x = mdist.ThreadAlltoall(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            lo, hi, ob, oe, at_end = mdist.shard_range(len(data), world, r)
            buf = data[lo:hi]
            e = mox.Engine(device=0)
            try:
                d = e.alloc(len(buf))
                try:
                    e.h2d(d, buf)
                    e.run_range(d, len(buf), ob, oe, at_end)
                    e.exchange_host(world, r, x.fn(r))
                    out[r] = {key: assert_hist(e, key)[1] for key in C.KEYS}
                finally:
                    e.free(d)
            finally:
                e.close()
        except BaseException as ex:  # noqa: BLE001
            errs.append(ex)
            x.barrier.abort()

    ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join(300) for t in ts]
    if errs:
        raise errs[0]
    whole = sorted(coracle.count(data)[0])
    for key in C.KEYS:
        parts = [tuple(np.array(col, dtype=np.uint64) for col in zip(*out[r][key])) for r in range(world)]
        keys, words, tokens, n_words, n_tokens = mdist.sum_histograms(parts)
        assert list(zip(keys.tolist(), words.tolist(), tokens.tolist())) == [b[:3] for b in C.expected(whole, key)]
        assert (n_words, n_tokens) == (len(whole), sum(c for _, c in whole))


# ---- 11. errors
def test_errors_leave_everything(eng, monkeypatch):
    with pytest.raises(mox.MoxError) as ei:
        eng.histogram()
    assert ei.value.code == mox.MOX_ESTATE  # no result yet
    words, counts = top_cases.many_equal()
    load(eng, words, counts)
    before = fetched(eng)
    info = mox.HistInfo(words=77)
    out = ctypes.POINTER(mox._HistTable)()

    def call(h, with_info=True):
        return eng._L.mox_hist_result(eng._h, ctypes.byref(h), ctypes.byref(out), ctypes.byref(info) if with_info else None)

    bad = [mox.Hist(key=4), mox.Hist(key=0xFFFFFFFF), mox.Hist(flags=2), mox.Hist(flags=0x80000001), mox.Hist(first=1), mox.Hist(rows=1)]
    for i in range(4):
        h = mox.Hist(key=1)
        h.reserved[i] = 1 << 40
        bad.append(h)
    for h in bad:
        assert call(h) == mox.MOX_EINVAL
        assert not out and info.words == 77
    assert eng._L.mox_hist_result(eng._h, None, ctypes.byref(out), None) == mox.MOX_EINVAL
    assert eng._L.mox_hist_result(eng._h, ctypes.byref(mox.Hist()), None, None) == mox.MOX_EINVAL
    assert fetched(eng) == before
    monkeypatch.setenv("MOX_TEST_FAIL_HIST", "1")
    for key in (C.COUNT, C.CHARS):
        assert call(mox.Hist(key=key)) == mox.MOX_ENOMEM
        assert not out and info.words == 77 and b"MOX_TEST_FAIL_HIST" in eng._L.mox_last_error()
    assert fetched(eng) == before
    monkeypatch.delenv("MOX_TEST_FAIL_HIST")
    assert call(mox.Hist(key=C.COUNT), with_info=False) == mox.MOX_OK and out  # info may be NULL
    t = out.contents
    assert (t.n, t.words, t.tokens) == (5, len(before[0]), before[1]) and [t.keys[i] for i in range(5)] == [1, 2, 3, 4, 5]
    eng._L.mox_hist_free(out)
    for key in C.KEYS:
        assert_hist(eng, key, table=before)
    eng.accumulate()  # still an unfolded result


# ---- 12. the other builds
@pytest.mark.parametrize("lib_path", [mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_other_builds(lib_path, shapes):
    e = mox.Engine(device=0, lib_path=lib_path)
    try:
        words, counts = shapes  # (forced collisions in reduce_pairs behind it)
        load(e, words, counts)
        table = fetched(e)
        for key in C.KEYS:
            assert_hist(e, key, table=table)
        assert_hist(e, "chars", 3, 40, table=table)
    finally:
        e.close()


# ---- 13. the command-line tool
def test_cli_histogram(tmp_path):
    from conftest import ROOT
    data = b"The cat and the other cat saw THE third cat\n" * 3 + b"a dog and a bird\n" + "ΟΔΟΣ οδος été €5\n".encode() + b"x" * 40 + b"\n"
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
    r = subprocess.run([cli, "--histogram", "count", "--histogram", "first"], cwd=tmp_path, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "final_result.txt").read_bytes() == plain_file and r.stdout.startswith(plain.stdout)
    items = sorted(counts.items())
    want = b""
    for key in ("count", "first"):
        bins = C.expected(items, key)
        want += b"Histogram %s: %d bins, %d words, %d tokens\n" % (key.encode(), len(bins), len(items), sum(counts.values()))
        for k, w, t, _ in bins:
            want += (b"%d" % k if key == "count" else mox.hist_first_bytes(k)) + b"\t%d\t%d\n" % (w, t)
    assert r.stdout[len(plain.stdout):] == want
    assert "€".encode() + b"\t1\t1\n" in want and b"\nt\t2\t12\n" in want  # "the" 9 times and "third" 3 times
    bad = subprocess.run([cli, "--histogram", "length"], cwd=tmp_path, capture_output=True, timeout=120)
    assert bad.returncode == 2 and b"Usage" in bad.stderr and bad.stdout == b""
