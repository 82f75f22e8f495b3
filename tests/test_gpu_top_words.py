"""GPU: the device top-k (mox_top_words, map-oxidize_amd/csrc/mox_topk.hip)
against the fetched table.  Every comparison is exact: the expectation is the
first k of a fetch() of the same device-resident result by (count descending,
table index ascending) -- mox_print_top_words' rule -- with no run in between
(the engine order of words longer than 16 bytes can differ from run to run).
Tables come from Engine.reduce_pairs: arbitrary 64-bit counts in milliseconds.
The case tables and the CPU checks of their shapes: top_cases.py,
test_top_words_abi.py."""
import threading

import numpy as np
import pytest

import coracle
import mox
from mox import corpus
from mox import dist as mdist
import top_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    e = mox.Engine(device=0)
    yield e
    e.close()


def fetched(e):
    """(items in table order, tokens) of the engine's resident result."""
    t = e.fetch()
    try:
        return list(t.items()), t.tokens
    finally:
        t.close()


def top(e, k):
    """(items, tokens, offs[0]) of top_words(k)."""
    t = e.top_words(k)
    try:
        counts, offs, _ = t.arrays()
        assert t.n == counts.size and offs.size == t.n + 1
        return list(t.items()), t.tokens, int(offs[0])
    finally:
        t.close()


def load(e, words, counts):
    """reduce_pairs(words, counts) on e; the fetched (items, tokens)."""
    e.reduce_pairs(words, counts).close()
    return fetched(e)


def assert_top(e, items, tokens, k):
    got, gtok, off0 = top(e, k)
    assert got == C.expected(items, k), k
    assert len(got) == min(k, len(items)) and gtok == tokens and off0 == 0


# ---- 1. k edges
def test_k_edges(eng):
    items, tokens = load(eng, *C.distinct(5000, 1))
    for k in (0, 1, 10, 4095, 4096):
        assert_top(eng, items, tokens, k)
    with pytest.raises(mox.MoxError) as ei:
        eng.top_words(4097)
    assert ei.value.code == mox.MOX_EINVAL
    assert_top(eng, items, tokens, 10)  # the refused call left the engine usable
    items, tokens = load(eng, *C.distinct(7, 2))
    for k in (6, 7, 8, 4096):
        assert_top(eng, items, tokens, k)


# ---- 2. n on wave / block / tile edges
@pytest.mark.parametrize("n", C.EDGE_NS)
def test_n_edges(eng, n):
    items, tokens = load(eng, *C.distinct(n, 100 + n))
    assert len(items) == n
    assert_top(eng, items, tokens, min(n, 10))


# ---- 3. all ties: every count 1 (the histogram's single bin; the answer is the table's head)
def test_all_ties(eng):
    n = 3 * C.TILE + 1
    items, tokens = load(eng, *C.all_ones(n))
    assert len(items) == n and tokens == n
    for k in (1, 10, 4096):
        got, _, _ = top(eng, k)
        assert got == items[:k]


# ---- 4. sparse ties across tiles
def test_sparse_ties_across_tiles(eng):
    items, tokens = load(eng, *C.sparse_ties())
    sevens = [i for i, (_, c) in enumerate(items) if c == 7]
    assert len(sevens) == 1000 and len({i // C.TILE for i in sevens}) == (40000 + C.TILE - 1) // C.TILE  # in every tile
    for k in (3, 4, 500, 1003, 1004):  # no seven taken, one, mid-run, the whole run, one past it (into the ones)
        assert_top(eng, items, tokens, k)
    got, _, _ = top(eng, 500)
    assert got[3:] == [items[i] for i in sevens[:497]]
    got, _, _ = top(eng, 1004)
    assert got[1003] == next(x for x in items if x[1] == 1)


# ---- 5. every bit of the count
@pytest.mark.parametrize("case,ks", [("every_bit", (1, 64, 70, 128)), ("last_digit", (1, 100, 256)),
                                      ("first_digit", (1, 100, 255))])
def test_count_bits(eng, case, ks):
    words, counts = getattr(C, case)()
    items, tokens = load(eng, words, counts)
    assert sorted(c for _, c in items) == sorted(counts)
    for k in ks:
        assert_top(eng, items, tokens, k)


# ---- 6. word shapes among the winners
def test_word_shapes(eng):
    words, counts, winners = C.word_shapes()
    items, tokens = load(eng, words, counts)
    got, _, _ = top(eng, 64)
    assert [w for w, _ in got] == winners  # bytes compared exactly
    assert got == C.expected(items, 64)
    assert_top(eng, items, tokens, 63)
    assert_top(eng, items, tokens, 200)


# ---- 7. order follows the resident table
def test_order_follows_sort_result(eng):
    items, tokens = load(eng, *C.many_equal())
    assert_top(eng, items, tokens, 50)
    eng.sort_result()
    sitems, stok = fetched(eng)
    assert sitems == sorted(items) and stok == tokens
    got, _, _ = top(eng, 50)
    assert got == C.expected(sitems, 50)
    for c in {c for _, c in got}:  # equal counts in bytewise ascending order
        ws = [w for w, cc in got if cc == c]
        assert ws == sorted(ws)
    assert got != C.expected(items, 50)  # (the tie order did change)


def test_sort_flag_alone_does_not_sort():
    """MOX_F_SORT_BYTES sorts at the fetch; top_words before any fetch sees the
    table in engine order, which is deterministic for short words."""
    words, counts = C.many_equal()
    plain, flagged = mox.Engine(device=0), mox.Engine(device=0, flags=mox.MOX_F_SORT_BYTES)
    try:
        items, tokens = load(plain, words, counts)
        want = C.expected(items, 50)
        _reduce_only(flagged, words, counts)
        got, gtok, _ = top(flagged, 50)
        assert got == want and gtok == tokens
        sitems, _ = fetched(flagged)  # now the flag sorts, and the next top_words follows
        assert sitems == sorted(items)
        got, _, _ = top(flagged, 50)
        assert got == C.expected(sitems, 50) != want
    finally:
        plain.close()
        flagged.close()


def _reduce_only(e, words, counts):
    """mox_reduce_pairs without the fetch Engine.reduce_pairs ends with."""
    import ctypes
    from mox import spill
    data, offs, cnt = spill.pack_pairs(list(words), list(counts))
    buf = ctypes.create_string_buffer(data, max(1, len(data)))
    e._c(e._L.mox_reduce_pairs(e._h, buf, ctypes.c_void_p(offs.ctypes.data), ctypes.c_void_p(cnt.ctypes.data), len(cnt)))


# ---- 8. result untouched, scratch reuse
def test_result_untouched_and_scratch_reuse(eng):
    eng.reduce_pairs(*C.distinct(30000, 8)).close()
    t = eng.fetch()
    before = t.arrays()
    items, tokens = list(t.items()), t.tokens
    t.close()
    for k in (10, 4096, 1):
        assert_top(eng, items, tokens, k)
    t = eng.fetch()
    after = t.arrays()
    t.close()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    # a small table after a big one on the same engine: nothing stale leaks
    items, tokens = load(eng, [b"e", b"d", b"c", b"b", b"a"], [5, 9, 5, 1, 9])
    for k in (4096, 3, 5):
        assert_top(eng, items, tokens, k)


# ---- 9. states
def test_fresh_engine_is_estate(eng):
    with pytest.raises(mox.MoxError) as ei:
        eng.top_words(10)
    assert ei.value.code == mox.MOX_ESTATE


def test_empty_result(eng):
    eng.count(b"  \n ").close()
    assert top(eng, 10) == ([], 0, 0)
    assert top(eng, 0) == ([], 0, 0)


def test_completes_a_pending_async_pass(eng):
    data = corpus.fill(corpus.ZIPF, 5, 0, 2 << 20).tobytes()
    d = eng.alloc(len(data))
    try:
        eng.h2d(d, data)
        eng.run_range(d, len(data), 0, len(data), True)  # sizes the buffers
        half = len(data) // 2  # (ASCII text: any cut is a valid corpus end)
        eng.run_range_async(d, half, 0, half, True)
        got, gtok, _ = top(eng, 25)  # no run_wait: top_words completes the pass
        items, tokens = fetched(eng)
        assert got == C.expected(items, 25) and gtok == tokens
        assert sorted(items) == coracle.count(data[:half])[0]
    finally:
        eng.free(d)


def test_count_against_the_oracle(eng):
    data = corpus.fill(corpus.ZIPF, 1, 0, 4 << 20).tobytes()
    eng.count(data).close()
    got, gtok, _ = top(eng, 10)
    want, wtok = coracle.count(data)
    wd = dict(want)
    assert [c for _, c in got] == sorted(wd.values(), reverse=True)[:10]
    assert all(wd[w] == c for w, c in got) and len({w for w, _ in got}) == 10
    assert gtok == wtok


# ---- 10. engine group
def test_engine_group():
    import test_gpu_group as G
    data = G.mixed(2 << 20, 90)
    g = G.group(2)
    try:
        g.count(data).close()
        got, gtok, _ = top(g, 100)
        items, tokens = fetched(g)
        assert got == C.expected(items, 100) and gtok == tokens
    finally:
        g.close()
    assert sorted(items) == coracle.count(data)[0]


# ---- 11. ranks without a gather
def test_ranks_merge_top_equals_gathered_top():
    """Two ranks on device 0 (host transport): after the exchange each rank's
    top_words(50), merged by dist.merge_top, is the top 50 of the table a
    gather in rank order puts on rank 0."""
    import test_gpu_exchange as X
    data = X.mixed_corpus(2 << 20, 33)
    world, k = 2, 50
    x = mdist.ThreadAlltoall(world)
    parts, gathered, errs = [None] * world, [None], []

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
                    parts[r] = top(e, k)[0]
                    e.gather_host(world, r, x.fn(r), root=0)
                    if r == 0:
                        gathered[0] = (fetched(e), top(e, k))
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
    (items, tokens), (gtop, gtok, _) = gathered[0]
    want = C.expected(items, k)
    assert mdist.merge_top(parts, k) == want
    assert gtop == want and gtok == tokens  # and the device top-k of the gathered table agrees
    assert all(len(p) == k for p in parts)
