"""GPU: the device text rendering (mox_write_result / mox_result_text,
map-oxidize_amd/csrc/mox_text.hip) against the fetched table.  Every
comparison is exact: the expectation is b"".join(word + b" %d\\n" % count) over
a fetch() of the same device-resident result, with no run in between (the
engine order of words longer than 16 bytes can differ from run to run).
Tables come from Engine.reduce_pairs (arbitrary 64-bit counts in milliseconds)
or a corpus of at most 4 MiB.  The case tables and the CPU checks of their
shapes: text_cases.py, test_result_text_abi.py."""
import os
import threading

import numpy as np
import pytest

import coracle
import mox
from mox import corpus
from mox import dist as mdist
import text_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    e = mox.Engine(device=0)
    yield e
    e.close()


def fetched(e):
    """The items of the engine's resident result in table order."""
    t = e.fetch()
    try:
        return list(t.items())
    finally:
        t.close()


def load(e, words, counts):
    e.reduce_pairs(words, counts).close()
    return fetched(e)


def written(e, path):
    e.write_result(str(path))
    with open(path, "rb") as f:
        return f.read()


def assert_renders(e, items, tmp_path):
    want = C.expected(items)
    assert e.result_text() == want
    assert written(e, tmp_path / "final_result.txt") == want
    return want


class slice_env:
    """MOX_TEXT_SLICE=S around a block, restored after."""

    def __init__(self, S):
        self.S = S

    def __enter__(self):
        self.old = os.environ.get("MOX_TEXT_SLICE")
        os.environ["MOX_TEXT_SLICE"] = str(self.S)

    def __exit__(self, *a):
        if self.old is None:
            del os.environ["MOX_TEXT_SLICE"]
        else:
            os.environ["MOX_TEXT_SLICE"] = self.old


def _reduce_only(e, words, counts):
    """mox_reduce_pairs without the fetch Engine.reduce_pairs ends with."""
    import ctypes
    from mox import spill
    data, offs, cnt = spill.pack_pairs(list(words), list(counts))
    buf = ctypes.create_string_buffer(data, max(1, len(data)))
    e._c(e._L.mox_reduce_pairs(e._h, buf, ctypes.c_void_p(offs.ctypes.data), ctypes.c_void_p(cnt.ctypes.data), len(cnt)))


# ---- 1. n on wave / workgroup / tile edges
@pytest.mark.parametrize("n", C.EDGE_NS)
def test_n_edges(eng, n, tmp_path):
    items = load(eng, *C.distinct(n, 100 + n))
    assert len(items) == n
    assert_renders(eng, items, tmp_path)


# ---- 2. digits, word shapes, the LDS limit, all counts 1
def test_digit_edges(eng, tmp_path):
    words, counts = C.digit_edges()
    items = load(eng, words, counts)
    assert sorted(items) == list(zip(words, counts))
    assert_renders(eng, items, tmp_path)  # engine order
    eng.sort_result()
    items = fetched(eng)
    assert items == list(zip(words, counts))  # the generator's order: every digit length next to every other
    assert C.digit_pairs([c for _, c in items]) >= {(a, b) for a in range(1, 21) for b in range(1, 21)}
    assert_renders(eng, items, tmp_path)


def test_count_zero_renders_as_zero(eng, tmp_path):
    """mox_reduce_pairs lets a count of 0 through: whatever the table then
    holds for it is rendered like the old writer does."""
    items = load(eng, [b"zero", b"one", b"nought"], [0, 1, 0])
    assert sorted(items) == [(b"nought", 0), (b"one", 1), (b"zero", 0)]
    want = assert_renders(eng, items, tmp_path)
    assert b"zero 0\n" in want and b"nought 0\n" in want


def test_word_shapes(eng, tmp_path):
    words, counts = C.word_shapes()
    items = load(eng, words, counts)
    assert sorted(items) == sorted(zip(words, counts))
    assert_renders(eng, items, tmp_path)  # engine order: the short words, then the long ones
    eng.sort_result()
    items = fetched(eng)
    i = next(k for k, (w, _) in enumerate(items) if len(w) == C.BIG_LEN)
    assert items[i - 1][0] == b"L" and items[i + 1][0] == b"M"  # a 1-byte word before and after the 100,000-byte word
    assert_renders(eng, items, tmp_path)


def test_tiles_on_either_side_of_the_lds_limit(eng, tmp_path):
    words, counts, lens = C.lds_edge_tiles()
    items = load(eng, words, counts)
    assert_renders(eng, items, tmp_path)
    eng.sort_result()
    items = fetched(eng)
    assert C.tile_text_lengths(items) == lens == [C.LDS - 1, C.LDS, C.LDS + 1, 5]
    assert_renders(eng, items, tmp_path)
    for S in C.SLICES:  # the slow path clips too
        with slice_env(S):
            assert eng.result_text() == C.expected(items)


def test_all_counts_one(eng, tmp_path):
    n = 3 * C.TILE + 1
    items = load(eng, *C.all_ones(n))
    assert len(items) == n
    assert_renders(eng, items, tmp_path)


# ---- 3. slices
def test_slices(eng, tmp_path):
    words, counts = C.mixed()
    load(eng, words, counts)
    eng.sort_result()  # the order test_result_text_abi.py checked the slice classes for
    items = fetched(eng)
    assert items == sorted(zip(words, counts))
    lines = C.lines_of(items)
    want = assert_renders(eng, items, tmp_path)  # the default slice
    for S in C.SLICES:
        cls = C.slice_classes(lines, S)
        assert all(cls[k] > 0 for k in C.CLASSES), (S, cls)
        assert any(len(w) + len(t) > S for w, t in lines) and C.slices_inside_a_word(lines, S) > 0
        old = os.environ.get("MOX_TEXT_SLICE")
        with slice_env(S):
            assert eng.result_text() == want, S
            path = tmp_path / ("s%d.txt" % S)
            assert written(eng, path) == want, S
            assert os.path.getsize(path) == len(want)
        assert os.environ.get("MOX_TEXT_SLICE") == old
    # engine order under small slices as well (the 100,000-byte word among the long words)
    load(eng, words, counts)
    items = fetched(eng)
    with slice_env(C.SLICES[0]):
        assert eng.result_text() == C.expected(items)


# ---- 4. equality with the old writer
def test_equals_the_old_writer(eng, tmp_path):
    words, counts = C.word_shapes()
    eng.reduce_pairs(words, counts).close()
    t = eng.fetch()
    try:
        t.write_final_result(str(tmp_path / "old.txt"))
    finally:
        t.close()
    eng.write_result(str(tmp_path / "new.txt"))
    with open(tmp_path / "old.txt", "rb") as f:
        old = f.read()
    with open(tmp_path / "new.txt", "rb") as f:
        new = f.read()
    assert new == old and len(new) > C.BIG_LEN


# ---- 5. order follows the table
def test_order_follows_sort_result(eng, tmp_path):
    words, counts = C.distinct(5000, 3)
    items = load(eng, words, counts)
    assert items != sorted(items)
    assert_renders(eng, items, tmp_path)
    eng.sort_result()
    assert eng.result_text() == C.expected(sorted(items))
    assert fetched(eng) == sorted(items)


def test_sort_flag_sorts_before_rendering(tmp_path):
    words, counts = C.distinct(5000, 4)
    e = mox.Engine(device=0, flags=mox.MOX_F_SORT_BYTES)
    try:
        _reduce_only(e, words, counts)  # no fetch yet: the result lies in engine order
        want = C.expected(sorted(zip(words, counts)))
        assert e.result_text() == want
        assert fetched(e) == sorted(zip(words, counts))
        assert written(e, tmp_path / "sorted.txt") == want
    finally:
        e.close()


def test_sort_flag_enomem_writes_nothing(tmp_path):
    words, counts = C.distinct(300, 5)
    e = mox.Engine(device=0, flags=mox.MOX_F_SORT_BYTES)
    path = tmp_path / "never.txt"
    old = os.environ.get("MOX_BSORT_MAX_WORDS")
    os.environ["MOX_BSORT_MAX_WORDS"] = "1"
    try:
        _reduce_only(e, words, counts)
        with pytest.raises(mox.MoxError) as ei:
            e.write_result(str(path))
        assert ei.value.code == mox.MOX_ENOMEM
        assert not os.path.exists(path)
        with pytest.raises(mox.MoxError) as ei:
            e.result_text()
        assert ei.value.code == mox.MOX_ENOMEM
        # the fall-back the header names: fetch + the old writer sort on the host
        t = e.fetch()
        try:
            assert list(t.items()) == sorted(zip(words, counts))
        finally:
            t.close()
    finally:
        if old is None:
            del os.environ["MOX_BSORT_MAX_WORDS"]
        else:
            os.environ["MOX_BSORT_MAX_WORDS"] = old
        e.close()


# ---- 6. result untouched, scratch reuse
def test_result_untouched_and_scratch_reuse(eng, tmp_path):
    eng.reduce_pairs(*C.distinct(30000, 8)).close()
    t = eng.fetch()
    before = t.arrays()
    items = list(t.items())
    t.close()
    first = assert_renders(eng, items, tmp_path)
    assert eng.result_text() == first  # two renders in a row
    t = eng.fetch()
    after = t.arrays()
    t.close()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and before[2] == after[2]
    # a small table after a big one on the same engine: nothing stale leaks
    items = load(eng, [b"e", b"d", b"c", b"b", b"a"], [5, 9, 5, 1, 9])
    assert len(items) == 5
    assert_renders(eng, items, tmp_path)


# ---- 7. states
def test_fresh_engine_is_estate(eng, tmp_path):
    with pytest.raises(mox.MoxError) as ei:
        eng.result_text()
    assert ei.value.code == mox.MOX_ESTATE
    with pytest.raises(mox.MoxError) as ei:
        eng.write_result(str(tmp_path / "x.txt"))
    assert ei.value.code == mox.MOX_ESTATE
    assert not os.path.exists(tmp_path / "x.txt")


def test_empty_result(eng, tmp_path):
    eng.count(b"  \n ").close()
    assert eng.result_text() == b""
    path = tmp_path / "empty.txt"
    path.write_bytes(b"stale")  # truncated on open
    assert written(eng, path) == b"" and os.path.getsize(path) == 0


def test_eio_leaves_the_engine_usable(eng, tmp_path):
    items = load(eng, *C.distinct(2000, 9))
    with pytest.raises(mox.MoxError) as ei:
        eng.write_result(str(tmp_path / "no_such_dir" / "final_result.txt"))
    assert ei.value.code == mox.MOX_EIO
    assert_renders(eng, items, tmp_path)


def test_completes_a_pending_async_pass(eng):
    data = corpus.fill(corpus.ZIPF, 5, 0, 2 << 20).tobytes()
    d = eng.alloc(len(data))
    try:
        eng.h2d(d, data)
        eng.run_range(d, len(data), 0, len(data), True)  # sizes the buffers
        half = len(data) // 2  # (ASCII text: any cut is a valid corpus end)
        eng.run_range_async(d, half, 0, half, True)
        got = eng.result_text()  # no run_wait: the call completes the pass
        items = fetched(eng)
        assert got == C.expected(items)
        assert sorted(items) == coracle.count(data[:half])[0]
    finally:
        eng.free(d)


# ---- 8. against the oracle
def test_count_against_the_oracle(eng):
    data = corpus.fill(corpus.ZIPF, 1, 0, 4 << 20).tobytes()
    eng.count(data).close()
    text = eng.result_text()
    assert text.endswith(b"\n")
    got = []
    for line in text[:-1].split(b"\n"):
        w, c = line.rsplit(b" ", 1)
        got.append((w, int(c)))
    want, wtok = coracle.count(data)
    assert sorted(got) == want and sum(c for _, c in got) == wtok


# ---- 9. run_file
def test_run_file(eng, tmp_path):
    data = corpus.fill(corpus.UNICODE, 3, 0, 1 << 20).tobytes() + "ΟΔΟΣ İ K The the".encode()
    src = tmp_path / "corpus.txt"
    src.write_bytes(data)
    eng.run_file(str(src))
    new = eng.result_text()
    assert new == C.expected(fetched(eng))
    t = eng.count_file(str(src))
    try:
        t.write_final_result(str(tmp_path / "old.txt"))
        assert t.sorted_items() == coracle.count(data)[0]
    finally:
        t.close()
    old = (tmp_path / "old.txt").read_bytes()
    # (engine order among words over 16 bytes may differ between the two runs)
    assert sorted(new.split(b"\n")) == sorted(old.split(b"\n")) and len(new) == len(old)
    with pytest.raises(mox.MoxError) as ei:
        eng.run_file(str(tmp_path / "missing.txt"))
    assert ei.value.code == mox.MOX_EIO


# ---- 10. engine group, and the root after a gather
def test_engine_group(tmp_path):
    import test_gpu_group as G
    data = G.mixed(2 << 20, 90)
    g = G.group(2)
    try:
        g.count(data).close()
        items = fetched(g)
        assert_renders(g, items, tmp_path)
    finally:
        g.close()
    assert sorted(items) == coracle.count(data)[0]


def test_root_after_a_gather(tmp_path):
    """Two ranks on device 0 (host transport): rank 0 renders the table a
    gather in rank order put into its gather buffers."""
    import test_gpu_exchange as X
    data = X.mixed_corpus(2 << 20, 33)
    world = 2
    x = mdist.ThreadAlltoall(world)
    out, errs = [None], []

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
                    e.gather_host(world, r, x.fn(r), root=0)
                    if r == 0:
                        text = e.result_text()
                        path = str(tmp_path / "gathered.txt")
                        e.write_result(path)
                        with open(path, "rb") as f:
                            out[0] = (fetched(e), text, f.read())
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
    items, text, filed = out[0]
    assert text == C.expected(items) == filed
    assert sorted(items) == coracle.count(data)[0]
