"""GPU: the device-resident accumulator (mox_accumulate / mox_accumulate_file,
map-oxidize_amd/csrc/mox_accum.hip).  Every comparison is exact: the
expectation is accum_cases.oracle_sum over the loaded (word, count) lists, or
coracle.count of the concatenated text.  Tables are loaded with
Engine.reduce_pairs (milliseconds) or come from corpora of at most 4 MiB.
conftest.assert_tables_equal rejects NUL bytes, so cases with NUL words compare
sorted Python lists.  Case tables and their CPU checks: accum_cases.py,
test_accum_abi.py."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import accum_cases as C
import coracle
import mox
from mox import corpus
from mox import dist as mdist
from conftest import ROOT, assert_tables_equal

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    e = mox.Engine(device=0)
    yield e
    e.close()


def code_of(call):
    try:
        call()
        return mox.MOX_OK
    except mox.MoxError as ex:
        return ex.code


def run_text(e, data):
    """One pass over a host text, the result left on the device."""
    d = e.alloc(max(1, len(data)))
    try:
        if data:
            e.h2d(d, data)
        e.run_device(d, len(data))
    finally:
        e.free(d)


def table_phases(e):
    """Start phases mod 8 of the short and of the long rows of the resident result."""
    t = e.fetch()
    try:
        _, offs, raw = t.arrays()
    finally:
        t.close()
    s, l = set(), set()
    for i in range(len(offs) - 1):
        w = raw[int(offs[i]):int(offs[i + 1])]
        (s if C.is_short(w) else l).add(int(offs[i]) % 8)
    return s, l


# ---- 1. row-count edges
@pytest.mark.parametrize("na,nb", C.EDGE_PAIRS)
def test_row_count_edges(eng, na, nb):
    for overlap in C.OVERLAPS:
        A, B = C.edge_tables(na, nb, overlap)
        eng.accumulate_reset()
        got, tok = C.fold_tables(eng, A, B)
        want, wtok = C.oracle_sum(A, B)
        assert got == want, (na, nb, overlap)
        assert tok == wtok == sum(c for _, c in got)
        info = eng.accumulate_info()
        assert (info["passes"], info["words"], info["tokens"]) == (2, len(want), wtok)


# ---- 2. word shapes
def test_word_shapes(eng):
    A, B = C.shape_tables()
    C.load(eng, A)
    sa, la = table_phases(eng)
    eng.accumulate()
    C.load(eng, B)
    sb, lb = table_phases(eng)
    # the resident tables the packer reads put words at every phase of an 8-byte word
    assert sa | sb == set(range(8)) and la | lb == set(range(8))
    eng.accumulate()
    got, tok = C.fetched(eng)
    want, wtok = C.oracle_sum(A, B)
    assert sorted(got) == want and tok == wtok
    d = dict(got)
    assert d[C.BIG_WORD] == dict(zip(*A))[C.BIG_WORD] + dict(zip(*B))[C.BIG_WORD]
    assert len({b"a", b"a\x00", b"a\x00b", b"\x00"} & set(d)) == 4  # the NUL words stay distinct
    # engine order: the 16-byte-key words first, every other word (NUL words included) behind them
    kinds = [C.is_short(w) for w, _ in got]
    assert kinds == sorted(kinds, reverse=True)


def test_one_byte_word_as_the_last_row(eng):
    """Sorted, LAST1's last row is a 1-byte word at the very end of the table's
    bytes: its key load reads the slack behind them.  As source 1 (the result)
    and, saved, as source 0 (the total)."""
    C.load(eng, C.LAST1)
    eng.sort_result()
    assert C.fetched(eng)[0][-1] == (b"z", 1)
    eng.accumulate()  # saved as it lies: sorted
    C.load(eng, C.LAST1_OTHER)
    eng.sort_result()
    assert C.fetched(eng)[0][-1][0] == b"z"
    eng.accumulate()
    got, tok = C.fetched(eng)
    assert (sorted(got), tok) == C.oracle_sum(C.LAST1, C.LAST1_OTHER)


# ---- 3. counts
def test_counts(eng):
    A, B = C.count_tables()
    got, tok = C.fold_tables(eng, A, B)
    want, wtok = C.oracle_sum(A, B)
    assert got == want and tok == wtok
    d = dict(got)
    assert d[b"big"] == (1 << 64) - 1 and d[b"zero"] == 0 and d[b"zf"] == 5 and d[b"a_long_word_with_count_zero"] == 0


def test_duplicate_zero_counts_in_one_reduce(eng):
    """The same zero-count word twice in one reduce-only pass (a merge of two
    tables that both hold it; duplicates in mox_reduce_pairs' input): the reduce
    table's "count 0 = not yet published" rule cannot take it, k_reduce_z does."""
    words = [b"nil", b"five", b"nil", b"five", b"nil", b"one"] + [b"z%d" % (i % 50) for i in range(3000)]
    counts = [0, 0, 0, 5, 0, 1] + [0] * 3000
    t = eng.reduce_pairs(words, counts)
    assert (t.sorted_items(), t.tokens) == C.oracle_sum((words, counts))
    t.close()


# ---- 4. every source form of the result
BASE = ([b"the", b"base", b"supercalifragilistic3expialidocious", b"~", "日本語".encode()], [7, 1, 2, 3, 4])


def base_text():
    return b" ".join(w for w, c in zip(*BASE) for _ in range(c))


def want_with_base(*texts):
    want, tok = coracle.count(b"\n".join((base_text(),) + texts))
    return want, tok


@pytest.fixture(scope="module")
def texts():
    return {"mixed": C.mixed_text(256 << 10, 11), "ascii": C.mixed_text(256 << 10, 13, ascii_only=True) + b" ~ "}


def test_source_pass_result(eng, texts):
    run_text(eng, base_text())
    eng.accumulate()
    run_text(eng, texts["mixed"])
    st = eng.stats()
    assert st["dict_words"] > 0 and st["unicode_tokens"] > 0 and st["long_tokens"] > 0
    eng.accumulate()
    got, tok = C.fetched(eng)
    assert (sorted(got), tok) == want_with_base(texts["mixed"])


def test_source_sorted_result(eng, texts):
    run_text(eng, base_text())
    eng.accumulate()
    run_text(eng, texts["ascii"])
    eng.sort_result()
    assert C.fetched(eng)[0][-1][0] == b"~"  # the last row: a 1-byte word
    eng.accumulate()
    got, tok = C.fetched(eng)
    assert (sorted(got), tok) == want_with_base(texts["ascii"])


def test_source_fetched_under_sort_flag(texts):
    e = mox.Engine(device=0, flags=mox.MOX_F_SORT_BYTES)
    try:
        run_text(e, base_text())
        e.accumulate()
        run_text(e, texts["ascii"])
        first, _ = C.fetched(e)  # sorts the result on the device
        assert first == sorted(first) and first[-1][0] == b"~"
        e.accumulate()
        got, tok = C.fetched(e)
    finally:
        e.close()
    assert (got, tok) == want_with_base(texts["ascii"])  # fetched under the flag: in bytewise order


def test_source_reduce_pairs_result(eng, texts):
    run_text(eng, texts["mixed"])
    eng.accumulate()
    C.load(eng, BASE)
    eng.accumulate()
    got, tok = C.fetched(eng)
    assert (sorted(got), tok) == want_with_base(texts["mixed"])


def test_source_gathered_group_result(texts):
    """A 2-member engine group on device 0 (copy transport): member 0's gathered
    result is folded, on member 0; with MOX_F_SORT_BYTES the gathered table is
    sorted, so its last row is the 1-byte word."""
    g = mox.Engine(device=0, n_gpus=2, transport=mox.XPORT_COPY, devices=[0, 0], flags=mox.MOX_F_SORT_BYTES)
    try:
        g.count(base_text()).close()
        g.accumulate()
        t = g.count(texts["ascii"])
        assert list(t.items())[-1][0] == b"~"
        t.close()
        g.accumulate()
        assert g.accumulate_info()["passes"] == 2
        got, tok = C.fetched(g)
    finally:
        g.close()
    assert (got, tok) == want_with_base(texts["ascii"])


# ---- 5. windows against one pass
@pytest.mark.parametrize("kind", ["zipf", "hicard"])
def test_windows_equal_one_pass(eng, kind):
    data = corpus.fill(corpus.KINDS[kind], 21, 0, 1 << 20).tobytes()
    cuts = C.ws_windows(data, 5)
    assert len(cuts) == 6 and all(b - a >= 4 for a, b in zip(cuts, cuts[1:]))
    d = eng.alloc(len(data))
    try:
        eng.h2d(d, data)
        for lo, hi in zip(cuts, cuts[1:]):
            eng.run_range(d, len(data), lo, hi, True)
            eng.accumulate()
        t = eng.fetch()
        got, got_items, got_tok = t.arrays(), list(t.items()), t.tokens
        t.close()
        assert eng.accumulate_info()["passes"] == 5
        eng.run_device(d, len(data))
        t = eng.fetch()
        one, one_items, one_tok = t.arrays(), list(t.items()), t.tokens
        t.close()
    finally:
        eng.free(d)
    assert got_tok == one_tok
    assert_tables_equal(got, one)
    # engine order: the words of at most 16 bytes lie exactly as one pass puts them
    assert [x for x in got_items if C.is_short(x[0])] == [x for x in one_items if C.is_short(x[0])]
    n_short = sum(1 for w, _ in got_items if C.is_short(w))
    assert all(C.is_short(w) for w, _ in got_items[:n_short])


# ---- 6. the result is the total for every consumer
def test_consumers_see_the_total(eng, tmp_path):
    A, B = C.shape_tables()
    C.fold_tables(eng, A, C.count_tables()[0], B)
    items, tok = C.fetched(eng)
    assert (sorted(items), tok) == C.oracle_sum(A, C.count_tables()[0], B)
    top = eng.top_words(10)
    order = sorted(range(len(items)), key=lambda i: (-items[i][1], i))[:10]
    assert list(top.items()) == [items[i] for i in order] and top.tokens == tok
    top.close()
    text = b"".join(w + b" %d\n" % c for w, c in items)
    assert eng.result_text() == text
    eng.write_result(str(tmp_path / "total.txt"))
    assert (tmp_path / "total.txt").read_bytes() == text
    eng.sort_result()
    assert C.fetched(eng) == (sorted(items), tok)
    assert code_of(eng.accumulate) == mox.MOX_ESTATE  # sorted, it is still the folded total


# ---- 7. once only, and reset
def test_once_only_and_reset(eng):
    assert code_of(eng.accumulate) == mox.MOX_ESTATE  # nothing has run
    zero = {"passes": 0, "words": 0, "tokens": 0, "device_bytes": 0}
    assert eng.accumulate_info() == zero
    tabs = [C.edge_tables(100, 70, "alternate")[0], C.edge_tables(100, 70, "alternate")[1], C.LAST1]
    for k, t in enumerate(tabs):
        C.load(eng, t)
        eng.accumulate()
        want, wtok = C.oracle_sum(*tabs[: k + 1])
        info = eng.accumulate_info()
        assert (info["passes"], info["words"], info["tokens"]) == (k + 1, len(want), wtok)
        assert info["device_bytes"] > 0
        assert code_of(eng.accumulate) == mox.MOX_ESTATE  # a result folds once
        assert eng.accumulate_info() == info
        got, tok = C.fetched(eng)
        assert (sorted(got), tok) == (want, wtok)
    eng.accumulate_reset()
    assert eng.accumulate_info() == zero
    C.load(eng, C.LAST1_OTHER)
    eng.accumulate()
    got, tok = C.fetched(eng)
    assert (sorted(got), tok) == C.oracle_sum(C.LAST1_OTHER)
    assert eng.accumulate_info()["passes"] == 1


# ---- 8. failure keeps the total
def test_failure_keeps_the_total(eng):
    """MOX_TEST_FAIL_ACCUM=1: the merge fails after both tables are packed, where
    the run's buffers may already be gone.  The total stays A, the result becomes
    that total (the result then lies in the accumulator's own buffers: every
    consumer reads it there), and a new run folds as if nothing had happened."""
    A, B = C.shape_tables()
    C.load(eng, A)
    eng.accumulate()
    before = eng.accumulate_info()
    C.load(eng, B)
    os.environ["MOX_TEST_FAIL_ACCUM"] = "1"
    try:
        assert code_of(eng.accumulate) == mox.MOX_ENOMEM
    finally:
        del os.environ["MOX_TEST_FAIL_ACCUM"]
    after = eng.accumulate_info()
    # (device_bytes may have grown: the packer's scratch is the accumulator's too)
    assert [after[k] for k in ("passes", "words", "tokens")] == [before[k] for k in ("passes", "words", "tokens")]
    got, tok = C.fetched(eng)
    assert (sorted(got), tok) == C.oracle_sum(A)
    assert eng.result_text() == b"".join(w + b" %d\n" % c for w, c in got)
    assert code_of(eng.accumulate) == mox.MOX_ESTATE
    C.load(eng, B)
    eng.accumulate()
    got, tok = C.fetched(eng)
    assert (sorted(got), tok) == C.oracle_sum(A, B)
    assert eng.accumulate_info()["passes"] == 2


# ---- 9. growth
def test_growth_from_a_tiny_first_run():
    e = mox.Engine(device=0)
    try:
        tiny = b"tiny first run " * 68  # ~1 KiB
        run_text(e, tiny)
        e.accumulate()
        A, B = C.half_shared(300000, seed=9)
        got, tok = C.fold_tables(e, A, B)
        info = e.accumulate_info()
    finally:
        e.close()
    want, wtok = C.oracle_sum(([b"tiny", b"first", b"run"], [68, 68, 68]), A, B)
    assert len(want) == 450003 and info["words"] == 450003 and info["passes"] == 3
    assert tok == wtok and got == want


# ---- 10. check builds (their own processes: one library per process)
CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import accum_cases as C, mox
e = mox.Engine(device=0)
"""


def run_child(body, lib):
    code = CHILD % (os.path.join(ROOT, "map-oxidize_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")) + body
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, MOX_LIB=lib), capture_output=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout


def test_bounds_check_build_merges_clean():
    out = run_child(r"""
A, B = C.shape_tables()
assert C.fold_tables(e, A, B) == C.oracle_sum(A, B)
e.accumulate_reset()
A, B = C.half_shared(20000)
assert C.fold_tables(e, A, B) == C.oracle_sum(A, B)
e.close()
print("check build clean")
""", mox.CHECK_LIB_PATH)
    assert b"check build clean" in out


def test_collision_build_merges_exactly():
    """libmox_hc.so: the packer's long-word hash is truncated to 8 bits like the
    map's, so 600 distinct long words collide in the merge pass's long table."""
    out = run_child(r"""
A, B = C.long_tables(300)
C.load(e, A); e.accumulate(); C.load(e, B)
before = e.stats()["path_hits"][mox.PATH_LONG_EQHASH]
e.accumulate()
after = e.stats()["path_hits"][mox.PATH_LONG_EQHASH]
got, tok = C.fetched(e)
assert (sorted(got), tok) == C.oracle_sum(A, B)
assert after > before and after > 0, (before, after)
e.accumulate_reset()
A, B = C.shape_tables()
assert C.fold_tables(e, A, B) == C.oracle_sum(A, B)
e.close()
print("collision build exact", after - before)
""", mox.HC_LIB_PATH)
    assert b"collision build exact" in out


# ---- 11. files
@pytest.fixture(scope="module")
def file64k():
    data = C.mixed_text(40 << 10, 31)
    data = (data + corpus.fill(corpus.ZIPF, 32, 0, 64 << 10).tobytes())[: 64 << 10]
    return data.decode("utf-8", "ignore").encode().ljust(64 << 10, b" ")


@pytest.mark.parametrize("chunk", [4096, 0, 1 << 20])
def test_accumulate_file_chunks(eng, tmp_path, file64k, chunk):
    p = C.data_path(tmp_path, "f.txt", file64k)
    eng.accumulate_file(p, chunk)
    got, tok = C.fetched(eng)
    t = eng.count_file(p)
    assert (sorted(got), tok) == (t.sorted_items(), t.tokens) == coracle.count(file64k)
    t.close()
    want_passes = len(C.chunk_cuts(file64k, chunk))
    assert eng.accumulate_info()["passes"] == want_passes
    assert want_passes == (16 if chunk == 4096 else 1)


def test_accumulate_files_one_after_the_other(eng, tmp_path, file64k):
    other = C.mixed_text(24 << 10, 33).decode("utf-8", "ignore").encode()
    pa, pb = C.data_path(tmp_path, "a.txt", file64k), C.data_path(tmp_path, "b.txt", other)
    empty = C.data_path(tmp_path, "empty.txt", b"")
    eng.accumulate_file(pa, 8192)
    eng.accumulate_file(empty, 4096)  # a valid part that adds nothing
    mid = eng.accumulate_info()
    eng.accumulate_file(pb, 0)
    eng.accumulate_file(empty, 0)
    got, tok = C.fetched(eng)
    assert (sorted(got), tok) == coracle.count(file64k + b"\n" + other)
    assert (mid["words"], mid["tokens"]) == (len(coracle.count(file64k)[0]), coracle.count(file64k)[1])
    assert eng.accumulate_info()["passes"] == len(C.chunk_cuts(file64k, 8192)) + 3
    t = mox.count_files([pa, pb], chunk_bytes=4096)
    assert (t.sorted_items(), t.tokens) == coracle.count(file64k + b"\n" + other)
    t.close()
    t = mox.count_files([])
    assert t.n == 0
    t.close()


def test_accumulate_file_errors(eng, tmp_path, file64k):
    p = C.data_path(tmp_path, "f.txt", file64k)
    assert code_of(lambda: eng.accumulate_file(p, 100)) == mox.MOX_EINVAL
    assert code_of(lambda: eng.accumulate_file(p, 255)) == mox.MOX_EINVAL
    assert code_of(lambda: eng.accumulate_file(str(tmp_path / "missing.txt"), 4096)) == mox.MOX_EIO
    assert eng.accumulate_info()["passes"] == 0
    chunks = C.chunk_cuts(file64k, 4096)
    lo, hi = chunks[2]
    pos = lo + 100
    while file64k[pos] in C.ASCII_WS or file64k[pos] >= 0x80 or file64k[pos + 1] >= 0x80:
        pos += 1
    bad = bytearray(file64k)
    bad[pos] = 0xFF
    assert lo < pos < hi and C.chunk_cuts(bytes(bad), 4096) == chunks
    pbad = C.data_path(tmp_path, "bad.txt", bytes(bad))
    with pytest.raises(mox.Utf8Error) as ex:
        eng.accumulate_file(pbad, 4096)
    assert "byte %d)" % pos in str(ex.value)  # the file's offset, not the chunk's
    info = eng.accumulate_info()
    assert info["passes"] == 2
    assert info["tokens"] == coracle.count(file64k[:lo])[1]


def test_accumulate_file_engine_group(tmp_path):
    data = C.mixed_text(200 << 10, 35).decode("utf-8", "ignore").encode()
    data = (data + corpus.fill(corpus.ZIPF, 36, 0, 256 << 10).tobytes())[: 256 << 10]
    p = C.data_path(tmp_path, "g.txt", data)
    g = mox.Engine(device=0, n_gpus=2, transport=mox.XPORT_COPY, devices=[0, 0])
    try:
        g.accumulate_file(p, 64 << 10)
        got, tok = C.fetched(g)
        assert g.accumulate_info()["passes"] == len(C.chunk_cuts(data, 64 << 10)) == 4
    finally:
        g.close()
    assert (sorted(got), tok) == coracle.count(data)


def test_cli_several_files_and_chunk(tmp_path, file64k):
    other = C.mixed_text(24 << 10, 37).decode("utf-8", "ignore").encode()
    C.data_path(tmp_path, "a.txt", file64k)
    C.data_path(tmp_path, "b.txt", other)
    cli = os.path.join(ROOT, "map-oxidize_amd", "mox", "meduce-gpu")
    out = tmp_path / "both.txt"
    r = subprocess.run([cli, "a.txt", "b.txt", "--chunk", "4096", "--out", str(out)], cwd=tmp_path, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want, _ = coracle.count(file64k + b"\n" + other)
    assert sorted(out.read_bytes().splitlines(keepends=True)) == sorted(w + b" %d\n" % c for w, c in want)
    lines = r.stdout.split(b"\n")
    assert lines[0] == b"Top 10 words:" and len([x for x in lines if x]) == 11
    assert [int(x.rsplit(b": ", 1)[1]) for x in lines[1:11]] == sorted((c for _, c in want), reverse=True)[:10]


# ---- 12. ranks: fold the local windows, then one exchange + gather
def test_ranks_fold_windows_then_exchange():
    data = C.mixed_text(1 << 20, 41).decode("utf-8", "ignore").encode()
    world = 2
    x = mdist.ThreadAlltoall(world)
    out, errs = [None] * world, []

    def rank_main(r):
        try:
            lo, hi, ob, oe, at_end = mdist.shard_range(len(data), world, r)
            buf = data[lo:hi]
            mid = ob + (oe - ob) // 2  # two windows of the owned range: any byte may start a window
            e = mox.Engine(device=0)
            try:
                d = e.alloc(len(buf))
                try:
                    e.h2d(d, buf)
                    for a, b in ((ob, mid), (mid, oe)):
                        e.run_range(d, len(buf), a, b, at_end)
                        e.accumulate()
                    e.exchange_host(world, r, x.fn(r))
                    e.gather_host(world, r, x.fn(r), root=0)
                    out[r] = C.fetched(e)
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
    items, tok = out[0]
    assert (sorted(items), tok) == coracle.count(data)
