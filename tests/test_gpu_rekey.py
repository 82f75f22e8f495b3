"""GPU: the device re-keying (mox_rekey_result, map-oxidize_amd/csrc/mox_rekey.hip)
against the Python model of include/mox.h's rules.  Every comparison is exact:
the expectation is rekey_cases.expected over a fetch() of the same
device-resident result taken immediately before the call, with no run in
between.  After the call four things are compared: the fetched table as a
sorted list; its tokens; every info field (ms and device_bytes: > 0); and the
order of the rows of at most 16 bytes without NUL, against a second engine's
reduce_pairs over the model's windowed rows (the order contract) -- or, when no
row changed, the whole table in order against what it was.  Tables come from
Engine.reduce_pairs unless the case says otherwise.  The model, the case tables
and the CPU checks of their shapes: rekey_cases.py, test_rekey_abi.py."""
import ctypes
import os
import subprocess
import threading

import pytest

import coracle
import lookup_cases
import mox
import rekey_cases as C
import top_cases
from conftest import ROOT
from mox import corpus
from mox import dist as mdist
from rekey_cases import fetched

pytestmark = pytest.mark.gpu


@pytest.fixture()
def eng():
    e = mox.Engine(device=0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def ref():
    """The second engine of the order contract."""
    e = mox.Engine(device=0)
    yield e
    e.close()


def load(e, table):
    e.reduce_pairs(table[0], table[1]).close()


def shorts(items):
    return [(w, c) for w, c in items if C.is_short(w)]


def assert_rekey(e, ref, **spec):
    """rekey_result(**spec) on e's resident result against the model over the
    fetch taken just before.  Returns (source items, new items, info)."""
    items, tok = fetched(e)
    table, rows, winfo = C.expected(items, tokens=tok, **spec)
    info = e.rekey_result(**spec)
    got, tokens = fetched(e)
    assert sorted(got) == sorted(table)
    assert tokens == winfo["tokens_out"]
    assert {k: info[k] for k in C.INFO_KEYS} == winfo
    assert info["device_bytes"] > 0 and info["ms"] > 0
    if winfo["words_changed"] == 0:
        assert got == items
    elif ref is not None:
        t = ref.reduce_pairs([w for w, _ in rows], [c for _, c in rows])
        try:
            assert shorts(got) == shorts(t.items())
        finally:
            t.close()
    return items, got, info


# ---- 1. row-count edges
@pytest.mark.parametrize("n", C.EDGE_NS)
def test_row_count_edges(eng, ref, n):
    load(eng, C.edge_table(n))
    items, got, info = assert_rekey(eng, ref, punct=True)
    assert len(items) == n and len(got) == n - n // 3 and info["words_changed"] == n // 3


# ---- 2. grid strides
def test_grid_strides(eng, ref, monkeypatch):
    table = C.edge_table(C.STRIDE_N)
    load(eng, table)
    _, free, _ = assert_rekey(eng, ref, punct=True)
    monkeypatch.setenv("MOX_REKEY_GRID", str(C.STRIDE_GRID))
    load(eng, table)
    _, capped, _ = assert_rekey(eng, ref, punct=True)
    assert sorted(capped) == sorted(free) and shorts(capped) == shorts(free)  # the grid does not matter


# ---- 3. window shapes
def test_lead_and_trail_runs(eng, ref):
    load(eng, C.run_table())
    items, got, info = assert_rekey(eng, ref, punct=True)
    assert len(items) == 125 and len(got) == 5 and info["words_dropped"] == 0 and info["words_changed"] == 120
    assert sorted(len(w) for w, _ in got) == [1, 5, 16, 17, 300]


@pytest.mark.parametrize("sort", [True, False])
def test_word_starts_and_leads(eng, ref, sort):
    words, counts = C.phase_table()
    load(eng, (words, counts))
    if sort:
        eng.sort_result()
        t = eng.fetch()
        _, offs, _ = t.arrays()
        got_words = [w for w, _ in t.items()]
        t.close()
        cover = {(int(offs[i]) % 8, len(w) - len(w.lstrip(b"-"))) for i, w in enumerate(got_words)}
        assert cover == {(o, lead) for o in range(8) for lead in range(9)}  # every start mod 8 with every lead
    items, got, info = assert_rekey(eng, ref, punct=True)
    assert info["words_dropped"] == 0 and len(got) == len(items) == 360 and info["words_changed"] > 300


def test_window_shapes(eng, ref):
    load(eng, C.shape_table())
    items, got, info = assert_rekey(eng, ref, punct=True)
    d = dict(got)
    assert info["words_dropped"] == 5 and C.BIG_WORD in d and "Σ".encode() in d and "Привет".encode() in d
    assert b"a\x00b" in d and b"\x00" in d and {15, 16, 17} <= {len(w) for w in d}
    src = dict(items)
    assert d[C.BIG_WORD] == src[C.BIG_WORD] + src[b"(" + C.BIG_WORD + b")"]
    assert d["Σ".encode()] == src["Σ".encode()] + src["Σ.".encode()]


def test_one_byte_word_at_the_end_of_a_sorted_table(eng, ref):
    load(eng, C.last_is_one_byte())
    eng.sort_result()
    items, _ = fetched(eng)
    assert items[-1][0] == b"~" and items[-2][0] == b"}~"
    _, got, info = assert_rekey(eng, ref, trim=b"}")
    assert dict(got)[b"~"] == items[-1][1] + items[-2][1] and info["words_changed"] == 1


# ---- 4. merging
def test_merging(eng, ref):
    load(eng, C.merge_table())
    _, got, info = assert_rekey(eng, ref, punct=True)
    d = dict(got)
    assert d[b"the"] == 100 and d[b"a_word_of_20_bytes_x"] == 10
    assert d[b"zz"] == 0 and d[b"zf"] == 5 and d[b"z_long_word_with_count_0"] == 0  # 0 + 0, 0 + 5: present
    assert d[b"wrap"] == 1 and d[b"a_long_word_that_wraps"] == 5  # mod 2^64
    assert info["words_dropped"] == 1 and info["tokens_dropped"] == 0 and len(d) == 7


# ---- 5. the cap
@pytest.mark.parametrize("spec", [dict(max_chars=1), dict(max_chars=2), dict(max_chars=16), dict(max_chars=17),
                                  dict(max_chars=1, punct=True), dict(max_chars=2, punct=True), dict(max_chars=3, trim=b"(")])
def test_cap(eng, ref, spec):
    load(eng, C.cap_table())
    items, got, info = assert_rekey(eng, ref, **spec)
    d = dict(got)
    if spec == dict(max_chars=1):  # letter frequencies, whatever the character's width
        src = dict(items)
        assert d["日".encode()] == src["日".encode()] + src["日本語".encode()] + src["日x".encode()]
        assert d["\U0001d11e".encode()] == sum(c for w, c in items if w.startswith("\U0001d11e".encode()))
        assert b"\x80\x80a" in d and b"\x80" * 20 in d and b"(" in d
    if spec.get("max_chars") in (16, 17):
        assert spec["max_chars"] in {len(w) for w in d} and info["words_changed"] >= 40


def test_cap_larger_than_every_word_is_a_noop(eng, ref):
    load(eng, C.cap_table())
    items, got, info = assert_rekey(eng, ref, max_chars=1000)
    assert info["words_changed"] == 0 and got == items and info["words_out"] == len(items)


# ---- 6. no-op and idempotence
def test_noop_keeps_order_and_flags(eng, ref):
    table = C.plain_words(3000)
    load(eng, table)
    eng.sort_result()
    items, got, info = assert_rekey(eng, ref, punct=True)
    assert info["words_changed"] == 0 and [w for w, _ in got] == sorted(table[0])
    eng.set_flags(mox.MOX_F_SORT_BYTES)  # still marked sorted: the implicit sort has nothing to do
    assert fetched(eng)[0] == got
    eng.set_flags(0)
    eng.rank_result()
    ranked, _ = fetched(eng)
    _, got, info = assert_rekey(eng, ref, punct=True, max_chars=100)
    assert info["words_changed"] == 0 and got == ranked
    eng.set_flags(mox.MOX_F_SORT_BYTES)  # still marked ranked: the implicit sort leaves it alone
    assert fetched(eng)[0] == ranked
    eng.set_flags(0)
    _, got, info = assert_rekey(eng, ref)  # the zeroed spec
    assert info["words_changed"] == 0 and got == ranked
    eng.accumulate()  # an unfolded result still: it folds, once
    assert_rekey(eng, ref, punct=True)
    with pytest.raises(mox.MoxError) as ei:
        eng.accumulate()
    assert ei.value.code == mox.MOX_ESTATE


def test_second_call_changes_nothing(eng, ref):
    load(eng, C.shape_table())
    assert_rekey(eng, ref, punct=True, max_chars=12)
    once, _ = fetched(eng)
    _, got, info = assert_rekey(eng, ref, punct=True, max_chars=12)
    assert info["words_changed"] == 0 and got == once and info["words_in"] == info["words_out"]


# ---- 7. sources
@pytest.fixture(scope="module")
def zipf256k():
    return corpus.fill(corpus.ZIPF, 23, 0, 256 << 10).tobytes()


def model_of_text(data, **spec):
    want, tok = coracle.count(data)
    table, _, info = C.expected(want, tokens=tok, **spec)
    return sorted(table), info


def test_a_runs_result(eng, ref, zipf256k):
    eng.count(zipf256k).close()
    items, got, info = assert_rekey(eng, ref, punct=True)
    want, winfo = model_of_text(zipf256k, punct=True)
    assert sorted(got) == want and {k: info[k] for k in C.INFO_KEYS} == winfo
    assert info["words_changed"] > 100 and info["words_out"] < info["words_in"]


@pytest.mark.parametrize("form", ["sorted", "ranked", "filtered"])
def test_other_forms(eng, ref, zipf256k, form):
    eng.count(zipf256k).close()
    if form == "sorted":
        eng.sort_result()
    elif form == "ranked":
        eng.rank_result()
    else:
        eng.filter_result(min_count=2)
    _, got, info = assert_rekey(eng, ref, punct=True)
    assert info["words_changed"] > 50
    if form != "filtered":
        assert sorted(got) == model_of_text(zipf256k, punct=True)[0]
    # the new table is neither sorted nor ranked: the implicit sort runs again
    eng.set_flags(mox.MOX_F_SORT_BYTES)
    assert fetched(eng)[0] == sorted(got)


def test_the_accumulators_total(eng, ref, zipf256k):
    half = zipf256k.rfind(b" ", 0, len(zipf256k) // 2) + 1
    for part in (zipf256k[:half], zipf256k[half:]):
        eng.count(part).close()
        eng.accumulate()
    before = eng.accumulate_info()
    _, got, info = assert_rekey(eng, ref, punct=True)
    assert sorted(got) == model_of_text(zipf256k, punct=True)[0]
    after = eng.accumulate_info()
    assert {k: after[k] for k in ("passes", "words", "tokens")} == {k: before[k] for k in ("passes", "words", "tokens")}
    assert after["words"] == info["words_in"] > info["words_out"]  # the accumulator is untouched
    with pytest.raises(mox.MoxError) as ei:
        eng.accumulate()  # a re-keyed folded total is folded
    assert ei.value.code == mox.MOX_ESTATE


def test_a_gathered_group_result(ref, zipf256k):
    g = mox.Engine(device=0, n_gpus=2, transport=mox.XPORT_COPY, devices=[0, 0])
    try:
        g.count(zipf256k).close()
        _, got, _ = assert_rekey(g, ref, punct=True)
    finally:
        g.close()
    assert sorted(got) == model_of_text(zipf256k, punct=True)[0]


# ---- 8. consumers
def test_consumers_see_the_new_table(eng, ref):
    words, counts = C.edge_table(3000)
    words += [b"the", b"the,", b"(the)", b"the."]
    counts += [1000, 2000, 3000, 4000]
    load(eng, (words, counts))
    _, got, _ = assert_rekey(eng, ref, punct=True)
    for k in (1, 10, 200):
        t = eng.top_words(k)
        assert list(t.items()) == top_cases.expected(got, k) and t.tokens == sum(c for _, c in got)
        t.close()
    assert eng.result_text() == b"".join(w + b" %d\n" % c for w, c in got)
    queries = [b"the", b"the,", b"w1", b"w2", b"absent"]
    got_c, got_i = eng.lookup(queries, with_index=True)
    want_c, want_i = lookup_cases.expected(got, queries)
    assert got_c.tolist() == want_c and got_i.tolist() == want_i and want_c[:2] == [10000, 0]
    t = eng.fetch_rows(5, 7)
    assert list(t.items()) == got[5:12]
    t.close()
    eng.filter_result(min_count=500)
    kept = [(w, c) for w, c in got if c >= 500]
    assert fetched(eng)[0] == kept
    eng.rank_result()
    ranked, _ = fetched(eng)
    assert ranked == sorted(kept, key=lambda wc: -wc[1]) and ranked[0] == (b"the", 10000)
    eng.sort_result()
    assert fetched(eng)[0] == sorted(kept)


# ---- 9. commutes with sums
def test_commutes_with_sums(ref, zipf256k):
    cuts = [0]
    for j in range(1, 4):
        cuts.append(zipf256k.rfind(b" ", 0, j * len(zipf256k) // 4) + 1)
    cuts.append(len(zipf256k))
    a, b = mox.Engine(device=0), mox.Engine(device=0)
    try:
        for lo, hi in zip(cuts, cuts[1:]):
            a.count(zipf256k[lo:hi]).close()
            a.rekey_result(punct=True)
            a.accumulate()
        folded, ftok = fetched(a)
        b.count(zipf256k).close()
        b.rekey_result(punct=True)
        once, otok = fetched(b)
        assert a.accumulate_info()["passes"] == 4
        with pytest.raises(mox.MoxError) as ei:
            a.rekey_result(punct=True)  # nothing changes ...
            a.accumulate()  # ... and the total is still folded
        assert ei.value.code == mox.MOX_ESTATE
    finally:
        a.close()
        b.close()
    assert sorted(folded) == sorted(once) == model_of_text(zipf256k, punct=True)[0] and ftok == otok


# ---- 10. distributed
def test_ranks_rekey_then_exchange():
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
                    info = e.rekey_result(punct=True)
                    assert info["words_changed"] > 0
                    e.exchange_host(world, r, x.fn(r))
                    e.gather_host(world, r, x.fn(r), root=0)
                    out[r] = fetched(e)
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
    want, winfo = model_of_text(data, punct=True)
    assert sorted(items) == want and tok == winfo["tokens_out"]


# ---- 11. failure
def test_injected_failure_leaves_the_result(eng, ref, monkeypatch):
    load(eng, C.shape_table())
    eng.sort_result()
    before = fetched(eng)
    monkeypatch.setenv("MOX_TEST_FAIL_REKEY", "1")
    with pytest.raises(mox.MoxError) as ei:
        eng.rekey_result(punct=True)
    assert ei.value.code == mox.MOX_ENOMEM
    assert fetched(eng) == before
    eng.set_flags(mox.MOX_F_SORT_BYTES)  # still marked sorted
    assert fetched(eng) == before
    eng.set_flags(0)
    monkeypatch.delenv("MOX_TEST_FAIL_REKEY")
    assert_rekey(eng, ref, punct=True)


def test_fresh_engine_is_estate(eng):
    with pytest.raises(mox.MoxError) as ei:
        eng.rekey_result(punct=True)
    assert ei.value.code == mox.MOX_ESTATE


def test_bad_arguments_are_einval(eng):
    load(eng, ([b"a,", b"b"], [1, 2]))
    before = fetched(eng)
    L = eng._L
    info = mox.RekeyInfo(words_in=77)
    bad = mox.Rekey()
    bad.reserved[0] = 1
    for k in (mox.Rekey(flags=2), mox.Rekey(flags=0x80000001), mox.Rekey(pad=1), bad):
        assert L.mox_rekey_result(eng._h, ctypes.byref(k), ctypes.byref(info)) == mox.MOX_EINVAL
    assert L.mox_rekey_result(eng._h, None, ctypes.byref(info)) == mox.MOX_EINVAL
    assert info.words_in == 77 and fetched(eng) == before
    with pytest.raises(ValueError):
        eng.rekey_result(trim=b"a\xc3")
    assert fetched(eng) == before
    k = mox.Rekey(flags=mox.REKEY_TRIM_ASCII_PUNCT)
    assert L.mox_rekey_result(eng._h, ctypes.byref(k), None) == mox.MOX_OK  # info may be NULL
    assert sorted(fetched(eng)[0]) == [(b"a", 1), (b"b", 2)]


# ---- 12. the other builds
@pytest.mark.parametrize("lib_path", [mox.CHECK_LIB_PATH, mox.HC_LIB_PATH])
def test_other_builds(lib_path):
    e = mox.Engine(device=0, lib_path=lib_path)
    try:
        for table in (C.run_table(), C.phase_table(), C.shape_table()):  # item 3
            load(e, table)
            assert_rekey(e, None, punct=True)
        if lib_path == mox.HC_LIB_PATH:
            load(e, C.merge_table())  # item 4
            assert_rekey(e, None, punct=True)
            words = [b"(a_long_word_number_%04d)" % i for i in range(400)] + [b"a_long_word_number_%04d," % i for i in range(400)]
            load(e, (words, list(range(800))))
            before = e.stats()["path_hits"][mox.PATH_LONG_EQHASH]  # (of the load's own reduce pass)
            _, got, _ = assert_rekey(e, None, punct=True)
            assert len(got) == 400
            assert e.stats()["path_hits"][mox.PATH_LONG_EQHASH] > before  # the re-keyed long words collide in the long table
    finally:
        e.close()


# ---- 13. the command-line tool
def test_cli_trim_punct(tmp_path):
    data = corpus.fill(corpus.ZIPF, 31, 0, 64 << 10).tobytes()
    (tmp_path / "shakes.txt").write_bytes(data)
    cli = os.path.join(ROOT, "map-oxidize_amd", "mox", "meduce-gpu")
    r = subprocess.run([cli, "--trim-punct"], cwd=tmp_path, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want, _ = model_of_text(data, punct=True)
    lines = (tmp_path / "final_result.txt").read_bytes().splitlines()
    assert set(lines) == {w + b" %d" % c for w, c in want} and len(lines) == len(want)
    top = r.stdout.split(b"\n")
    assert top[0] == b"Top 10 words:" and len([x for x in top if x]) == 11
    assert [int(x.rsplit(b": ", 1)[1]) for x in top[1:11]] == sorted((c for _, c in want), reverse=True)[:10]
    plain = subprocess.run([cli], cwd=tmp_path, capture_output=True, timeout=120)
    assert plain.returncode == 0 and len((tmp_path / "final_result.txt").read_bytes().splitlines()) > len(want)
