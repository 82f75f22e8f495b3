"""GPU: sequences of calls over the device-resident result, an engine and the
state model (result_model.py) in lockstep.  After every mutating step, error
steps included, every reader runs and everything is compared for equality: the
error codes, the info structs, the fetched table, its pages, the text, the
lookups, the searches, the top-k, the histograms, the accumulator's info.
Integers and bytes only: there is no tolerance anywhere.  No expectation comes
from the library, with one exception the model names: the row order of a run, a
re-key or a merge is the engine's own, so the first fetch after one is compared
as a multiset and its order then holds exactly for everything that follows.

A failure's message carries the sequence as a string (sequence_cases.decode
reads it back), the step and the model's state: add the string to
sequence_cases.REPLAYS to keep it."""
import os

import pytest

import filter_cases
import join_cases
import mox
import rank_cases
import sequence_cases as S
from result_model import ACCUM_INFO_KEYS, OK, REKEY_INFO_KEYS, ResultModel

pytestmark = pytest.mark.gpu

INFO_KEYS = {"rank": rank_cases.INFO_KEYS, "filter": filter_cases.INFO_KEYS, "join": join_cases.INFO_KEYS, "rekey": REKEY_INFO_KEYS}


def table_of(t):
    try:
        return list(t.items()), t.tokens
    finally:
        t.close()


def engine_step(e, tok, n):
    """One step on the engine: (error code or OK, info or None, the table a run fetched or None)."""
    method, kw, fail = S.call_of(tok, n)
    env = S.FAIL_ENV.get(method) if fail else None
    if env:
        os.environ[env] = "1"
    try:
        if method == "run":
            return OK, None, table_of(e.reduce_pairs(kw["words"], kw["counts"]))
        if method == "sort":
            return OK, e.sort_result(), None
        if method == "rank":
            info = e.rank_result(**kw)
        elif method == "filter":
            info = e.filter_result(**kw)
        elif method == "join":
            info = e.join_total(**kw)
        elif method == "rekey":
            info = e.rekey_result(**kw)
        else:
            return OK, getattr(e, method)(), None
        return OK, {k: info[k] for k in INFO_KEYS[method]}, None
    except mox.MoxError as ex:
        return ex.code, None, None
    finally:
        if env:
            del os.environ[env]


def engine_read_all(e, rows, n):
    """sequence_cases.read_all's sweep on the engine, in the same order and form."""
    out = []

    def put(reader, tag, fn):
        try:
            out.append((reader, tag, fn()))
        except mox.MoxError as ex:
            out.append((reader, tag, ("error", ex.code)))

    def find(mode):
        first, last, sums = e.find(S.find_keys(n), mode)
        return first.tolist(), last.tolist(), sums.tolist()

    def lookup():
        counts, index = e.lookup(S.queries(n), with_index=True)
        return counts.tolist(), index.tolist()

    def hist(key):
        hk, hw, ht, hr, words, tokens = e.histogram(key)
        return list(zip(hk.tolist(), hw.tolist(), ht.tolist(), hr.tolist())), words, tokens

    def accumulate_info():
        info = e.accumulate_info()
        return {k: info[k] for k in ACCUM_INFO_KEYS}

    put("fetch", "", lambda: table_of(e.fetch()))
    for first, cnt in S.pages(rows):
        put("fetch_rows", (first, cnt), lambda: table_of(e.fetch_rows(first, cnt)))
    put("result_text", "", e.result_text)
    put("find_prefix", "", lambda: find("prefix"))
    put("find_exact", "", lambda: find("exact"))
    put("lookup", "", lookup)
    put("top_words", 10, lambda: table_of(e.top_words(10)))
    put("hist_count", "", lambda: hist("count"))
    put("hist_first", "", lambda: hist("first"))
    put("top_rows", (1, 1500, 7), lambda: table_of(e.top_rows(1, 1500, 7)))
    put("complete", b"w1", lambda: table_of(e.complete(b"w1", 5)))
    put("accumulate_info", "", accumulate_info)
    return out


def brief(x, limit=300):
    s = repr(x)
    return s if len(s) <= limit else s[:limit] + "... (%d characters)" % len(s)


def first_difference(got, want):
    if isinstance(got, (list, tuple)) and isinstance(want, (list, tuple)) and type(got) is type(want):
        if len(got) != len(want):
            return "lengths %d and %d" % (len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            if g != w:
                return "[%d]: %s" % (i, first_difference(g, w))
    return "got %s, want %s" % (brief(got), brief(want))


def run_sequence(seq, lib_path=None):
    n, sort_flag, steps = S.decode(seq)
    m = ResultModel(sort_flag)
    e = mox.Engine(device=0, flags=mox.MOX_F_SORT_BYTES if sort_flag else 0, lib_path=lib_path)
    try:
        for i, tok in enumerate(steps):
            def where(what):
                return "%s\n  sequence: %s\n  step %d: %s\n  model after it: %s" % (what, seq, i, tok, m.state_line())

            code, info, run_table = engine_step(e, tok, n)
            want_code, want_info = S.model_step(m, tok, n)
            assert code == want_code, where("the call returned %d, the model says %d" % (code, want_code))
            if want_info is not None:
                assert info == {k: want_info[k] for k in info}, where("the info differs: %s" % first_difference(info, want_info))

            # the first fetch: the engine's own order is taken from it where the model cannot know it
            # (a run's table comes back from the run itself: mox.Engine.reduce_pairs fetches)
            try:
                first = run_table if run_table is not None else table_of(e.fetch())
            except mox.MoxError as ex:
                first = ("error", ex.code)
            try:
                want_first = m.fetch()
            except S.ModelError as ex:
                want_first = ("error", ex.code)
            if not m.order_known and first[0] != "error":
                assert (sorted(first[0]), first[1]) == (sorted(want_first[0]), want_first[1]), where(
                    "the fetched rows differ as a multiset: %s" % first_difference((sorted(first[0]), first[1]), (sorted(want_first[0]), want_first[1])))
                m.adopt_order(first[0])
                want_first = m.fetch()
            assert first == want_first, where("the fetched table differs: %s" % first_difference(first, want_first))

            want = S.read_all(m, n)
            got = engine_read_all(e, m.n, n)
            for (reader, tag, g), (_, _, w) in zip(got, want):
                assert g == w, where("%s %r differs: %s" % (reader, tag, first_difference(g, w)))
            assert [r for r, _, _ in got] == [r for r, _, _ in want]

            # the readers changed nothing (under the sort flag: nothing more)
            try:
                again = table_of(e.fetch())
            except mox.MoxError as ex:
                again = ("error", ex.code)
            assert again == first, where("a second fetch differs from the first: %s" % first_difference(again, first))
    finally:
        e.close()


# 1. every ordered pair of kinds, each from a fresh run; and the same sweep where sorted and ranked hold at once
@pytest.mark.parametrize("first", S.KINDS)
def test_pairs(first):
    run_sequence(S.pair_sequence(first, S.PAIR_N))


@pytest.mark.parametrize("n", S.SMALL_NS)
def test_pairs_at_small_sizes(n):
    for seq in S.pair_set(n):
        run_sequence(seq)


# every kind applied to a result in each of its homes
@pytest.mark.parametrize("state", list(S.STATE_PATHS))
def test_every_kind_in_every_home(state):
    run_sequence(S.home_sequence(state, S.PAIR_N))


# 2. seeded walks from 4097 rows, and both buffer pairs at a small, a large and a small size
@pytest.mark.parametrize("group", range(0, len(S.WALK_SEEDS), S.WALK_GROUP))
def test_walks(group):
    for seed in S.WALK_SEEDS[group:group + S.WALK_GROUP]:
        run_sequence(S.walk(seed))


@pytest.mark.parametrize("i", range(len(S.PINGPONG)))
def test_pingpong(i):
    run_sequence(S.PINGPONG[i])


# 3. the pair sweep under MOX_F_SORT_BYTES: fetch, pages, text and find may sort, a ranking survives them
@pytest.mark.parametrize("first", S.KINDS)
def test_pairs_with_the_sort_flag(first):
    run_sequence(S.pair_sequence(first, S.PAIR_N, sort_flag=True))


# 4. the bounds-checking build and the forced-collision build
@pytest.mark.parametrize("i", range(4))
@pytest.mark.parametrize("build", ("check", "hc"))
def test_other_builds(build, i):
    run_sequence(S.other_build_walks(4)[i], lib_path=mox.CHECK_LIB_PATH if build == "check" else mox.HC_LIB_PATH)


# 5. sequences kept by name
@pytest.mark.parametrize("i", range(len(S.REPLAYS)))
def test_replays(i):
    run_sequence(S.REPLAYS[i])
