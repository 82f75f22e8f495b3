"""CPU: the state model of the device-resident result (result_model.py) and the
committed sequence sets (sequence_cases.py) check themselves.  The hand-written
sequences pin the model's rules with literal tables and flags; the coverage
assertions run the sets on the model alone.  Nothing here touches a GPU."""
import pytest

import find_cases
import sequence_cases as S
from result_model import EINVAL, ENOMEM, ESTATE, F0, F1, PASS, R0, R1, SORT, TOTAL, U64, ModelError, ResultModel

WORDS = [b"pear", b"fig,", b"apple", b"fig", b"kiwi"]
COUNTS = [3, 5, 3, 2, 0]
ROWS = list(zip(WORDS, COUNTS))


def fresh(words=WORDS, counts=COUNTS, sort_flag=False):
    """A model after a run whose engine order is the order given."""
    m = ResultModel(sort_flag)
    m.run(words, counts)
    if not m.order_known:
        m.adopt_order(list(zip(words, counts)))
    return m


def state(m):
    return (m.items, m.tokens, m.sorted, m.ranked, m.folded, m.home)


def code_of(fn, *a, **kw):
    with pytest.raises(ModelError) as ex:
        fn(*a, **kw)
    return ex.value.code


# ---- hand-written sequences: one rule of the state table each
def test_run_gives_a_new_table_in_unknown_order():
    m = ResultModel()
    assert code_of(m.fetch) == ESTATE and code_of(m.sort) == ESTATE and code_of(m.accumulate) == ESTATE
    m.run(WORDS, COUNTS)
    assert sorted(m.items) == sorted(ROWS) and not m.order_known
    assert (m.tokens, m.sorted, m.ranked, m.folded, m.home) == (13, False, False, False, PASS)
    with pytest.raises(ValueError):
        m.adopt_order(ROWS[:-1] + [(b"kiwi", 1)])
    m.adopt_order(ROWS[::-1])
    assert m.items == ROWS[::-1] and m.order_known
    m.sort()
    m.rank()
    m.accumulate()
    m.run([b"x", b"x"], [U64, 2])  # equal words are summed, mod 2^64; tokens too
    assert state(m) == ([(b"x", 1)], 1, False, False, False, PASS) and m.order_known


def test_sort_orders_bytewise_and_clears_ranked():
    m = fresh()
    m.rank()
    m.sort()
    assert state(m) == ([(b"apple", 3), (b"fig", 2), (b"fig,", 5), (b"kiwi", 0), (b"pear", 3)], 13, True, False, False, SORT)
    m.filter(keep=[b"fig"])
    m.rank()
    assert (m.sorted, m.ranked, m.home) == (True, True, F0)
    m.sort()  # already sorted: only ranked clears, nothing moves
    assert state(m) == ([(b"fig", 2)], 2, True, False, False, F0)


def test_sort_and_rank_leave_a_table_of_at_most_one_row_where_it_is():
    for words, counts in (([], []), ([b"only"], [7])):
        m = fresh(words, counts)
        m.sort()  # nothing to order: no flag is needed for the search to take the table
        assert state(m) == (list(zip(words, counts)), sum(counts), False, False, False, PASS)
        assert m.find([b"o"], find_cases.PREFIX) == ([0], [len(words)], [sum(counts)])
        info = m.rank()
        assert state(m) == (list(zip(words, counts)), sum(counts), False, True, False, PASS)
        assert info == {"words": len(words), "tokens": sum(counts), "max_count": sum(counts), "digit_passes": 0}
        m.sort()
        assert not m.ranked and m.home == PASS
    m = fresh()
    m.sort()
    m.filter(keep=[b"kiwi"])
    m.rank()  # one row: sorted stays beside ranked
    assert state(m) == ([(b"kiwi", 0)], 0, True, True, False, F0)


def test_rank_is_stable_and_alternates_its_two_sets():
    m = fresh()
    info = m.rank()
    assert state(m) == ([(b"fig,", 5), (b"pear", 3), (b"apple", 3), (b"fig", 2), (b"kiwi", 0)], 13, False, True, False, R0)
    assert info == {"words": 5, "tokens": 13, "max_count": 5, "digit_passes": 1}
    m.rank(ascending=True)
    assert state(m) == ([(b"kiwi", 0), (b"fig", 2), (b"pear", 3), (b"apple", 3), (b"fig,", 5)], 13, False, True, False, R1)
    m.rank()
    assert m.home == R0
    m.sort()
    m.rank()
    assert (m.sorted, m.ranked, m.home) == (False, True, R0)
    assert m.items == [(b"fig,", 5), (b"apple", 3), (b"pear", 3), (b"fig", 2), (b"kiwi", 0)]


def test_filter_keeps_order_and_flags_and_alternates_its_two_sets():
    m = fresh()
    m.rank()
    info = m.filter(min_count=2)
    assert state(m) == ([(b"fig,", 5), (b"pear", 3), (b"apple", 3), (b"fig", 2)], 13, False, True, False, F0)
    assert info == {"words_in": 5, "words_kept": 4, "tokens_in": 13, "tokens_kept": 13, "bytes_kept": 16, "list_found": 0}
    before = state(m)
    info = m.filter(max_len=4, count_only=True)
    assert state(m) == before and info["words_kept"] == 3
    m.filter(max_len=4)
    assert state(m) == ([(b"fig,", 5), (b"pear", 3), (b"fig", 2)], 10, False, True, False, F1)
    m.filter(prefix=b"fig")
    assert state(m) == ([(b"fig,", 5), (b"fig", 2)], 7, False, True, False, F0)
    info = m.filter(drop=[b"fig", b"plum"])
    assert state(m) == ([(b"fig,", 5)], 5, False, True, False, F1) and info["list_found"] == 1
    m.filter(keep=[])
    assert state(m) == ([], 0, False, True, False, F0)


def test_join_substitutes_counts_and_clears_ranked_only_for_two_rows_or_more():
    m = fresh()
    info = m.join("semi", "result", count_only=True)  # no total: the empty table
    assert (info["words_total"], info["words_matched"], info["words_kept"]) == (0, 0, 0) and m.items == ROWS
    assert code_of(m.join, "anti", "min") == EINVAL and code_of(m.join, "anti", "total") == EINVAL
    assert code_of(ResultModel().join, "anti", "min") == EINVAL and code_of(ResultModel().join) == ESTATE
    m.accumulate()
    m.run([b"fig", b"apple", b"plum", b"pear"], [9, 1, 4, 3])
    m.adopt_order([(b"plum", 4), (b"pear", 3), (b"fig", 9), (b"apple", 1)])
    m.rank()
    ranked = [(b"fig", 9), (b"plum", 4), (b"pear", 3), (b"apple", 1)]
    assert m.items == ranked
    info = m.join("anti", "result")
    assert state(m) == ([(b"plum", 4)], 4, False, True, False, F0)
    assert (info["words_matched"], info["tokens_matched_result"], info["tokens_matched_total"], info["tokens_min"]) == (3, 13, 8, 6)
    m.run([b"fig", b"apple", b"plum", b"pear"], [9, 1, 4, 3])
    m.adopt_order(ranked)
    m.rank()
    m.join("semi", "result")  # own counts: still in count order
    assert state(m) == ([(b"fig", 9), (b"pear", 3), (b"apple", 1)], 13, False, True, False, F0)
    m.join("semi", "min")  # substituted counts, three rows: in no count order
    assert state(m) == ([(b"fig", 2), (b"pear", 3), (b"apple", 1)], 6, False, False, False, F1)
    m.rank()
    m.filter(keep=[b"pear"])
    m.join("semi", "total")  # one row kept: ranked stays
    assert state(m) == ([(b"pear", 3)], 3, False, True, False, F1)


def test_rekey_merges_rows_and_a_rekey_that_changes_nothing_leaves_everything():
    m = fresh()
    m.rank()
    m.accumulate()
    before = state(m)
    info = m.rekey(trim=b"#")
    assert state(m) == before and m.order_known and (info["words_changed"], info["words_out"], info["tokens_out"]) == (0, 5, 13)
    assert m.rekey(trim=b"#", fail=True) == info  # the hook lies behind the early return
    info = m.rekey(punct=True)
    assert sorted(m.items) == [(b"apple", 3), (b"fig", 7), (b"kiwi", 0), (b"pear", 3)] and not m.order_known
    assert (m.tokens, m.sorted, m.ranked, m.folded, m.home) == (13, False, False, True, PASS)  # a folded total stays folded
    assert (info["words_in"], info["words_out"], info["words_changed"], info["words_dropped"], info["bytes_out"]) == (5, 4, 1, 0, 16)
    m = fresh([b"ab", b"ac", b"b", b"..."], [1, 2, 4, 8])
    info = m.rekey(punct=True, max_chars=1)
    assert sorted(m.items) == [(b"a", 3), (b"b", 4)] and m.tokens == 7
    assert (info["words_changed"], info["words_dropped"], info["tokens_dropped"], info["tokens_out"]) == (3, 1, 8, 7)


def test_accumulate_first_fold_copies_and_later_folds_merge():
    m = fresh()
    m.sort()
    sorted_rows = sorted(ROWS)
    m.accumulate()  # the first fold: the result is untouched except folded; the total inherits the order flags
    assert state(m) == (sorted_rows, 13, True, False, True, SORT)
    assert (m.acc_items, m.acc_tokens, m.acc_passes, m.acc_sorted, m.acc_ranked) == (sorted_rows, 13, 1, True, False)
    assert m.accumulate_info() == {"passes": 1, "words": 5, "tokens": 13}
    before = state(m)
    assert code_of(m.accumulate) == ESTATE and state(m) == before
    m.run([b"fig", b"plum", b"kiwi"], [U64, 1, 0])
    m.adopt_order([(b"plum", 1), (b"kiwi", 0), (b"fig", U64)])
    m.rank()
    m.accumulate()  # a merge: counts and tokens mod 2^64, the result becomes the total in the engine's order
    want = [(b"apple", 3), (b"fig", 1), (b"fig,", 5), (b"kiwi", 0), (b"pear", 3), (b"plum", 1)]
    assert sorted(m.items) == want and not m.order_known
    assert (m.tokens, m.sorted, m.ranked, m.folded, m.home) == (13, False, False, True, PASS)
    assert (m.acc_sorted, m.acc_ranked, m.acc_passes) == (False, False, 2)
    m.adopt_order(want[::-1])  # the total lies in the same order
    assert m.acc_items == want[::-1] and m.acc_order_known
    assert m.accumulate_info() == {"passes": 2, "words": 6, "tokens": 13}


def test_reset_empties_the_total_and_takes_a_result_that_lives_in_it():
    m = fresh()
    m.accumulate()
    m.accumulate_reset()
    assert state(m) == (ROWS, 13, False, False, False, PASS) and not m.acc_have
    assert m.accumulate_info() == {"passes": 0, "words": 0, "tokens": 0}
    m.accumulate()  # folds again, into the empty total
    assert m.acc_passes == 1 and m.folded
    m.run([b"plum"], [1])
    assert code_of(m.accumulate, fail=True) == ENOMEM
    assert m.home == TOTAL
    m.accumulate_reset()
    assert not m.have_result and m.n == 0
    for call in (m.fetch, m.sort, m.rank, m.filter, m.join, m.rekey, m.accumulate, m.result_text, lambda: m.lookup([b"a"]),
                 lambda: m.top_words(3), lambda: m.histogram("count"), lambda: m.find([b"a"], find_cases.EXACT)):
        assert code_of(call) == ESTATE


def test_injected_failures_change_nothing():
    m = fresh()
    m.sort()
    m.accumulate()
    before = state(m)
    assert code_of(m.rank, fail=True) == ENOMEM and state(m) == before
    assert code_of(m.filter, min_count=3, fail=True) == ENOMEM and state(m) == before
    assert code_of(m.join, "semi", "min", fail=True) == ENOMEM and state(m) == before
    assert code_of(m.rekey, punct=True, fail=True) == ENOMEM and state(m) == before
    assert m.filter(min_count=3, count_only=True, fail=True)["words_kept"] == 3 and state(m) == before  # count_only returns before the hook
    one = fresh([b"a"], [1])
    assert code_of(one.rank, fail=True) == ENOMEM and not one.ranked


def test_a_failed_fold_makes_the_total_the_result_with_the_totals_flags():
    m = fresh()
    m.accumulate(fail=True)  # the first fold has no hook point: it succeeds
    assert m.folded and m.acc_passes == 1 and m.home == PASS
    m.accumulate_reset()
    m.rank()
    ranked = list(m.items)
    m.accumulate()
    m.run([b"plum", b"fig"], [1, 1])
    m.adopt_order([(b"plum", 1), (b"fig", 1)])
    m.sort()
    assert code_of(m.accumulate, fail=True) == ENOMEM
    assert state(m) == (ranked, 13, False, True, True, TOTAL)  # the run's contribution is lost
    assert (m.acc_items, m.acc_tokens, m.acc_passes) == (ranked, 13, 1)
    assert code_of(m.accumulate) == ESTATE
    m.filter(min_count=3)  # the result leaves the total's buffers: a reset no longer takes it
    m.accumulate_reset()
    assert state(m) == ([(b"fig,", 5), (b"pear", 3), (b"apple", 3)], 11, False, True, False, F0)


def test_the_sort_flag_sorts_for_fetch_pages_text_and_find_but_a_ranking_survives():
    for read in (lambda m: m.fetch(), lambda m: m.fetch_rows(1, 2), lambda m: m.result_text(), lambda m: m.find([b"fig"], find_cases.PREFIX)):
        m = fresh(sort_flag=True)
        for other in (lambda: m.lookup([b"fig"]), lambda: m.top_words(2), lambda: m.histogram("first"), lambda: m.top_rows(0, 5, 2),
                      m.accumulate_info):
            other()
            assert state(m) == (ROWS, 13, False, False, False, PASS)  # these readers do not sort
        read(m)
        assert state(m) == (sorted(ROWS), 13, True, False, False, SORT)
        m.rank()
        ranked = state(m)
        try:
            read(m)
        except ModelError as ex:  # the search does not take a ranked table, and does not sort it either
            assert ex.code == ESTATE
        assert state(m) == ranked and m.home == R0
    m = fresh(sort_flag=True)
    m.rank()
    assert code_of(m.find, [b"fig"], find_cases.PREFIX) == ESTATE  # ranked: not sorted behind the caller's back
    assert m.fetch() == ([(b"fig,", 5), (b"pear", 3), (b"apple", 3), (b"fig", 2), (b"kiwi", 0)], 13)
    one = fresh([b"a"], [1], sort_flag=True)
    one.fetch()
    assert state(one) == ([(b"a", 1)], 1, False, False, False, PASS)  # one row: the implicit sort moves nothing either
    plain = fresh()
    plain.fetch()
    assert state(plain) == (ROWS, 13, False, False, False, PASS)


def test_readers_see_the_table_in_its_order():
    m = fresh()
    assert code_of(m.find, [b"fig"], find_cases.EXACT) == ESTATE
    assert m.fetch_rows(3, 5) == ([(b"fig", 2), (b"kiwi", 0)], 13) and m.fetch_rows(9, 2) == ([], 13)
    assert m.lookup([b"fig", b"fi", b"kiwi"]) == ([2, 0, 0], [3, U64, 4])
    assert m.top_words(2) == ([(b"fig,", 5), (b"pear", 3)], 13)  # the tie breaks by table order
    assert m.top_rows(2, 9, 1) == ([(b"apple", 3)], 13)
    assert m.result_text() == b"pear 3\nfig, 5\napple 3\nfig 2\nkiwi 0\n"
    assert m.histogram("count") == ([(0, 1, 0, 4), (2, 1, 2, 3), (3, 2, 6, 0), (5, 1, 5, 1)], 5, 13)
    m.sort()
    assert m.histogram("count")[0][2] == (3, 2, 6, 0)  # the lowest row of a bin follows the order: "apple" now
    assert m.find([b"fig", b"g"], find_cases.PREFIX) == ([1, 3], [3, 3], [7, 0])
    assert m.find([b"fig"], find_cases.EXACT) == ([1], [2], [2])
    assert m.complete(b"fig", 1) == ([(b"fig,", 5)], 13)


# ---- the tables
@pytest.mark.parametrize("n", S.SIZES)
def test_tables_have_the_shapes_they_claim(n):
    (a, ca), (b, cb) = S.table(n, "A"), S.table(n, "B")
    assert len(a) == len(b) == len(set(a)) == len(set(b)) == n
    if n:
        assert S.LONG in map(len, a) and S.LONG in map(len, b) and max(ca) >= 1 << 32 and max(cb) >= 1 << 32
    if n >= 1025:
        assert S.MID in map(len, a) and 0 in ca and len(set(ca)) < n // 4  # zeros and ties
        assert 0.6 * n <= len(set(a) & set(b)) <= 0.7 * n
        assert all(a[i] == a[i - 1] + b"," for i in range(9, n, 10))
        shared63 = [w for w, c in zip(a, ca) if c == 1 << 63]
        assert len(shared63) == 1 and dict(zip(b, cb))[shared63[0]] == 1 << 63  # A + B wraps on this word


# ---- the generators
def test_generators_are_deterministic_and_sequences_decode():
    assert S.walk_set() == S.walk_set() and len(set(S.walk_set())) == len(S.WALK_SEEDS)
    assert S.walk(7) == S.walk(7) != S.walk(8)
    for seq in S.pair_set() + S.pair_set(2, True) + S.home_set() + S.walk_set() + list(S.PINGPONG) + list(S.REPLAYS):
        n, flag, steps = S.decode(seq)
        assert S.encode(n, flag, steps) == seq
        assert all(S.kind_of(t) in S.KINDS for t in steps)
    n, flag, steps = S.decode(S.walk(S.WALK_SEEDS[0]))
    assert (n, flag, steps[0], len(steps)) == (S.WALK_N, False, "run:A", 1 + S.WALK_STEPS)
    assert S.decode("n=1025/sort run:A sort") == (1025, True, ["run:A", "sort"])
    assert sorted(S.kind_of(t) for t in S.ALPHABET if t in ("!rank+", "filter:min50?", "run:B", "acc")) == ["!rank", "acc", "filter", "run"]
    with pytest.raises(AssertionError):
        S.decode("n=3 run:C")


# ---- coverage of the committed sets, by the model alone
@pytest.fixture(scope="module")
def measured():
    return S.trace_all(S.measured_sets())


@pytest.fixture(scope="module")
def reach():
    return S.reachable(depth=4)


def test_every_ordered_pair_of_kinds_is_adjacent(measured):
    every = {(a, b) for a in S.KINDS for b in S.KINDS}
    assert not every - measured.pairs
    for sets in (S.pair_set(sort_flag=True),) + tuple(S.pair_set(n) for n in S.SMALL_NS):
        assert not every - S.trace_all(sets).pairs


def test_every_reader_follows_every_kind(measured):
    assert measured.readers_after == {(k, r) for k in S.KINDS for r in S.READERS}


def test_every_reachable_flag_combination_is_entered(measured, reach):
    flags = reach[0]
    assert (True, True, False) in flags and (True, True, True) in flags  # one row: sorted and ranked at once
    assert not flags - measured.flags


def test_every_home_and_kind_the_model_reaches_in_four_steps_is_reached(measured, reach):
    want = reach[1]
    assert {h for h, _ in want} == set(S.HOMES)
    assert not want - measured.home_kind


def test_both_buffer_pairs_go_small_large_small(measured):
    assert measured.pingpong == {"F": True, "R": True}


def test_conditions_on_the_sets(measured):
    assert measured.errors * 4 <= measured.steps              # at most a quarter of all steps expect an error code
    assert measured.rows2 * 4 >= 3 * measured.steps           # three quarters act on two rows or more
    assert measured.rows1025 * 3 >= measured.steps            # a third act on more than 1024 rows
    walks = S.trace_all(S.walk_set())                         # and the walks meet them on their own
    assert walks.errors * 4 <= walks.steps and walks.rows2 * 4 >= 3 * walks.steps and walks.rows1025 * 3 >= walks.steps


def test_the_walks_of_the_other_builds_hold_every_kind():
    walks = S.other_build_walks(4)
    assert len(walks) == 4 and set(walks) <= set(S.walk_set())
    assert {S.kind_of(t) for w in walks for t in S.decode(w)[2]} == set(S.KINDS)


def test_replays_run_on_the_model():
    t = S.trace_all(S.REPLAYS)
    assert t.steps == sum(len(S.decode(s)[2]) for s in S.REPLAYS)
    assert (True, True, True) in t.flags and (TOTAL, "reset") in t.home_kind
