"""A plain Python model of what one engine holds after any sequence of calls
over its device-resident result: the table, its order, its tokens, the flags
of mox_engine::Res (sorted, ranked, folded), the buffers it lives in and the
accumulator (include/mox.h; DESIGN.md §4, "The state of the result").  Each
operator is the model its own test file already uses (filter_cases.expected,
join_cases.expected, rank_cases.expected, rekey_cases.expected, ...); this
class composes them and carries the state between them.  No expectation comes
from the library: nothing here imports it.

A mutator changes the state or raises ModelError(code) and leaves it alone.
A reader returns the expected answer; with MOX_F_SORT_BYTES (sort_flag) the
fetch, the pages, the text and the search first sort a result that is neither
sorted nor ranked, which is a state change.

Order.  The engine's order after a run, a re-key that changed a word or a merge
is unspecified.  While order_known is false the items are in an arbitrary
order; a driver compares the first fetch as a multiset and hands its order in
with adopt_order(), and from then on everything is exact.
"""
import filter_cases
import find_cases
import hist_cases
import join_cases
import lookup_cases
import rank_cases
import rekey_cases
import text_cases
import top_cases

U64 = (1 << 64) - 1
OK, EINVAL, ENOMEM, ESTATE = 0, -1, -3, -7  # MOX_OK, MOX_EINVAL, MOX_ENOMEM, MOX_ESTATE
CODE_NAMES = {OK: "OK", EINVAL: "EINVAL", ENOMEM: "ENOMEM", ESTATE: "ESTATE"}

# where the result lives: the pass's t_* buffers, the sort's s_*, a filter set,
# a rank set, the total's a_tab (after a failed fold)
PASS, SORT, F0, F1, R0, R1, TOTAL = HOMES = ("PASS", "SORT", "F0", "F1", "R0", "R1", "TOTAL")
REKEY_INFO_KEYS = rekey_cases.INFO_KEYS
ACCUM_INFO_KEYS = ("passes", "words", "tokens")


class ModelError(Exception):
    """The modelled call returns this error code; the state is what it was."""

    def __init__(self, code):
        super().__init__(CODE_NAMES.get(code, str(code)))
        self.code = code


class ResultModel:
    def __init__(self, sort_flag=False):
        self.sort_flag = sort_flag
        self.have_result = False
        self.items = []           # [(word, count)] in table order (arbitrary while order_known is false)
        self.order_known = True
        self.tokens = 0           # carried beside the counts, as the engine does
        self.sorted = self.ranked = self.folded = False
        self.home = PASS
        # the accumulator; acc_items in the total's own row order
        self.acc_have = False
        self.acc_items = []
        self.acc_order_known = True
        self.acc_tokens = 0
        self.acc_passes = 0
        self.acc_sorted = self.acc_ranked = False
        # the result and the total are the same rows in the same (still unknown) order:
        # after a merge, and while the result lives in the total's buffers
        self._acc_alias = False

    # ---- helpers
    @property
    def n(self):
        return len(self.items) if self.have_result else 0

    def state_line(self):
        return ("result=%s n=%d tokens=%d sorted=%d ranked=%d folded=%d home=%s order_known=%d | total=%s n=%d tokens=%d passes=%d "
                "sorted=%d ranked=%d | sort_flag=%d" % (
                    "yes" if self.have_result else "no", self.n, self.tokens, self.sorted, self.ranked, self.folded, self.home,
                    self.order_known, "yes" if self.acc_have else "no", len(self.acc_items), self.acc_tokens, self.acc_passes,
                    self.acc_sorted, self.acc_ranked, self.sort_flag))

    def flags(self):
        return (self.sorted, self.ranked, self.folded)

    def _need_result(self):
        if not self.have_result:
            raise ModelError(ESTATE)

    def _moved(self):
        self._acc_alias = False

    def adopt_order(self, fetched_items):
        """The engine's order of an unspecified-order table, as a fetch showed it."""
        fetched_items = list(fetched_items)
        if sorted(fetched_items) != sorted(self.items):
            raise ValueError("adopt_order: not a permutation of the model's rows")
        self.items = fetched_items
        self.order_known = True
        if self._acc_alias and not self.acc_order_known:
            self.acc_items = list(fetched_items)
            self.acc_order_known = True

    # ---- mutators
    def run(self, words, counts):
        """mox_reduce_pairs: a new table in the engine's order."""
        d = {}
        for w, c in zip(words, counts):
            d[w] = (d.get(w, 0) + c) & U64
        self.items = list(d.items())
        self.tokens = sum(counts) & U64
        self.order_known = len(self.items) <= 1
        self.have_result = True
        self.sorted = self.ranked = self.folded = False
        self.home = PASS
        self._moved()

    def _sort_rows(self):
        """bsort_table: a table of at most one row is left as it is, flags included."""
        if len(self.items) < 2:
            return
        self.items = sorted(self.items)
        self.order_known = True
        self.sorted = True
        self.ranked = False
        self.home = SORT
        self._moved()

    def sort(self):
        self._need_result()
        if not self.sorted:
            self._sort_rows()
        self.ranked = False

    def rank(self, ascending=False, fail=False):
        self._need_result()
        info = dict(rank_cases.info_of(self.items), tokens=self.tokens)
        if fail:
            raise ModelError(ENOMEM)
        if len(self.items) > 1:
            self.items = rank_cases.expected(self.items, ascending)
            self.sorted = False
            self.home = R1 if self.home == R0 else R0
            self._moved()
        self.ranked = True
        return info

    def _other_filter_set(self):
        return F1 if self.home == F0 else F0

    def filter(self, count_only=False, fail=False, **spec):
        self._need_result()
        kept, info = filter_cases.expected(self.items, **spec)
        info["tokens_in"] = self.tokens
        if count_only:
            return info
        if fail:
            raise ModelError(ENOMEM)
        self.items = kept
        self.tokens = info["tokens_kept"]
        self.home = self._other_filter_set()
        self._moved()
        return info

    def join(self, mode="semi", counts="result", count_only=False, fail=False):
        if mode == "anti" and counts != "result":
            raise ModelError(EINVAL)
        self._need_result()
        total = self.acc_items if self.acc_have else []
        kept, info = join_cases.expected(self.items, total, mode, counts)
        info["tokens_in"] = self.tokens
        info["tokens_total"] = self.acc_tokens if self.acc_have else 0
        if count_only:
            return info
        if fail:
            raise ModelError(ENOMEM)
        self.items = kept
        self.tokens = info["tokens_kept"]
        if counts != "result" and len(kept) > 1:
            self.ranked = False
        self.home = self._other_filter_set()
        self._moved()
        return info

    def rekey(self, trim=b"", punct=False, max_chars=0, fail=False):
        self._need_result()
        table, _, info = rekey_cases.expected(self.items, trim=trim, punct=punct, max_chars=max_chars, tokens=self.tokens)
        if not info["words_changed"]:
            return info  # no window differs: table, order, flags and home stay (the hook is not reached)
        if fail:
            raise ModelError(ENOMEM)
        self.items = table
        self.order_known = len(table) <= 1
        self.tokens = info["tokens_out"]
        self.sorted = self.ranked = False  # folded stays
        self.home = PASS
        self._moved()
        return info

    def accumulate(self, fail=False):
        if not self.have_result or self.folded:
            raise ModelError(ESTATE)
        if not self.acc_have:
            # the first fold has no hook point: the result is saved as it is
            self.acc_have = True
            self.acc_items = list(self.items)
            self.acc_order_known = self.order_known
            self._acc_alias = not self.order_known
            self.acc_tokens = self.tokens
            self.acc_sorted, self.acc_ranked = self.sorted, self.ranked
            self.acc_passes = 1
            self.folded = True
            return
        if fail:
            # the total is what it was and becomes the result
            self.items = list(self.acc_items)
            self.order_known = self.acc_order_known or len(self.items) <= 1
            self.tokens = self.acc_tokens
            self.sorted, self.ranked = self.acc_sorted, self.acc_ranked
            self.folded = True
            self.home = TOTAL
            self._acc_alias = True
            raise ModelError(ENOMEM)
        d = dict(self.acc_items)
        for w, c in self.items:
            d[w] = (d.get(w, 0) + c) & U64
        self.items = list(d.items())
        self.order_known = len(self.items) <= 1
        self.tokens = (self.acc_tokens + self.tokens) & U64
        self.sorted = self.ranked = False
        self.folded = True
        self.home = PASS
        self.acc_items = list(self.items)
        self.acc_order_known = self.order_known
        self._acc_alias = True
        self.acc_tokens = self.tokens
        self.acc_sorted = self.acc_ranked = False
        self.acc_passes += 1

    def accumulate_reset(self):
        if self.have_result and self.home == TOTAL:
            self.have_result = False
            self.items = []
            self.order_known = True
        self.acc_have = False
        self.acc_items = []
        self.acc_order_known = True
        self.acc_tokens = self.acc_passes = 0
        self.acc_sorted = self.acc_ranked = False
        self.folded = False
        self._acc_alias = False

    # ---- readers
    def _implicit_sort(self):
        """sort_for_fetch / tx_prepare: MOX_F_SORT_BYTES, neither sorted nor ranked."""
        if self.sort_flag and not self.sorted and not self.ranked:
            self._sort_rows()

    def fetch(self):
        self._need_result()
        self._implicit_sort()
        return list(self.items), self.tokens

    def fetch_rows(self, first, n):
        self._need_result()
        self._implicit_sort()
        return self.items[first:first + n], self.tokens

    def result_text(self):
        self._need_result()
        self._implicit_sort()
        return text_cases.expected(self.items)

    def find(self, keys, mode):
        """(first, last, sums); mode: find_cases.EXACT / PREFIX / LOWER.  At least one key."""
        assert keys
        self._need_result()
        self._implicit_sort()
        if not self.sorted and len(self.items) > 1:
            raise ModelError(ESTATE)
        return find_cases.expected(self.items, keys, mode)

    def lookup(self, queries):
        self._need_result()
        return lookup_cases.expected(self.items, queries)

    def top_words(self, k):
        self._need_result()
        return top_cases.expected(self.items, k), self.tokens

    def top_rows(self, first, n, k):
        self._need_result()
        lo = min(first, len(self.items))
        return find_cases.top_of(self.items, lo, min(len(self.items), lo + n), k), self.tokens

    def complete(self, prefix, k):
        first, last, _ = self.find([prefix], find_cases.PREFIX)
        return self.top_rows(first[0], last[0] - first[0], k)

    def histogram(self, key):
        self._need_result()
        return hist_cases.expected(self.items, key), len(self.items), sum(c for _, c in self.items) & U64

    def accumulate_info(self):
        return {"passes": self.acc_passes, "words": len(self.acc_items), "tokens": self.acc_tokens}
