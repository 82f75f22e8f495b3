"""Sequences of calls over the device-resident result, for result_model.py's
state model: the word tables, the step alphabet and its string form, the
generated sets (the pair sweep, the seeded walks, the ping-pong sequences, the
replays) and the coverage they are measured by.  Shared by test_result_model.py
(CPU: the model and the sets check themselves) and test_gpu_result_sequences.py
(GPU: an engine and the model in lockstep).

A sequence is a string: "n=1025 run:A sort rank- filter:min5 acc join:semi/min".
n is the rows of a run's table ("n=1025/sort": the engine has MOX_F_SORT_BYTES);
every other token is one mutating call.  "!" in front injects the call's
failure (MOX_TEST_FAIL_*), "?" behind is count_only.  After every step a driver
runs every reader.
"""
import functools
import random
from collections import deque

import find_cases
from result_model import F0, F1, HOMES, OK, PASS, R0, R1, SORT, TOTAL, ModelError, ResultModel  # noqa: F401 (HOMES, ModelError: for the tests)

LONG = 300        # one word of this many bytes ...
MID = 70          # ... and one of more than 64 (the lane / wave edge of lookup and histogram)
PAIR_N = 1025     # the pair sweep: one row past the 1024-row tile of filter, re-key, find and text
WALK_N = 4097     # the walks: one row past the 4096-row tile of the sort, the ranking and top-k
SMALL_NS = (0, 1, 2)
SIZES = SMALL_NS + (PAIR_N, WALK_N)
WALK_STEPS = 8


# ---- tables
@functools.lru_cache(maxsize=None)
def _table(n, which):
    words, counts = _build_table(n, which)
    return tuple(words), tuple(counts)


def table(n, which):
    """(words, counts) of a word list as fresh lists (_build_table has the rules)."""
    words, counts = _table(n, which)
    return list(words), list(counts)


def _build_table(n, which):
    """(words, counts) of word list "A" or "B" at n rows.  Words are distinct; word
    n // 2 is LONG bytes and word n // 3 MID bytes long (n >= 3); every tenth word
    is its predecessor plus ","; counts have ties, zeros, one value >= 2^32 and
    (n >= 30) one of 2^63, on a word both lists hold, so that sums wrap.  B
    shares the rows i % 3 != 1 of A, with other counts."""
    assert which in ("A", "B")
    words = [(b"b%d" if which == "B" and i % 3 == 1 else b"w%d") % i + b"q" * (i % 23) for i in range(n)]
    if n >= 3:
        words[n // 3] = b"V" * MID
    if n:
        words[n // 2] = b"W" * LONG
    for i in range(9, n, 10):
        words[i] = words[i - 1] + b","
    counts = [((i * 37) % 101) if which == "A" else ((i * 53) % 97) for i in range(n)]
    if n:
        counts[n // 4] = (1 << 32) + (5 if which == "A" else 9)
    if n >= 30:
        counts[(n // 5) // 30 * 30] = 1 << 63
    assert len(set(words)) == n
    return words, counts


# ---- the step alphabet
FILTERS = {
    "min5": dict(min_count=5),               # a count bound that keeps most rows
    "min50": dict(min_count=50),             # ... about half
    "max3": dict(max_count=3),               # ... a few
    "len4-9": dict(min_len=4, max_len=9),    # a length bound
    "pre:w1": dict(prefix=b"w1"),            # a prefix: about a tenth
    "drop3": "drop",                         # a drop list: every third word of A, and a word no table holds
    "keep4": "keep",                         # a keep list: three of every four words of A
    "one": "one",                            # a keep list of one word: at most one row stays
    "none": "none",                          # the empty keep list: nothing stays
}
JOINS = ("semi/result", "semi/total", "semi/min", "anti/result", "anti/min")  # the last one is MOX_EINVAL
REKEYS = {
    "punct": dict(punct=True),               # the trailing commas go, rows merge
    "hash": dict(trim=b"#"),                 # a trim set that matches no word: nothing changes
    "max3": dict(max_chars=3),               # a cap that merges most rows
    "max40": dict(max_chars=40),             # a cap only the two long words feel
}
KINDS = ("run", "sort", "rank", "filter", "join", "rekey", "acc", "reset", "!filter", "!join", "!rank", "!rekey", "!acc")
READERS = ("fetch", "fetch_rows", "lookup", "find_prefix", "find_exact", "top_words", "result_text", "hist_count", "hist_first",
           "top_rows", "complete", "accumulate_info")


def kind_of(tok):
    bang = tok.startswith("!")
    name = tok.lstrip("!").rstrip("?").split(":")[0]
    name = "rank" if name in ("rank-", "rank+") else name
    return ("!" if bang else "") + name


def tokens_of(kind):
    """Every token of a kind."""
    bang, name = ("!", kind[1:]) if kind.startswith("!") else ("", kind)
    if name == "run":
        return ["run:A", "run:B"]
    if name == "rank":
        return [bang + "rank-", bang + "rank+"]
    if name == "filter":
        out = [bang + "filter:" + v for v in FILTERS]
        return out + ([] if bang else ["filter:min50?"])
    if name == "join":
        out = [bang + "join:" + v for v in JOINS]
        return out + ([] if bang else ["join:semi/min?"])
    if name == "rekey":
        return [bang + "rekey:" + v for v in REKEYS]
    return [bang + name]


ALPHABET = [t for k in KINDS for t in tokens_of(k)]


def decode(seq):
    """"n=1025/sort run:A sort" -> (1025, True, ["run:A", "sort"])."""
    head, *steps = seq.split()
    assert head.startswith("n="), seq
    n, _, flag = head[2:].partition("/")
    assert flag in ("", "sort"), seq
    for t in steps:
        assert t in ALPHABET, t
    return int(n), flag == "sort", steps


def encode(n, sort_flag, steps):
    return " ".join(["n=%d%s" % (n, "/sort" if sort_flag else "")] + list(steps))


def filter_spec(name, n):
    """The keyword arguments of Engine.filter_result / ResultModel.filter for a filter name at table size n."""
    spec = FILTERS[name]
    if isinstance(spec, dict):
        return dict(spec)
    words = table(n, "A")[0]
    if spec == "drop":
        return dict(drop=words[::3] + [b"nowhere"])
    if spec == "keep":
        return dict(keep=[w for i, w in enumerate(words) if i % 4])
    if spec == "one":
        return dict(keep=words[:1] + [b"nowhere"])
    return dict(keep=[])


def call_of(tok, n):
    """(method, kwargs, fail): the call a token stands for, by the names ResultModel
    and the GPU driver share.  fail: the failure hook is set around it."""
    fail = tok.startswith("!")
    body = tok.lstrip("!")
    count_only = body.endswith("?")
    name, _, arg = body.rstrip("?").partition(":")
    if name == "run":
        words, counts = table(n, arg)
        return "run", dict(words=words, counts=counts), fail
    if name in ("rank-", "rank+"):
        return "rank", dict(ascending=name == "rank+"), fail
    if name == "filter":
        return "filter", dict(filter_spec(arg, n), count_only=count_only), fail
    if name == "join":
        mode, counts = arg.split("/")
        return "join", dict(mode=mode, counts=counts, count_only=count_only), fail
    if name == "rekey":
        return "rekey", dict(REKEYS[arg]), fail
    return {"sort": "sort", "acc": "accumulate", "reset": "accumulate_reset"}[name], {}, fail


FAIL_ENV = {"filter": "MOX_TEST_FAIL_FILTER", "join": "MOX_TEST_FAIL_JOIN", "rank": "MOX_TEST_FAIL_RANK", "rekey": "MOX_TEST_FAIL_REKEY",
            "accumulate": "MOX_TEST_FAIL_ACCUM"}


def model_step(m, tok, n):
    """One step on the model: (error code or OK, info or None)."""
    method, kw, fail = call_of(tok, n)
    if fail:
        kw["fail"] = True
    try:
        return OK, getattr(m, method)(**kw)
    except ModelError as ex:
        return ex.code, None


# ---- the reader sweep
def queries(n):
    """Lookup words: present ones, absent ones, the long word and a near miss of it; an odd number."""
    a, b = table(n, "A")[0], table(n, "B")[0]
    q = a[::3] + b[1::7] + [b"none%d" % i for i in range(4)] + [b"W" * LONG, b"W" * (LONG - 1), b"V" * MID, b"V" * (MID + 1)]
    return q + [b"odd"] * (1 - len(q) % 2)


def find_keys(n):
    a = table(n, "A")[0]
    return [b"", b"w", b"w1", b"w10", b"b", b"W", b"W" * LONG, b"W" * (LONG + 1), b"V" * MID, b"x", b"a", b"w8,"] + a[::97]


def pages(n):
    """(first, rows) of the pages read: across the 1024-row tile, across the table's end, past it."""
    return ((0, 3), (1020, 10), (max(0, n - 2), 5), (n + 7, 2))


def read_all(m, n):
    """Every reader's expected answer for the model's state, in sweep order:
    [(reader, tag, answer or ("error", code))].  The fetch comes first (it may
    sort under MOX_F_SORT_BYTES, and its order is what adopt_order takes)."""
    out = []

    def put(reader, tag, fn):
        try:
            out.append((reader, tag, fn()))
        except ModelError as ex:
            out.append((reader, tag, ("error", ex.code)))

    put("fetch", "", m.fetch)
    for first, rows in pages(m.n):
        put("fetch_rows", (first, rows), lambda: m.fetch_rows(first, rows))
    put("result_text", "", m.result_text)
    put("find_prefix", "", lambda: m.find(find_keys(n), find_cases.PREFIX))
    put("find_exact", "", lambda: m.find(find_keys(n), find_cases.EXACT))
    put("lookup", "", lambda: m.lookup(queries(n)))
    put("top_words", 10, lambda: m.top_words(10))
    put("hist_count", "", lambda: m.histogram("count"))
    put("hist_first", "", lambda: m.histogram("first"))
    put("top_rows", (1, 1500, 7), lambda: m.top_rows(1, 1500, 7))
    put("complete", b"w1", lambda: m.complete(b"w1", 5))
    put("accumulate_info", "", m.accumulate_info)
    return out


# ---- running a sequence on the model alone
class Trace:
    """What a set of sequences did, by the model: the coverage the tests assert."""

    def __init__(self):
        self.steps = self.errors = self.rows2 = self.rows1025 = 0
        self.pairs = set()          # (kind, kind) adjacent
        self.readers_after = set()  # (kind, reader)
        self.flags = set()          # (sorted, ranked, folded) entered with a result
        self.home_kind = set()      # (home, kind): the kind applied to a result living there
        self.pingpong = {"F": False, "R": False}
        self.kinds = set()

    def add(self, other):
        for k in ("steps", "errors", "rows2", "rows1025"):
            setattr(self, k, getattr(self, k) + getattr(other, k))
        for k in ("pairs", "readers_after", "flags", "home_kind", "kinds"):
            getattr(self, k).update(getattr(other, k))
        for k in self.pingpong:
            self.pingpong[k] = self.pingpong[k] or other.pingpong[k]
        return self


def settle(m):
    """Without an engine the unknown order is the model's own arbitrary one."""
    if m.have_result and not m.order_known:
        m.adopt_order(m.items)


class PingPong:
    """The writes into one pair of table buffer sets (h0, h1) on one engine.  A
    ping-pong is three writes in a row into h0, h1, h0 with nothing else moving
    the table in between; its size is the rows of its first write.  The pair has
    gone small-large-small when three ping-pongs, in order, have sizes a < b > c:
    both sets regrown for a larger table after a smaller one, then reused by a
    smaller one again."""

    def __init__(self, h0, h1):
        self.sets = (h0, h1)
        self.row = []     # (home, rows) of the writes in a row so far
        self.sizes = []   # the size of every ping-pong, in order

    def step(self, ok, home_before, home_after, rows_after):
        if ok and home_after in self.sets and home_after != home_before:
            self.row.append((home_after, rows_after))
            if [h for h, _ in self.row[-3:]] == [self.sets[0], self.sets[1], self.sets[0]]:
                self.sizes.append(self.row[-3][1])
        elif home_after not in self.sets:
            self.row = []

    def small_large_small(self):
        z = self.sizes
        return any(z[i] < z[j] > z[k] for i in range(len(z)) for j in range(i + 1, len(z)) for k in range(j + 1, len(z)))


def trace(seq):
    """Runs one sequence on the model alone, every reader after every step."""
    n, sort_flag, steps = decode(seq)
    m = ResultModel(sort_flag)
    t = Trace()
    prev = None
    pp = {"F": PingPong(F0, F1), "R": PingPong(R0, R1)}
    for tok in steps:
        kind = kind_of(tok)
        home, have = m.home, m.have_result
        acted = n if kind == "run" else m.n  # the rows the step acts on: a run's new table, else the result as it is
        code, _ = model_step(m, tok, n)
        t.steps += 1
        t.errors += code != OK
        t.rows2 += acted >= 2
        t.rows1025 += acted > 1024
        t.kinds.add(kind)
        if prev is not None:
            t.pairs.add((prev, kind))
        prev = kind
        if have:
            t.home_kind.add((home, kind))
        for x in pp.values():
            x.step(code == OK, home, m.home, m.n)
        for reader, _, _ in read_all(m, n):
            t.readers_after.add((kind, reader))
        settle(m)
        if m.have_result:
            t.flags.add(m.flags())
    t.pingpong = {k: x.small_large_small() for k, x in pp.items()}
    return t


def trace_all(seqs):
    t = Trace()
    for s in seqs:
        t.add(trace(s))
    return t


# ---- what the model can reach: breadth-first search
BFS_N = 40  # the search's table: large enough for every filter to leave two rows or more where it does at PAIR_N


def _key(m):
    return (m.have_result, tuple(m.items), m.tokens, m.sorted, m.ranked, m.folded, m.home, m.acc_have, tuple(m.acc_items), m.acc_tokens,
            m.acc_sorted, m.acc_ranked)


def _clone(m):
    c = ResultModel(m.sort_flag)
    c.__dict__.update(m.__dict__)
    c.items, c.acc_items = list(m.items), list(m.acc_items)
    return c


def reachable(depth=4, n=BFS_N):
    """(flags, home_kind, paths): every (sorted, ranked, folded) the model enters and
    every (home, kind) it can apply within ``depth`` steps of a fresh run, and a
    shortest token path to each (home, kind)."""
    m0 = ResultModel()
    model_step(m0, "run:A", n)
    settle(m0)
    seen = {_key(m0)}
    flags = {m0.flags()}
    paths = {}
    queue = deque([(m0, ())])
    while queue:
        m, path = queue.popleft()  # len(path) < depth: the next step is one of the first ``depth``
        for tok in ALPHABET:
            if m.have_result:
                paths.setdefault((m.home, kind_of(tok)), path + (tok,))
            c = _clone(m)
            model_step(c, tok, n)
            settle(c)
            if c.have_result:
                flags.add(c.flags())
            k = _key(c)
            if k not in seen and len(path) + 1 < depth:
                seen.add(k)
                queue.append((c, path + (tok,)))
    return flags, set(paths), paths


# ---- the committed sets
def _variant(kind, salt):
    toks = tokens_of(kind)
    return toks[salt % len(toks)]


def pair_sequence(first, n, sort_flag=False):
    """Every kind after ``first``, each pair from a fresh run: "run:A first second"
    thirteen times on one engine, so the total and the scratch buffers carry over."""
    i = KINDS.index(first)
    steps = []
    for j, second in enumerate(KINDS):
        steps += ["run:" + "AB"[j % 2], _variant(first, i + j), _variant(second, 2 * i + 3 * j + 1)]
    return encode(n, sort_flag, steps)


# How a fresh run's result gets into each of its seven homes, and into the one
# state where sorted and ranked can hold at once: a sorted table filtered to one row.
STATE_PATHS = {
    PASS: ("run:A",),
    SORT: ("run:A", "sort"),
    F0: ("run:A", "filter:min5"),
    F1: ("run:A", "filter:min5", "filter:len4-9"),
    R0: ("run:A", "rank-"),
    R1: ("run:A", "rank-", "rank+"),
    TOTAL: ("run:A", "!acc"),
    "ONE": ("run:A", "sort", "filter:one"),
}


def home_sequence(state, n, sort_flag=False):
    """Every kind applied to a result in ``state`` (a key of STATE_PATHS), each time
    reached again from a fresh run, on one engine that holds a total."""
    i = list(STATE_PATHS).index(state)
    steps = ["run:B", "acc"]
    for j, kind in enumerate(sorted(KINDS, key=lambda k: k == "reset")):  # the reset last: every other kind meets the total
        steps += list(STATE_PATHS[state]) + [_variant(kind, i + 5 * j)]
    return encode(n, sort_flag, steps)


def home_set(n=PAIR_N):
    return [home_sequence(s, n) for s in STATE_PATHS]


# the weights of a walk's alphabet: shrinking steps are rare enough for a third of all steps to see more than 1024 rows
WALK_WEIGHTS = {"run": 3, "sort": 3, "rank": 4, "filter": 4, "join": 3, "rekey": 2, "acc": 4, "reset": 1, "!filter": 1, "!join": 1, "!rank": 1,
                "!rekey": 1, "!acc": 2}
# within a kind: the mild variants more often than the ones that empty the table
TOKEN_WEIGHTS = {"filter:one": 0.3, "filter:none": 0.2, "filter:max3": 0.5, "rekey:max3": 0.5, "join:anti/min": 0.4}


def walk(seed, n=WALK_N, steps=WALK_STEPS, sort_flag=False):
    """A seeded walk: a fresh run, then ``steps`` weighted random steps."""
    rng = random.Random(seed)

    def pick(pairs):
        x = rng.random() * sum(w for _, w in pairs)
        for v, w in pairs:
            x -= w
            if x < 0:
                return v
        return pairs[-1][0]

    out = ["run:A"]
    for _ in range(steps):
        kind = pick([(k, WALK_WEIGHTS[k]) for k in KINDS])
        out.append(pick([(t, TOKEN_WEIGHTS.get(t.lstrip("!"), 1.0)) for t in tokens_of(kind)]))
    return encode(n, sort_flag, out)


WALK_SEEDS = tuple(range(101, 141))  # forty walks: what the coverage conditions need (test_result_model.py) and a margin
WALK_GROUP = 5                       # walks per GPU test case

# Both sets of both buffer pairs written at a small, a large and a small table size on one engine.
PINGPONG = (
    "n=4097 run:A filter:pre:w1 filter:min5 filter:len4-9 filter:min50 run:A filter:min5 filter:drop3 filter:keep4 filter:min50 "
    "run:B filter:max3 filter:len4-9 filter:min5 rank- filter:one rank+ filter:none",
    "n=4097 run:A filter:pre:w1 rank- rank+ rank- rank+ run:A rank- rank+ rank- sort rank+ run:B filter:max3 rank+ rank- rank+ filter:min5 "
    "rank- sort rank-",
)

# Sequences kept by name: the paths no per-operator test reaches, and every sequence that exposed a bug.
REPLAYS = (
    # rank, then join with substituted counts, then rank again, then find
    "n=1025 run:B acc run:A rank- join:semi/total rank+ sort join:semi/min rank-",
    # sort, first accumulate, filter, reset, accumulate, join
    "n=1025 run:A sort acc filter:min50 reset acc join:semi/result join:anti/result",
    # a re-key that changes nothing on a ranked folded table, then a fetch under the sort flag
    "n=1025/sort run:A rekey:punct rank- acc rekey:hash rekey:max40 sort",
    # two filters and a rank alternating: both sets of both buffer pairs at shrinking sizes
    "n=4097 run:A filter:min5 rank- filter:keep4 rank+ filter:min50 rank- filter:len4-9 rank+ filter:pre:w1 rank- filter:one rank+",
    # a failed fold makes the total the result; it is filtered, re-keyed and dropped with the total
    "n=1025 run:A sort acc run:B !acc filter:min5 join:semi/min reset run:B !acc acc run:A !acc rekey:punct reset filter:min5",
    "n=1025 run:A acc run:B !acc reset sort acc run:A acc !acc",
    # a ranked total comes back ranked; a sorted one sorted
    "n=1025 run:A rank- acc run:B !acc rank+ run:A sort reset acc run:B !acc join:anti/result",
    # one row: sorted and ranked at once, carried through the accumulator
    "n=1025 run:A sort filter:one rank- acc sort run:B !acc rank- sort join:semi/total",
    # under the sort flag a join that substitutes counts ends the ranking: the next fetch sorts again
    "n=1025/sort run:B acc run:A rank- join:semi/total rank+ join:semi/min rank- join:semi/result rank- filter:one join:semi/total",
    # a re-keyed total is still folded: it is not taken twice
    "n=1025 run:A acc rekey:punct acc rekey:max3 acc run:B acc rekey:punct acc reset acc",
    # the 2^63 counts wrap in the merged total
    "n=1025 run:A acc run:A acc run:B acc rank- join:semi/min rekey:max3",
)


def pair_set(n=PAIR_N, sort_flag=False):
    return [pair_sequence(k, n, sort_flag) for k in KINDS]


def walk_set():
    return [walk(s) for s in WALK_SEEDS]


def measured_sets():
    """The sets the coverage and the three conditions are measured on: the pair
    sweep and the home sweep at PAIR_N, the seeded walks and the ping-pong
    sequences.  (The pair sweeps at SMALL_NS rows are left out: they are there to
    act on tables of fewer than two rows.)"""
    return pair_set() + home_set() + walk_set() + list(PINGPONG)


@functools.lru_cache(maxsize=None)
def other_build_walks(count=4):
    """``count`` walks that between them hold every kind (greedy over the seed list)."""
    left, chosen = set(KINDS), []
    traces = {s: trace(walk(s)).kinds for s in WALK_SEEDS}
    while len(chosen) < count:
        best = max((s for s in WALK_SEEDS if s not in chosen), key=lambda s: (len(traces[s] & left), -s))
        chosen.append(best)
        left -= traces[best]
    assert not left, left
    return [walk(s) for s in chosen]
