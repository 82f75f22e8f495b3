"""CPU: the shard-window model of window_cases.py against the C oracle's
moxo_count_range, and the geometry and outcome balance of the case lists that
test_gpu_window.py runs, so that a GPU test there cannot pass while missing the
branch it is there for.  No GPU code runs here."""
import coracle
import pyoracle
import window_cases as W


def test_whitespace_sets_agree():
    """The model's byte pattern is built from pyoracle's set: the C oracle has the same one."""
    ws = {cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000 and coracle.is_whitespace(cp)}
    assert ws == {ord(ch) for ch in pyoracle.RUST_WHITESPACE}


def oracle_corpora():
    items = b"".join(b"".join(f(900 + i)) for i, (_, f) in enumerate(W.ITEMS))
    return {"items": items, "dense": W.sweep_corpus("dense")[0], "ascii": W.sweep_corpus("ascii")[0][1900:2100],
            "halo_row0": W.halo_corpus("row0")[0][:420]}


def test_model_matches_oracle_ranges():
    """Every own_begin (inside 2-, 3- and 4-byte characters and multi-byte
    whitespace too) with three own_end each, and every own_end from 0."""
    ran = want = 0
    for name, D in oracle_corpora().items():
        m = W.Model(D)
        n = len(D)
        ranges = [(a, b) for a in range(n + 1) for b in (n, min(n, a + 37), a)] + [(0, b) for b in range(n + 1)]
        want += 4 * (n + 1)
        for a, b in ranges:
            got = m.expected(0, n, a, b, True)
            assert got[0] == "table", (name, a, b)
            assert (got[1], got[2]) == coracle.count_range(D, a, b), (name, a, b)
            ran += 1
    assert ran == want and ran > 10000


def test_model_whole_corpus_is_the_plain_count():
    for D in oracle_corpora().values():
        m = W.Model(D)
        assert m.expected(0, len(D), 0, len(D), True)[1:] == coracle.count(D)
        assert [D[a:b] for a, b, _ in m.tokens()] == [t.encode() for t in pyoracle.split_whitespace(D.decode())]


def test_row_edge_cases_geometry():
    """3a: every (item, delta) at an edge between non-edge rows, at the edge
    after row 0 and at one of the last three edges; the big
    buffer has more than twice 256 rows, so that a workgroup of a grid of 256
    owns consecutive rows."""
    cases = W.row_edge_cases()
    assert len(cases) == 1 + len(W.PAIRS) and len(W.PAIRS) == len(W.ITEMS) * 21
    seen = {}
    for c in cases:
        rows = W.nrows(len(c.data))
        for pi, pos in c.plants:
            k, d = divmod(pos - W.PAIRS[pi][1], W.PAY)
            assert d == 0
            seen.setdefault(pi, set()).update(W.edge_kind(k, rows))
        W.Model(c.data)  # valid UTF-8
    assert W.nrows(len(cases[0].data)) == W.BIG_ROWS > 2 * 256
    assert all(seen.get(pi) == {"first", "last3", "interior"} for pi in range(len(W.PAIRS))), seen
    # the planted words are there, once per site (the kelvin pair twice)
    big = cases[0]
    m = W.Model(big.data)
    counts = dict(m.expected(0, len(big.data), 0, len(big.data), True)[1])
    for pi, pos in big.plants:
        name = W.ITEMS[W.PAIRS[pi][0]][0]
        k = (pos - W.PAIRS[pi][1]) // W.PAY  # the site number of a plant in the big buffer is its edge
        if name == "kelvin":
            assert counts[b"kelvinscale%04d" % k] == 2
        if name == "q17":
            assert counts[b"qqqqqq%04dqqqqqqq" % k] == 1


def test_lane_cases_geometry():
    """3a: every (item, delta) at a 16-byte lane boundary inside non-edge rows."""
    seen = set()
    for c in W.lane_cases():
        rows = W.nrows(len(c.data))
        assert rows == W.LANE_ROWS
        for pi, pos in c.plants:
            at = pos - W.PAIRS[pi][1]
            assert at % W.LANE == 0 and 2 * W.PAY <= at < 5 * W.PAY and 5 <= rows - 4
            seen.add(pi)
        W.Model(c.data)
    assert seen == set(range(len(W.PAIRS)))


def test_sweep_corpus_windows():
    """3b: each swept window of the dense text holds a multi-byte whitespace, a
    multi-byte letter, a NUL word and a 17-byte word, each wholly inside it."""
    D, where = W.sweep_corpus("dense")
    assert len(D) == W.SWEEP_LEN and len(where) == len(W.SWEEP_WINDOWS)
    for (a, b), spans in where:
        got = {name: (s, e) for name, s, e in spans}
        for name, size in (("word17", 17), ("nulword", 3), ("ws", 3), ("letter", 4), ("ws2", 2)):
            s, e = got[name]
            assert a < s and e < b and e - s == size, (a, b, name)
        assert D[got["ws"][0]:got["ws"][1]] == "　".encode() and D[got["letter"][0]:][:2] == "é".encode()
        assert b"\x00" in D[got["nulword"][0]:got["nulword"][1]]
    A, _ = W.sweep_corpus("ascii")
    assert len(A) == W.SWEEP_LEN and max(A) < 0x80
    ctl = [i for i, x in enumerate(A) if x < 9]
    assert ctl and all(W.SWEEP_WINDOWS[2][0] <= i < W.SWEEP_WINDOWS[2][1] for i in ctl)
    ranges = W.sweep_ranges(W.SWEEP_LEN, 1)
    assert len(ranges) >= 700
    for need in ((0, 0), (W.SWEEP_LEN // 2, W.SWEEP_LEN // 2), (W.SWEEP_LEN, W.SWEEP_LEN)):
        assert need in ranges
    assert {1, 2, 15, 16, 17} <= {oe - ob for ob, oe in ranges}
    assert all(ob == 0 or ob >= 4 for ob, _ in ranges)
    # every outcome of the sweep is a table (the whole text is valid and final)
    ran = 0
    for text in (D, A):
        m = W.Model(text)
        for ob, oe in ranges:
            assert m.expected(0, len(text), ob, oe, True)[0] == "table"
            ran += 1
    assert ran == 2 * len(ranges)


def test_halo_cases_balance():
    """3c: both outcomes, and each halo rule alone, occur often enough at every
    placement that a kernel answering one way throughout cannot pass."""
    for place in W.HALO_PLACES:
        D, a, b, spans = W.halo_corpus(place)
        assert 55 <= b - a <= 90 and a == W.HALO_PLACES[place]
        assert [n for n, _, _ in spans] == ["short", "word16", "word17", "nulword", "ws3", "letter2", "emoji", "tail"]
        assert all(9 <= x < 0x80 for x in D[len(W.HEAD):spans[3][1]])  # plain ASCII from HEAD up to the NUL word
        m = W.Model(D)
        cases = W.halo_cases(place)
        n = {"halo": 0, "table": 0, "a": 0, "b": 0, "sep": 0}
        for lo, hi, ob, oe in cases:
            out = m.expected(lo, hi, ob, oe, False)
            n[out[0]] += 1
            if out[0] == "halo":
                oa, obb = m.halo_rules(lo, hi, ob, oe)
                n["a"] += oa is not None and obb is None
                n["b"] += oa is None and obb is not None
                j = m.starts.index(oa + lo) if oa is not None else None
                n["sep"] += j is not None and m.ends[j] < hi < m.seps[j]
        assert n["halo"] + n["table"] == len(cases)
        assert n["halo"] >= 50 and n["table"] >= 50 and n["a"] >= 10 and n["b"] >= 10 and n["sep"] >= 2, (place, n)
        assert {lo for lo, _, _, _ in cases} == set(W.LO_KINDS)
        assert {hi for _, hi, _, _ in cases} == set(range(a, b + 1))
    # lo = 1 is a character boundary inside a word, lo = 4 the middle of a 3-byte letter
    assert W.HEAD[:3].isalpha() and (W.HEAD[4] & 0xC0) == 0x80 and (W.HEAD[3] & 0xF0) == 0xE0
