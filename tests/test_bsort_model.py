"""CPU: the record layout and level scheme of the device bytewise sort
(map-oxidize_amd/csrc/mox_bsort.hip) restated in Python and checked against
Python's bytes order (= Rust String Ord).

Each level sorts records by (run, key) with key = the word's 7-byte window at
that level big-endian in bits 63..8 and aux = min(bytes left, 8) in bits 7..0;
records tied on (run, key) with aux == 8 form runs that the next level
re-sorts on the next window.  The GPU does the per-level sort as an LSD radix
(stable); here a stable sort by the same key stands in for it.  No GPU code
runs here: this pins the key construction and the tie rule the kernels use."""
import random

import bsort_cases as C

WIN, AUX_MORE = 7, 8


def window(word, level):
    a = WIN * level
    have = max(0, len(word) - a)
    k = 0
    for j in range(min(have, WIN)):
        k |= word[a + j] << (8 * (7 - j))
    return k | (AUX_MORE if have > WIN else have)


def model_sort(words):
    recs = [(0, window(w, 0), i) for i, w in enumerate(words)]  # (run, key, idx)
    recs.sort(key=lambda r: (r[0], r[1]))
    run_base, level = 1, 1
    while True:
        # tie runs: equal (run, key) with aux == AUX_MORE on both sides
        tied = [False] * len(recs)
        heads = []
        for j in range(1, len(recs)):
            a, b = recs[j - 1], recs[j]
            if (a[1] & 0xFF) == AUX_MORE and a[0] == b[0] and a[1] == b[1]:
                if not tied[j - 1]:
                    heads.append(j - 1)
                tied[j - 1] = tied[j] = True
        if not heads:
            break
        # subset in sorted position order, run id = base + index of its run
        run_of, r = {}, -1
        for j in range(len(recs)):
            if j in heads:
                r += 1
            if tied[j]:
                run_of[j] = run_base + r
        pos = sorted(run_of)
        sub = [(run_of[j], window(words[recs[j][2]], level), recs[j][2]) for j in pos]
        sub.sort(key=lambda x: (x[0], x[1]))
        for j, s in zip(pos, sub):
            recs[j] = s
        run_base += len(heads)
        level += 1
    return [words[r[2]] for r in recs]


def test_model_matches_bytes_order():
    rng = random.Random(7)
    alphabet = b"ab\x01z\xff"
    for trial in range(200):
        n = rng.randint(0, 60)
        words = set()
        base = bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 20)))
        while len(words) < n:
            kind = rng.random()
            if kind < 0.4:  # shared long prefixes: ties over several levels
                w = base[:rng.randint(0, len(base))] + bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 9)))
            else:
                w = bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 30)))
            if w:
                words.add(w)
        words = list(words)
        rng.shuffle(words)
        assert model_sort(words) == sorted(words)


def test_window_prefix_and_length_classes():
    # a proper prefix sorts first; equal windows order by the bytes left
    assert window(b"abc", 0) < window(b"abcd", 0) < window(b"abcdefg", 0) < window(b"abcdefgh", 0)
    assert window(b"abcdefgh", 0) == window(b"abcdefgz", 0)  # both go on past the window: a tie
    assert window(b"abcdefgh", 0) & 0xFF == AUX_MORE and window(b"abcdefg", 0) & 0xFF == 7
    assert window(b"abcdefgh", 1) == (ord("h") << 56) | 1


def levels_and_order(words):
    """([(subset size, run lengths in subset order, first run id)] for levels
    1, 2, ..., sorted words): the tie levels of the device sort, with one scan
    per level (model_sort's `j in heads` is quadratic).  The subset of a level
    is every record in a run of >= 2, in sorted position order, so a run's
    subset position is the sum of the run lengths before it.  first run id is
    the level's run-id base (rbs[] in bsort_once): the kernels number its runs
    base + 1 .. base + runs, and the checked mode's radix sorts on the bytes of
    top = base + runs."""
    recs = sorted(((0, window(w, 0), i) for i, w in enumerate(words)), key=lambda r: (r[0], r[1]))
    out, run_base, level, n = [], 1, 1, len(recs)
    while True:
        runs, j = [], 0  # (first sorted position, length)
        while j < n:
            a, k = recs[j], j + 1
            if (a[1] & 0xFF) == AUX_MORE:
                while k < n and recs[k][0] == a[0] and recs[k][1] == a[1]:
                    k += 1
            if k - j >= 2:
                runs.append((j, k - j))
            j = k
        if not runs:
            break
        out.append((sum(L for _, L in runs), [L for _, L in runs], run_base))
        for r, (j, L) in enumerate(runs):
            sub = [(run_base + r, window(words[i], level), i) for _, _, i in recs[j:j + L]]
            sub.sort(key=lambda x: x[1])
            recs[j:j + L] = sub
        run_base += len(runs)
        level += 1
    return out, [words[r[2]] for r in recs]


def levels(words):
    return levels_and_order(words)[0]


def run_starts(run_lens):
    out, c = [], 0
    for L in run_lens:
        out.append(c)
        c += L
    return out


def nrb_of(level):
    """Run-id digits of the checked mode's radix over this level's subset."""
    top = level[2] + len(level[1])
    return 1 if top < 1 << 8 else 2 if top < 1 << 16 else 3 if top < 1 << 24 else 4


def test_levels_agree_with_model_sort():
    rng = random.Random(11)
    for trial in range(50):
        words = list({bytes(rng.choice(b"ab") for _ in range(rng.randint(1, 25))) for _ in range(rng.randint(0, 80))})
        lv, order = levels_and_order(words)
        assert order == sorted(words) == model_sort(words)
        assert all(m == sum(runs) and min(runs) >= 2 for m, runs, _ in lv)
        assert [rb for _, _, rb in lv] == [1 + sum(len(r) for _, r, _ in lv[:k]) for k in range(len(lv))]


def test_case_generators_are_distinct_and_non_empty():
    tables = [C.sizes(n) for n in C.SIZE_NS] + [C.run_geometry(), C.run_geometry_over(), C.run_digits(300), C.deep_ties()]
    tables += list(C.out_stage())
    for words in tables:
        assert all(isinstance(w, bytes) and w for w in words) and len(set(words)) == len(words)
        assert words != sorted(words)  # the sort has something to do
    assert C.pref(0) == b"aaaaaaa" and C.pref(27) == b"aaaaabb" and C.pref(26 ** 7 - 1) == b"zzzzzzz"
    assert sorted(C.pref(g) for g in range(0, 80000, 97)) == [C.pref(g) for g in range(0, 80000, 97)]
    for L in (1, 2, 64, 65, 5000):
        g = C.group(b"ppppppp", L)
        assert len(set(g)) == L and all(w.startswith(b"ppppppp") and 8 <= len(w) <= 15 for w in g)


def test_case_sizes():
    assert C.SIZE_NS == (2, 3, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193)
    for n in C.SIZE_NS:
        words = C.sizes(n)
        assert len(words) == n and all(1 <= len(w) <= 12 for w in words)
        assert levels_and_order(words)[1] == sorted(words)
    big = C.sizes(8193)
    assert {w[0] for w in big} >= {0x00, 0x7F, 0x80, 0xFF} and levels(big)  # extreme bytes lead words; ties exist
    # a last output block of one short word: k_bs_out2's branch without a whole 16-byte line
    for n in (257, 4097, 8193):
        b0, b1 = C.block_spans(C.sizes(n))[-1]
        assert 0 < b1 - b0 < 16 and ((b0 + 15) & ~15) >= (b1 & ~15)


def test_case_run_geometry():
    words = C.run_geometry()
    lv, order = levels_and_order(words)
    assert order == sorted(words) and len(words) == 8326
    m, runs, rb = lv[0]
    assert (m, len(runs), rb, max(runs)) == (8205, 1906, 1, C.RUN_LMAX) and runs == C.RUN_LENGTHS
    at = dict(zip(run_starts(runs), runs))
    # the SEG_MAX run's head is the last record of chunk 0: it needs the SEG_MAX overhang and is
    # skipped by chunk 1 (prev_run); the SEG_MAX + 1 run behind it is the shortest listed one
    assert at[C.SEG_CH - 1] == C.SEG_MAX and at[C.SEG_CH - 1 + C.SEG_MAX] == C.SEG_MAX + 1
    # a listed run across the second chunk boundary, and the longest run k_bs_longsort takes
    # right behind it (it spans two more boundaries)
    assert at[3976] == 130 and 3976 < 2 * C.SEG_CH < 3976 + 130
    assert at[4106] == C.RUN_LMAX
    assert 47 in runs and runs.count(2) == 1900  # short runs inside a chunk; a 47-run ends at 2,047
    # level 2: the two tails sharing 7 bytes in each group longer than SEG_MAX; then done
    assert lv[1:] == [(6, [2, 2, 2], 1907)]
    # unchecked mode finishes: no run past RUN_LMAX, far fewer listed runs than the list holds
    assert sum(1 for L in runs if L > C.SEG_MAX) == 3


def test_case_run_geometry_over():
    words = C.run_geometry_over()
    lv, order = levels_and_order(words)
    assert order == sorted(words) and len(words) == 8327
    m, runs, rb = lv[0]
    assert (m, len(runs), rb, max(runs)) == (8206, 1906, 1, C.RUN_LMAX + 1)
    assert dict(zip(run_starts(runs), runs))[4106] == C.RUN_LMAX + 1
    assert nrb_of(lv[0]) == 2


def test_case_run_digits():
    lv, order = levels_and_order(C.run_digits(300))
    m, runs, rb = lv[0]
    assert (m, len(runs), rb) == (5600, 301, 1) and runs == [2] * 300 + [5000] and nrb_of(lv[0]) == 2
    assert lv[1:] == [(2, [2], 302)]
    words = C.run_digits(70_000)
    lv, order = levels_and_order(words)
    assert order == sorted(words) and len(words) == 145_000
    m, runs, rb = lv[0]
    assert (m, len(runs), rb) == (145_000, 70_001, 1) and max(runs) == 5000 > C.RUN_LMAX
    assert rb + len(runs) == 70_002 >= 1 << 16 and nrb_of(lv[0]) == 3
    assert lv[1:] == [(2, [2], 70_002)]


def test_case_out_stage():
    a, b, c = C.out_stage()
    assert len(a) == len(b) == C.OUT_BLOCK and {len(w) for w in a} == {64} and sorted(len(w) for w in b)[-2:] == [64, 65]
    sa, sb = C.block_spans(a), C.block_spans(b)
    assert sa == [(0, C.OUT_STAGE)] and C.staged(sa[0])
    assert sb == [(0, C.OUT_STAGE + 1)] and not C.staged(sb[0])
    sc = C.block_spans(c)
    assert len(c) % C.OUT_BLOCK == 1 and len(sc) == 6
    assert [C.staged(s) for s in sc] == [True, True, False, False, False, True]
    order = sorted(c)
    kinds = ["".join(sorted({"k" if len(w) <= 7 else "t" for w in order[j:j + 256]})) for j in range(0, len(c), 256)]
    assert kinds == ["k", "k", "kt", "t", "t", "t"]  # k: bytes from the level-0 key, t: from the table
    assert sum(len(w) <= 7 for w in order[512:768]) == 5 and all(100 <= len(w) <= 300 for w in order[517:])
    for t in (a, b, c):
        assert levels_and_order(t)[1] == sorted(t)


def test_case_deep_ties():
    words = C.deep_ties()
    lv, order = levels_and_order(words)
    assert order == sorted(words)
    assert len(lv) == 5  # levels 1..5 have work: the & 3 rings of lvt / rbs wrap at level 4
    fam = [w for w in words if w.startswith(C.DEEP_PREFIX) and len(w) > 35]
    assert lv[4][1] == [len(fam)] and len({w[35] for w in fam}) > 1  # one run settled on byte 36
    lens = {len(w) for w in words}
    assert lens >= {7, 8, 9, 14, 15, 21, 22, 23, 35, 36, 42}
    for a, b in ((7, 8), (8, 9), (14, 15), (21, 22), (22, 23)):
        assert any(len(x) == a and len(y) == b and y.startswith(x) for x in words for y in words)
    # every word the reduce lays out last (longer than 16 bytes) is in a run at level 2 or deeper
    for w in words:
        if len(w) > 16:
            assert any(v != w and v[:14] == w[:14] and len(v) > 14 for v in words), w
