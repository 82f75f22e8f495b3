"""The shard-window rule of mox_run_range restated over the whole corpus, and
the texts that put its edges on the row geometry of k_map
(map-oxidize_amd/csrc/mox_kernels.hip).  Shared by the CPU tests
(test_window_model.py: the model against the C oracle, and the geometry and
outcome balance of the case lists) and the GPU tests (test_gpu_window.py).

The rule (include/mox.h, mox_run_range): the buffer is D[lo:hi] of a corpus D,
the own range [own_begin, own_end) is relative to lo.  A token belongs to the
range that holds its first byte.  A buffer that does not end the corpus
(at_end false) is MOX_EHALO when an owned token cannot be seen to end inside
it, or when a character whose first byte is owned is cut by hi."""
import bisect
import random
import re
from collections import Counter

import coracle
import pyoracle

PAY = 992   # payload bytes of one k_map row (mox_internal.h, PAY): row r of a pass covers
            # buffer bytes [B + PAY r, B + PAY (r + 1)), B = ((own_begin + mis) & ~15) - mis
            # for a device pointer with mis = address & 15
LANE = 16   # bytes per lane of a row
MIS = (0, 1, 7, 13)          # device pointer offsets of the row-edge plants
DELTAS = tuple(range(-18, 3))  # item start against the edge

# Rust's White_Space set (pyoracle.RUST_WHITESPACE) as UTF-8 byte sequences: on
# valid UTF-8 a whole encoded character matches only at a character boundary
_WS = re.compile(b"|".join(re.escape(ch.encode()) for ch in pyoracle.RUST_WHITESPACE))

_lowered = {}


def _lower(tok):
    w = _lowered.get(tok)
    if w is None:
        w = _lowered[tok] = coracle.lowercase(tok)
    return w


class Model:
    """Tokens of the whole corpus D: starts[i], ends[i], the end seps[i] of the
    whitespace character after token i (ends[i] at the corpus end) and the
    lowercased words[i]."""

    def __init__(self, D):
        D.decode("utf-8")  # the corpus itself is valid
        self.D = D
        self.starts, self.ends, self.seps, self.words = [], [], [], []
        pos = 0
        for m in _WS.finditer(D):
            if m.start() > pos:
                self._add(pos, m.start(), m.end())
            pos = m.end()
        if pos < len(D):
            self._add(pos, len(D), len(D))

    def _add(self, a, b, sep):
        self.starts.append(a)
        self.ends.append(b)
        self.seps.append(sep)
        self.words.append(_lower(self.D[a:b]))

    def tokens(self):
        return list(zip(self.starts, self.ends, self.words))

    def cut_lead(self, hi):
        """Corpus offset of the first byte of the character that hi cuts, or None."""
        D = self.D
        if hi >= len(D) or (D[hi] & 0xC0) != 0x80:
            return None
        p = hi - 1
        while (D[p] & 0xC0) == 0x80:
            p -= 1
        return p

    def halo_rules(self, lo, hi, own_begin, own_end):
        """(off_a, off_b) for a non-final buffer, None where the rule does not hold.
        (a) the last owned token reaches hi: it ends at or after hi (ending
            exactly at hi counts: the separator is not in the buffer), or the
            whitespace character after it is cut by hi, which the buffer cannot
            tell from a letter; off_a = its start.
        (b) a character whose first byte is owned is cut by hi (utf8_check
            returning 2); off_b = that byte."""
        a, b = lo + own_begin, lo + own_end
        i, j = bisect.bisect_left(self.starts, a), bisect.bisect_left(self.starts, b)
        off_a = off_b = None
        if j > i and (self.ends[j - 1] >= hi or self.seps[j - 1] > hi):
            off_a = self.starts[j - 1] - lo
        cut = self.cut_lead(hi)
        if cut is not None and a <= cut < b:
            off_b = cut - lo
        return off_a, off_b

    def expected(self, lo, hi, own_begin, own_end, at_end):
        """("utf8",), ("halo", off) or ("table", sorted [(word, count)], tokens)."""
        assert 0 <= lo <= hi <= len(self.D) and 0 <= own_begin <= own_end <= hi - lo
        a, b = lo + own_begin, lo + own_end
        cut = self.cut_lead(hi)
        assert cut is None or cut >= lo
        if at_end:
            if cut is not None and a <= cut < b:
                return ("utf8",)
            # (a cut character in the look-ahead of a final buffer is out of scope)
            assert cut is None
        else:
            off_a, off_b = self.halo_rules(lo, hi, own_begin, own_end)
            if off_a is not None or off_b is not None:
                assert off_a is None or off_b is None or off_a <= off_b
                return ("halo", off_a if off_a is not None else off_b)
        i, j = bisect.bisect_left(self.starts, a), bisect.bisect_left(self.starts, b)
        return ("table", sorted(Counter(self.words[i:j]).items()), j - i)

    def occurrences(self, word, lo):
        """Buffer offsets at which tokens lowering to `word` start."""
        return [s - lo for s, w in zip(self.starts, self.words) if w == word]


# ------------------------------------------------------------------ items
# An item is (pre, core, post): core is what a case places against an edge,
# pre / post are written around it.  Words carry their site number.

def _tag(s):
    return b"%04d" % (s % 10000)


def _ascii(n, ch):
    k = (n - 4) // 2
    return lambda s: (b" ", ch * k + _tag(s) + ch * (n - 4 - k), b" ")


def _word(fmt):
    return lambda s: (b" ", fmt.replace("#", _tag(s).decode()).encode(), b" ")


def _sep(ws):
    return lambda s: (b" l" + _tag(s), ws.encode(), b"r" + _tag(s) + b" ")


ITEMS = [
    ("ascii1", lambda s: (b" ", bytes([65 + s % 26]), b" ")),
    ("ascii15", _ascii(15, b"h")),
    ("Q16", _ascii(16, b"Q")),
    ("q17", _ascii(17, b"q")),
    ("W40", _ascii(40, b"W")),
    ("nulword", lambda s: (b" ", b"a" + _tag(s) + b"\x00b", b" ")),   # a NUL: a long-table word
    ("nul", lambda s: (b" ", b"\x00", b" ")),
    ("ctl01", lambda s: (b" ", b"a" + _tag(s) + b"\x01b", b" ")),
    ("ws0085", _sep("\u0085")),
    ("ws00a0", _sep("\u00a0")),
    ("ws2003", _sep("\u2003")),
    ("ws3000", _sep("\u3000")),
    ("e_acute", _word("é#é")),
    ("nihon", _word("日本#")),
    ("emoji", _word("\U0001F600z#")),
    ("dotted_I", _word("xİy#")),                      # lowercasing grows it by one byte
    ("kelvin", _word("Kelvinscale# Kelvinscale#")),    # 17 bytes raw, 15 lowered: merges with the plain word
    ("sigma2", _word("ΣΣ#")),
    ("odysseus", _word("ὈΔΥΣΣΕΎΣ#")),
    ("crlf", _sep("\r\n")),
]
PAIRS = [(i, d) for i in range(len(ITEMS)) for d in DELTAS]

_FILL = b"the Quick brown fox JUMPS over a lazy dog\nand Then some more of it\tgoes by "


def filler(n, at=0):
    """n bytes of plain ASCII words (no control bytes)."""
    k = at % len(_FILL)
    return (_FILL[k:] + _FILL * (n // len(_FILL) + 1))[:n]


def plant(buf, pos, item, site):
    """Writes item so that its core starts at buf[pos]."""
    pre, core, post = ITEMS[item][1](site)
    a = pos - len(pre)
    b = pos + len(core) + len(post)
    assert 0 <= a and b <= len(buf), (pos, len(buf))
    buf[a:b] = pre + core + post


# ------------------------------------------------------------------ 3a: row-edge plants
class Planted:
    """A whole-buffer case: data and its plants [(pair index, buffer offset the
    core starts at)]."""

    def __init__(self, name, data, plants):
        self.name, self.data, self.plants = name, bytes(data), plants


def nrows(n, own_begin=0, mis=0):
    base = ((own_begin + mis) & ~15) - mis
    return -(-(n - base) // PAY)


def edge_kind(k, rows):
    """Kind of the row edge PAY k of a pass of `rows` rows: k_map treats rows 0, 1
    and the last three as edge rows (e_lo, e_hi)."""
    kinds = set()
    if k == 1:
        kinds.add("first")
    if rows - 3 <= k <= rows - 1:
        kinds.add("last3")
    if 3 <= k <= rows - 4:  # rows k - 1 and k both in 2 .. rows - 4
        kinds.add("interior")
    return kinds


BIG_ROWS = 600


def row_edge_cases():
    """One buffer of BIG_ROWS rows with a different (item, delta) at each edge
    between non-edge rows, and one 6-row buffer per pair with that pair at the
    edge after row 0 and another pair at one of the last three edges."""
    cases = []
    n = BIG_ROWS * PAY - 300
    buf = bytearray(filler(n))
    plants = []
    for k in range(3, BIG_ROWS - 3):
        pi = (k - 3) % len(PAIRS)
        pos = PAY * k + PAIRS[pi][1]
        plant(buf, pos, PAIRS[pi][0], k)
        plants.append((pi, pos))
    cases.append(Planted("big", buf, plants))
    half = len(PAIRS) // 2
    for i in range(len(PAIRS)):
        n = 5 * PAY + 80 + (37 * i) % 900
        buf = bytearray(filler(n, i))
        j = (i + half) % len(PAIRS)
        kl = 3 + i % 3
        p1, p2 = PAY + PAIRS[i][1], PAY * kl + PAIRS[j][1]
        plant(buf, p1, PAIRS[i][0], 1000 + i)
        plant(buf, p2, PAIRS[j][0], 2000 + i)
        cases.append(Planted("small%d" % i, buf, [(i, p1), (j, p2)]))
    return cases


LANE_ROWS, LANE_STEP = 9, 6 * LANE


def lane_cases():
    """Every (item, delta) at a 16-byte lane boundary inside rows 2-4 of a 9-row
    buffer (non-edge rows), whatever the row size is: the plants of buffer b
    sit LANE_STEP apart from lane 2 PAY / 16 + b % 6 on."""
    per = (3 * PAY) // LANE_STEP
    cases = []
    for b in range(-(-len(PAIRS) // per)):
        buf = bytearray(filler(LANE_ROWS * PAY - 100, 7 * b))
        plants = []
        for k in range(per):
            pi = b * per + k
            if pi >= len(PAIRS):
                break
            pos = 2 * PAY + LANE * (b % 6) + LANE_STEP * k + PAIRS[pi][1]
            plant(buf, pos, PAIRS[pi][0], 3000 + pi)
            plants.append((pi, pos))
        cases.append(Planted("lane%d" % b, buf, plants))
    return cases


# ------------------------------------------------------------------ 3b: own-range sweep
def _kit(s, controls=True, unicode_=True):
    """The four kinds a swept window must hold, as (kind, bytes) in order."""
    t = _tag(s)
    parts = [("word17", b"q" * 6 + t + b"q" * 7), ("sp", b" ")]
    parts += [("nulword", b"a\x00b" if controls else b"a+b")]
    parts += [("ws", "\u3000".encode() if unicode_ else b"\r\n")]
    parts += [("letter", ("é" + t.decode()[:2]).encode() if unicode_ else b"E" + t[:2])]
    parts += [("ws2", "\u0085".encode() if unicode_ else b"\t"), ("tail", b"z" + t[:2]), ("sp", b" ")]
    return parts


def _dense(n, s0):
    """n bytes dense in the items, separated by assorted whitespace."""
    seps = [b" ", b"\n", "\u2003".encode(), b"\t", "\u00a0".encode(), b"\r\n"]
    out = bytearray()
    s = s0
    while True:
        pre, core, post = ITEMS[s % len(ITEMS)][1](s)
        piece = pre.strip(b" ") + core + post.strip(b" ") + seps[s % len(seps)]
        if len(out) + len(piece) > n:
            break
        out += piece
        s += 1
    if len(out) < n:
        out += b"p" * (n - len(out) - 1) + b" "
    return bytes(out)


SWEEP_LEN = 4500
SWEEP_WINDOWS = ((4, 52), (970, 1030), (1962, 2022), (SWEEP_LEN - 60, SWEEP_LEN))


def sweep_corpus(kind):
    """(text, [(window, [(kind, start, end)])]): SWEEP_LEN bytes with a kit 4
    bytes into each swept window.  "dense": the items of ITEMS throughout, so
    every row takes the Unicode walk.  "ascii": plain ASCII, control bytes only
    in the third window, so the rows of the other windows take the common list
    builder and the third the checked one."""
    out = bytearray()
    where = []
    for wi, (a, b) in enumerate(SWEEP_WINDOWS):
        gap = a + 4 - len(out)
        out += _dense(gap, 40 * wi) if kind == "dense" else filler(gap - 1, 11 * wi) + b" "
        spans = []
        for name, piece in _kit(wi, controls=(kind == "dense" or wi == 2), unicode_=(kind == "dense")):
            spans.append((name, len(out), len(out) + len(piece)))
            out += piece
        assert len(out) <= b
        where.append(((a, b), spans))
    gap = SWEEP_LEN - len(out)
    out += filler(gap - 3, 5) + b" zq"  # the corpus ends inside a token
    assert len(out) == SWEEP_LEN
    return bytes(out), where


def sweep_ranges(n, seed):
    """(own_begin, own_end) of the sweep over a text of n bytes."""
    (a0, b0), (a1, b1), (a2, b2), (a3, b3) = SWEEP_WINDOWS
    begins = [0] + list(range(a0, b0)) + list(range(a1, b1)) + list(range(a3, b3))
    ends = list(range(0, b0)) + list(range(a1, b1)) + list(range(a2, b2)) + list(range(a3, b3))
    out = [(ob, n) for ob in begins] + [(0, oe) for oe in ends]
    rng = random.Random(seed)
    out += [(0, 0), (n // 2, n // 2), (n, n)]
    for w in (1, 2, 15, 16, 17):
        for _ in range(8):
            ob = rng.randrange(4, n - w)
            out.append((ob, ob + w))
    while len(out) < len(begins) + len(ends) + 300:
        ob = rng.choice([0, rng.randrange(4, n)])
        out.append((ob, rng.randrange(ob, n + 1)))
    return out


# ------------------------------------------------------------------ 3c: non-final buffers
HEAD = b"con" + "日本".encode() + b"text "   # lo = 1: inside a word; lo = 4: inside U+65E5
LO_KINDS = (0, 1, 4)
HALO_PLACES = {"row0": 200, "past_edge": 2 * PAY, "before_edge": 3 * PAY - 52}


def halo_window(s):
    """(kind, bytes) in order: the plain-ASCII ends first, so that hi sweeps them
    in rows without a control or non-ASCII byte."""
    t = _tag(s)
    return [("short", b"ab "), ("word16", b"Q" * 6 + t + b"Q" * 6 + b" "), ("word17", b"q" * 6 + t + b"q" * 7 + b" "),
            ("nulword", b"a\x00b"), ("ws3", "\u3000".encode()), ("letter2", "zéy ".encode()),
            ("emoji", "w\U0001F600z ".encode()), ("tail", b"end ")]


def halo_corpus(place):
    """(D, window start, window end, [(kind, start, end)]): HEAD, plain ASCII
    filler, the window at HALO_PLACES[place] and 1200 bytes after it."""
    at = HALO_PLACES[place]
    out = bytearray(HEAD + filler(at - len(HEAD) - 1, 3) + b" ")
    spans = []
    for name, piece in halo_window(len(place)):
        spans.append((name, len(out), len(out) + len(piece)))
        out += piece
    end = len(out)
    out += filler(1200, 9)
    return bytes(out), at, end, spans


def halo_cases(place):
    """[(lo, hi, own_begin, own_end)] over halo_corpus(place), all with
    at_end false.  own_begin = 0 only with lo = 0 (it means "corpus start")."""
    D, a, b, _ = halo_corpus(place)
    out = []
    for lo in LO_KINDS:
        for hi in range(a, b + 1):
            n = hi - lo
            for back in (0, 1, 5, 16, 17, 48, 49, 1000, 1100):
                oe = n - back
                if oe < 0:
                    continue
                for ob in sorted({0, 4, oe - 1}):
                    if ob < 0 or ob > oe or 0 < ob < 4 or (lo and ob == 0):
                        continue
                    out.append((lo, hi, ob, oe))
    return out
