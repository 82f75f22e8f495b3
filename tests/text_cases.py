"""Word tables for the device text rendering (map-oxidize_amd/csrc/mox_text.hip,
mox_write_result / mox_result_text) and the expectation they are checked
against: b"".join(word + b" %d\\n" % count) over the fetched table in its
order.  Shared by test_result_text_abi.py (CPU: the constants match the source,
the generators have the shape they claim) and test_gpu_result_text.py (GPU).

Engine order puts every word of at most 16 bytes before every longer one, so a
generator that needs its words next to each other in the table (digit lengths
side by side, a 100,000-byte word between two 1-byte words, a tile of exactly
so many text bytes) names its words so that BYTEWISE order is the order it
wants; the GPU tests render those tables after sort_result() as well as in
engine order, and assert the adjacency on the fetched table."""
import random

TILE = 1024   # TX_TILE: words per tile
LDS = 24576   # TX_LDS: a tile whose text is longer takes the slow path
U64 = (1 << 64) - 1

# n on the wave (64), workgroup (256) and tile edges of the kernels
EDGE_NS = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)

# MOX_TEXT_SLICE values of the slice tests: the smallest slices the engine
# takes with odd edges everywhere, and a size at which slices hold many lines.
# (4,096 is the natural second value; on mixed()'s text its 38 edges miss the
# space and the newline, 4,112 hits all five classes: test_result_text_abi.py
# checks it.)
SLICES = (272, 4112)


def expected(items):
    """The text of a table given as its (word, count) list in table order."""
    return b"".join(w + b" %d\n" % c for w, c in items)


def lines_of(items):
    return [(w, b" %d\n" % c) for w, c in items]


def names(n, tag=b"w"):
    """n distinct short words."""
    return [tag + b"%d" % i for i in range(n)]


def ordered_names(n, tag=b"k"):
    """n distinct short words whose bytewise order is their index order."""
    return [tag + b"%07d" % i for i in range(n)]


def by_digits(d, high):
    """The smallest (high: the largest) count of d decimal digits that fits 64 bits."""
    return min(10 ** d - 1, U64) if high else 10 ** (d - 1)


def distinct(n, seed):
    """n short words, counts of every digit length 1..20."""
    rng = random.Random(seed)
    counts = [min(U64, rng.randrange(10 ** (d - 1), 10 ** d)) for d in (rng.randint(1, 20) for _ in range(n))]
    return names(n), counts


def all_ones(n):
    return names(n), [1] * n


def digit_edges():
    """(words, counts) in bytewise order: first 10^(d-1) and 10^d - 1 for
    d = 1..20 (2^64 - 1 for d = 20) and 2^64 - 1, each once; then for every
    ordered pair (a, b) of digit lengths a count of a digits followed by one of
    b digits, so the in-tile scan meets every digit count next to every other."""
    counts = []
    for d in range(1, 21):
        counts += [by_digits(d, False), by_digits(d, True)]
    counts.append(U64)
    flip = False
    for a in range(1, 21):
        for b in range(1, 21):
            counts += [by_digits(a, flip), by_digits(b, not flip)]
            flip = not flip
    return ordered_names(len(counts)), counts


def digit_pairs(counts):
    """The ordered pairs of digit lengths of neighbouring counts."""
    ds = [len(b"%d" % c) for c in counts]
    return set(zip(ds, ds[1:]))


BIG_LEN = 100000


def word_shapes(seed=6):
    """(words, counts): words of every length 1..40 (every source and
    destination alignment mod 16), non-ASCII words, words far over 16 bytes (over
    the 64 bytes from which a workgroup moves a word together), and one
    100,000-byte word that bytewise order puts between the 1-byte words b"L"
    and b"M" (no other word starts with b"L"); 3,000 words, counts of 1..20
    digits."""
    rng = random.Random(seed)
    words = [bytes([97 + (L % 26)]) * L for L in range(1, 41)]
    words += ["żółć".encode(), "ΣΊΣΥΦΟΣ".encode(), "日本語".encode(), "naïve-café".encode(), b"\xf0\x9f\x98\x80" * 5]
    words += [b"K" * 100 + b"%d" % i for i in range(17)] + [b"J" * (65 + 37 * i) for i in range(12)]
    big = b"L" + bytes(rng.randrange(33, 127) for _ in range(BIG_LEN - 1))
    words += [b"L", big, b"M"]
    words += names(3000 - len(words), b"r")
    assert len(set(words)) == len(words) == 3000
    counts = [min(U64, rng.randrange(10 ** (d - 1), 10 ** d)) for d in (rng.randint(1, 20) for _ in words)]
    order = list(range(len(words)))
    rng.shuffle(order)
    return [words[i] for i in order], [counts[i] for i in order]


def mixed():
    """The table of the slice tests: word_shapes (rendered in bytewise order)."""
    return word_shapes(seed=11)


def lds_edge_tiles():
    """(words, counts, tile text lengths): three full tiles in bytewise order
    whose texts are LDS - 1, LDS and LDS + 1 bytes -- the last two on either
    side of the fast path's limit -- then a one-word tile.  Every word is 5
    bytes with count 1 (an 8-byte line) but each tile's first, which is padded
    to fill the tile."""
    words, lens = [], []
    for tile, target in enumerate((LDS - 1, LDS, LDS + 1)):
        tw = [b"%d%04d" % (tile, i) for i in range(TILE)]
        tw[0] += b"_" * (target - 8 * TILE)
        words += tw
        lens.append(target)
    words.append(b"zz")
    lens.append(5)
    return words, [1] * len(words), lens


def tile_text_lengths(items):
    return [len(expected(items[i:i + TILE])) for i in range(0, len(items), TILE)]


CLASSES = ("start", "word", "space", "digits", "newline")


def slice_classes(text_lines, S):
    """Where the slice edges k S (0 < k S < text length) fall: a dict class ->
    number of edges, for text_lines = [(word, b" <count>\\n")] in text order.
    start: a line's first byte; word: another byte of the word; space; digits;
    newline."""
    out = dict.fromkeys(CLASSES, 0)
    pos = 0  # text offset of the line
    nxt = S  # the next edge
    for w, tail in text_lines:
        end = pos + len(w) + len(tail)
        while nxt < end:
            x = nxt - pos
            if x == 0:
                c = "start"
            elif x < len(w):
                c = "word"
            elif x == len(w):
                c = "space"
            elif x < len(w) + len(tail) - 1:
                c = "digits"
            else:
                c = "newline"
            out[c] += 1
            nxt += S
        pos = end
    return out


def slices_inside_a_word(text_lines, S):
    """Slices [k S, (k + 1) S) that hold nothing but bytes of one word."""
    n, pos = 0, 0
    for w, tail in text_lines:
        first = -(-pos // S)  # the first edge at or after the word's start
        n += max(0, (pos + len(w)) // S - first)
        pos += len(w) + len(tail)
    return n
