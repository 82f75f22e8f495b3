"""Word tables and queries for the device lookup (mox_lookup_words,
map-oxidize_amd/csrc/mox_lookup.hip) and the expectation they are checked
against: a dictionary over the fetched table.  Shared by test_lookup_abi.py
(CPU: the constants match the sources, the generators have the shapes they
claim) and test_gpu_lookup.py (GPU)."""
import random

import top_cases

TILE = 1024       # WS_TILE (mox_wordset.h): table words (and queries) per workgroup step, WS_T x WS_PER
LANE_MAX = 64     # WS_LANE_MAX: a longer word is hashed and compared by a whole wave
IDX_BITS = 21     # LkWords::IDX_BITS: a slot's query index + 1 ...
TAG_BITS = 43     # LkWords::TAG_BITS: ... below the hash's upper bits
LOOKUP_MAX = 1 << 20
NONE = (1 << 64) - 1

# table sizes on the wave (64), workgroup (256) and tile edges of the stream
TABLE_NS = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1)
STRIDE_GRID = 2              # MOX_LOOKUP_GRID for the stride case: two workgroups ...
STRIDE_N = 5 * TILE + 1      # ... over six tiles, the last one of a single word: three strides each
QUERY_NS = (0, 1, 2, 63, 64, 65, 1023, 1024, 1025)
SHAPE_LENS = (7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65)


def expected(items, queries):
    """(counts, index) of ``queries`` against a table given as its (word, count)
    list in table order: the word's count and position, (0, NONE) when absent."""
    pos = {}
    for i, (w, c) in enumerate(items):
        assert w not in pos, w
        pos[w] = (c, i)
    got = [pos.get(q, (0, NONE)) for q in queries]
    return [c for c, _ in got], [i for _, i in got]


def table_words(n, seed):
    """n distinct words of 1..24 bytes (short and long rows of the engine mixed)
    with counts 1..n shuffled."""
    rng = random.Random(seed)
    words = [b"t%d" % i + b"_" * (i % 23) for i in range(n)]
    counts = list(range(1, n + 1))
    rng.shuffle(counts)
    return words, counts


def absent_words(n):
    """n distinct words no table here holds, with the lengths of table_words."""
    return [b"A%d" % i + b"_" * (i % 23) for i in range(n)]


def present_and_absent(words, seed):
    """Every table word plus as many absent words, shuffled."""
    q = list(words) + absent_words(len(words))
    random.Random(seed).shuffle(q)
    return q


def near_misses(w):
    """The words next to w that a sloppy compare would take for it."""
    out = [w[:-1], w + b"a", w + b"\x00", w[:-1] + bytes([w[-1] ^ 1]), w.upper()]
    return [x for x in out if x != w]


NUL_WORDS = [b"a\x00b", b"\x00", b"\x00\x00", b"ab\x00", b"x" * 20 + b"\x00" + b"y" * 20, b"n" * 63 + b"\x00"]
PREFIX_CHAIN = [b"a" * k for k in range(1, 71)]


def shape_table(seed=11):
    """(words, counts): top_cases.word_shapes() (lengths 1..40, a 100,000-byte
    word, non-ASCII words) plus words on the 8-byte-word and lane / wave edges,
    words with a NUL byte inside and the chain of prefixes a, aa, ... (70 bytes)."""
    words, counts, _ = top_cases.word_shapes()
    words, counts = list(words), list(counts)
    have = set(words)
    extra = [bytes([65 + (L % 26)]) * (L - 1) + b"!" for L in SHAPE_LENS] + NUL_WORDS + PREFIX_CHAIN
    rng = random.Random(seed)
    for w in extra:
        if w not in have:
            have.add(w)
            words.append(w)
            counts.append(rng.randint(1, 10 ** 9))
    return words, counts


def shape_queries(words, seed=12):
    """Every table word, its near misses and the empty word, shuffled (a near
    miss that is itself a table word -- the prefix chain -- stays in)."""
    q = list(words) + [b""]
    for w in words:
        if len(w) <= 200:
            q += near_misses(w)
        else:  # one near miss of each kind for the 100,000-byte word
            q += near_misses(w)[:4]
    random.Random(seed).shuffle(q)
    return q


def last_is_one_byte():
    """(words, counts): short words whose bytewise-last one, "~", has one byte:
    after sort_result it is the last word of the table's bytes."""
    words = top_cases.names(300) + [b"~"]
    return words, list(range(1, len(words) + 1))


def collide_table(seed=13):
    """(words, counts, queries): 4,000 table words, words over LANE_MAX bytes
    among them, and 2,000 queries, half of them absent."""
    rng = random.Random(seed)
    words = []
    for i in range(4000):
        if i % 10 == 0:
            words.append(b"L%d-" % i + bytes(rng.randrange(97, 123) for _ in range(62 + i % 300)))
        else:
            words.append(b"c%d" % i + b"." * (i % 19))
    counts = [rng.randint(1, 1 << 40) for _ in words]
    present = rng.sample(words, 1000)
    absent = [b"L%d+" % i + bytes(rng.randrange(97, 123) for _ in range(62 + i % 300)) for i in range(0, 1000, 10)]
    absent += absent_words(1000 - len(absent))
    queries = present + absent
    rng.shuffle(queries)
    return words, counts, queries


def fixed_width_queries(n):
    """n distinct 6-byte words as (uint8 matrix [n, 6], offs uint64[n + 1]): "k"
    and five letters a..p, the base-16 digits of the word's number."""
    import numpy as np

    idx = np.arange(n, dtype=np.uint32)
    mat = np.empty((n, 6), dtype=np.uint8)
    mat[:, 0] = ord("k")
    for j in range(5):
        mat[:, 1 + j] = 97 + ((idx >> (4 * j)) & 15)
    return mat, np.arange(n + 1, dtype=np.uint64) * 6


def fixed_width_number(word):
    """The number of a fixed_width_queries word."""
    assert len(word) == 6 and word[:1] == b"k"
    return sum((word[1 + j] - 97) << (4 * j) for j in range(5))
