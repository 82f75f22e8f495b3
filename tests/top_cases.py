"""Word tables for the device top-k (map-oxidize_amd/csrc/mox_topk.hip,
mox_top_words) and the expectation they are checked against: the first k of
the fetched table by (count descending, table index ascending), which is the
rule of mox_print_top_words.  Shared by test_top_words_abi.py (CPU: the
constants match the sources, the generators have the shape they claim) and
test_gpu_top_words.py (GPU)."""
import random

TILE = 4096     # TK_TILE: the tie-count tile (one wave ranks 64 x 64 consecutive indices)
TOP_MAX = 4096  # MOX_TOP_MAX
U64 = (1 << 64) - 1

# n on the wave (64), workgroup (256) and tile edges of the selection kernels
EDGE_NS = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


def expected(items, k):
    """The top k of a table given as its (word, count) list in table order."""
    return [wc for _, wc in sorted(enumerate(items), key=lambda t: (-t[1][1], t[0]))[:k]]


def names(n, tag=b"w"):
    """n distinct short words."""
    return [tag + b"%d" % i for i in range(n)]


def distinct(n, seed):
    """n short words with the distinct counts 1..n, shuffled."""
    counts = list(range(1, n + 1))
    random.Random(seed).shuffle(counts)
    return names(n), counts


def all_ones(n):
    return names(n), [1] * n


def sparse_ties(seed=4):
    """40,000 words: 3 above 7, 1,000 with count exactly 7, the rest 1.  Where
    the sevens lie in the table is the engine's business (hash order): they
    spread over all ten tiles."""
    n = 40000
    counts = [1] * n
    pos = random.Random(seed).sample(range(n), 1003)
    for p in pos[:1000]:
        counts[p] = 7
    for j, p in enumerate(pos[1000:]):
        counts[p] = 1000 + j
    return names(n), counts


def every_bit():
    """128 words with counts 1 << b and (1 << b) + 1 (2**63 among them; 2**64 - 1
    replaces the second 2, which b = 0 and b = 1 would both give)."""
    counts = []
    for b in range(64):
        counts += [1 << b, (1 << b) + 1]
    assert counts[1] == 2 == counts[2]
    counts[1] = U64
    return names(128), counts


def last_digit():
    return names(256), [0xFFFFFFFFFFFFFF00 + j for j in range(256)]


def first_digit():
    return names(255), [j << 56 for j in range(1, 256)]


def word_shapes(seed=6):
    """(words, counts, winners): 3,000 words whose 64 most frequent are lengths
    1..40 (byte offsets of every alignment), non-ASCII words, words far over
    16 bytes, and a 100,000-byte word with a 1-byte word as its neighbour in
    the ranking."""
    rng = random.Random(seed)
    winners = [bytes([97 + (L % 26)]) * L for L in range(2, 41)]  # lengths 2..40
    winners += ["żółć".encode(), "ΣΊΣΥΦΟΣ".encode(), "日本語".encode(), "naïve-café".encode(), b"\xf0\x9f\x98\x80" * 5]
    winners += [b"L" * 100 + b"%d" % i for i in range(17)]
    big = bytes(rng.randrange(33, 127) for _ in range(100000))
    winners += [big, b"Q"]  # adjacent ranks: a 100,000-byte word, then a 1-byte word
    winners.append(b"x" * 17)
    assert len(winners) == 64 and len(set(winners)) == 64
    rest = names(3000 - 64, b"r")
    words = winners + rest
    counts = [10 ** 6 - i for i in range(64)] + [1 + (i % 50) for i in range(len(rest))]
    order = list(range(len(words)))
    rng.shuffle(order)
    return [words[i] for i in order], [counts[i] for i in order], winners


def many_equal(seed=7):
    """6,000 short words, counts in 1..5: every top-50 is decided by the tie order."""
    rng = random.Random(seed)
    words = sorted({bytes(rng.choice(b"abcdefghijklmnop") for _ in range(rng.randint(1, 12))) for _ in range(7000)})[:6000]
    rng.shuffle(words)
    return words, [rng.randint(1, 5) for _ in words]
