"""Word tables and keys for the device search of the sorted result
(mox_find_ranges / mox_top_rows, map-oxidize_amd/csrc/mox_find.hip) and the
model they are checked against: Python ``bytes`` comparison -- unsigned bytes,
a proper prefix first, which is Rust String Ord -- and ``bisect`` over the
fetched table.  Shared by test_find_abi.py (CPU: the model against a brute-force
scan, the tables have the shapes they claim) and test_gpu_find.py (GPU)."""
import bisect
import random

TILE = 1024          # FD_TILE: rows per tile of the count sums
FIND_MAX = 1 << 20
U64 = (1 << 64) - 1
EXACT, PREFIX, LOWER = 0, 1, 2
MODES = (("exact", EXACT), ("prefix", PREFIX), ("lower", LOWER))

# table sizes: empty, below / at / past one tile, past two, and six tiles with a one-row last tile
TABLE_NS = (0, 1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 1)
STRIDE_N = 5 * TILE + 1
STRIDE_GRID = 2      # MOX_FIND_GRID for the stride case: two workgroups over six tiles, three strides


def prefix_end(key):
    """The smallest byte string above every string that starts with ``key``; None: there is none."""
    k = key.rstrip(b"\xff")
    return k[:-1] + bytes([k[-1] + 1]) if k else None


def expected(items, keys, mode):
    """(first, last, sums) of ``keys`` against a table given as its (word, count)
    list in bytewise order."""
    words = [w for w, _ in items]
    assert all(a < b for a, b in zip(words, words[1:])), "the table is not in bytewise order"
    pre = [0]
    for _, c in items:
        pre.append((pre[-1] + c) & U64)
    first, last, sums = [], [], []
    for k in keys:
        lo = hi = bisect.bisect_left(words, k)
        if mode == EXACT:
            hi = lo + (lo < len(words) and words[lo] == k)
        elif mode == PREFIX:
            end = prefix_end(k)
            hi = len(words) if end is None else bisect.bisect_left(words, end)
        first.append(lo)
        last.append(hi)
        sums.append((pre[hi] - pre[lo]) & U64)
    return first, last, sums


def brute(items, keys, mode):
    """The same by a scan over every row: the definition, not the search."""
    first, last, sums = [], [], []
    for k in keys:
        lo = sum(1 for w, _ in items if w < k)
        if mode == EXACT:
            rows = [i for i, (w, _) in enumerate(items) if w == k]
        elif mode == PREFIX:
            rows = [i for i, (w, _) in enumerate(items) if w[:len(k)] == k]
        else:
            rows = []
        assert rows == list(range(lo, lo + len(rows))), "a range is contiguous and starts at the lower bound"
        first.append(lo)
        last.append(lo + len(rows))
        sums.append(sum(items[i][1] for i in rows) & U64)
    return first, last, sums


def info_of(first, last):
    return {"queries": len(first), "matched": sum(1 for a, b in zip(first, last) if b > a),
            "rows": sum(b - a for a, b in zip(first, last))}


def holds_tile(first, last):
    """Rows [first, last) contain a whole tile aligned at a multiple of TILE."""
    return last // TILE > (first + TILE - 1) // TILE


def top_of(items, first, last, k):
    """The k most frequent of rows [first, last): count descending, ties by table index."""
    rows = sorted(range(first, last), key=lambda i: (-items[i][1], i))[:k]
    return [items[i] for i in rows]


def neighbours(w):
    """The keys next to w: one byte more, its last byte gone, its last byte one down and one up."""
    out = [w + b"\x00", w + b"a", w[:-1]]
    if w[-1] > 0:
        out.append(w[:-1] + bytes([w[-1] - 1]))
    if w[-1] < 255:
        out.append(w[:-1] + bytes([w[-1] + 1]))
    return out


def keys_around(words, seed=3):
    """Every table word, its neighbours (most of them absent) and the empty key, shuffled."""
    keys = list(words) + [b""]
    for w in words:
        keys += neighbours(w)
    random.Random(seed).shuffle(keys)
    return keys


def table_words(n, seed):
    """n distinct words of 2..30 bytes (short and long rows of the engine mixed,
    bytes over 0x7F among them) with counts below 2^40."""
    rng = random.Random(seed)
    words = [(b"\xc3" if i % 5 == 0 else b"t") + b"%d" % i + b"_" * (i % 24) for i in range(n)]
    return words, [rng.randint(0, 1 << 40) for _ in range(n)]


# ---- compare edges
EDGE_LENS = tuple(range(0, 19)) + (63, 64, 65, 300)
EDGE_BYTES = (0x00, 0x7F, 0x80, 0xFF)
EDGE_POS = (0, 7, 8, 11)  # first, eighth, ninth and last byte of a 12-byte word


def edge_table(seed=5):
    """(words, counts): the chain m, mm, ... over EDGE_LENS (every word a proper
    prefix of the next; reduce_pairs takes no empty word, so length 0 is a key
    only), 12-byte words with each of EDGE_BYTES at each of EDGE_POS, 200-byte
    words that differ only in their last byte, and "ab" / "ab\\0"."""
    words = [b"m" * L for L in EDGE_LENS if L]
    for p in EDGE_POS:
        for v in EDGE_BYTES:
            w = bytearray(b"q" * 12)
            w[p] = v
            words.append(bytes(w))
    words += [b"z" * 199 + bytes([v]) for v in (0x00, 0x01, 0x61, 0x7F, 0x80, 0xFE, 0xFF)]
    words += [b"ab", b"ab\x00", b"\x00", b"\xff", b"\xff\xff"]
    assert len(set(words)) == len(words)
    rng = random.Random(seed)
    return words, [rng.randint(1, 10 ** 12) for _ in words]


def edge_keys(words):
    return keys_around(words) + [b"m" * L for L in EDGE_LENS] + [b"q" * 12, b"q" * 7, b"q" * 8, b"z" * 199, b"z" * 200, b"\xff\xff\xff"]


# ---- sums across the tile logic
def group_table(groups, seed):
    """(words, counts) of a table made of groups (prefix, rows): the group's words
    are the prefix plus a five-digit number, so a prefix's range is its groups'
    rows; counts are any u64."""
    rng = random.Random(seed)
    words = [p + b"%05d" % i for p, rows in groups for i in range(rows)]
    return words, [rng.randint(0, U64) for _ in words]


# "b1" is rows [1, 1023), "cd" [1024, 2048), "c" [1023, 2049), "" everything
TILE_GROUPS_A = ((b"a0", 1), (b"b1", TILE - 2), (b"cc", 1), (b"cd", TILE), (b"ce", 1), (b"zz", 551))
TILE_RANGES_A = ((b"b1", 1, TILE - 1), (b"cd", TILE, 2 * TILE), (b"c", TILE - 1, 2 * TILE + 1), (b"", 0, 2 * TILE + 552),
                 (b"nope", 2 * TILE + 1, 2 * TILE + 1))
# "b" is rows [1000, 1030): across a tile edge, no whole tile
TILE_GROUPS_B = ((b"a", 1000), (b"b", 30), (b"c", 70))
TILE_RANGES_B = ((b"b", 1000, 1030),)

WRAP_COUNTS = (0, 1, U64, U64, 5, 0, U64 - 1)  # inside one prefix range: the sum wraps twice
