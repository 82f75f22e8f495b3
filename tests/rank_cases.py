"""Count tables for the device ranking (mox_rank_result,
map-oxidize_amd/csrc/mox_rank.hip) and the expectation they are checked
against: Python's stable sorted() over the fetched table.  Shared by
test_rank_abi.py (CPU: the constants match the sources, expected() checks
itself) and test_gpu_rank.py (GPU)."""
import random

from top_cases import names

TILE = 4096        # RK_TILE: table rows per workgroup step, RK_T x RK_STEPS
WAVE_ROWS = 1024   # RK_WROWS: consecutive rows one wave of a tile ranks
TOP_STEP = 1024    # RK_TOP_T: tiles (and chunk sums) per step of the one-workgroup scans
TOP_MAX = 4096     # MOX_TOP_MAX
U64 = (1 << 64) - 1
INFO_KEYS = ("words", "tokens", "max_count", "digit_passes")

# table sizes on the wave (64), workgroup (256) and tile edges of the passes
TABLE_NS = (0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1)
STRIDE_GRID = 4                          # MOX_RANK_GRID for the stride case: four workgroups ...
STRIDE_N = 3 * STRIDE_GRID * TILE + 1    # ... over thirteen tiles, the last one of a single word: four strides for workgroup 0
ZIPF_N = 200000
BIG_CORPUS = 64 << 20                    # bytes of HICARD text whose table has more than TOP_STEP tiles: the scan's carry runs

# (largest count, radix passes it needs): ceil(bitlen / 8)
DIGIT_EDGES = ((0, 0), (1, 1), (255, 1), (256, 2), (65535, 2), (65536, 3), (1 << 32, 5), (1 << 56, 8), (U64, 8))


def passes_of(max_count):
    return (max_count.bit_length() + 7) // 8


def expected(items, ascending=False):
    """The (word, count) items by count, descending unless ``ascending``; equal
    counts in the order they have in ``items`` (sorted() is stable)."""
    return sorted(items, key=(lambda wc: wc[1]) if ascending else (lambda wc: -wc[1]))


def ranked_arrays(counts, offs, data, ascending=False):
    """expected() over a table given as its arrays (Table.arrays()), with numpy:
    (counts, offs, bytes) of the ranked table.  For tables too big for lists."""
    import numpy as np

    order = np.argsort(counts if ascending else ~counts, kind="stable")  # (the complement of a u64 descends, ties in table order)
    lens = np.diff(offs.astype(np.int64))[order]
    new_offs = np.zeros(order.size + 1, dtype=np.uint64)
    np.cumsum(lens, out=new_offs[1:])
    idx = np.repeat(offs[:-1].astype(np.int64)[order] - new_offs[:-1].astype(np.int64), lens) + np.arange(int(new_offs[-1]), dtype=np.int64)
    return counts[order], new_offs, np.frombuffer(data, dtype=np.uint8)[idx].tobytes()


def info_of(items):
    """The info fields mox_rank_result reports for a table (tokens modulo 2**64,
    as the engine sums them; a table of at most one word runs no pass)."""
    m = max((c for _, c in items), default=0)
    return {"words": len(items), "tokens": sum(c for _, c in items) & U64, "max_count": m,
            "digit_passes": passes_of(m) if len(items) > 1 else 0}


def spread_counts(n, values, seed):
    """n counts drawn at random from the few ``values``: wherever the engine
    puts the words, every value then lies on both sides of every wave,
    workgroup and tile boundary (straddles() checks it on the fetched table)."""
    rng = random.Random(seed)
    return [rng.choice(values) for _ in range(n)]


def straddles(items, values):
    """Every full step of 64 consecutive rows of the table holds every value."""
    counts = [c for _, c in items]
    return all(set(counts[i:i + 64]) >= set(values) for i in range(0, len(counts) - 63, 64))


def zipf_counts(n, seed, top=3000000):
    """Zipf-like counts: rank r gets about top / r (many ties in the tail), shuffled; the largest needs three digit passes."""
    counts = [max(1, top // r) for r in range(1, n + 1)]
    random.Random(seed).shuffle(counts)
    return counts


def digit_edge_counts(max_count, n=300, seed=1):
    """n counts of at most max_count, max_count itself and (where it fits) zeros,
    ones and the values around its highest digit among them."""
    rng = random.Random(seed ^ max_count)
    pool = {0, max_count, max_count >> 1, max_count >> 8, max_count // 3, min(1, max_count), max(0, max_count - 1)}
    counts = [rng.choice(sorted(pool)) for _ in range(n - 1)] + [max_count]
    rng.shuffle(counts)
    return counts


def byte7_only(n=600, seed=2):
    """Counts that differ only in byte 7 (bytes 0..6 equal everywhere)."""
    rng = random.Random(seed)
    return [(rng.randrange(1, 256) << 56) | 0x00ABCDEF01234567 for _ in range(n)]


def byte0_only(n=600, seed=3):
    """Counts that differ only in byte 0, with byte 3 set everywhere (four passes, three of them over equal digits)."""
    rng = random.Random(seed)
    return [0x7F000000 | rng.randrange(256) for _ in range(n)]


def table(n, counts):
    assert len(counts) == n
    return names(n), list(counts)
