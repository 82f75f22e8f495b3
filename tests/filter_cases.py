"""Word tables and predicates for the device filter (mox_filter_result,
map-oxidize_amd/csrc/mox_filter.hip) and the expectation they are checked
against: a plain Python filter over the fetched table.  Shared by
test_filter_abi.py (CPU: the constants match the sources, expected() checks
itself) and test_gpu_filter.py (GPU)."""
import random

import lookup_cases
import top_cases
from lookup_cases import NUL_WORDS, PREFIX_CHAIN, last_is_one_byte, near_misses, shape_table, table_words  # noqa: F401
from top_cases import names, word_shapes  # noqa: F401

TILE = 1024        # FL_TILE: table rows per workgroup step, FL_T x FL_PER
PREFIX_MAX = 16    # MOX_FILTER_PREFIX_MAX
LOOKUP_MAX = lookup_cases.LOOKUP_MAX
U64 = (1 << 64) - 1

# table sizes on the wave (64), workgroup (256) and tile edges of the two passes
TABLE_NS = (1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1)
STRIDE_GRID = 2            # MOX_FILTER_GRID for the stride case: two workgroups ...
STRIDE_N = 5 * TILE + 1    # ... over six tiles, the last one of a single word: three strides each
LIST_NS = (1, 64, 65, 1025)
INFO_KEYS = ("words_in", "words_kept", "tokens_in", "tokens_kept", "bytes_kept", "list_found")


def expected(items, min_count=0, max_count=None, min_len=0, max_len=None, prefix=b"", drop=None, keep=None):
    """(kept, info): the (word, count) items that satisfy every term, in order,
    and the info fields mox_filter_result reports for them.  max_count /
    max_len of None or 0: no upper bound (the C struct's rule).  Sums are taken
    modulo 2**64, as the engine's u64 sums are."""
    assert drop is None or keep is None
    listed = set(keep if keep is not None else (drop or []))
    kept = []
    for w, c in items:
        if c < min_count or (max_count and c > max_count):
            continue
        if len(w) < min_len or (max_len and len(w) > max_len):
            continue
        if keep is not None and w not in listed:
            continue
        if drop is not None and w in listed:
            continue
        if not w.startswith(prefix):
            continue
        kept.append((w, c))
    have = {w for w, _ in items}
    info = {
        "words_in": len(items),
        "words_kept": len(kept),
        "tokens_in": sum(c for _, c in items) & U64,
        "tokens_kept": sum(c for _, c in kept) & U64,
        "bytes_kept": sum(len(w) for w, _ in kept),
        "list_found": len(listed & have),
    }
    return kept, info


def random_words(n, seed):
    """n distinct words of 1..30 bytes over a small alphabet (many share their
    first bytes) with counts in 0..40."""
    rng = random.Random(seed)
    words = set()
    while len(words) < n:
        words.add(bytes(rng.choice(b"abcun") for _ in range(rng.randint(1, 30))))
    words = sorted(words)
    rng.shuffle(words)
    return words, [rng.randint(0, 40) for _ in words]


def list_words(words, n, seed):
    """A list of n words: a third present, a third absent, a third duplicates of
    the others (n == 1: one present word)."""
    rng = random.Random(seed)
    present = rng.sample(words, min(len(words), max(1, n // 3)))
    absent = lookup_cases.absent_words(n // 3)
    out = present + absent
    while len(out) < n:
        out.append(rng.choice(present + absent))
    rng.shuffle(out)
    return out[:n]
