"""Word tables for the device join (mox_join_total,
map-oxidize_amd/csrc/mox_join.hip) and the expectation it is checked against:
a plain Python dict join over the two fetched tables.  Shared by
test_join_abi.py (CPU: the constants match the sources, expected() checks
itself) and test_gpu_join.py (GPU)."""
import random

import filter_cases
import lookup_cases
import top_cases
from lookup_cases import NUL_WORDS, PREFIX_CHAIN, last_is_one_byte, near_misses, shape_table, table_words  # noqa: F401
from top_cases import names  # noqa: F401

TILE = 1024   # WS_TILE (mox_wordset.h): rows per workgroup step of k_jn_build / k_jn_stream, WS_T x WS_PER
U64 = (1 << 64) - 1
assert TILE == filter_cases.TILE == lookup_cases.TILE  # the compaction's and the lookup's tiles are the same rows

# table sizes on the wave (64), workgroup (256) and tile edges of every pass
TABLE_NS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
STRIDE_N = 5 * TILE + 1    # six tiles, the last one of a single row ...
STRIDE_GRID = 2            # ... under MOX_JOIN_GRID=2: three strides of every kernel

MODES = ("semi", "anti")
COUNTS = ("result", "total", "min")
# every info key that is a pure function of the two tables, the mode and the counts value
INFO_KEYS = ("words_in", "words_total", "words_matched", "words_kept", "tokens_in", "tokens_total", "tokens_matched_result",
             "tokens_matched_total", "tokens_min", "tokens_kept", "bytes_kept")


def expected(r_items, t_items, mode="semi", counts="result"):
    """(kept, info): the (word, count) items of the result R that the total T
    holds (mode "semi") or lacks ("anti"), in R's order, with their own count,
    T's ("total") or the smaller of both ("min"), and the info fields
    mox_join_total reports.  Words match as bytes objects do: verbatim, the
    length included.  Sums are taken modulo 2**64, as the engine's are."""
    assert mode in MODES and counts in COUNTS and (mode == "semi" or counts == "result")
    total = {}
    for w, c in t_items:
        assert w not in total, w
        total[w] = c
    kept = []
    matched = tok_r = tok_t = tok_min = 0
    for w, c in r_items:
        held = w in total
        if held:
            matched += 1
            tok_r += c
            tok_t += total[w]
            tok_min += min(c, total[w])
        if held == (mode == "semi"):
            kept.append((w, c if counts == "result" else total[w] if counts == "total" else min(c, total[w])))
    info = {
        "words_in": len(r_items),
        "words_total": len(t_items),
        "words_matched": matched,
        "words_kept": len(kept),
        "tokens_in": sum(c for _, c in r_items) & U64,
        "tokens_total": sum(c for _, c in t_items) & U64,
        "tokens_matched_result": tok_r & U64,
        "tokens_matched_total": tok_t & U64,
        "tokens_min": tok_min & U64,
        "tokens_kept": sum(c for _, c in kept) & U64,
        "bytes_kept": sum(len(w) for w, _ in kept),
    }
    return kept, info


def pair(n_r, n_t, seed):
    """((r_words, r_counts), (t_words, t_counts)): two tables of n_r and n_t
    distinct words of 1..24 bytes that share about a third of the smaller one's
    words (at least one, where both have a word to spare); the shared words
    carry different counts on the two sides, larger on either side in turn."""
    rng = random.Random(seed)
    shared_n = max(1, min(n_r, n_t) // 3)
    shared = [b"s%d" % i + b"_" * (i % 23) for i in range(shared_n)]
    r_only = [b"r%d" % i + b"_" * (i % 23) for i in range(n_r - shared_n)]
    t_only = [b"t%d" % i + b"_" * (i % 23) for i in range(n_t - shared_n)]
    r_words, t_words = shared + r_only, shared + t_only
    rng.shuffle(r_words)
    rng.shuffle(t_words)
    r_counts = {w: rng.randint(1, 1000) for w in r_words}
    t_counts = {w: rng.randint(1, 1000) for w in t_words}
    for i, w in enumerate(shared):  # never equal on a shared word
        t_counts[w] = r_counts[w] + 7 if i % 2 else r_counts[w] // 2
    return (r_words, [r_counts[w] for w in r_words]), (t_words, [t_counts[w] for w in t_words])
