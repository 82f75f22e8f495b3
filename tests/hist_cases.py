"""The model of the device histograms (mox_hist_result,
map-oxidize_amd/csrc/mox_hist.hip) -- the four keys in plain Python and the
bins of a table -- and the case tables they are checked on.  Shared by
test_hist_abi.py (CPU: the constants match the sources, expected() checks
itself) and test_gpu_hist.py (GPU)."""
import rank_cases

TILE = 4096        # HG_TILE: rows (and sorted positions) per workgroup step, HG_T x HG_ROUNDS
ROUND = 256        # HG_T: consecutive rows of one round of a tile
TOP_STEP = 1024    # HG_TOP_T: tiles per step of the one-workgroup scan
LANE_MAX = 64      # HG_LANE_MAX: a longer word's characters are counted by a whole wave
U64 = (1 << 64) - 1
COUNT, BYTES, CHARS, FIRST = 0, 1, 2, 3  # MOX_HIST_*
RANGE = 1                                # MOX_HIST_RANGE
MAX_WORDS = (1 << 32) - 1                # MOX_HIST_MAX_WORDS
KEYS = ("count", "bytes", "chars", "first")
INFO_KEYS = ("words", "tokens", "bins", "max_key", "digit_passes")

# table sizes on the wave (64), workgroup (256) and tile edges of the passes
TABLE_NS = (0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1)
STRIDE_GRID = 4                          # MOX_HIST_GRID for the stride case: four workgroups ...
STRIDE_N = 3 * STRIDE_GRID * TILE + 1    # ... over thirteen tiles, the last one of a single row


def is_cont(b):
    return (b & 0xC0) == 0x80


def key_count(word, count):
    return count


def key_bytes(word, count):
    return len(word)


def key_chars(word, count):
    """Character starts: bytes that are no continuation byte (mox_rekey_result's rule)."""
    return sum(1 for b in word if not is_cont(b))


def first_window(word):
    """The word's first byte and the continuation bytes behind it, at most 4 bytes in all."""
    n = min(1, len(word))
    while n and n < min(4, len(word)) and is_cont(word[n]):
        n += 1
    return word[:n]


def key_first(word, count):
    w = first_window(word)
    return (int.from_bytes(w.ljust(4, b"\0"), "big") << 8) | len(w)


KEY_FNS = {"count": key_count, "bytes": key_bytes, "chars": key_chars, "first": key_first}


def expected(items, key, first=None, n=None):
    """[(key, words, tokens & U64, first_row)] ascending by key for the (word,
    count) items in table order; first / n: only rows [first, first + n),
    first_row staying an index into the whole table."""
    fn = KEY_FNS[key]
    lo = 0 if first is None else min(first, len(items))
    hi = len(items) if n is None else min(len(items), lo + n)
    bins = {}
    for row in range(lo, hi):
        w, c = items[row]
        b = bins.setdefault(fn(w, c), [0, 0, row])
        b[0] += 1
        b[1] = (b[1] + c) & U64
    return [(k, b[0], b[1], b[2]) for k, b in sorted(bins.items())]


def info_of(want):
    """The info fields mox_hist_result reports for expected()'s bins."""
    m = max((k for k, _, _, _ in want), default=0)
    return {"words": sum(b[1] for b in want), "tokens": sum(b[2] for b in want) & U64, "bins": len(want), "max_key": m,
            "digit_passes": rank_cases.passes_of(m)}


# ---- word shapes: what the three word keys can get wrong
TWO_BYTE_BIG = "é".encode() * 50000                    # 100,000 bytes, 50,000 characters: the wave path
FIRST_WORDS = [b"a", "é".encode(), "€".encode(), "😀".encode(), b"\x80\x80a", b"\x80" * 5,
               b"ab", "éa".encode(), "€uro".encode(), "😀!".encode(), b"\xbf", b"\x80a", b"a\x80\x80\x80\x80",
               b"\xf0\x9f", b"\xe2\x82", b"nul\x00in", b"\x00", b"\x00\x80"]


def utf8_words():
    """Words whose first character is 1, 2, 3 and 4 bytes long, words that open
    with continuation bytes, a word containing NUL, words whose characters
    straddle the 8-byte steps of the count and the 64-byte lane / wave edge,
    and the 100,000-byte word of 2-byte characters."""
    words = list(FIRST_WORDS)
    for lead in (b"", b"x", b"xx", b"xxx", b"xxxxxxx"):    # a 2-, 3- and 4-byte character across every 8-byte edge
        for ch in ("é", "€", "😀"):
            for reps in (2, 5, 8, 16, 21, 33):
                words.append(lead + ch.encode() * reps)
    words += [b"z" * 56 + "€".encode() * 2 + b"zz", b"z" * 61 + "€".encode(), b"z" * 62 + "€".encode(), TWO_BYTE_BIG,
              b"\x80" * 64, b"\x80" * 65, b"\xc3" * 63 + b"\xa9"]
    words = list(dict.fromkeys(words))
    return words, [3 * i + 1 for i in range(len(words))]
