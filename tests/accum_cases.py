"""Case tables and models for the device-resident accumulator (mox_accumulate,
map-oxidize_amd/csrc/mox_accum.hip), shared by test_accum_abi.py (CPU: their
shapes, the classification rule, the chunk-cut rule) and test_gpu_accumulate.py
(GPU: every fold exact against `oracle_sum` or coracle)."""
import os

TILE = 1024  # rows per packer tile (AC_TILE, mox_accum.hip)
ASCII_WS = b" \t\n\x0b\x0c\r"


# ---- models
def is_short(word):
    """reduce_pairs_impl's and the packer's rule: a 16-byte key holds the word."""
    return 1 <= len(word) <= 16 and b"\x00" not in word


def oracle_sum(*tables):
    """[(word, count)] sorted bytewise: counts summed mod 2^64, a word of any table
    present (a count of 0 included); and the tokens (the sum of all counts)."""
    d, tok = {}, 0
    for words, counts in tables:
        for w, c in zip(words, counts):
            d[w] = (d.get(w, 0) + c) & ((1 << 64) - 1)
            tok = (tok + c) & ((1 << 64) - 1)
    return sorted(d.items()), tok


def chunk_cuts(data, chunk_bytes):
    """mox_accumulate_file's chunks of `data` as [(lo, hi)]: cut k is the first
    position >= k chunk_bytes that follows an ASCII whitespace byte (or the end);
    equal cuts give no chunk; chunk_bytes 0 or an empty input: one chunk."""
    n = len(data)
    if chunk_bytes == 0 or n == 0:
        return [(0, n)]
    cuts, k = [0], 1
    while k * chunk_bytes < n:
        p = max(k * chunk_bytes, cuts[-1])
        while p < n and data[p - 1] not in ASCII_WS:
            p += 1
        k += 1
        if p >= n:
            break
        if p > cuts[-1]:
            cuts.append(p)
    cuts.append(n)
    return list(zip(cuts[:-1], cuts[1:]))


def phases(words):
    """({start mod 8 of the short words}, {... of the long words}) when the words
    lie one after another, as in a table's bytes."""
    s, l, o = set(), set(), 0
    for w in words:
        (s if is_short(w) else l).add(o % 8)
        o += len(w)
    return s, l


# ---- 1. row-count edges
EDGE_NS = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
# every value once on each side
EDGE_PAIRS = [(EDGE_NS[i], EDGE_NS[(i + 4) % len(EDGE_NS)]) for i in range(len(EDGE_NS))]
OVERLAPS = ["disjoint", "identical", "alternate"]


def gen_word(tag, i):
    """Distinct per (tag, i); 2..15 bytes with a sprinkling of 17..24-byte words."""
    w = b"%s%d" % (tag, i) + b"x" * (i % 7)
    return w + b"_long_tail_" if i % 11 == 5 else w


def gen_count(tag, i):
    return (i * 2654435761 + tag[0]) % 100000 + 1


def edge_tables(na, nb, overlap):
    """(words A, counts A), (words B, counts B) of na / nb distinct rows."""
    wa = [gen_word(b"a", i) for i in range(na)]
    if overlap == "disjoint":
        wb = [gen_word(b"b", i) for i in range(nb)]
    elif overlap == "identical":
        wb = [gen_word(b"a", i) for i in range(nb)]
    else:  # every second word shared
        wb = [gen_word(b"a" if i % 2 == 0 else b"b", i) for i in range(nb)]
    return (wa, [gen_count(b"a", i) for i in range(na)]), (wb, [gen_count(b"b", i) for i in range(nb)])


# ---- 2. word shapes
def len_word(n):
    return (b"%02d" % n + b"qwertyuiopasdfghjklzxcvbnm" * 2)[:n]


W16 = b"sixteen_bytes_ok"
NUL_WORDS = [b"a", b"a\x00", b"a\x00b", b"\x00"]
UTF8_WORDS = ["é".encode(), "日".encode(), "\U0001d11e".encode(), "日本語".encode(),
              "é日\U0001d11eé日".encode(), "σίσυφοςσ".encode(),
              ("日" * 6).encode()]
BIG_WORD = bytes((i * 31 + 7) % 251 + 1 for i in range(100000))  # no NUL byte
LONG_BOTH = b"a_long_word_in_both_tables"
SHORT_BOTH = b"both"


def shape_tables():
    """One pair of tables: lengths 1..40 (A all of them, B the odd ones), the
    16 / 17-byte pair, the NUL words, UTF-8 words of 2, 3 and 4 bytes per
    character, a 100,000-byte word in both, a short and a long word in both."""
    assert len(W16) == 16
    wa = [len_word(n) for n in range(1, 41)] + [W16, W16 + b"!"] + NUL_WORDS + UTF8_WORDS + [BIG_WORD, LONG_BOTH, SHORT_BOTH]
    wb = [len_word(n) for n in range(1, 41, 2)] + [W16 + b"!", NUL_WORDS[1], NUL_WORDS[3]] + UTF8_WORDS[::2] + \
         [SHORT_BOTH, LONG_BOTH, b"only_in_b", BIG_WORD, BIG_WORD[:-1], b"b" * 300]
    return (wa, list(range(1, len(wa) + 1))), (wb, [1000 + 3 * i for i in range(len(wb))])


# a table whose bytewise-last row is a 1-byte word: sorted, its key load runs past the table's bytes
LAST1 = ([b"apple", b"kiwi", b"x" * 20, b"melon", b"z"], [5, 4, 3, 2, 1])
LAST1_OTHER = ([b"kiwi", b"z", b"x" * 20, b"new"], [10, 20, 30, 40])


# ---- 3. counts
def count_tables():
    wa = [b"big", b"zero", b"zf"] + [b"bit%02d" % i for i in range(64)]
    ca = [1 << 63, 0, 0] + [1 << i for i in range(64)]
    wb = [b"big", b"zero", b"zf"] + [b"bit%02d" % i for i in range(64)] + [b"a_long_word_with_count_zero"]
    cb = [(1 << 63) - 1, 0, 5] + [1 << ((i + 1) % 64) for i in range(64)] + [0]
    return (wa, ca), (wb, cb)


# ---- 4 / 5. corpora
def mixed_text(n, seed, ascii_only=False):
    """Zipf text (dictionary words) with Unicode-lane words and long words mixed in."""
    from mox import corpus
    z = corpus.fill(corpus.ZIPF, seed, 0, n).tobytes()
    u = b"" if ascii_only else corpus.fill(corpus.UNICODE, seed + 1, 0, n // 8).tobytes().decode("utf-8", "ignore").encode()
    extra = b" ".join(b"Supercalifragilistic%dexpialidocious" % (i % 37) for i in range(300))
    return z[: n // 2] + b" " + u + b"\n" + extra + b" " + z[n // 2:]


def ws_windows(data, k):
    """k + 1 cut positions of `data` at ASCII whitespace (each after a delimiter)."""
    cuts = [0]
    for j in range(1, k):
        p = max(cuts[-1], len(data) * j // k)
        while p < len(data) and data[p - 1] not in ASCII_WS:
            p += 1
        cuts.append(p)
    cuts.append(len(data))
    return cuts


# ---- 9 / 10. bigger tables
def half_shared(n, seed=0):
    """Two tables of n distinct words each, half of them shared."""
    wa = [b"g%d_%d" % (seed, i) for i in range(n)]
    wb = [b"g%d_%d" % (seed, i + n // 2) for i in range(n)]
    return (wa, [i % 1000 + 1 for i in range(n)]), (wb, [i % 77 + 1 for i in range(n)])


def long_tables(n=300):
    """n distinct long words per side (none shared) plus a few shared ones."""
    wa = [b"left_side_long_word_number_%05d" % i for i in range(n)] + [LONG_BOTH]
    wb = [b"right_side_long_word_number_%05d" % i for i in range(n)] + [LONG_BOTH]
    return (wa, list(range(1, n + 2))), (wb, list(range(7, n + 8)))


# ---- GPU helpers (an engine in, plain lists out), shared with the check-build children
def fetched(e):
    t = e.fetch()
    try:
        return list(t.items()), t.tokens
    finally:
        t.close()


def load(e, table):
    """The table becomes the engine's device-resident result (mox_reduce_pairs)."""
    e.reduce_pairs(table[0], table[1]).close()


def fold_tables(e, *tables):
    """Every table loaded and folded in turn; the total as (sorted items, tokens)."""
    for t in tables:
        load(e, t)
        e.accumulate()
    items, tok = fetched(e)
    return sorted(items), tok


def data_path(tmp, name, data):
    p = os.path.join(str(tmp), name)
    with open(p, "wb") as f:
        f.write(data)
    return p
