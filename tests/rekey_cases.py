"""Word tables and specs for the device re-keying (mox_rekey_result,
map-oxidize_amd/csrc/mox_rekey.hip) and the expectation they are checked
against: a plain Python model of include/mox.h's rules over the fetched table.
Shared by test_rekey_abi.py (CPU: the constants match the sources, the model
checks itself) and test_gpu_rekey.py (GPU)."""
import string

from accum_cases import BIG_WORD, fetched, is_short, load  # noqa: F401

TILE = 1024  # RQ_TILE: table rows per workgroup step, RQ_T x RQ_PER
COOP = 256   # RQ_COOP: a longer long window is copied by a whole wave
U64 = (1 << 64) - 1
PUNCT = string.punctuation.encode()
PUNCT_MASKS = (0xFC00FFFE00000000, 0x78000001F8000001)  # MOX_REKEY_PUNCT_LO / _HI

EDGE_NS = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
STRIDE_GRID = 3          # MOX_REKEY_GRID for the stride case: three workgroups ...
STRIDE_N = 5 * TILE      # ... over five tiles: two strides for two of them
RUNS = (0, 1, 7, 8, 9)   # stripped bytes at either end: none, one, around one 8-byte word
INFO_KEYS = ("words_in", "words_out", "words_changed", "words_dropped", "tokens_in", "tokens_out", "tokens_dropped", "bytes_out")


# ---- the model
def masks_of(chars):
    """The two 64-bit set words of ASCII bytes (mox_rekey.trim_set)."""
    m = [0, 0]
    for b in bytes(chars):
        assert b < 128
        m[b >> 6] |= 1 << (b & 63)
    return tuple(m)


def window(word, strip, max_chars=0):
    """The re-keyed word: bytes of `strip` (a set of values < 128) dropped from
    the front, then from the back; then cut before the (max_chars + 1)-th
    character start (a byte b with b & 0xC0 != 0x80)."""
    s, e = 0, len(word)
    while s < e and word[s] < 128 and word[s] in strip:
        s += 1
    while e > s and word[e - 1] < 128 and word[e - 1] in strip:
        e -= 1
    if max_chars:
        starts = 0
        for p in range(s, e):
            if word[p] & 0xC0 != 0x80:
                if starts == max_chars:
                    e = p
                    break
                starts += 1
    return word[s:e]


def expected(items, trim=b"", punct=False, max_chars=0, tokens=None):
    """(table, rows, info) for the (word, count) items of a fetched table, in
    table order.  rows: the windowed rows that survive, unmerged, in order (what
    mox_reduce_pairs is given by the order contract).  table: the rows summed by
    word mod 2^64, first occurrence first -- or the items themselves, order
    included, when no window differs from its word.  info: the mox_rekey_info
    fields but ms and device_bytes.  tokens: the source's (default: the sum of
    its counts)."""
    strip = set(bytes(trim)) | (set(PUNCT) if punct else set())
    assert all(b < 128 for b in strip)
    tokens_in = (sum(c for _, c in items) & U64) if tokens is None else tokens
    rows, changed, dropped, tdrop = [], 0, 0, 0
    for w, c in items:
        x = window(w, strip, max_chars)
        changed += x != w or not x
        if not x:
            dropped += 1
            tdrop = (tdrop + c) & U64
        else:
            rows.append((x, c))
    if changed:
        d = {}
        for w, c in rows:
            d[w] = (d.get(w, 0) + c) & U64
        table = list(d.items())
    else:
        table = list(items)
    info = {
        "words_in": len(items),
        "words_out": len(table),
        "words_changed": changed,
        "words_dropped": dropped,
        "tokens_in": tokens_in,
        "tokens_out": (tokens_in - tdrop) & U64,
        "tokens_dropped": tdrop,
        "bytes_out": sum(len(w) for w, _ in table),
    }
    return table, rows, info


# ---- tables
def edge_table(n):
    """n distinct rows: every third word carries a trailing "," and its bare form
    is present too (the row before it), a few words are longer than 16 bytes."""
    words = []
    for i in range(n):
        if i % 3 == 2:
            words.append(words[i - 1] + b",")
        else:
            w = b"w%d" % i + b"y" * (i % 5)
            words.append(w + b"_a_tail_past_16_bytes" if i % 13 == 4 else w)
    return words, [(i * 2654435761) % 1000 + 1 for i in range(n)]


def body(n, tag=b""):
    """n bytes of letters and digits, distinct per (n, tag)."""
    return (tag + b"%03d" % n + b"qwertyuiopasdfghjklzxcvbnm" * (n // 26 + 1))[:n] if n >= len(tag) + 3 else (tag + b"qwe")[:n]


def run_table():
    """Lead and trail runs of RUNS stripped bytes around bodies of 1, 5, 16, 17 and
    300 bytes (short, long and wave-copied windows)."""
    words = []
    for lead in RUNS:
        for trail in RUNS:
            for n in (1, 5, 16, 17, 300):
                words.append(b"(" * lead + body(n) + b")" * trail)
    return words, list(range(1, len(words) + 1))


def phase_table():
    """Leads of 0..8 in front of bodies of 2..41 bytes: sorted bytewise and laid
    one after another the words start at every offset mod 8 with every lead
    (phase_cover checks it)."""
    words = []
    for lead in range(9):
        for n in range(2, 42):
            words.append(b"-" * lead + body(n, b"%d" % lead) + b"." * (n % 3))
    assert len(set(words)) == len(words)
    return words, [3 * i + 1 for i in range(len(words))]


def phase_cover(words, lead_byte=b"-"):
    """{(start mod 8, lead)} of words laid one after another."""
    out, o = set(), 0
    for w in words:
        out.add((o % 8, len(w) - len(w.lstrip(lead_byte))))
        o += len(w)
    return out


UTF8 = ["é", "日", "\U0001d11e", "日本語", "σίσυφος", "é日\U0001d11eé日"]


def shape_table():
    """Everything else of the window-shape case."""
    words = []
    # windowed lengths 15, 16, 17 reached from longer words (long -> short, long -> long)
    for n in (15, 16, 17):
        words += [b"((" + body(n) + b"))", b"<<<<<<<<<" + body(n, b"x")]
    # 16-byte words whose window is the word; one with punctuation inside only
    words += [body(16, b"u"), b"in.ner-punct'16b", b"don't", b"a.b"]
    # a NUL inside the window: short by length, long by the rule
    words += [b"(a\x00b)", b"a\x00b,", b"\x00", b"(\x00)", b"." * 9 + b"nul\x00" + b"x" * 20 + b"!"]
    # all punctuation: dropped
    words += [b"!", b"-" * 16, b"-" * 15 + b"!!", b"#" * 300]
    # UTF-8 with punctuation around, and the corpus vocabulary's two
    for u in UTF8:
        words += [u.encode(), b"(" + u.encode() + b")", u.encode() + b"...", b"\"" + u.encode()]
    words += ["Σ.".encode(), "Σ".encode(), "Привет,".encode(), "Привет".encode(), "¿qué?".encode(), "«x»".encode()]
    # 100,000 bytes: the wave path, merging with the bare form; and one of dashes alone
    words += [b"(" + BIG_WORD + b")", BIG_WORD, b"-" * 100000]
    assert len(set(words)) == len(words)
    return words, [7 * i + 2 for i in range(len(words))]


def last_is_one_byte():
    """Short words whose bytewise-last one, "~", has one byte, and "}~" before
    it: after sort_result "~" is the last byte of the table, and the trailing
    walk of "}~" ends at the table's last but one."""
    words = [b"n%03d" % i for i in range(300)] + [b"}~", b"~", b"|x"]
    return words, list(range(1, len(words) + 1))


def merge_table():
    the = [b"the", b"the,", b"(the)", b"the."]
    long20 = b"a_word_of_20_bytes_x"
    assert len(long20) == 20
    lng = [long20, long20 + b",", b"(" + long20 + b")", long20 + b"."]
    zero = [b"zz", b"zz,", b"zf", b"zf!", b"...", b"z_long_word_with_count_0", b"z_long_word_with_count_0;"]
    wrap = [b"wrap", b"wrap?", b"a_long_word_that_wraps", b"[a_long_word_that_wraps]"]
    words = the + lng + zero + wrap
    counts = [10, 20, 30, 40, 1, 2, 3, 4, 0, 0, 0, 5, 0, 0, 0, U64, 2, (1 << 63) + 5, 1 << 63]
    return words, counts


def cap_table():
    """Words for the cap: ASCII, 2-, 3- and 4-byte characters, 20-character ASCII
    words, words that begin with continuation bytes, punctuation in front."""
    words = [b"a", b"ab", b"abc", b"b", b"bcd", "é".encode(), "éa".encode(), "éé".encode(), "日".encode(), "日本語".encode(),
             "日x".encode(), "\U0001d11e".encode(), "\U0001d11e\U0001d11e".encode(), "\U0001d11ez".encode()]
    words += [b"%c" % (97 + i % 26) + b"twenty_chars_%06d" % i for i in range(40)]  # 20 bytes each
    words += [b"\x80", b"\x80\x80a", b"\x80\x80ab", b"\xbf\x80" + "日本".encode(), b"\x80" * 20, b"\x80" * 17 + b"xy"]
    words += [b"(abc)", b"((b", b"a.b.c", "«é»".encode(), b"(" + "日本語".encode() + b"!)"]
    assert len(set(words)) == len(words)
    return words, [i + 1 for i in range(len(words))]


def plain_words(n, seed=0):
    """n distinct words of letters, digits and inner punctuation only: nothing to trim."""
    return [b"p%d" % seed + b"%d" % i + b"'x" * (i % 3) + b"_long_tail_x" * (i % 7 == 0) for i in range(n)], [(i * 7919) % 50 for i in range(n)]
