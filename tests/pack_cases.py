"""The word list of test_gpu_pack.py: the shapes at which the pieces the
receive-layout packers share (map-oxidize_amd/csrc/mox_pack.h: the short-row
classifier, the per-lane and the whole-wave copy + hash) can go wrong.  The
models it is checked against are accum_cases.oracle_sum and
rekey_cases.expected."""
from accum_cases import is_short, phases

COOP = 256  # AC_COOP / RQ_COOP: a longer long word is copied and hashed by a whole wave
# around the 8- and 16-byte key words and the short / long rule; the per-lane /
# whole-wave boundary; exactly 64 8-byte words of one wave step (505..512 bytes)
# and one word either side; a third wave step
LENGTHS = (1, 7, 8, 9, 15, 16, 17, 23, 24, 25, COOP - 1, COOP, COOP + 1, 504, 511, 512, 513, 520, 1025)
VARIANTS = 16  # words per length: more than one round of a packer tile's 256 threads in all
NUL_WORDS = (b"a\x00b", b"\x00", b"a_long_word_with_a_\x00_inside")
FILLERS = tuple(b"z" * k for k in range(1, 8))  # shift what follows them through the phases of an 8-byte word
LETTERS = b"qwertyuiopasdfghjklzxcvbnm"


def word(n, v):
    """n bytes, NUL-free, distinct per (n, v), no parenthesis."""
    return (b"%c%d_" % (65 + v, n) + LETTERS * (n // len(LETTERS) + 1))[:n]


def table():
    """(words, counts A, counts B): every length VARIANTS times with a filler
    between the groups, the NUL words; counts with zeros on a short and a long
    word in both."""
    words = []
    for v in range(VARIANTS):
        for n in LENGTHS:
            words.append(word(n, v))
        words.append(FILLERS[v % len(FILLERS)] if v < len(FILLERS) else NUL_WORDS[v % len(NUL_WORDS)])
    words = list(dict.fromkeys(words))
    assert set(FILLERS) | set(NUL_WORDS) <= set(words) and b"\x00" not in b"".join(w for w in words if w not in NUL_WORDS)
    assert len(words) == VARIANTS * len(LENGTHS) + len(FILLERS) + len(NUL_WORDS) > 256
    assert not any(w[:1] in b"()" or w[-1:] in b"()" for w in words)
    # in list order, and in bytewise order too, short and long words start at every phase
    for order in (words, sorted(words)):
        s, l = phases(order)
        assert s == l == set(range(8))
    ca = [(i * 2654435761) % 1000 + 1 for i in range(len(words))]
    cb = [(i * 40503) % 77 + 1 for i in range(len(words))]
    for w in (word(8, 0), word(COOP + 1, 0)):
        ca[words.index(w)] = cb[words.index(w)] = 0
    return words, ca, cb


def wrapped(words):
    """Every word in parentheses: trimmed of b"()" it is the word again, one byte into its row."""
    return [b"(" + w + b")" for w in words]


def kinds(words):
    """(short rows, long rows by one lane, long rows by a whole wave)."""
    s = sum(is_short(w) for w in words)
    big = sum(len(w) > COOP for w in words)
    return s, len(words) - s - big, big
