"""Deterministic word tables for the device bytewise sort (mox_bsort.hip),
shared by the CPU geometry tests (test_bsort_model.py) and the GPU tests
(test_gpu_bsort.py).  Every generator returns a list of distinct non-empty
bytes in no particular order; the expected result is always sorted(words).

Each table is built to put a tie run, a table size or a block of output bytes
on one edge of the kernels (the constants below restate the kernels').  The CPU
tests assert that geometry with the level model, so that a GPU test cannot
pass while missing the branch it is there for."""
import random

WIN = 7            # window bytes per level
SEG_CH = 2048      # k_bs_segsort: subset records per chunk
SEG_MAX = 64       # ... longest run it sorts itself
RUN_LMAX = 4096    # k_bs_longsort: longest run; a longer one needs the checked mode's radix
OS_TILE = 4096     # k_os_pass: records per tile
OUT_BLOCK = 256    # k_bs_out2: sorted words per block
OUT_STAGE = 16384  # ... bytes of its LDS stage

# wave and tile edges, odd sizes, one and two tiles +- 1
SIZE_NS = (2, 3, 63, 64, 65, 255, 256, 257, OS_TILE - 1, OS_TILE, OS_TILE + 1, 2 * OS_TILE - 1, 2 * OS_TILE, 2 * OS_TILE + 1)


def pref(g):
    """7 bytes, base 26 big-endian in g: groups sort in g order, and a group's
    words tie on the whole level-0 window."""
    out = bytearray(WIN)
    for j in range(WIN - 1, -1, -1):
        out[j] = 97 + g % 26
        g //= 26
    assert g == 0
    return bytes(out)


def _tail(k):
    """Tail k of a group: k in base 8 over b"abcdefgh", padded with b"a" to
    1 + 5 k mod 8 bytes (or as long as k needs).  Distinct for distinct k; the
    8-byte tails (k = 3 mod 8) differ within their first 7 bytes, so none tie
    on the level-1 window."""
    want = 1 + (5 * k) % 8
    digits = []  # least significant first
    while k or not digits:
        digits.append(k % 8)
        k //= 8
    digits += [0] * (want - len(digits))
    assert len(digits) <= 8
    return bytes(97 + d for d in reversed(digits))


def group(p, L):
    """L distinct words p + a 1-8-byte tail over b"abcdefgh": one tie run of L
    records at the level after p.  A group longer than SEG_MAX ends with two
    8-byte tails that share 7 bytes, i.e. one run of 2 a level further down."""
    tails = [_tail(k) for k in range(L)]
    if L > SEG_MAX:
        tails[-2:] = [b"hhhhhhha", b"hhhhhhhb"]
    return [p + t for t in tails]


def shuffled(words, seed=1):
    out = list(words)
    random.Random(seed).shuffle(out)
    return out


def sizes(n):
    """n words of 1-12 bytes over an alphabet with the extreme byte values."""
    rng = random.Random(1000 + n)
    alphabet = b"\x00\x7f\x80\xffab"
    words = set()
    while len(words) < n:
        words.add(bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 12))))
    return shuffled(sorted(words), n)


RUN_LENGTHS = [2] * 1000 + [47, SEG_MAX, SEG_MAX + 1] + [2] * 900 + [130, RUN_LMAX, 3]


def run_geometry(longest=RUN_LMAX):
    """Groups of RUN_LENGTHS in this order, 100 bare 7-byte prefixes (length
    class 7: never tied) and 21 3-byte words.  Level 1's subset then holds the
    SEG_MAX run from position 2,047 across the first SEG_CH boundary, the
    130-run from 3,976 across the second, and the RUN_LMAX run from 4,106."""
    lens = [longest if L == RUN_LMAX else L for L in RUN_LENGTHS]
    words = []
    for g, L in enumerate(lens):
        words += group(pref(g), L)
    words += [pref(g) for g in range(0, 2000, 20)]
    words += [pref(g * 26 ** 4)[:3] for g in range(21)]
    return shuffled(words, 2)


def run_geometry_over():
    """run_geometry() with one run of RUN_LMAX + 1: the unchecked mode gives up
    (-1) and the checked mode radix-sorts level 1's subset."""
    return run_geometry(RUN_LMAX + 1)


def run_digits(pairs):
    """`pairs` runs of 2 and one of 5,000 (> RUN_LMAX): the checked mode's radix
    sorts level 1's subset on 8 key digits and the bytes of run ids up to
    pairs + 2."""
    words = []
    for g in range(pairs):
        p = pref(g)
        words += [p + b"a", p + b"b"]
    words += group(pref(pairs), 5000)
    return shuffled(words, 3)


def out_stage():
    """(a) one block of 256 x 64 bytes = OUT_STAGE exactly (staged), (b) the
    same with one word of 65 bytes (OUT_STAGE + 1: byte by byte), (c) 517 words
    of 1-7 bytes (written from their level-0 key) before 764 words of 100-300
    bytes that start with 0xff (from the table): sorted blocks 0-1 are staged
    in-key words, block 2 holds 5 in-key and 251 table words and is not staged,
    blocks 3-4 are unstaged table words and block 5 is the single last word."""
    rng = random.Random(5)
    a = [bytes([65 + i // 16, 65 + i % 16]) + bytes(rng.choice(b"xyz\x80") for _ in range(62)) for i in range(OUT_BLOCK)]
    b = list(a)
    b[128] += b"!"
    alphabet = b"abc\x00\x7f\x80"
    short = set()
    while len(short) < 2 * OUT_BLOCK + 5:
        short.add(bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 7))))
    long_ = []
    for i in range(3 * OUT_BLOCK - 5 + 1):
        body = b"\xff" + b"L" * 20 + bytes([65 + i // 26, 97 + i % 26])
        n = 100 + (37 * i) % 201
        long_.append(body + bytes(rng.choice(b"mno\xfe") for _ in range(n - len(body))))
    c = sorted(short) + long_
    assert len(c) % OUT_BLOCK == 1
    return shuffled(a, 6), shuffled(b, 7), shuffled(c, 8)


DEEP_PREFIX = b"deeptie" * 5  # 35 bytes = 5 windows


def deep_ties():
    """Proper-prefix pairs whose lengths sit on the window (7 k) and record
    (8 = window + length class) edges, and a family identical over 35 bytes
    that differs from byte 36 on: tied through levels 0-4, settled at level 5,
    so the level rings (level & 3) wrap.  Every word longer than 16 bytes is
    tied at least through level 1: the reduce lays such words out last, so the
    table's last word reads its deeper windows at the very end of the byte
    buffer (its 64 bytes of slack)."""
    words = [b"a", b"zz", b"m\x00", b"\xff"]
    for i, (a, b) in enumerate([(7, 8), (8, 9), (14, 15), (21, 22), (22, 23)]):
        base = (bytes([80 + i]) + b"proper-prefix-pair-words")[:b]
        assert len(base) == b
        words += [base[:a], base]
    P = DEEP_PREFIX
    words += [P, P + b"\x00", P + b"a", P + b"ab", P + b"a" * 7, P + b"b", P + b"b" * 20, P + b"\xff"]
    words += [P + bytes([x, y]) for x in b"cdefgh" for y in b"\x01z"]
    assert len(set(words)) == len(words)
    return shuffled(words, 9)


def block_spans(words):
    """(first byte, end byte) of every k_bs_out2 block of the sorted table."""
    offs = [0]
    for w in sorted(words):
        offs.append(offs[-1] + len(w))
    n = len(words)
    return [(offs[j], offs[min(j + OUT_BLOCK, n)]) for j in range(0, n, OUT_BLOCK)]


def staged(span):
    """k_bs_out2's test: the block, from the 16-byte line below its first byte, fits the stage."""
    return span[1] - (span[0] & ~15) <= OUT_STAGE
