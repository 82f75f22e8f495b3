"""Corpora that land on the unit cut-offs of the reduce half of the pass
(map-oxidize_amd/csrc/mox_kernels.hip: k_split_count .. k_reduce_sort2), built
from words with chosen key hashes.  No GPU code runs here: test_reduce_model.py
checks on the CPU that every case has the geometry it claims, and
test_gpu_reduce_edges.py runs the cases on the device.

The lever: hash32 = max(hash_fin(hash_fold(k0..k3)), 1), hash_fin is a
bijection (multiply by an odd constant, a ^= a >> 16) and hash_fold is
k0 ^ k1 * 0x85EBCA77 ^ rotl(k2, 21) ^ rotl(k3, 6).  For a word of at most 8
bytes k2 = k3 = 0, so for any target hash and any bytes 4..7, bytes 0..3
follow; about 0.5 % of the choices give four printable non-uppercase ASCII
bytes (words_for).

The cut-offs come from mox_internal.h and mox_kernels.hip by parsing (K): a
change there fails test_reduce_model.py instead of moving the cases off their
edges in silence.  The hash functions and the list rule of k_split_scatter are
restated here; the device table order (test_gpu_reduce_edges.py, model_order)
checks the restated hashes bit for bit."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "map-oxidize_amd", "csrc")
U32 = np.uint32
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- constants
def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _parse(text, name):
    """The integer value of `constexpr T NAME = <expr>;` or `#define NAME <int>`
    (an expression may name other constants of the same file)."""
    m = re.search(r"^\s*constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text, re.M)
    if not m:
        m = re.search(r"^\s*#\s*define\s+%s\s+(\S+)\s*(?://.*)?$" % name, text, re.M)
    if not m:
        raise KeyError("constant %s not found" % name)
    expr = re.sub(r"\b(\d+)(?:u|ull|ul)\b", r"\1", m.group(1).strip())
    expr = re.sub(r"\(\s*(?:u?int\d+_t|int|size_t)\s*\)", "", expr)
    names = set(re.findall(r"[A-Za-z_]\w*", expr))
    env = {n: _parse(text, n) for n in names}
    return int(eval(expr, {"__builtins__": {}}, env))  # noqa: S307 (arithmetic over parsed integers only)


class K:
    """The cut-offs of the reduce path, parsed from the sources."""
    _h, _k = _source("mox_internal.h"), _source("mox_kernels.hip")
    NB_LOG2 = _parse(_h, "NB_LOG2")
    NB = 1 << NB_LOG2
    SPLIT_MIN = _parse(_h, "SPLIT_MIN")
    SPLIT_TARGET = _parse(_h, "SPLIT_TARGET")
    SMALL_CAP = _parse(_h, "SMALL_CAP")
    RED_CAP = _parse(_h, "RED_CAP")
    RED_BK = _parse(_h, "RED_BK")
    RED_SORTB = _parse(_h, "RED_SORTB")
    SUB_BITS_MAX = _parse(_h, "SUB_BITS_MAX")
    QF_MAX = _parse(_h, "QF_MAX")
    PAY = _parse(_h, "PAY")
    MAX_MAP_GRID = _parse(_h, "MAX_MAP_GRID")
    DICT_SLOTS = _parse(_h, "DICT_SLOTS")
    SR_TSLOTS = _parse(_k, "SR_TSLOTS")
    SR_BIN_BITS = _parse(_k, "SR_BIN_BITS")
    DICT_MIN_COVER_INV = _parse(_k, "DICT_MIN_COVER_INV")
    HASH_FIN1 = _parse(_k, "MOX_HASH_FIN1")
    SAMPLE_PIECE = _parse(_h, "SAMPLE_PIECE")
    SAMPLE_PIECES = int(re.search(r"\bsample_pieces = (\d+);", _source("mox_host.h")).group(1))  # an engine's default


RED_BIN_BITS = 11  # red_bin: the RED_SORTB-way split of the 11 bits below `shift`
GRID = 256         # map workgroups on an MI355X (one per CU): the region model below
# reserve_bytes the GPU tests pass: initial_caps gives max(64, n / (grid * NB * 8)) records per region
RESERVE = 256 << 20
COLD_CAP = max(64, RESERVE // (GRID * K.NB * 8))


# ---------------------------------------------------------------- hash model
FIN_MUL, FOLD_MUL = 0x9E3779B1, 0x85EBCA77
FIN_INV = pow(FIN_MUL, -1, 1 << 32)


def _u32(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64)).astype(U32)  # (1-d: numpy scalars warn when they wrap)


def _rotl(x, r):
    x = _u32(x)
    return (x << U32(r)) | (x >> U32(32 - r))


def hash_fold(k0, k1, k2, k3):
    return _u32(k0) ^ (_u32(k1) * U32(FOLD_MUL)) ^ _rotl(k2, 21) ^ _rotl(k3, 6)


def hash_fin(a):
    a = _u32(a) * U32(FIN_MUL)
    return a ^ (a >> U32(16))


def hash_unfin(h):
    """hash_fin's inverse."""
    h = _u32(h)
    return (h ^ (h >> U32(16))) * U32(FIN_INV)


def hash_raw(k0, k1, k2, k3):
    """hash32 before its clamp (k_map's hash32_map)."""
    return hash_fin(hash_fold(k0, k1, k2, k3))


def hash32(k0, k1, k2, k3):
    return np.maximum(hash_raw(k0, k1, k2, k3), U32(1))


def hash32b(k0, k1, k2, k3):
    a = _u32(k1) ^ (_u32(k0) * U32(0x2127599B)) ^ (_u32(k3) * U32(0x165667B1)) ^ (_u32(k2) * U32(0xD3A2646D))
    a = a * U32(0x2C1B3C6D)
    a = a ^ (a >> U32(12))
    a = a * U32(0x297A2D39)
    return a ^ (a >> U32(15))


def pack(words):
    """Keys of short words: each word zero-padded to 16 bytes, as four
    little-endian dwords; an (n, 4) uint32 array."""
    buf = np.zeros((len(words), 16), np.uint8)
    for i, w in enumerate(words):
        if not 0 < len(w) <= 16 or b"\0" in w:
            raise ValueError("not a short word: %r" % (w,))
        buf[i, :len(w)] = np.frombuffer(w, np.uint8)
    return buf.view("<u4")


class Hashed:
    """Words with their key hashes (numpy arrays, one entry per word)."""

    def __init__(self, words):
        self.words = list(words)
        k = pack(self.words) if self.words else np.zeros((0, 4), U32)
        self.k = k
        self.raw = hash_raw(k[:, 0], k[:, 1], k[:, 2], k[:, 3])
        self.h = np.maximum(self.raw, U32(1))
        self.hb = hash32b(k[:, 0], k[:, 1], k[:, 2], k[:, 3])
        self.w0 = k[:, 0].astype(np.uint64) | (k[:, 1].astype(np.uint64) << np.uint64(32))
        self.w1 = k[:, 2].astype(np.uint64) | (k[:, 3].astype(np.uint64) << np.uint64(32))


def hbits(h, shift, nbits):
    """The nbits hash bits below the top `shift` ones."""
    h = np.asarray(h, dtype=np.uint64)
    if nbits == 0 or shift >= 32:
        return np.zeros(h.shape, np.uint64)
    return ((h << np.uint64(shift)) & np.uint64(M32)) >> np.uint64(32 - nbits)


def bucket_of(h):
    return np.asarray(h, dtype=np.uint64) >> np.uint64(32 - K.NB_LOG2)


def red_bucket(h):
    return ((np.asarray(h, dtype=np.uint64) & np.uint64(0xFFFF)) * np.uint64(K.RED_BK)) >> np.uint64(16)


def red_bin(h, shift):
    h = np.asarray(h, dtype=np.uint64)
    if shift >= 32:
        return np.zeros(h.shape, np.uint64)
    return ((h << np.uint64(shift)) & np.uint64(M32)) >> np.uint64(32 - RED_BIN_BITS)


def sr_slot(h):
    bits = K.SR_TSLOTS.bit_length() - 1
    return ((np.asarray(h, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(M32)) >> np.uint64(32 - bits)


def dict_s1(h):
    return ((np.asarray(h, dtype=np.uint64) & np.uint64(0xFFFF)) * np.uint64(K.DICT_SLOTS)) >> np.uint64(16)


def dict_s2(h):
    return ((np.asarray(h, dtype=np.uint64) >> np.uint64(16)) * np.uint64(K.DICT_SLOTS)) >> np.uint64(16)


def sort_key_bits(h, hb, kk, per):
    """The hash bits of k_reduce_sort1's (per = 8) / k_reduce_sort2's (per = 16)
    32-bit sort key in a unit of 2^kk sub-buckets: the top 32 - IB bits of
    (h32 below the unit bits, hash32b)."""
    ib = 9 if per == 8 else 10
    shift = K.NB_LOG2 + kk
    h, hb = np.asarray(h, dtype=np.uint64), np.asarray(hb, dtype=np.uint64)
    pre = ((h << np.uint64(shift)) & np.uint64(M32)) | (hb >> np.uint64(32 - shift))
    return pre >> np.uint64(ib)


def order_key(word):
    """key_less as a sort key: (h32, hash32b, w0, w1), w0 and w1 as u64."""
    x = Hashed([word])
    return (int(x.h[0]), int(x.hb[0]), int(x.w0[0]), int(x.w1[0]))


def model_order(words):
    """The distinct words in the table order every reduce kernel writes."""
    x = Hashed(sorted(set(words)))
    order = np.lexsort((x.w1, x.w0, x.hb, x.h))
    return [x.words[i] for i in order]


# ---------------------------------------------------------------- builder
ALPHA = np.array([c for c in range(0x21, 0x7F) if not 0x41 <= c <= 0x5A], np.uint8)
_OK = np.zeros(256, bool)
_OK[ALPHA] = True
# two-byte UTF-8 sequences that are lowercase already: U+00E0..U+00FF without
# the division sign, Cyrillic U+0430..U+044F
PAIRS2 = np.array([(0xC3, b) for b in range(0xA0, 0xC0) if b != 0xB7] + [(0xD0, b) for b in range(0xB0, 0xC0)] +
                  [(0xD1, b) for b in range(0x80, 0x90)], np.uint8)


class CannotBuild(RuntimeError):
    pass


def words_for(h32, n, mask=M32, seed=0, nonascii=False, raw=False, where=None, tries=60):
    """n distinct words whose key hash agrees with h32 on the bits of `mask`
    (all 32 by default), by inverting hash_fin and hash_fold: 5..8 bytes of
    printable ASCII without whitespace, A-Z or NUL; nonascii: bytes 4..5 are a
    lowercase two-byte UTF-8 sequence (6..8 bytes), so the word goes through the
    Unicode lane.  raw: h32 is the hash before hash32's clamp (0 is allowed);
    otherwise a target of 1 under a full mask stands for the raw hashes 0 and 1.
    where(Hashed) -> bool array: a further filter (hash32b bits, sr_slot ...).
    Seeded and deterministic; raises CannotBuild."""
    h32, mask = int(h32) & M32, int(mask) & M32
    rng = np.random.default_rng([h32, mask, seed, int(nonascii), int(raw)])
    out, seen = [], set()
    batch = min(max(1 << 12, 320 * n), 1 << 19)  # about 0.5 % of the draws give a word
    for t in range(tries):
        if t:
            batch = min(2 * batch, 1 << 19)
        a = (U32(h32 & mask) | (rng.integers(0, 1 << 32, batch, dtype=np.uint64).astype(U32) & U32(~mask & M32)))
        if not raw and mask == M32 and h32 == 1:
            a = a & U32(rng.integers(0, 2, batch, dtype=np.uint64).astype(U32))  # raw 0 or 1
        tail = ALPHA[rng.integers(0, ALPHA.size, (batch, 4))]
        length = rng.integers(6 if nonascii else 5, 9, batch)
        tail[np.arange(4)[None, :] >= (length - 4)[:, None]] = 0
        if nonascii:
            tail[:, :2] = PAIRS2[rng.integers(0, len(PAIRS2), batch)]
        k1 = np.ascontiguousarray(tail).view("<u4").ravel()
        k0 = hash_unfin(a) ^ (k1 * U32(FOLD_MUL))
        head = np.ascontiguousarray(k0.astype("<u4")).view(np.uint8).reshape(-1, 4)
        good = np.nonzero(_OK[head].all(axis=1))[0]
        if good.size == 0:
            continue
        # (an 'S8' string drops its trailing NUL bytes: the words come out at their lengths)
        cand = np.ascontiguousarray(np.concatenate([head[good], tail[good]], axis=1)).view("S8").ravel().tolist()
        if where is not None:
            keep = where(Hashed(cand))
            cand = [w for w, k in zip(cand, keep) if k]
        for w in cand:
            if w not in seen:
                seen.add(w)
                out.append(w)
                if len(out) == n:
                    return out
    raise CannotBuild("words_for(%#x, %d, mask %#x): only %d words" % (h32, n, mask, len(out)))


def hash_with_words(base, free_bits, n, seed=0, accept=None, **kw):
    """(h, words): the first hash base | j (j below 2^free_bits, in a seeded
    order) among those `accept` (array -> bool array) takes that has n words (words_for(h, n, **kw)).
    A non-ASCII word's first byte follows from its hash and the lead byte of
    its two-byte sequence, so four hashes in ten have no such word."""
    rng = np.random.default_rng([int(base), free_bits, seed])
    hs = (np.uint64(int(base) & M32) | rng.permutation(1 << free_bits).astype(np.uint64))
    if accept is not None:
        hs = hs[accept(hs)]
    for h in hs[:256].tolist():
        try:
            return h, words_for(h, n, seed=seed, tries=3, **kw)
        except CannotBuild:
            continue
    raise CannotBuild("hash_with_words(%#x, %d bits, %d)" % (base, free_bits, n))


def part_mask():
    return (M32 << (32 - K.NB_LOG2)) & M32


def unit_mask(kk):
    return (M32 << (32 - K.NB_LOG2 - kk)) & M32


def unit_hash(part, kk, sub):
    return ((part << kk) | sub) << (32 - K.NB_LOG2 - kk)


# ---------------------------------------------------------------- geometry model
SORT1, SORT2, RED, SMALL, WHOLE = "sort1", "sort2", "k_reduce", "k_reduce_small", "whole"


def kk_for(total, fraction=1.0):
    """k_split_count's kk for a partition of `total` records whose sample says
    `fraction` of them are distinct."""
    if total <= K.SPLIT_MIN or fraction < 0.5:
        return 0
    kk = 0
    while kk < K.SUB_BITS_MAX and total * fraction > K.SPLIT_TARGET * (1 << kk):
        kk += 1
    return kk


def unit_list(c, d):
    """k_split_scatter's rule for a unit of c cold and d weighted records."""
    if d == 0 and K.SMALL_CAP < c <= 2 * K.SMALL_CAP:
        return SORT2
    if c + d > K.SMALL_CAP:
        return RED
    if d != 0:
        return SMALL
    return SORT1


def subpasses(h, shift):
    """k_reduce's sub-passes over distinct keys of hashes h in a unit whose hash
    bits below `shift` are free: the smallest 2^k such that every sub-pass over
    the next k bits holds at most RED_CAP keys."""
    for k in range(0, 33 - shift):
        if h.size == 0 or np.bincount(hbits(h, shift, k).astype(np.int64)).max() <= K.RED_CAP:
            return 1 << k
    raise CannotBuild("more than RED_CAP keys share every hash bit")


class Unit:
    def __init__(self, part, kk, sub, cold, weighted, where, subpasses):
        self.part, self.kk, self.sub, self.cold, self.weighted = part, kk, sub, cold, weighted
        self.list, self.subpasses = where, subpasses

    @property
    def records(self):
        return self.cold + self.weighted


class Geometry:
    """What the pass does with a list of (word, copies, weighted): every copy
    of a cold word is one cold record, every copy of a weighted word one
    weighted record.  fraction: the distinct fraction k_split_count is assumed
    to sample (it only matters near a kk boundary; see Case.check_kk)."""

    def __init__(self, items, fraction=1.0):
        x = Hashed([w for w, _, _ in items])
        copies = np.array([c for _, c, _ in items], np.int64)
        wt = np.array([bool(f) for _, _, f in items], bool)
        part = bucket_of(x.h).astype(np.int64)
        self.cold = np.bincount(part, np.where(wt, 0, copies), K.NB).astype(np.int64)
        self.weighted = np.bincount(part, np.where(wt, copies, 0), K.NB).astype(np.int64)
        self.records = self.cold + self.weighted
        self.kk = [kk_for(int(t), fraction) for t in self.records]
        self.units = {}   # (part, sub) -> Unit; whole partitions: sub = None
        for b in np.nonzero(self.records)[0]:
            sel = part == b
            hb_, cb, wb = x.h[sel], copies[sel], wt[sel]
            words_b = np.nonzero(sel)[0]
            kk = self.kk[b]
            if kk == 0:
                hd = self._distinct_hashes(x, words_b)
                self.units[(int(b), None)] = Unit(int(b), 0, None, int(self.cold[b]), int(self.weighted[b]), WHOLE,
                                                  subpasses(hd, K.NB_LOG2))
                continue
            sub = hbits(hb_, K.NB_LOG2, kk).astype(np.int64)
            c = np.bincount(sub, np.where(wb, 0, cb), 1 << kk).astype(np.int64)
            d = np.bincount(sub, np.where(wb, cb, 0), 1 << kk).astype(np.int64)
            for s in range(1 << kk):
                where = unit_list(int(c[s]), int(d[s]))
                sp = subpasses(self._distinct_hashes(x, words_b[sub == s]), K.NB_LOG2 + kk) if where == RED else 1
                self.units[(int(b), s)] = Unit(int(b), kk, s, int(c[s]), int(d[s]), where, sp)

    @staticmethod
    def _distinct_hashes(x, idx):
        first = {}
        for j in idx:
            first.setdefault(x.words[j], j)
        return x.h[np.array(sorted(first.values()), np.int64)] if first else np.zeros(0, U32)

    def unit(self, part, sub=None):
        return self.units.get((part, sub)) or Unit(part, 0, None, 0, 0, WHOLE, 1)

    def count(self, where):
        return sum(1 for u in self.units.values() if u.list == where)

    def summary(self):
        """The figures of the MOX_VERBOSE attempt line and of mox_stats."""
        split = [b for b in range(K.NB) if self.kk[b]]
        return {
            "units": sum(1 << k for k in self.kk),
            "sort2": self.count(SORT2),
            "k_reduce": self.count(RED),
            "k_reduce_small": self.count(SMALL),
            "split": len(split),
            "max_sub": max([u.subpasses for u in self.units.values()] + [1]),
            "cold_records": int(self.cold.sum()),
            "weighted_records": int(self.weighted.sum()),
        }


# ---------------------------------------------------------------- cases
class Case:
    """items: (word, copies, weighted) of a corpus case, or (word, count) pairs
    of a pairs_* case; claims: the geometry the case says it has (checked in
    test_reduce_model.py against Geometry); default_engine: what the run with a
    dictionary-enabled engine may assert -- "same" (no dictionary forms: all of
    it), "lists" (a dictionary forms, but every partition stays whole: the lists
    and sub-passes), "hot" (the dictionary takes exactly the words of `hot`,
    each then one weighted record: dict_geometry), "exact" (exactness and order
    only)."""

    def __init__(self, name, items, claims, default_engine="same", pairs=None, hot=()):
        self.name, self.items, self.claims, self.default_engine, self.pairs, self.hot = (
            name, items, claims, default_engine, pairs, list(hot))
        if pairs is None:
            words = [w for w, _, _ in items]
            if len(set(words)) != len(words):
                raise CannotBuild("%s: a word was drawn twice" % name)
        self._geo = None

    @property
    def geometry(self):
        if self._geo is None:
            items = self.items if self.pairs is None else [(w, 1, True) for w, _ in self.pairs]
            self._geo = Geometry(items)
        return self._geo

    @property
    def dict_geometry(self):
        """The geometry with every word of `hot` in the dictionary: its copies
        leave the cold records and come back as one weighted record."""
        hot = set(self.hot)
        return Geometry([(w, 1, True) if w in hot else (w, c, f) for w, c, f in self.items])

    def words(self):
        return [w for w, _, _ in self.items] if self.pairs is None else [w for w, _ in self.pairs]

    def expected(self):
        """{word: count} of the case."""
        out = {}
        src = [(w, c) for w, c, _ in self.items] if self.pairs is None else self.pairs
        for w, c in src:
            out[w] = out.get(w, 0) + c
        return out

    def tokens(self):
        """The corpus tokens in a seeded shuffle."""
        toks = [w for w, c, _ in self.items for _ in range(c)]
        rng = np.random.default_rng([0x5EED, len(toks)])
        return [toks[i] for i in rng.permutation(len(toks))]

    def text(self):
        """The corpus: the tokens separated by whitespace, padded so that the
        text has MIN_ROWS rows of PAY bytes or a few more: every map workgroup
        of a grid of GRID gets a few rows (a short text would load few
        workgroups' regions with everything), and no dictionary forms unless
        the case repeats words."""
        toks = self.tokens()
        body = sum(len(t) for t in toks)
        gap = max(1, -(-(MIN_ROWS * K.PAY - body) // len(toks)))
        seps = [b" ", b"\n", b"\t", b" \n", b"\r\n"]
        parts = []
        for i, t in enumerate(toks):
            s = seps[i % len(seps)]
            parts.append(t)
            parts.append(s + b" " * (gap - len(s)))
        return b"".join(parts)

    def region_fill(self, grid=GRID, text=None):
        """The largest number of cold records one map workgroup of `grid` writes
        into one slice (QF_MAX per region, by the two hash bits below the
        partition bits) of one partition's region: row r holds the tokens that
        start in bytes [PAY r, PAY r + PAY), workgroup g rows [rb, rb + n)."""
        text = self.text() if text is None else text
        starts, toks = [], []
        for m in re.finditer(rb"\S+", text):
            starts.append(m.start())
            toks.append(m.group())
        cold = {w for w, _, f in self.items if not f}
        uniq = sorted(set(toks))
        hx = Hashed(uniq)
        hof = dict(zip(uniq, hx.h.tolist()))
        nrows = -(-len(text) // K.PAY)
        per, rem = divmod(nrows, grid)
        # first row of workgroup g: g per + min(g, rem)
        first = np.array([g * per + min(g, rem) for g in range(grid + 1)], np.int64)
        row = np.array(starts, np.int64) // K.PAY
        wg = np.searchsorted(first, row, side="right") - 1
        is_cold = np.array([t in cold for t in toks], bool)
        h = np.array([hof[t] for t in toks], np.uint64)
        key = (wg * K.NB + bucket_of(h).astype(np.int64)) * K.QF_MAX + hbits(h, K.NB_LOG2, 2).astype(np.int64)
        return int(np.bincount(key[is_cold]).max()) if is_cold.any() else 0

    def repeat_fraction(self):
        """Share of the ASCII tokens that belong to a word present more than once
        (k_dict_pick builds no dictionary under 1 / DICT_MIN_COVER_INV)."""
        asc = [(w, c) for w, c, _ in self.items if max(w) < 0x80]
        tot = sum(c for _, c in asc)
        return sum(c for _, c in asc if c > 1) / max(tot, 1)


# Rows of the padded text: more than 3 per workgroup of a grid of 256, and more
# bytes than the SAMPLE_PIECES pieces of SAMPLE_PIECE bytes the dictionary
# sample reads -- over a shorter text the pieces overlap, the words in the
# overlaps count twice and a dictionary of them forms although every word is
# there once.
MIN_ROWS = 830
KK = 5          # every split partition here: (SPLIT_MIN, 32 SPLIT_TARGET] records, nearly all distinct


def _filler(n, seed, avoid):
    """n distinct words anywhere outside the partitions of `avoid`."""
    got = words_for(0, n + n // 8 + 64, mask=0, seed=seed)
    x = Hashed(got)
    keep = [w for w, p in zip(got, bucket_of(x.h).tolist()) if p not in avoid]
    if len(keep) < n:
        raise CannotBuild("filler")
    return [(w, 1, False) for w in keep[:n]]


def _unit_words(part, sub, n, seed=0, nonascii=False, where=None, kk=KK):
    return words_for(unit_hash(part, kk, sub), n, mask=unit_mask(kk), seed=seed, nonascii=nonascii, where=where)


def _cold(words, copies=1):
    return [(w, copies, False) for w in words]


def _wt(words, copies=1):
    return [(w, copies, True) for w in words]


def _split_partition(part, special, total, seed):
    """Items of a partition of 2^KK units: `special` {sub: items} as given, the
    other units filled with distinct cold words so that each of the QF_MAX
    slices of the partition (units by their top two bits) holds about a
    quarter of `total` records."""
    nsub = 1 << KK
    per_slice = nsub // K.QF_MAX
    items, sizes = [], {}
    for s, its in special.items():
        items += its
        sizes[s] = sum(c for _, c, _ in its)
    for q in range(K.QF_MAX):
        subs = range(q * per_slice, (q + 1) * per_slice)
        free = [s for s in subs if s not in special]
        room = total // K.QF_MAX - sum(sizes.get(s, 0) for s in subs)
        if not free:
            continue
        if room < len(free):
            raise CannotBuild("slice %d of partition %d is over its share" % (q, part))
        base = room // len(free)
        for j, s in enumerate(free):
            n = min(base + (j * 7) % 11 - 5, K.SMALL_CAP) if base > 8 else base
            items += _cold(_unit_words(part, s, n, seed=seed + s))
    return items


def unit_sizes():
    """One split partition of 32 units; cold-only units of exactly 0, 1, 64, 65,
    511, 512, 513, 1023, 1024 and 1025 records, a 512-record and a 1024-record
    unit that are one word each, repeats of 9 and 17 across a lane boundary."""
    P = 0x155
    sp = {}

    def distinct(sub, n):
        sp[sub] = _cold(_unit_words(P, sub, n, seed=sub))

    # slice 0 (units 0..7), slice 1 (8..15), slice 2 (16..23); slice 3 is filler
    distinct(0, 1025)
    sp[1] = _cold(_unit_words(P, 1, 1, seed=1), 512)
    w = _unit_words(P, 2, 511 - 9 + 1, seed=2)
    sp[2] = _cold(w[:1], 9) + _cold(w[1:])       # 511 records
    distinct(3, 65)
    sp[4] = []                                     # 0 records
    distinct(8, 1024)
    distinct(9, 513)
    distinct(10, 512)
    distinct(11, 64)
    distinct(12, 1)
    sp[16] = _cold(_unit_words(P, 16, 1, seed=16), 1024)
    w = _unit_words(P, 17, 1023 - 17 + 1, seed=17)
    sp[17] = _cold(w[:1], 17) + _cold(w[1:])     # 1023 records
    items = _split_partition(P, sp, 9400, seed=100)
    items += _filler(36000, 7, {P})
    claims = {
        "part": P,
        "unit_records": {0: 1025, 1: 512, 2: 511, 3: 65, 4: 0, 8: 1024, 9: 513, 10: 512, 11: 64, 12: 1, 16: 1024, 17: 1023},
        "unit_lists": {0: RED, 1: SORT1, 2: SORT1, 3: SORT1, 4: SORT1, 8: SORT2, 9: SORT2, 10: SORT1, 11: SORT1, 12: SORT1,
                       16: SORT2, 17: SORT2},
        "summary": {"split": 1, "units": K.NB - 1 + 32, "sort2": 4, "k_reduce": 1, "k_reduce_small": 0, "max_sub": 1},
        # With a dictionary: the repeats are under a twentieth of the tokens, so
        # k_dict_pick sets its threshold past the last count class (256) -- which
        # the two one-word units' words still reach (their sampled counts are not
        # capped at the class), and only they.  Without their 1,536 records the
        # partition is under SPLIT_MIN: whole, ~7,840 keys, and units 8..9 alone
        # hold 1,537 of them, so sixteen sub-passes.
        "summary_dict": {"split": 0, "units": K.NB, "sort2": 0, "k_reduce": 0, "k_reduce_small": 0, "max_sub": 16,
                         "weighted_records": 2},
    }
    return Case("unit_sizes", items, claims, default_engine="hot", hot=[sp[1][0][0], sp[16][0][0]])


def _tie_groups(part, sub, per, seed):
    """In unit (part, sub): groups of 2 and 5 distinct words with one h32 and
    the same sort-key bits of hash32b (the 64-bit re-sort), and groups of 2 and
    5 with one h32 whose sort-key bits differ (the first sort tells them apart).
    Returns (items, groups)."""
    top = 32 - (9 if per == 8 else 10) - (32 - K.NB_LOG2 - KK)  # hash32b bits in the sort key
    items, groups = [], []
    for g, (n, same) in enumerate([(2, True), (5, True), (2, False), (5, False)]):
        h = unit_hash(part, KK, sub) | (0x1234 + 0x1111 * g + seed)
        cand = words_for(h, 600, seed=seed + g)
        x = Hashed(cand)
        t = (x.hb >> U32(32 - top)).tolist()
        if same:
            by = {}
            for w, b in zip(cand, t):
                by.setdefault(b, []).append(w)
            ws = next(v for v in by.values() if len(v) >= n)[:n]
        else:
            ws, used = [], set()
            for w, b in zip(cand, t):
                if b not in used:
                    used.add(b)
                    ws.append(w)
                if len(ws) == n:
                    break
        if len(ws) != n:
            raise CannotBuild("tie group")
        groups.append((ws, same))
        items += [(w, 1 + (i % 3), False) for i, w in enumerate(ws)]  # some repeat: run lengths after the re-sort
    return items, groups


def sort_key_ties():
    """k_reduce_sort1 and k_reduce_sort2 units with keys that share all of h32:
    with the same sort-key bits of hash32b (both sorts run) and with different
    ones."""
    P = 0x2A3
    sp, groups = {}, {}
    for sub, per, n in ((5, 8, 400), (13, 16, 700), (21, 8, 512), (29, 16, 1024)):
        its, groups[sub] = _tie_groups(P, sub, per, seed=sub)
        rest = n - sum(c for _, c, _ in its)
        have = {w for w, _, _ in its}
        more = [w for w in _unit_words(P, sub, rest + 16, seed=50 + sub) if w not in have][:rest]
        sp[sub] = its + _cold(more)
    items = _split_partition(P, sp, 9400, seed=200) + _filler(3000, 8, {P})
    claims = {
        "part": P,
        "unit_records": {5: 400, 13: 700, 21: 512, 29: 1024},
        "unit_lists": {5: SORT1, 13: SORT2, 21: SORT1, 29: SORT2},
        "tie_groups": groups,
        "per": {5: 8, 13: 16, 21: 8, 29: 16},
        "summary": {"split": 1, "units": K.NB - 1 + 32, "sort2": 2, "k_reduce": 0, "k_reduce_small": 0, "max_sub": 1},
    }
    return Case("sort_key_ties", items, claims)


def weighted_mix():
    """Non-ASCII (weighted) words at the lists' cut-offs: 511 cold + 1 weighted
    (k_reduce_small at exactly SMALL_CAP), 512 cold + 1 weighted (k_reduce at
    SMALL_CAP + 1), weighted-only units of 40 and of 513 records, exactly 512
    weighted records, and a whole partition of weighted records only."""
    P, Q = 0x0C7, 0x311
    sp = {
        3: _cold(_unit_words(P, 3, 511, seed=3)) + _wt(_unit_words(P, 3, 1, seed=3, nonascii=True)),
        6: _cold(_unit_words(P, 6, 512, seed=6)) + _wt(_unit_words(P, 6, 1, seed=6, nonascii=True)),
        11: [(w, 2, True) for w in _unit_words(P, 11, 20, seed=11, nonascii=True)],
        19: _wt(_unit_words(P, 19, 513, seed=19, nonascii=True)),
        27: _wt(_unit_words(P, 27, 512, seed=27, nonascii=True)),
    }
    items = _split_partition(P, sp, 9400, seed=300)
    items += _wt(words_for(Q << (32 - K.NB_LOG2), 30, mask=part_mask(), seed=31, nonascii=True))
    items += _filler(3000, 9, {P, Q})
    claims = {
        "part": P,
        "unit_records": {3: 512, 6: 513, 11: 40, 19: 513, 27: 512},
        "unit_lists": {3: SMALL, 6: RED, 11: SMALL, 19: RED, 27: SMALL},
        "whole_weighted_only": Q,
        "summary": {"split": 1, "units": K.NB - 1 + 32, "sort2": 0, "k_reduce": 2, "k_reduce_small": 3, "max_sub": 1},
    }
    return Case("weighted_mix", items, claims)


def _whole_partition(part, per_sub, nbits, seed, copies=1):
    """Distinct cold words of partition `part`: per_sub[s] of them in the
    sub-pass s of the nbits hash bits below the partition bits."""
    items = []
    for s, n in enumerate(per_sub):
        h = ((part << nbits) | s) << (32 - K.NB_LOG2 - nbits)
        items += _cold(words_for(h, n, mask=unit_mask(nbits), seed=seed + s), copies)
    return items


def split_min_edge(over=False):
    """Partition A: exactly SPLIT_MIN all-distinct records, whole, RED_CAP keys
    in each of its four sub-passes (over: RED_CAP + 1 in one of them, so eight
    sub-passes); partition B: SPLIT_MIN + 1 records, split into 32 units."""
    A, B = 0x09A, 0x1F3
    per = [K.RED_CAP] * 4
    if over:
        per = [K.RED_CAP + 1, K.RED_CAP - 1, K.RED_CAP, K.RED_CAP]
    assert sum(per) == K.SPLIT_MIN
    items = _whole_partition(A, per, 2, seed=400)
    nb = K.SPLIT_MIN + 1
    base, extra = divmod(nb, 32)
    for s in range(32):
        items += _cold(_unit_words(B, s, base + (1 if s < extra else 0), seed=440 + s))
    claims = {
        "whole": {A: K.SPLIT_MIN}, "split_parts": {B: nb},
        "summary": {"split": 1, "units": K.NB - 1 + 32, "sort2": 0, "k_reduce": 0, "k_reduce_small": 0,
                    "max_sub": 8 if over else 4},
    }
    return Case("split_min_edge_over" if over else "split_min_edge", items, claims)


def red_cap_edge(over=False):
    """Whole partitions of exactly RED_CAP distinct keys (one pass; over:
    RED_CAP + 1, two sub-passes), every key once and every key three times."""
    n = K.RED_CAP + (1 if over else 0)
    P1, P3 = 0x05B, 0x2EE
    items = _cold(words_for(P1 << (32 - K.NB_LOG2), n, mask=part_mask(), seed=500))
    items += _cold(words_for(P3 << (32 - K.NB_LOG2), n, mask=part_mask(), seed=501), 3)
    claims = {
        "whole": {P1: n, P3: 3 * n}, "distinct": {P1: n, P3: n},
        "summary": {"split": 0, "units": K.NB, "sort2": 0, "k_reduce": 0, "k_reduce_small": 0, "max_sub": 2 if over else 1},
    }
    return Case("red_cap_edge_over" if over else "red_cap_edge", items, claims, default_engine="lists")


def bucket_clusters():
    """k_reduce's table in whole partitions of fewer than RED_CAP keys: 9, 12
    and 40 keys under one tag, 40 keys in one bucket under different tags, a
    20-key cluster from bucket RED_BK - 1 through the spare bucket to bucket 0,
    and 100 keys in one sort bin."""
    top = 32 - K.NB_LOG2
    parts = {"tag9": 0x021, "tag12": 0x022, "tag40": 0x023, "low16": 0x024, "wrap": 0x025, "bin": 0x026}
    low_last = 0xFFFF                      # red_bucket(0xFFFF) = RED_BK - 1
    clusters = {}
    items = []
    for name, n in (("tag9", 9), ("tag12", 12), ("tag40", 40)):
        h = (parts[name] << top) | 0x0ABCD + n
        clusters[name] = words_for(h, n, seed=600 + n)
    clusters["low16"] = words_for((parts["low16"] << top) | 0x5A5A, 40, mask=part_mask() | 0xFFFF, seed=640)
    clusters["wrap"] = words_for((parts["wrap"] << top) | (0x15 << 16) | low_last, 20, seed=650)
    clusters["bin"] = words_for((parts["bin"] << top) | (0x2B3 << (top - RED_BIN_BITS)), 100,
                                mask=(M32 << (top - RED_BIN_BITS)) & M32, seed=660)
    for name, ws in clusters.items():
        items += [(w, 2 if i % 8 == 3 else 1, False) for i, w in enumerate(ws)]
        have = set(ws)
        more = words_for(parts[name] << top, 260, mask=part_mask(), seed=670 + parts[name])
        items += _cold([w for w in more if w not in have][:200])
    items += _filler(6000, 10, set(parts.values()))
    claims = {
        "parts": parts, "clusters": clusters,
        "summary": {"split": 0, "units": K.NB, "sort2": 0, "k_reduce": 0, "k_reduce_small": 0, "max_sub": 1},
    }
    return Case("bucket_clusters", items, claims)


def small_table_clusters():
    """k_reduce_small units (weighted records present, at most SMALL_CAP in
    all): 100 keys with one h32 (one linear-probe chain), a chain that starts
    at slot SR_TSLOTS - 1 and wraps to 0, and one word present as 300 records."""
    P = 0x1B6
    last = K.SR_TSLOTS - 1
    free = 32 - K.NB_LOG2 - KK
    _, chain = hash_with_words(unit_hash(P, KK, 4), free, 100, seed=700, nonascii=True)
    # hashes of unit 14 whose sr_slot is the last slot: three tags, four keys each
    wrap, used = [], set()
    for j in range(3):
        h, ws = hash_with_words(unit_hash(P, KK, 14), free, 4, seed=710 + j, nonascii=True,
                                accept=lambda hs: (sr_slot(hs) == last) & ~np.isin(hs, list(used)))
        used.add(h)
        wrap += ws
    hot = _unit_words(P, 22, 1, seed=22, nonascii=True)
    sp = {
        4: _wt(chain) + _cold(_unit_words(P, 4, 200, seed=40)),
        14: [(w, 1 + (i % 2), True) for i, w in enumerate(wrap)] + _cold(_unit_words(P, 14, 150, seed=41)),
        22: _wt(hot, 300) + _cold(_unit_words(P, 22, 212, seed=42)),
    }
    items = _split_partition(P, sp, 9400, seed=720) + _filler(3000, 11, {P})
    claims = {
        "part": P, "chain": chain, "wrap": wrap, "hot": hot[0],
        "unit_records": {4: 300, 14: 150 + sum(1 + (i % 2) for i in range(len(wrap))), 22: 512},
        "unit_lists": {4: SMALL, 14: SMALL, 22: SMALL},
        "summary": {"split": 1, "units": K.NB - 1 + 32, "sort2": 0, "k_reduce": 0, "k_reduce_small": 3, "max_sub": 1},
    }
    return Case("small_table_clusters", items, claims)


HOT = 2000


def hash_zero():
    """Words whose hash before the clamp is 0 and 1 (both hash32 = 1), rare and
    hot: the free-slot marker of the dictionary and of k_reduce's tags."""
    z = words_for(0, 2, raw=True, seed=800)
    o = words_for(1, 3, raw=True, seed=801)
    other = words_for(0, 3, mask=0, seed=802)
    rare = [z[0], o[0], o[1]]
    hot = [z[1], o[2]] + other
    items = _cold(rare) + [(w, HOT - 37 * i, False) for i, w in enumerate(hot)]
    have = {w for w, _, _ in items}
    items += [it for it in _filler(3000, 12, set()) if it[0] not in have]
    claims = {"raw0": [z[0], z[1]], "raw1": [o[0], o[1], o[2]], "hot": hot}
    return Case("hash_zero", items, claims, default_engine="exact", hot=hot)


def dictionary_same_hash():
    """Four hot words with one h32 (the dictionary has two slots for them) and
    three rare words with that h32."""
    h = 0x6B8B4567
    ws = words_for(h, 7, seed=810)
    other = words_for(0, 3, mask=0, seed=811)
    hot = ws[:4] + other
    items = [(w, HOT - 100 * i, False) for i, w in enumerate(hot)] + _cold(ws[4:])
    have = {w for w, _, _ in items}
    items += [it for it in _filler(3000, 13, set()) if it[0] not in have]
    claims = {"h32": h, "same": ws, "hot": hot}
    return Case("dictionary_same_hash", items, claims, default_engine="exact", hot=hot)


def dict_placed(hot):
    """How many of the hot words (hottest first) k_dict_build's two-choice
    placement seats when nothing else competes: s1, else s2."""
    x = Hashed(hot)
    taken, n = set(), 0
    for s1, s2 in zip(dict_s1(x.h).tolist(), dict_s2(x.h).tolist()):
        for s in (s1, s2):
            if s not in taken:
                taken.add(s)
                n += 1
                break
    return n


def pairs_split_min():
    """mox_reduce_pairs (every record weighted): partition A of exactly
    SPLIT_MIN distinct words stays whole; partition B of SPLIT_MIN + 1 records
    splits, with units of exactly SMALL_CAP records (k_reduce_small) and of
    SMALL_CAP + 1 (k_reduce); duplicate words sum; counts of 2^32 - 1,
    2^53 + 1 and two of 2^62 that add."""
    A, B = 0x0D4, 0x27C
    a_items = _whole_partition(A, [K.RED_CAP] * 4, 2, seed=900)
    pairs = [(w, 1 + (i % 5)) for i, (w, _, _) in enumerate(a_items)]
    sizes = [K.SMALL_CAP] * 7 + [K.SMALL_CAP + 1] * 6
    rest = K.SPLIT_MIN + 1 - sum(sizes)
    base, extra = divmod(rest, 32 - len(sizes))
    sizes += [base + (1 if j < extra else 0) for j in range(32 - len(sizes))]
    # spread the big units over the partition: unit s gets sizes[(s * 5) % 32]
    unit_records = {}
    big = [(1 << 32) - 1, (1 << 53) + 1, 1 << 62, 1 << 62]
    for s in range(32):
        n = sizes[(s * 5) % 32]
        unit_records[s] = n
        dup = 3 if n >= 8 else 0               # `dup` words appear twice: n records, n - dup words
        ws = _unit_words(B, s, n - dup, seed=940 + s)
        recs = [(w, 7 + (i % 11)) for i, w in enumerate(ws)] + [(w, 1000 + i) for i, w in enumerate(ws[:dup])]
        if s == 0:  # the first unit's duplicated words carry the wide counts
            recs[0] = (ws[0], big[2])
            recs[len(ws)] = (ws[0], big[3])
            recs[1] = (ws[1], big[0])
            recs[2] = (ws[2], big[1])
        pairs += recs
    rng = np.random.default_rng(0xBA1)
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    claims = {
        "whole": {A: K.SPLIT_MIN}, "split_parts": {B: K.SPLIT_MIN + 1}, "part": B, "unit_records": unit_records,
        "unit_lists": {s: (SMALL if n <= K.SMALL_CAP else RED) for s, n in unit_records.items()},
        "summary": {"split": 1, "units": K.NB - 1 + 32, "sort2": 0, "k_reduce": 6, "k_reduce_small": 26, "max_sub": 4},
    }
    return Case("pairs_split_min", None, claims, pairs=pairs)


CORPUS_CASES = {
    "unit_sizes": unit_sizes,
    "sort_key_ties": sort_key_ties,
    "weighted_mix": weighted_mix,
    "split_min_edge": split_min_edge,
    "split_min_edge_over": lambda: split_min_edge(over=True),
    "red_cap_edge": red_cap_edge,
    "red_cap_edge_over": lambda: red_cap_edge(over=True),
    "bucket_clusters": bucket_clusters,
    "small_table_clusters": small_table_clusters,
    "hash_zero": hash_zero,
    "dictionary_same_hash": dictionary_same_hash,
}
PAIRS_CASES = {"pairs_split_min": pairs_split_min}

_built = {}


def case(name):
    """The case `name`, built once per process."""
    if name not in _built:
        _built[name] = (CORPUS_CASES.get(name) or PAIRS_CASES[name])()
    return _built[name]
