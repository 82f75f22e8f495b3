"""Corpora that run out of one device buffer at a time, and a host model of the
buffer-growth ladder they climb (map-oxidize_amd/csrc/mox_engine.hip:
initial_caps, realloc_sized, grow_for, cold_cap_for, run_corpus; the overflow
bits are set in mox_kernels.hip).  No GPU code runs here: test_growth_model.py
checks on the CPU that every case exceeds the capacity it names and no other,
and test_gpu_growth.py compares the engine's MOX_VERBOSE attempt lines with the
ladder predicted here.

The model of one attempt (Figures.attempt) restates, from the text alone:
  k_map        tokens that start in row r (PAY bytes) belong to the workgroup
               that owns row r; a short ASCII word that is not in the dictionary
               is one cold record of region (workgroup, partition, slice), a
               region holds rc = cold_cap / QF records (QF = 4 slices without a
               dictionary, 1 with one) and every record past rc spills
               (cold_pair writes in pairs, and rc is even: c records leave
               max(0, c - rc) spills whichever records win the races); a
               workgroup keeps spill_cap spills (OVF_POOL past that); tokens with
               a non-ASCII byte go to the Unicode lane (OVF_U past u_cap), ASCII
               tokens of more than 16 bytes or with a NUL byte to the long table
  k_unicode    the first min(u_n, u_cap) Unicode tokens reserve len + len / 2 + 4
               arena bytes each (OVF_ARENA past arena_cap: the token is dropped);
               a lowered word of at most 16 bytes without NUL is one weighted
               record, any other goes to the long table
  long_insert  OVF_LONG when more distinct long words than long_cap slots arrive
  k_hist       weighted records + kept spills past w_cap: OVF_W
  k_unit_scan  (only without a rerun bit) a partition of more than SPLIT_MIN
               records, most of them distinct, is split: OVF_SPLIT while the
               split buffers are too small
  k_final_scan (only without a rerun or split bit) OVF_TABLE, OVF_BYTES
Which tokens win a capped buffer is a race on the device, so tokens that compete
for one are of one length and one kind in every case: the figures then do not
depend on the winners (Figures raises NotDeterministic otherwise).

The formulas' coefficients are restated here; the constants come from the
sources by parsing (C).  test_gpu_growth.py is what checks the restatement: a
wrong coefficient moves a capacity or a mask off the engine's attempt lines."""
import re

import numpy as np

import reduce_cases as R
from reduce_cases import GRID, K, Hashed, bucket_of, hbits, words_for

OVF_POOL, OVF_W, OVF_U, OVF_LONG, OVF_ARENA, OVF_PROBE, OVF_TABLE, OVF_BYTES, OVF_REDUCE, OVF_SPLIT = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
BIT_NAMES = {OVF_POOL: "POOL", OVF_W: "W", OVF_U: "U", OVF_LONG: "LONG", OVF_ARENA: "ARENA", OVF_PROBE: "PROBE",
             OVF_TABLE: "TABLE", OVF_BYTES: "BYTES", OVF_REDUCE: "REDUCE", OVF_SPLIT: "SPLIT"}


def mask_names(mask):
    return "|".join(n for b, n in BIT_NAMES.items() if mask & b) or "0"


class C:
    """Constants of the growth machinery, parsed from the sources."""
    _h, _host = R._source("mox_internal.h"), R._source("mox_host.h")
    NB = R._parse(_h, "NB")
    QF_MAX = R._parse(_h, "QF_MAX")
    COLD_CAP_MAX = R._parse(_h, "COLD_CAP_MAX")
    SPLIT_PER_REGION = R._parse(_h, "SPLIT_PER_REGION")
    SUB_N = R._parse(_h, "SUB_N")
    SPLIT_MIN = R._parse(_h, "SPLIT_MIN")
    GROW_RETRIES = R._parse(_host, "GROW_RETRIES")
    PAY = R._parse(_h, "PAY")
    OVF = None  # {name: bit} of the enum in mox_internal.h (set below)


def _ovf_bits(text):
    m = re.search(r"OVF_POOL = 1u,[^}]*?OVF_RERUN", text, re.S)
    return {n: int(v) for n, v in re.findall(r"OVF_(\w+) = (\d+)u", m.group(0))}


C.OVF = _ovf_bits(C._h)


# ---------------------------------------------------------------- capacities
CAP_NAMES = ("cold", "spill", "w", "u", "arena", "long", "table", "bytes", "split_k", "split_w")


def next_pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def initial_caps(n, grid=GRID):
    table = 65536 + n // 64
    return {"cold": max(64, n // (grid * C.NB * 8)), "spill": max(1024, n // (grid * 64)), "w": 65536 + n // 64,
            "u": 4096 + n // 64, "arena": 65536 + n // 16, "long": 65536, "table": table, "bytes": table * 8,
            "split_k": 0, "split_w": 0}


def realloc_sized(c):
    """The capacities realloc_sized allocates for the request c."""
    step = 2 * C.QF_MAX
    out = dict(c)
    out["cold"] = min((c["cold"] + step - 1) // step * step, C.COLD_CAP_MAX)
    out["spill"] = min(c["spill"], 0xFFFFFFF0)
    out["long"] = next_pow2(c["long"])
    return out


def uniq_cap(caps, grid=GRID):
    return grid * C.NB * caps["cold"] + caps["w"]


def ensure_caps(have, need):
    """(capacities, reallocated)."""
    if have is not None and all(have[k] >= need[k] for k in CAP_NAMES):
        return have, False
    c = need if have is None else {k: max(have[k], need[k]) for k in CAP_NAMES}
    return realloc_sized(c), True


def cold_cap_for(caps, h, grid=GRID):
    want = h["cold_need"] + h["cold_need"] // 8 + 16
    bound = 4 * h["tokens"] // (grid * C.NB) + 64
    return min(want, max(bound, caps["cold"]))


def grow_for(caps, h, grid=GRID):
    need = dict(caps)
    m = h["overflow"]
    if m & OVF_POOL:
        need["cold"] = max(need["cold"], cold_cap_for(caps, h, grid))
        need["spill"] = max(need["spill"], h["spill_need"] + h["spill_need"] // 4 + 1024)
    if m & OVF_W:
        wn = max(h["w_total"], h["w_n"])
        need["w"] = max(need["w"], wn + wn // 4 + 1024)
    if m & OVF_U:
        need["u"] = h["u_n"] + h["u_n"] // 4 + 1024
    if m & OVF_ARENA:
        need["arena"] = h["arena_n"] + h["arena_n"] // 4 + 65536
    if m & OVF_LONG:
        need["long"] = next_pow2(2 * h["long_n"] + 1024)
    if m & OVF_TABLE:
        need["table"] = h["n_total"] + h["n_total"] // 4 + 1024
    if m & OVF_BYTES:
        need["bytes"] = h["bytes_total"] + h["bytes_total"] // 4 + 65536
    if m & OVF_SPLIT:
        k, wv = h["split_k"] + h["split_k"] // 8 + 4096, h["split_w"] + h["split_w"] // 8 + 4096
        if need["split_k"] or need["split_w"]:
            k = max(k, h["cold_recs"] + h["cold_recs"] // 8 + C.NB * (C.SUB_N + 2))
            wv = max(wv, h["w_total"] + h["w_total"] // 8 + 4096)
        need["split_k"] = max(need["split_k"], k)
        need["split_w"] = max(need["split_w"], wv)
    if m & OVF_TABLE:
        need["bytes"] = max(need["bytes"], need["table"] * 16)
    return need


# ---------------------------------------------------------------- one attempt
class NotDeterministic(RuntimeError):
    """The figures of this attempt depend on which tokens win a race."""


WS = np.zeros(256, bool)
WS[[9, 10, 11, 12, 13, 32]] = True  # the cases use ASCII whitespace only


def token_spans(text):
    a = np.frombuffer(text, np.uint8)
    ws = WS[a]
    starts = np.nonzero(~ws & np.concatenate(([True], ws[:-1])))[0]
    ends = np.nonzero(~ws & np.concatenate((ws[1:], [True])))[0] + 1
    return starts, ends


def lowered(tok):
    return tok.lower() if max(tok) < 0x80 else tok.decode("utf-8").lower().encode("utf-8")


def is_short(word):
    return len(word) <= 16 and b"\0" not in word


def split_span(n, kk):
    return (n + (1 << kk) + 1) & ~1


class Figures:
    """What the kernels count over `text` on a grid of `grid` map workgroups,
    with `dictionary` (lowered words; empty: no dictionary, QF = QF_MAX)."""

    def __init__(self, text, dictionary=(), grid=GRID):
        self.text, self.grid, self.n = text, grid, len(text)
        self.dict = set(dictionary)
        self.qf = 1 if self.dict else C.QF_MAX
        starts, ends = token_spans(text)
        self.tokens = int(starts.size)
        nrows = -(-self.n // C.PAY)
        per, rem = divmod(nrows, grid)
        first = np.array([g * per + min(g, rem) for g in range(grid + 1)], np.int64)  # (k_map: rb)
        self.rows_of = np.diff(first)
        wg = np.searchsorted(first, starts // C.PAY, side="right") - 1
        uniq, inv = {}, np.empty(starts.size, np.int64)
        for i, (s, e) in enumerate(zip(starts.tolist(), ends.tolist())):
            inv[i] = uniq.setdefault(text[s:e], len(uniq))
        toks = list(uniq)
        low = [lowered(t) for t in toks]
        uni = np.array([max(t) >= 0x80 for t in toks], bool)
        short = np.array([is_short(w) for w in low], bool)
        tlen = np.array([len(t) for t in toks], np.int64)
        count = np.bincount(inv, minlength=len(toks))
        self.distinct_tokens, self.low = toks, low
        # Unicode lane
        self.u_n = int(count[uni].sum())
        self.u_lens = sorted(set(tlen[uni].tolist()))
        self.u_short_n = int(count[uni & short].sum())
        self.u_long_n = self.u_n - self.u_short_n
        self.u_arena = int((count[uni] * (tlen[uni] + tlen[uni] // 2 + 4)).sum())
        # long lane
        self.ascii_long_n = int(count[~uni & ~short].sum())
        self.long_words = {w for w, s in zip(low, short) if not s}
        self.ascii_long_words = {w for w, s, u in zip(low, short, uni) if not s and not u}
        # short words
        self.short_words = sorted({w for w, s in zip(low, short) if s})
        hx = Hashed(self.short_words)
        hof = dict(zip(self.short_words, hx.h.tolist()))
        self.short_part = bucket_of(hx.h).astype(np.int64)
        self.n_total = len(self.short_words) + len(self.long_words)
        self.bytes_total = sum(len(w) for w in self.short_words) + sum(len(w) for w in self.long_words)
        # cold candidates: short ASCII tokens outside the dictionary
        hot = np.array([w in self.dict for w in low], bool)
        self.dict_hit_words = len({w for w, a, u in zip(low, hot, uni) if a and not u})
        cold_d = ~uni & short & ~hot
        h_d = np.array([hof[w] if s else 0 for w, s in zip(low, short)], np.uint64)
        sel = cold_d[inv]
        h = h_d[inv][sel]
        sl = hbits(h, K.NB_LOG2, 2).astype(np.int64) if self.qf > 1 else np.zeros(h.shape, np.int64)
        key = (wg[sel] * C.NB + bucket_of(h).astype(np.int64)) * C.QF_MAX + sl
        self.slot_key, self.slot_cnt = np.unique(key, return_counts=True)
        # weighted records that do not depend on the capacities: Unicode short words by partition
        us = uni & short
        self.u_short_part = np.bincount(bucket_of(h_d[us]).astype(np.int64), count[us], C.NB).astype(np.int64)
        self.dict_part = np.bincount(bucket_of(np.array([hof[w] for w in self.dict if w in hof], np.uint64)).astype(np.int64),
                                     minlength=C.NB).astype(np.int64) if self.dict else np.zeros(C.NB, np.int64)

    # -- region fills
    def slot_wg(self):
        return self.slot_key // (C.NB * C.QF_MAX)

    def fills(self):
        """{(workgroup, partition, slice): cold records}."""
        return {(int(k) // (C.NB * C.QF_MAX), int(k) // C.QF_MAX % C.NB, int(k) % C.QF_MAX): int(c)
                for k, c in zip(self.slot_key, self.slot_cnt)}

    def spills_per_wg(self, cold_cap):
        rc = cold_cap // self.qf
        over = np.maximum(self.slot_cnt - rc, 0)
        return np.bincount(self.slot_wg(), over, self.grid).astype(np.int64)

    def attempt(self, caps):
        """The control block of one attempt at capacities `caps`."""
        rc = caps["cold"] // self.qf
        assert rc % 2 == 0 or self.qf == 1
        spills = self.spills_per_wg(caps["cold"])
        kept = np.minimum(spills, caps["spill"])
        h = {"tokens": self.tokens, "u_n": self.u_n, "qf": self.qf,
             "cold_need": int(self.slot_cnt.max()) * self.qf if self.slot_cnt.size else 0,
             "spill_need": int(spills.max()), "spills": int(spills.sum())}
        mask = OVF_POOL if (spills > caps["spill"]).any() else 0
        cold_n = np.minimum(self.slot_cnt, rc)
        h["cold_recs"] = int(cold_n.sum())
        # Unicode lane
        done = min(self.u_n, caps["u"])
        if self.u_n > caps["u"]:
            mask |= OVF_U
        if done == self.u_n and self.u_arena <= caps["arena"]:
            h["arena_n"], u_short, u_long, complete = self.u_arena, self.u_short_n, self.u_long_n, True
        else:
            if len(self.u_lens) != 1 or (self.u_short_n and self.u_long_n):
                raise NotDeterministic("Unicode tokens of several lengths or kinds compete for u[] or the arena")
            per = self.u_lens[0] + self.u_lens[0] // 2 + 4
            h["arena_n"] = done * per
            ok = min(done, caps["arena"] // per)
            u_short, u_long, complete = (ok, 0, False) if self.u_short_n else (0, ok, False)
        if h["arena_n"] > caps["arena"]:
            mask |= OVF_ARENA
        # long table
        h["long_n"] = self.ascii_long_n + u_long
        if complete:
            distinct_long = len(self.long_words)
        elif len(self.long_words) <= caps["long"]:
            distinct_long = None  # some subset: it fits whichever tokens were processed
        elif len(self.ascii_long_words) > caps["long"]:
            distinct_long = len(self.ascii_long_words)
        else:
            raise NotDeterministic("the long table's overflow depends on which Unicode tokens were processed")
        if distinct_long is not None and distinct_long > caps["long"]:
            mask |= OVF_LONG
        # weighted records
        h["w_n"] = self.dict_hit_words + u_short
        h["w_total"] = min(h["w_n"], caps["w"]) + int(kept.sum())
        if h["w_n"] > caps["w"] or h["w_total"] > caps["w"]:
            mask |= OVF_W
        if h["cold_recs"] + h["w_total"] > uniq_cap(caps, self.grid):
            mask |= OVF_POOL
        h.update(n_total=0, bytes_total=0, split_k=0, split_w=0, n_split=0)
        if not mask:
            assert complete
            nc = np.bincount(self.slot_key // C.QF_MAX % C.NB, cold_n, C.NB).astype(np.int64)
            over = np.maximum(self.slot_cnt - rc, 0)
            nw = (np.bincount(self.slot_key // C.QF_MAX % C.NB, over, C.NB).astype(np.int64) + self.u_short_part +
                  self.dict_part)
            distinct = np.bincount(self.short_part, minlength=C.NB)
            for b in np.nonzero(nc + nw > C.SPLIT_MIN)[0]:
                frac = distinct[b] / float(nc[b] + nw[b])
                if 0.25 <= frac < 0.75:
                    raise NotDeterministic("partition %d: a sampled distinct fraction near 0.5 decides its split" % b)
                if frac >= 0.75:  # (the estimate is capped at 1: kk for all records distinct)
                    kk = R.kk_for(int(nc[b] + nw[b]))
                    h["split_k"] += split_span(int(nc[b]), kk)
                    h["split_w"] += int(nw[b])
                    h["n_split"] += 1
            if h["split_k"] > caps["split_k"] or h["split_w"] > caps["split_w"]:
                mask |= OVF_SPLIT
        if not mask:
            h["n_total"], h["bytes_total"] = self.n_total, self.bytes_total
            if self.n_total > caps["table"]:
                mask |= OVF_TABLE
            if self.bytes_total > caps["bytes"]:
                mask |= OVF_BYTES
        h["overflow"] = mask
        return h


class EngineModel:
    """run_corpus over successive texts of one engine (reserve_bytes = 0)."""

    def __init__(self, grid=GRID):
        self.grid, self.caps, self.next_cold_cap = grid, None, 0

    def run(self, fig):
        """The ladder: one (control block, capacities) per attempt.  Raises
        RuntimeError where run_corpus gives up (GROW_RETRIES)."""
        want = initial_caps(fig.n, self.grid)
        want["cold"] = max(want["cold"], self.next_cold_cap)
        self.caps, _ = ensure_caps(self.caps, want)
        ladder = []
        for attempt in range(C.GROW_RETRIES + 1):
            h = fig.attempt(self.caps)
            ladder.append((h, dict(self.caps)))
            if not h["overflow"]:
                if h["spill_need"]:
                    self.next_cold_cap = max(self.next_cold_cap, cold_cap_for(self.caps, h, self.grid))
                return ladder
            if attempt >= C.GROW_RETRIES:
                break
            self.caps, _ = ensure_caps(self.caps, grow_for(self.caps, h, self.grid))
        raise RuntimeError("buffer growth did not converge: %s" % [mask_names(h["overflow"]) for h, _ in ladder])


def ladder_of(case):
    return EngineModel().run(case.figures)


def describe(ladder):
    return ["%s cold %d spill %d w %d" % (mask_names(h["overflow"]), c["cold"], c["spill"], c["w"]) for h, c in ladder]


# ---------------------------------------------------------------- dictionary sample model
def sample_counts(text):
    """{lowered word: count} of k_sample: the short NUL-free ASCII tokens that
    start in SAMPLE_PIECES pieces of SAMPLE_PIECE bytes (a word in two
    overlapping pieces counts twice)."""
    starts, ends = token_spans(text)
    n, pieces = len(text), K.SAMPLE_PIECES
    stride = n // pieces
    out = {}
    for i in range(pieces):
        ps = ((16 + stride * i) & ~15) - 16  # (internal coordinates start at 16)
        lo, hi = np.searchsorted(starts, ps), np.searchsorted(starts, ps + K.SAMPLE_PIECE)
        for s, e in zip(starts[lo:hi].tolist(), ends[lo:hi].tolist()):
            t = text[s:e]
            if len(t) <= 16 and max(t) < 0x80 and b"\0" not in t:
                w = t.lower()
                out[w] = out.get(w, 0) + 1
    return out


def dictionary_pick(text, max_words=None):
    """(words k_dict_pick takes, coverage of the gate): classes of 255 and more
    count as 255, the threshold is the smallest class from 2 whose suffix fits."""
    max_words = max_words or min(K.DICT_SLOTS, 4096)
    counts = sample_counts(text)
    cls = {w: min(c, 255) for w, c in counts.items()}
    hist = np.bincount(list(cls.values()) or [0], minlength=256)
    t = next((cc for cc in range(2, 256) if hist[cc:].sum() <= max_words), 256)
    cov_all = int((hist * np.arange(256)).sum())
    cov = int((hist[t:] * np.arange(t, 256)).sum()) if t < 256 else 0
    if cov < cov_all // K.DICT_MIN_COVER_INV:
        t = 256
    picked = [w for w, c in cls.items() if c >= t]
    if 2 <= t - 1 < 255:
        picked += [w for w, c in cls.items() if c == t - 1][:max_words - len(picked)]
    return picked, (cov, cov_all)


# ---------------------------------------------------------------- text builders
def spread(tokens, min_bytes=0):
    """The tokens in order, one per field of equal width (the width of the
    longest token + 1, or what reaches min_bytes), padded with spaces."""
    width = max(max(len(t) for t in tokens) + 1, -(-min_bytes // len(tokens)))
    return b"".join(t.ljust(width) for t in tokens)


def rows_text(rows):
    """A text whose row r (PAY bytes) holds exactly the tokens rows[r]."""
    out = []
    for toks in rows:
        line = b" ".join(toks)
        if len(line) >= C.PAY:
            raise R.CannotBuild("row of %d bytes" % len(line))
        out.append(line.ljust(C.PAY))
    return b"".join(out)


def first_rows(nrows, grid=GRID):
    per, rem = divmod(nrows, grid)
    return [g * per + min(g, rem) for g in range(grid + 1)]


def numbered(prefix, n, width, start=0):
    """n distinct ASCII words of prefix + a zero-padded number, `width` bytes."""
    return [prefix + (b"%0*d" % (width - len(prefix), i)) for i in range(start, start + n)]


def lettered(n, length=5):
    """n distinct lowercase words of `length` letters."""
    i = np.arange(n, dtype=np.int64)
    cols = [(i // 26 ** k % 26 + 97).astype(np.uint8) for k in range(length)]
    return np.stack(cols[::-1], axis=1).copy().view("S%d" % length).ravel().tolist()


NO_OVERLAP = R.MIN_ROWS * K.PAY  # a text of this size: the dictionary sample's pieces do not overlap


class Case:
    """A corpus, the engine flags it runs under and the ladder it claims.
    dictionary: the words the model assumes in the dictionary (a default engine
    with repeats); nodict: the engine runs with MOX_F_NO_DICT."""

    def __init__(self, name, text, ladder, nodict=False, dictionary=(), targets=None, claims=None):
        self.name, self.text, self.claimed, self.nodict, self.dictionary = name, text, ladder, nodict, list(dictionary)
        self.targets, self.claims = targets, claims or {}
        self._fig = None

    @property
    def figures(self):
        if self._fig is None:
            self._fig = Figures(self.text, self.dictionary)
        return self._fig


# ---------------------------------------------------------------- the cases
def table_alone():
    """100,000 distinct 5-byte words, each once: more than table_cap, and their
    500,000 bytes under bytes_cap."""
    return Case("table_alone", spread(lettered(100000), NO_OVERLAP), [OVF_TABLE, 0], targets="table")


def bytes_alone():
    """40,000 distinct 20-byte words: under table_cap and long_cap, their
    800,000 bytes over bytes_cap = 8 table_cap."""
    return Case("bytes_alone", spread(numbered(b"bytes", 40000, 20)), [OVF_BYTES, 0], targets="bytes")


LONG_EXTRA = 64


def long_fill():
    """65,536 + LONG_EXTRA distinct 17-byte words: the long table fills, every
    word after that probes all of it; LONG_EXTRA words are there twice, once in
    capitals.  The table then regrows to 2^18 slots (another mask), and the
    words' bytes overflow bytes_cap once the pass gets that far."""
    words = numbered(b"long", 65536 + LONG_EXTRA, 17)
    toks = list(words)
    step = len(words) // LONG_EXTRA
    for j in range(LONG_EXTRA):  # the repeat far from its first copy
        toks.insert((j * step * 7 + 31) % len(toks), words[j * step].upper())
    return Case("long_fill", spread(toks), [OVF_LONG, OVF_BYTES, 0], targets="long",
                claims={"distinct": len(words), "long_tokens": len(toks)})


def u_alone():
    """8,000 two-byte non-ASCII tokens: more than u_cap, while the arena (7
    bytes each) and w_cap hold all of them."""
    toks = [bytes(R.PAIRS2[i % len(R.PAIRS2)]) for i in range(8000)]
    return Case("u_alone", b" ".join(toks) + b" ", [OVF_U, 0], targets="u")


ARENA_TOKENS, ARENA_CHARS = 96, 1024
GROWING = ["\u0130", "\u023a", "\u023e"]  # 2 bytes each, 3 once lowered (i + U+0307, U+2C65, U+2C66)


def arena_alone():
    """96 non-ASCII tokens of 2,048 bytes; a third of them only of the letters
    that grow from 2 to 3 bytes when lowered (3,072 bytes into a reservation of
    3,076), the others of two-byte letters in both cases.  A quarter of the
    tokens repeat an earlier one: every word reaches the long table by arena
    reference, and a repeat compares two arena references over all its bytes."""
    rng = np.random.default_rng(0xA7E4A)
    two = [chr(c) for c in list(range(0xC0, 0xD7)) + list(range(0xE0, 0xF7)) + list(range(0x410, 0x450))]
    distinct = []
    for t in range(ARENA_TOKENS * 3 // 4):
        pool = GROWING if t % 3 == 0 else two
        distinct.append("".join(pool[i] for i in rng.integers(0, len(pool), ARENA_CHARS)).encode("utf-8"))
    toks = distinct + [distinct[(5 * j) % len(distinct)] for j in range(ARENA_TOKENS - len(distinct))]
    toks = [toks[i] for i in rng.permutation(len(toks))]
    return Case("arena_alone", b"\n".join(toks) + b"\n", [OVF_ARENA, 0], targets="arena",
                claims={"growing": sum(1 for t in range(len(distinct)) if t % 3 == 0)})


def w_alone():
    """One 1-byte word, 373 rows of 496 tokens: a workgroup has one or two rows,
    so at most 992 - 16 spills (spill_cap is 1,024), and all 256 together more
    than w_cap."""
    return Case("w_alone", b"a " * (373 * C.PAY // 2), [OVF_W, 0], nodict=True, targets="w")


def pool_ladder():
    """The same word over 2 MiB: eight or nine rows a workgroup, about 4,000
    spills each.  (The first attempt also reports OVF_W: k_hist counts the
    1,024 spills every workgroup kept, 262,144 in all, against w_cap.)"""
    return Case("pool_ladder", b"a " * (1 << 20), [OVF_POOL | OVF_W, OVF_W, 0], nodict=True)


EDGE_WGS = (3, 100, 177, 255)


def spill_edges(dictionary):
    """Count-1 words of one region slice, planted in the first row of four
    workgroups: rc - 1, rc, rc + 1 and rc + 2 of them (rc = 16 without a
    dictionary: the slice of one partition; rc = 64 with one: the partition).
    Without a dictionary the rest is count-1 filler of other partitions; with
    one it is 40 hot words that fill the dictionary, and six Unicode tokens."""
    P, q = 0x133, 2
    rc = 64 if dictionary else 16
    fills = [rc - 1, rc, rc + 1, rc + 2]
    if dictionary:
        ws = words_for(P << (32 - K.NB_LOG2), sum(fills), mask=R.part_mask(), seed=0x5ED)
    else:
        ws = words_for(((P << 2) | q) << (30 - K.NB_LOG2), sum(fills), mask=(R.M32 << (30 - K.NB_LOG2)) & R.M32, seed=0x5EE)
    first = first_rows(R.MIN_ROWS)
    planted, at = {}, 0
    for g, f in zip(EDGE_WGS, fills):
        planted[first[g]] = ws[at:at + f]
        at += f
    rng = np.random.default_rng(0x5E0)
    if dictionary:
        hot = [w for w, _, _ in R._filler(40, 0x5E1, {P})]
        uni = [w for w in words_for(0, 6, mask=0, seed=0x5E2, nonascii=True)]
        rows = []
        for r in range(R.MIN_ROWS):
            row = [hot[i] for i in rng.integers(0, len(hot), 100 if r not in planted else 30)]
            if r in planted:
                row = row[:15] + planted[r] + row[15:]
            if r % 131 == 7 and r // 131 < len(uni):
                row.append(uni[r // 131])
            rows.append(row)
        have = hot
    else:
        fill = [w for w, _, _ in R._filler(R.MIN_ROWS * 20, 0x5E3, {P})]
        rows = [planted.get(r, []) + fill[20 * r:20 * r + 20] for r in range(R.MIN_ROWS)]
        have = []
    return Case("spill_edges_dict" if dictionary else "spill_edges_nodict", rows_text(rows), [0], nodict=not dictionary,
                dictionary=have, claims={"part": P, "slice": 0 if dictionary else q, "fills": dict(zip(EDGE_WGS, fills)), "rc": rc,
                                         "spills": 3, "unicode": 6 if dictionary else 0})


KELVIN = "\u212a"


def long_refs():
    """The long table's byte compare (ref_byte) across reference kinds: one word
    as an ASCII token (corpus reference) and with KELVIN SIGN, which lowers to
    k (arena reference); two words of one length that differ in the last byte;
    a 3-byte word with a NUL byte in both spellings; words of 16 and 17 bytes
    with the same first 16."""
    u = lambda s: s.encode("utf-8")  # noqa: E731
    kel = [b"kelvinkelvinkelvin01", b"KelvinKELVINkelvin01", u(KELVIN + "elvin" + KELVIN + "ELVINkelvin01"),
           b"kelvinkelvinkelvin01", u("kelvin" + KELVIN + "elvinkelvin01"), b"KELVINKELVINKELVIN01", u(KELVIN + "ELVINKELVINKELVIN01"),
           b"kelvinkelvinkelvin01"]
    last = [b"abcdefghijklmnopqrstuvwxyA", b"abcdefghijklmnopqrstuvwxyB", b"ABCDEFGHIJKLMNOPQRSTUVWXYa", u("abcdefghij" + KELVIN + "lmnopqrstuvwxyb")]
    nul = [b"a\0k", b"A\0K", u("a\0" + KELVIN), u("A\0" + KELVIN), b"a\0k"]
    edge = [b"kixteen_bytes_wd", b"Kixteen_bytes_wdX", u(KELVIN + "ixteen_bytes_wd"), u(KELVIN + "ixteen_bytes_wdx"), b"kixteen_bytes_wdx",
            b"KIXTEEN_BYTES_WD"]
    plain = [b"the", b"quick", b"brown", b"fox", b"the", b"lazy", b"dog"]
    toks = []
    for i in range(max(len(kel), len(last), len(nul), len(edge), len(plain))):
        for group in (plain, kel, last, nul, edge):
            if i < len(group):
                toks.append(group[i])
    text = b"".join(t + (b" ", b"\n", b"\t")[i % 3] for i, t in enumerate(toks))
    expected = {b"kelvinkelvinkelvin01": 8, b"abcdefghijklmnopqrstuvwxya": 2, b"abcdefghijklmnopqrstuvwxyb": 2, b"a\0k": 5,
                b"kixteen_bytes_wd": 3, b"kixteen_bytes_wdx": 3, b"the": 2, b"quick": 1, b"brown": 1, b"fox": 1, b"lazy": 1,
                b"dog": 1}
    # (without a dictionary: on a text this small the sample's pieces overlap and the
    # few short words would form one, which the model of the regions does not follow)
    return Case("long_refs", text, [0], nodict=True, claims={"expected": expected, "kelvin": b"kelvinkelvinkelvin01"})


def ladder_all():
    """Short of everything at once, under 2 MiB, without a dictionary: a hot
    word over the first eight rows (one workgroup's spills past spill_cap),
    100,000 two-byte Unicode tokens (u_cap, the arena, w_cap), 65,600 distinct
    17-byte words (the long table), 8,300 distinct words of one partition (it
    splits: the split buffers start empty) and 33,000 more short words (with the
    others over table_cap and bytes_cap)."""
    P = 0x2C4
    hot = b"a " * (8 * C.PAY // 2)
    toks = [bytes(R.PAIRS2[i % len(R.PAIRS2)]) for i in range(100000)]
    toks += numbered(b"long", 65536 + LONG_EXTRA, 17)
    toks += words_for(P << (32 - K.NB_LOG2), 8300, mask=R.part_mask(), seed=0xA11)
    toks += [b"z" + w for w in lettered(33000)]
    rng = np.random.default_rng(0xA110)
    toks = [toks[i] for i in rng.permutation(len(toks))]
    text = hot + b"".join(t + b" " for t in toks)
    want = OVF_POOL | OVF_W | OVF_U | OVF_ARENA | OVF_LONG | OVF_SPLIT | OVF_TABLE | OVF_BYTES
    return Case("ladder_all", text, None, nodict=True, claims={"union": want, "part": P})


CASES = {
    "table_alone": table_alone,
    "bytes_alone": bytes_alone,
    "long_fill": long_fill,
    "u_alone": u_alone,
    "arena_alone": arena_alone,
    "w_alone": w_alone,
    "pool_ladder": pool_ladder,
    "spill_edges_nodict": lambda: spill_edges(False),
    "spill_edges_dict": lambda: spill_edges(True),
    "long_refs": long_refs,
    "ladder_all": ladder_all,
}
ALONE = [n for n in CASES if n.endswith("_alone")]

_built = {}


def case(name):
    """The case `name`, built once per process."""
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]
