"""GPU: the shard-window contract of mox_run_range at the row geometry of k_map
(map-oxidize_amd/csrc/mox_kernels.hip), against the model of window_cases.py
(pinned to the C oracle by test_window_model.py, which also asserts that the
case lists reach the edges they are built for).  Word counts are integers:
every comparison is exact.

Every case runs with and without the dictionary (the `eng` fixture), on
buffers uploaded once per test.  A case asserts the sorted (word, count) list,
the token count and that the counts sum to it -- or, for a non-final buffer,
HaloError exactly when the model says so, naming the model's byte.

Test -> what it reaches in k_map:
  row_edge_plants -> tokens, multi-byte whitespace and letters, NUL and control words across
      the edge between two ordinary rows, after row 0 and among the last three rows (edge rows:
      e_lo, e_hi, fix16), with the row grid shifted by the pointer's misalignment
  own_range_sweep -> the own_lo / own_hi start masks of do_row and the own range of slow_starts,
      byte by byte across each kind of item, in rows of the common list builder ("ascii"), of the
      checked one (its control bytes) and of the Unicode walk ("dense")
  non_final_buffers -> near_end / lim and `p + len >= lim` of do_row, generic_token's halo_err,
      utf8_check's 2 in slow_starts, fix16's padding past hi, and the host's MOX_EHALO check
  final_buffer_ends_at_hi -> the same windows with at_end set: fix16 and the clamps of byte_at
      hide the device memory past hi
  long_token_reaches_the_end -> generic_token's halo_err from rows far before hi
  cut_character, invalid_byte -> utf8_check's 1 against its 2, and the host's order of checks
  async_halo -> the same through complete_async

One-line changes of k_map that these tests were seen to catch (each rebuilt and
run once, nothing of it kept): `p + len > lim` for `>=` in do_row
(non_final_buffers), the own_hi start mask deleted (own_range_sweep[ascii],
non_final_buffers), the own_lo mask one bit short (own_range_sweep,
non_final_buffers), `p > own_hi` in slow_starts (own_range_sweep[dense],
non_final_buffers)."""
import functools
import re

import pytest

import mox
import window_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[0, mox.MOX_F_NO_DICT], ids=["dict", "nodict"])
def eng(request):
    e = mox.Engine(device=0, flags=request.param)
    yield e
    e.close()


class Blob:
    """Buffers packed 256 bytes apart in one device allocation, uploaded once
    at `mis` bytes past an aligned address."""

    def __init__(self, e, bufs, mis=0):
        self.e = e
        self.offs = []
        blob = bytearray()
        for b in bufs:
            self.offs.append(len(blob))
            blob += b
            blob += b" " * (-len(blob) % 256)
        self.d = e.alloc(len(blob) + 256)
        assert self.d % 16 == 0
        self.mis = mis
        e.h2d(self.d + mis, bytes(blob) or b" ")

    def ptr(self, i=0):
        return self.d + self.mis + self.offs[i]

    def free(self):
        self.e.free(self.d)


def run(e, ptr, n, own_begin, own_end, at_end):
    """The outcome of one pass in the model's terms."""
    try:
        e.run_range(ptr, n, own_begin, own_end, at_end)
    except mox.HaloError as ex:
        assert ex.code == mox.MOX_EHALO
        return ("halo", int(re.search(r"token at byte (\d+) runs past", str(ex)).group(1)))
    except mox.Utf8Error as ex:
        assert ex.code == mox.MOX_EUTF8
        return ("utf8",)
    t = e.fetch()
    try:
        items, tokens = t.sorted_items(), t.tokens
    finally:
        t.close()
    assert sum(c for _, c in items) == tokens, (own_begin, own_end, tokens)
    return ("table", items, tokens)


def explain(what, got, want, model, lo):
    """Case parameters, the first word that differs and where it stands in the buffer."""
    if got[0] != "table" or want[0] != "table":
        return "%s: got %r, want %r" % (what, got[:2] if got[0] != "table" else ("table", got[2]),
                                        want[:2] if want[0] != "table" else ("table", want[2]))
    g, w = dict(got[1]), dict(want[1])
    for word in sorted(set(g) | set(w)):
        if g.get(word, 0) != w.get(word, 0):
            return "%s: word %r counted %d, want %d (tokens %d, want %d); it starts at buffer offsets %r" % (
                what, word, g.get(word, 0), w.get(word, 0), got[2], want[2], model.occurrences(word, lo)[:8])
    return "%s: tokens %d, want %d" % (what, got[2], want[2])


class Failures:
    def __init__(self):
        self.msgs, self.ran = [], 0

    def check(self, what, got, want, model, lo=0):
        self.ran += 1
        if got != want:
            self.msgs.append(explain(what, got, want, model, lo))

    def done(self, expected_cases):
        assert self.ran == expected_cases
        assert not self.msgs, "%d of %d cases differ:\n%s" % (len(self.msgs), self.ran, "\n".join(self.msgs[:12]))


AFTER = b"a b a"


def assert_usable(e, ptr):
    """After an error the engine counts AFTER (at ptr) correctly."""
    assert run(e, ptr, len(AFTER), 0, len(AFTER), True) == ("table", [(b"a", 2), (b"b", 1)], 3)


# ------------------------------------------------------------------ 3a
@functools.lru_cache(maxsize=None)
def planted():
    cases = W.row_edge_cases() + W.lane_cases()
    out = []
    for c in cases:
        m = W.Model(c.data)
        out.append((c, m, m.expected(0, len(c.data), 0, len(c.data), True)))
    return out


@pytest.mark.parametrize("mis", W.MIS)
def test_row_edge_plants(eng, mis):
    """Whole buffers, final: every (item, delta) of window_cases.PAIRS across a
    row edge of each kind and at lane boundaries (test_row_edge_cases_geometry,
    test_lane_cases_geometry), the device pointer `mis` bytes past a 16-byte
    line, which moves the row grid by as much against the text."""
    cases = planted()
    blob = Blob(eng, [c.data for c, _, _ in cases], mis)
    f = Failures()
    try:
        for i, (c, m, want) in enumerate(cases):
            got = run(eng, blob.ptr(i), len(c.data), 0, len(c.data), True)
            f.check("%s mis %d (%d bytes, plants %r)" % (c.name, mis, len(c.data), [(W.ITEMS[W.PAIRS[pi][0]][0], W.PAIRS[pi][1], pos) for pi, pos in c.plants][:4]),
                    got, want, m)
    finally:
        blob.free()
    f.done(1 + len(W.PAIRS) + len(W.lane_cases()))


# ------------------------------------------------------------------ 3b
@pytest.mark.parametrize("mis", [0, 9])
@pytest.mark.parametrize("kind", ["dense", "ascii"])
def test_own_range_sweep(eng, kind, mis):
    """own_begin and own_end byte by byte through four windows of a final
    4,500-byte buffer (test_sweep_corpus_windows) and 300 seeded pairs; the row
    grid starts at the 16-byte line of own_begin, which `mis` moves."""
    D, _ = W.sweep_corpus(kind)
    m = W.Model(D)
    ranges = W.sweep_ranges(len(D), 7 if kind == "dense" else 8)
    blob = Blob(eng, [D], mis)
    f = Failures()
    try:
        for ob, oe in ranges:
            f.check("%s mis %d own [%d, %d) of %d" % (kind, mis, ob, oe, len(D)), run(eng, blob.ptr(), len(D), ob, oe, True),
                    m.expected(0, len(D), ob, oe, True), m)
    finally:
        blob.free()
    f.done(len(ranges))


def test_own_begin_needs_left_context(eng):
    D, _ = W.sweep_corpus("ascii")
    blob = Blob(eng, [D, AFTER])
    try:
        for ob in (1, 2, 3):
            with pytest.raises(mox.MoxError) as ei:
                eng.run_range(blob.ptr(), len(D), ob, len(D), True)
            assert ei.value.code == mox.MOX_EINVAL and not isinstance(ei.value, (mox.HaloError, mox.Utf8Error))
            assert_usable(eng, blob.ptr(1))
    finally:
        blob.free()


# ------------------------------------------------------------------ 3c
@pytest.mark.parametrize("place", list(W.HALO_PLACES))
def test_non_final_buffers(eng, place):
    """Buffers D[lo:hi] that do not end the corpus, hi at every byte of a window
    of word ends, a NUL word, a 3-byte whitespace, a 2-byte letter and an emoji
    (test_halo_cases_balance): HaloError naming the model's byte where the model
    says so, the model's table otherwise; after every error the engine still
    counts.  The device holds the corpus past hi, so a read past hi would find
    the separators that the buffer lacks."""
    D, _, _, _ = W.halo_corpus(place)
    m = W.Model(D)
    cases = W.halo_cases(place)
    blob = Blob(eng, [D, AFTER])
    f = Failures()
    errors = 0
    try:
        for lo, hi, ob, oe in cases:
            want = m.expected(lo, hi, ob, oe, False)
            got = run(eng, blob.ptr() + lo, hi - lo, ob, oe, False)
            f.check("%s D[%d:%d] own [%d, %d)" % (place, lo, hi, ob, oe), got, want, m, lo)
            if got[0] != "table":
                errors += 1
                assert_usable(eng, blob.ptr(1))
    finally:
        blob.free()
    assert errors >= 50
    f.done(len(cases))


@pytest.mark.parametrize("place", list(W.HALO_PLACES))
def test_final_buffer_ends_at_hi(eng, place):
    """The same windows as the end of the corpus: the buffer D[lo:hi] is final
    while the device memory goes on with the rest of D, so the last token is
    what D[:hi] ends with and nothing of D[hi:] may show."""
    D, a, b, _ = W.halo_corpus(place)
    blob = Blob(eng, [D])
    f = Failures()
    ran = 0
    try:
        for hi in range(a, b + 1):
            m = W.Model(D[:hi].decode("utf-8", "ignore").encode())  # (a cut character: test_cut_character_...)
            if len(m.D) != hi:
                continue
            for lo, ob in ((0, 0), (0, 4), (1, 4), (4, 4)):
                f.check("%s final D[%d:%d] own [%d, %d)" % (place, lo, hi, ob, hi - lo),
                        run(eng, blob.ptr() + lo, hi - lo, ob, hi - lo, True), m.expected(lo, hi, ob, hi - lo, True), m, lo)
                ran += 1
    finally:
        blob.free()
    assert ran == 4 * (b + 1 - a - 6)
    f.done(ran)


def test_long_token_reaches_the_end_from_rows_back(eng):
    """A token of 2,500 bytes that starts rows before hi: MOX_EHALO when hi lies
    in it or at its end and its first byte is owned, however far own_end is
    from hi; the table when it is not owned or a space follows inside the buffer."""
    start = 1500
    D = W.filler(start - 1) + b" " + b"Xy" * 1250 + b" " + W.filler(300, 2)
    end = start + 2500
    m = W.Model(D)
    blob = Blob(eng, [D, AFTER])
    f = Failures()
    n = halos = 0
    try:
        for hi in (start + 1, start + 17, start + 1000, end - 1, end, end + 1, end + 40):
            for oe in (start, start + 1, min(hi, start + 16), hi):
                for lo, ob in ((0, 0), (1, 4), (0, start), (0, start + 1)):
                    if ob > oe - lo:
                        continue
                    want = m.expected(lo, hi, ob, oe - lo, False)
                    got = run(eng, blob.ptr() + lo, hi - lo, ob, oe - lo, False)
                    f.check("long token D[%d:%d] own [%d, %d)" % (lo, hi, ob, oe - lo), got, want, m, lo)
                    n += 1
                    halos += want[0] == "halo"
                    if got[0] != "table":
                        assert_usable(eng, blob.ptr(1))
    finally:
        blob.free()
    assert n > 80 and halos >= 20 and n - halos >= 20
    f.done(n)


def cut_sites():
    """(hi, first byte of the cut character) for every way hi cuts a character of the halo window."""
    D, _, _, spans = W.halo_corpus("row0")
    out = []
    for p in range(spans[0][1], spans[-1][2]):
        if (D[p] & 0xC0) == 0x80:
            lead = p
            while (D[lead] & 0xC0) == 0x80:
                lead -= 1
            out.append((p, lead))
    assert len(out) == 2 + 1 + 3
    return D, out


def test_cut_character_at_corpus_end_is_utf8(eng):
    """The cut that is MOX_EHALO in a non-final buffer is invalid UTF-8 in a final one."""
    D, sites = cut_sites()
    m = W.Model(D)
    blob = Blob(eng, [D, AFTER])
    try:
        for hi, lead in sites:
            assert m.expected(0, hi, 0, hi, True) == ("utf8",)
            assert run(eng, blob.ptr(), hi, 0, hi, True) == ("utf8",), hi
            assert_usable(eng, blob.ptr(1))
            assert run(eng, blob.ptr(), hi, lead, hi, False) == ("halo", lead), hi
            assert_usable(eng, blob.ptr(1))
    finally:
        blob.free()


def test_invalid_byte_comes_before_halo(eng):
    """An invalid byte in the own range and a token that reaches the end of a
    non-final buffer: the UTF-8 error is the one reported."""
    bufs = [b"abc \xffx tail", b"one \xc3( two", W.filler(2000) + b" \xf0\x9f\x98 x " + W.filler(50, 4)[:-1] + b"z"]
    blob = Blob(eng, bufs + [AFTER])
    try:
        for i, b in enumerate(bufs):
            assert b[-1:] not in b" \t\n"
            assert run(eng, blob.ptr(i), len(b), 0, len(b), False) == ("utf8",), i
            assert_usable(eng, blob.ptr(len(bufs)))
    finally:
        blob.free()


def test_async_halo_is_reported_by_the_completing_call(eng):
    """run_range_async: a halo pass fails the call that completes it -- the next
    async call, whose own pass then yields its exact table, or run_wait."""
    D, _, _, spans = W.halo_corpus("row0")
    m = W.Model(D)
    hi = spans[1][2] - 1  # the end of the 16-byte word: it reaches hi exactly
    want_halo = m.expected(0, hi, 0, hi, False)
    assert want_halo == ("halo", spans[1][1])
    want = m.expected(0, len(D), 0, len(D), True)
    blob = Blob(eng, [D, AFTER])
    try:
        # (sizes the engine's buffers: an async call that has to grow them completes the pending pass first)
        assert run(eng, blob.ptr(), len(D), 0, len(D), True) == want
        eng.run_range_async(blob.ptr(), hi, 0, hi, False)
        with pytest.raises(mox.HaloError) as ei:
            eng.run_range_async(blob.ptr(), len(D), 0, len(D), True)
        assert ei.value.code == mox.MOX_EHALO and "byte %d " % want_halo[1] in str(ei.value)
        eng.run_wait()
        t = eng.fetch()
        try:
            assert (t.sorted_items(), t.tokens) == (want[1], want[2])
        finally:
            t.close()
        eng.run_range_async(blob.ptr(), hi, 0, hi, False)
        with pytest.raises(mox.HaloError) as ei:
            eng.run_wait()
        assert "byte %d " % want_halo[1] in str(ei.value)
        with pytest.raises(mox.MoxError) as ei:
            eng.fetch()
        assert ei.value.code == mox.MOX_ESTATE
        assert_usable(eng, blob.ptr(1))
    finally:
        blob.free()
