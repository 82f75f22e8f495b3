"""Python binding of the MI355X word-count engine (ctypes over include/mox.h).

Host-side mirror of the reference's hot path (/root/reference/src/main.rs):

* ``count_words(data)`` / ``Engine.count`` -- ``split_file`` + ``map_phase`` +
  ``reduce_phase`` (main.rs:16-22): bytes -> {word: count}.  Invalid UTF-8 raises
  ``Utf8Error`` (the reference's ``io::ErrorKind::InvalidData`` abort, main.rs:44).
* ``Engine.count_file(path)`` -- the same from a file (main.rs:10, :36-51).
* ``write_final_result`` / ``top_words`` -- the reference's output layer
  (main.rs:170-192).

The compute runs in libmox.so (HIP kernels for gfx950).  There is no CPU
fallback: if the library is missing or no GPU is present, calls raise.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmox.so")

MOX_OK = 0
MOX_EINVAL = -1
MOX_EUTF8 = -2
MOX_ENOMEM = -3
MOX_EHIP = -4
MOX_EIO = -5
MOX_ERCCL = -6
MOX_ESTATE = -7
MOX_EHALO = -8

MOX_F_NO_DICT = 0x1
MOX_F_SORT_BYTES = 0x2  # fetch returns the words bytewise ascending (Rust String Ord)
MOX_F_TIMING = 0x4
MOX_F_TIMING_MAP = 0x8  # HIP events around the map kernel only

UNIQUE_ID_BYTES = 128
TOP_MAX = 4096  # MOX_TOP_MAX: the most words Engine.top_words selects
LOOKUP_MAX = 1 << 20  # MOX_LOOKUP_MAX: the most words one Engine.lookup call takes
LOOKUP_NONE = (1 << 64) - 1  # MOX_LOOKUP_NONE: the index of a word the result does not hold
FILTER_PREFIX_MAX = 16  # MOX_FILTER_PREFIX_MAX: the longest prefix Engine.filter_result takes
FILTER_WORDS_DROP = 0   # MOX_FILTER_WORDS_DROP: listed words are removed (stop list)
FILTER_WORDS_KEEP = 1   # MOX_FILTER_WORDS_KEEP: only listed words survive (vocabulary)
FILTER_COUNT_ONLY = 0x1  # MOX_FILTER_COUNT_ONLY: fill the info, leave the result as it is
JOIN_SEMI = 0  # MOX_JOIN_SEMI: Engine.join_total keeps the result's words the total holds
JOIN_ANTI = 1  # MOX_JOIN_ANTI: ... the result's words the total lacks
JOIN_COUNTS_RESULT = 0  # MOX_JOIN_COUNTS_RESULT: kept rows keep their own count
JOIN_COUNTS_TOTAL = 1   # MOX_JOIN_COUNTS_TOTAL: kept rows take the total's count (semi only)
JOIN_COUNTS_MIN = 2     # MOX_JOIN_COUNTS_MIN: kept rows take the smaller of both counts (semi only)
JOIN_COUNT_ONLY = 0x1   # MOX_JOIN_COUNT_ONLY: fill the info, leave the result as it is
JOIN_MAX_WORDS = 0xFFFFFFFE  # MOX_JOIN_MAX_WORDS: the most rows of the result Engine.join_total takes
_JOIN_MODES = {"semi": JOIN_SEMI, "anti": JOIN_ANTI}
_JOIN_COUNTS = {"result": JOIN_COUNTS_RESULT, "total": JOIN_COUNTS_TOTAL, "min": JOIN_COUNTS_MIN}
RANK_ASCENDING = 0x1  # MOX_RANK_ASCENDING: Engine.rank_result orders least frequent first
RANK_MAX_WORDS = (1 << 32) - 1  # MOX_RANK_MAX_WORDS: the most words Engine.rank_result takes
REKEY_TRIM_ASCII_PUNCT = 0x1  # MOX_REKEY_TRIM_ASCII_PUNCT: Engine.rekey_result strips ASCII punctuation
# {MOX_REKEY_PUNCT_LO, MOX_REKEY_PUNCT_HI}: string.punctuation as a 128-bit set, bit (b & 63) of word b >> 6
ASCII_PUNCT = (0xFC00FFFE00000000, 0x78000001F8000001)
FIND_EXACT = 0   # MOX_FIND_EXACT: Engine.find gives the row whose word equals the key
FIND_PREFIX = 1  # MOX_FIND_PREFIX: the rows whose word starts with the key
FIND_LOWER = 2   # MOX_FIND_LOWER: first = last = the number of rows bytewise below the key
FIND_MAX = 1 << 20  # MOX_FIND_MAX: the most keys one Engine.find call takes
_FIND_MODES = {"exact": FIND_EXACT, "prefix": FIND_PREFIX, "lower": FIND_LOWER}
HIST_COUNT = 0  # MOX_HIST_COUNT: Engine.histogram bins by the row's count (the frequency spectrum)
HIST_BYTES = 1  # MOX_HIST_BYTES: ... by the word's length in bytes
HIST_CHARS = 2  # MOX_HIST_CHARS: ... by the word's character starts (bytes b with (b & 0xC0) != 0x80)
HIST_FIRST = 3  # MOX_HIST_FIRST: ... by the word's first character (hist_first_bytes decodes the key)
HIST_RANGE = 0x1  # MOX_HIST_RANGE: only rows [first, first + rows)
HIST_MAX_WORDS = (1 << 32) - 1  # MOX_HIST_MAX_WORDS: the most rows one Engine.histogram call takes
_HIST_KEYS = {"count": HIST_COUNT, "bytes": HIST_BYTES, "chars": HIST_CHARS, "first": HIST_FIRST}


def hist_first_bytes(key):
    """The bytes of a HIST_FIRST key: the word's first byte and the continuation
    bytes behind it, at most 4 (for valid UTF-8: the first character's encoding);
    b"" for key 0."""
    key = int(key)
    return (key >> 8).to_bytes(4, "big")[:key & 0xFF]


class MoxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mox error %d: %s" % (code, msg))
        self.code = code


class Utf8Error(MoxError):
    """Input is not valid UTF-8 (reference: tokio lines() -> InvalidData)."""


class HaloError(MoxError):
    """MOX_EHALO: an owned token or character runs past the end of a non-final shard buffer."""


MAX_GPUS = 16
XPORT_RCCL = 0  # engine group: RCCL communicators over xGMI
XPORT_COPY = 1  # engine group: device-to-device copies (members may share a GPU)


class Config(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int),
        ("flags", ctypes.c_uint32),
        ("dict_words", ctypes.c_uint32),
        ("sample_pieces", ctypes.c_uint32),
        ("reserve_bytes", ctypes.c_uint64),
        ("n_gpus", ctypes.c_uint32),
        ("transport", ctypes.c_uint32),
        ("n_devices", ctypes.c_uint32),
        ("devices", ctypes.c_int32 * MAX_GPUS),
        ("reserved", ctypes.c_uint32 * 5),
    ]


class Shard(ctypes.Structure):
    _fields_ = [
        ("d_buf", ctypes.c_void_p),
        ("buf_len", ctypes.c_size_t),
        ("own_begin", ctypes.c_size_t),
        ("own_end", ctypes.c_size_t),
        ("at_corpus_end", ctypes.c_int),
    ]


class AccumInfo(ctypes.Structure):
    """mox_accum_info: the accumulator's folds, distinct words, tokens and device bytes."""
    _fields_ = [
        ("passes", ctypes.c_uint64),
        ("words", ctypes.c_uint64),
        ("tokens", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
    ]


class LookupInfo(ctypes.Structure):
    """mox_lookup_info: queries, distinct query words, found positions, equal-tag byte mismatches."""
    _fields_ = [
        ("queries", ctypes.c_uint64),
        ("distinct", ctypes.c_uint64),
        ("found", ctypes.c_uint64),
        ("tag_mismatch", ctypes.c_uint64),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class Filter(ctypes.Structure):
    """mox_filter: the predicate of mox_filter_result."""
    _fields_ = [
        ("min_count", ctypes.c_uint64),
        ("max_count", ctypes.c_uint64),
        ("min_len", ctypes.c_uint64),
        ("max_len", ctypes.c_uint64),
        ("prefix", ctypes.c_void_p),
        ("prefix_len", ctypes.c_uint64),
        ("words", ctypes.c_void_p),
        ("word_offs", ctypes.POINTER(ctypes.c_uint64)),
        ("n_words", ctypes.c_uint64),
        ("words_mode", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class FilterInfo(ctypes.Structure):
    """mox_filter_info: words and tokens in and kept, kept bytes, list words found, device bytes, ms."""
    _fields_ = [
        ("words_in", ctypes.c_uint64),
        ("words_kept", ctypes.c_uint64),
        ("tokens_in", ctypes.c_uint64),
        ("tokens_kept", ctypes.c_uint64),
        ("bytes_kept", ctypes.c_uint64),
        ("list_found", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms", ctypes.c_double),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class Join(ctypes.Structure):
    """mox_join: the spec of mox_join_total."""
    _fields_ = [
        ("mode", ctypes.c_uint32),
        ("counts", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("pad", ctypes.c_uint32),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class JoinInfo(ctypes.Structure):
    """mox_join_info: rows and tokens of the result and of the total, matched and kept words, the overlap sums, device bytes, ms."""
    _fields_ = [
        ("words_in", ctypes.c_uint64),
        ("words_total", ctypes.c_uint64),
        ("words_matched", ctypes.c_uint64),
        ("words_kept", ctypes.c_uint64),
        ("tokens_in", ctypes.c_uint64),
        ("tokens_total", ctypes.c_uint64),
        ("tokens_matched_result", ctypes.c_uint64),
        ("tokens_matched_total", ctypes.c_uint64),
        ("tokens_min", ctypes.c_uint64),
        ("tokens_kept", ctypes.c_uint64),
        ("bytes_kept", ctypes.c_uint64),
        ("tag_mismatch", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms", ctypes.c_double),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class RankInfo(ctypes.Structure):
    """mox_rank_info: words and tokens of the result, its largest count, radix passes run, device bytes, ms."""
    _fields_ = [
        ("words", ctypes.c_uint64),
        ("tokens", ctypes.c_uint64),
        ("max_count", ctypes.c_uint64),
        ("digit_passes", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms", ctypes.c_double),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class Rekey(ctypes.Structure):
    """mox_rekey: the spec of mox_rekey_result."""
    _fields_ = [
        ("trim_set", ctypes.c_uint64 * 2),
        ("max_chars", ctypes.c_uint64),
        ("flags", ctypes.c_uint32),
        ("pad", ctypes.c_uint32),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class RekeyInfo(ctypes.Structure):
    """mox_rekey_info: words in, out, changed and dropped, tokens in, out and dropped, bytes out, device bytes, ms."""
    _fields_ = [
        ("words_in", ctypes.c_uint64),
        ("words_out", ctypes.c_uint64),
        ("words_changed", ctypes.c_uint64),
        ("words_dropped", ctypes.c_uint64),
        ("tokens_in", ctypes.c_uint64),
        ("tokens_out", ctypes.c_uint64),
        ("tokens_dropped", ctypes.c_uint64),
        ("bytes_out", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms", ctypes.c_double),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class FindInfo(ctypes.Structure):
    """mox_find_info: keys, keys with a non-empty range, rows in all ranges, whether the tile pass ran, device bytes, ms."""
    _fields_ = [
        ("queries", ctypes.c_uint64),
        ("matched", ctypes.c_uint64),
        ("rows", ctypes.c_uint64),
        ("tile_pass", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms", ctypes.c_double),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class Hist(ctypes.Structure):
    """mox_hist: the key (HIST_*), the flags (HIST_RANGE) and the row range."""
    _fields_ = [
        ("key", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
        ("first", ctypes.c_uint64),
        ("rows", ctypes.c_uint64),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class HistInfo(ctypes.Structure):
    """mox_hist_info: rows and tokens histogrammed, bins, the largest key, radix passes, device bytes, ms."""
    _fields_ = [
        ("words", ctypes.c_uint64),
        ("tokens", ctypes.c_uint64),
        ("bins", ctypes.c_uint64),
        ("max_key", ctypes.c_uint64),
        ("digit_passes", ctypes.c_uint64),
        ("device_bytes", ctypes.c_uint64),
        ("ms", ctypes.c_double),
        ("reserved", ctypes.c_uint64 * 4),
    ]


class _HistTable(ctypes.Structure):
    """mox_hist_table: library-owned until mox_hist_free."""
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("words", ctypes.c_uint64),
        ("tokens", ctypes.c_uint64),
        ("keys", ctypes.POINTER(ctypes.c_uint64)),
        ("bin_words", ctypes.POINTER(ctypes.c_uint64)),
        ("bin_tokens", ctypes.POINTER(ctypes.c_uint64)),
        ("first_row", ctypes.POINTER(ctypes.c_uint64)),
    ]


class _Table(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint64),
        ("tokens", ctypes.c_uint64),
        ("counts", ctypes.POINTER(ctypes.c_uint64)),
        ("offs", ctypes.POINTER(ctypes.c_uint64)),
        ("bytes", ctypes.POINTER(ctypes.c_uint8)),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("bytes", ctypes.c_uint64),
        ("tokens", ctypes.c_uint64),
        ("uniques", ctypes.c_uint64),
        ("dict_words", ctypes.c_uint64),
        ("cold_records", ctypes.c_uint64),
        ("weighted_records", ctypes.c_uint64),
        ("unicode_tokens", ctypes.c_uint64),
        ("long_tokens", ctypes.c_uint64),
        ("chunks", ctypes.c_uint64),
        ("retries", ctypes.c_uint32),
        ("max_subpasses", ctypes.c_uint32),
        ("ms_run", ctypes.c_double),
        ("ms_dict", ctypes.c_double),
        ("ms_map", ctypes.c_double),
        ("ms_lanes", ctypes.c_double),
        ("ms_reduce", ctypes.c_double),
        ("ms_finalize", ctypes.c_double),
        ("ms_h2d", ctypes.c_double),
        ("ms_d2h", ctypes.c_double),
        ("ms_exchange", ctypes.c_double),
        ("reduce_units", ctypes.c_uint64),
        ("split_partitions", ctypes.c_uint32),
        ("async_reruns", ctypes.c_uint32),
        ("x_bytes_sent", ctypes.c_uint64),
        ("x_bytes_recv", ctypes.c_uint64),
        ("gather_bytes", ctypes.c_uint64),
        ("ms_gather", ctypes.c_double),
        ("path_hits", ctypes.c_uint64 * 8),
        ("ms_sort", ctypes.c_double),
        ("ms_local", ctypes.c_double),
        ("n_gpus", ctypes.c_uint32),
        ("async_dropped", ctypes.c_uint32),
        ("x_ranged", ctypes.c_uint32),
        ("x_pad", ctypes.c_uint32),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["path_hits"] = [int(x) for x in self.path_hits]
        return d


# int (*)(void* user, const void* send, const uint64_t* send_bytes, void* recv, const uint64_t* recv_bytes)
_A2A_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                           ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64))

# exactness-fallback counters (mox_stats.path_hits; collision check build only)
PATH_DICT_SAMEHASH, PATH_LONG_EQHASH, PATH_SORT_RESORT, PATH_SORT_TO_RED, PATH_RED_TAG, PATH_SMALL_TAG = range(6)
HC_LIB_PATH = os.path.join(_HERE, "libmox_hc.so")  # forced-collision check build (Makefile `hc`)
CHECK_LIB_PATH = os.path.join(_HERE, "libmox_check.so")  # bounds-check build (Makefile `check`)

_libs = {}


def lib(path=None):
    """Load libmox.so, or the library at ``path`` (a check build), once per path.
    Fails loudly: there is no fallback path."""
    if path is None:
        path = os.environ.get("MOX_LIB", LIB_PATH)  # diagnostics builds only (tools/)
    _lib = _libs.get(path)
    if _lib is None:
        if not os.path.exists(path):
            raise MoxError(MOX_ESTATE, "%s not built (run `make` or __graft_entry__.build())" % path)
        L = ctypes.CDLL(path)
        P, U64, I, VP = ctypes.POINTER, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p
        sz = ctypes.c_size_t
        sig = {
            "mox_last_error": ([], ctypes.c_char_p),
            "mox_abi_version": ([], I),
            "mox_engine_create": ([P(Config), P(VP)], I),
            "mox_engine_destroy": ([VP], None),
            "mox_set_flags": ([VP, ctypes.c_uint32], I),
            "mox_count": ([VP, VP, sz, P(P(_Table))], I),
            "mox_count_file": ([VP, ctypes.c_char_p, P(P(_Table))], I),
            "mox_table_free": ([P(_Table)], None),
            "mox_table_sort_bytes": ([P(_Table)], I),
            "mox_run_device": ([VP, VP, sz], I),
            "mox_run_range": ([VP, VP, sz, sz, sz, I], I),
            "mox_run_range_async": ([VP, VP, sz, sz, sz, I], I),
            "mox_run_wait": ([VP], I),
            "mox_fetch_table": ([VP, P(P(_Table))], I),
            "mox_sort_result": ([VP], I),
            "mox_top_words": ([VP, sz, P(P(_Table))], I),
            "mox_write_result": ([VP, ctypes.c_char_p], I),
            "mox_result_text": ([VP, P(P(ctypes.c_uint8)), P(U64)], I),
            "mox_text_free": ([P(ctypes.c_uint8)], None),
            "mox_run_file": ([VP, ctypes.c_char_p], I),
            "mox_accumulate": ([VP], I),
            "mox_accumulate_file": ([VP, ctypes.c_char_p, U64], I),
            "mox_accumulate_reset": ([VP], I),
            "mox_accumulate_info": ([VP, P(AccumInfo)], I),
            "mox_lookup_words": ([VP, VP, P(U64), U64, P(U64), P(U64), P(LookupInfo)], I),
            "mox_filter_result": ([VP, P(Filter), P(FilterInfo)], I),
            "mox_join_total": ([VP, P(Join), P(JoinInfo)], I),
            "mox_rank_result": ([VP, ctypes.c_uint32, P(RankInfo)], I),
            "mox_fetch_rows": ([VP, U64, U64, P(P(_Table))], I),
            "mox_rekey_result": ([VP, P(Rekey), P(RekeyInfo)], I),
            "mox_find_ranges": ([VP, VP, P(U64), U64, ctypes.c_uint32, P(U64), P(U64), P(U64), P(FindInfo)], I),
            "mox_top_rows": ([VP, U64, U64, sz, P(P(_Table))], I),
            "mox_hist_result": ([VP, P(Hist), P(P(_HistTable)), P(HistInfo)], I),
            "mox_hist_free": ([P(_HistTable)], None),
            "mox_get_stats": ([VP, P(Stats)], I),
            "mox_device_alloc": ([VP, sz, P(VP)], I),
            "mox_device_free": ([VP, VP], I),
            "mox_memcpy_h2d": ([VP, VP, VP, sz], I),
            "mox_memcpy_d2h": ([VP, VP, VP, sz], I),
            "mox_synchronize": ([VP], I),
            "mox_comm_unique_id": ([ctypes.c_char_p], I),
            "mox_comm_init": ([VP, I, I, ctypes.c_char_p], I),
            "mox_exchange": ([VP], I),
            "mox_exchange_host": ([VP, I, I, _A2A_FN, VP], I),
            "mox_gather": ([VP, I], I),
            "mox_gather_host": ([VP, I, I, I, _A2A_FN, VP], I),
            "mox_write_final_result": ([P(_Table), ctypes.c_char_p], I),
            "mox_print_top_words": ([P(_Table), sz], I),
            "mox_reduce_pairs": ([VP, VP, VP, VP, U64], I),
            "mox_run_shards": ([VP, P(Shard)], I),
            "mox_group_size": ([VP], I),
            "mox_group_member": ([VP, I], VP),
        }
        for name, (args, res) in sig.items():
            f = getattr(L, name)
            f.argtypes = args
            f.restype = res
        _lib = _libs[path] = L
    return _lib


def _check(rc, L=None):
    if rc != MOX_OK:
        msg = (L or lib()).mox_last_error().decode("utf-8", "replace")
        if rc == MOX_EUTF8:
            raise Utf8Error(rc, msg)
        if rc == MOX_EHALO:
            raise HaloError(rc, msg)
        raise MoxError(rc, msg)


def _info_dict(info):
    """An info struct as a dict: its fields but ``reserved``, ms as a float."""
    return {k: (float(info.ms) if k == "ms" else int(getattr(info, k))) for k, _ in info._fields_ if k != "reserved"}


def _packed(data, offs, what):
    """A packed list of ``what`` ("words", "keys") as (uint8 array, uint64 offsets,
    n): item i is data[offs[i]:offs[i+1]], data bytes or a numpy uint8 array
    (None is no bytes object: TypeError, as np.frombuffer raises it)."""
    import numpy as np

    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = offs.size - 1
    if n < 0:
        raise ValueError("offs needs n + 1 entries")
    buf = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    if n and int(offs[-1]) > buf.size:
        raise ValueError("offsets run past the %s' bytes" % what)
    return buf, offs, n


class Table:
    """Owning wrapper of a mox_table (words are bytes, counts are ints)."""

    def __init__(self, ptr, L=None):
        self._L = L or lib()
        self._p = ptr
        t = ptr.contents
        self.n = int(t.n)
        self.tokens = int(t.tokens)

    def _c(self, rc):
        _check(rc, self._L)

    def _raw(self):
        import numpy as np

        t = self._p.contents
        n = self.n
        counts = np.ctypeslib.as_array(t.counts, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
        offs = np.ctypeslib.as_array(t.offs, shape=(n + 1,)).copy()
        nb = int(offs[-1]) if n else 0
        # (ctypes.string_at takes a C int size: tables above 2 GiB of bytes need numpy)
        data = np.ctypeslib.as_array(t.bytes, shape=(nb,)).tobytes() if nb else b""
        return counts, offs, data

    def arrays(self):
        """(counts uint64[n], offs uint64[n+1], bytes) in table order."""
        return self._raw()

    def items(self):
        counts, offs, data = self._raw()
        for i in range(self.n):
            yield data[offs[i]:offs[i + 1]], int(counts[i])

    def as_dict(self):
        return dict(self.items())

    def sorted_items(self):
        """Deterministic key sort (bytewise, Rust String Ord) used for parity."""
        return sorted(self.items(), key=lambda kv: kv[0])

    def sort_bytes(self):
        """Reorder this table bytewise ascending in place (mox_table_sort_bytes)."""
        self._c(self._L.mox_table_sort_bytes(self._p))
        return self

    def write_final_result(self, path):
        self._c(self._L.mox_write_final_result(self._p, path.encode()))

    def close(self):
        if self._p is not None:
            self._L.mox_table_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    def __init__(self, device=-1, flags=0, dict_words=0, sample_pieces=0, reserve_bytes=0, lib_path=None,
                 n_gpus=0, transport=XPORT_RCCL, devices=None, _handle=None):
        """lib_path: a check build instead of libmox.so (CHECK_LIB_PATH, HC_LIB_PATH).
        n_gpus > 1: an engine group (include/mox.h) on ``devices`` (default 0..n_gpus-1)
        over ``transport``."""
        self._L = lib(lib_path)
        self._borrowed = _handle is not None
        if _handle is not None:  # a group member's engine: owned by the group
            self._h = ctypes.c_void_p(_handle)
            return
        cfg = Config()
        cfg.device = device
        cfg.flags = flags
        cfg.dict_words = dict_words
        cfg.sample_pieces = sample_pieces
        cfg.reserve_bytes = reserve_bytes
        cfg.n_gpus = n_gpus
        cfg.transport = transport
        if devices is not None:
            cfg.n_devices = len(devices)
            for i, d in enumerate(devices):
                cfg.devices[i] = d
        h = ctypes.c_void_p()
        self._c(self._L.mox_engine_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h

    # -- engine group (mox_config.n_gpus > 1)
    def group_size(self):
        return int(self._L.mox_group_size(self._h))

    def member(self, i):
        """Member i's engine (device allocations / copies for its shard)."""
        h = self._L.mox_group_member(self._h, i)
        if not h:
            raise MoxError(MOX_EINVAL, "no group member %d" % i)
        return Engine(lib_path=self._L._name, _handle=h)

    def run_shards(self, shards):
        """One group call over device-resident shards: [(d_ptr, buf_len, own_begin, own_end, at_end)]
        per member (mox_run_shards)."""
        arr = (Shard * len(shards))()
        for i, (d, n, a, b, end) in enumerate(shards):
            arr[i] = Shard(ctypes.c_void_p(d), n, a, b, 1 if end else 0)
        self._c(self._L.mox_run_shards(self._h, arr))

    def _c(self, rc):
        _check(rc, self._L)

    def set_flags(self, flags):
        self._c(self._L.mox_set_flags(self._h, flags))

    # -- drop-in for main.rs:16-22
    def count(self, data):
        buf = bytes(data)
        t = ctypes.POINTER(_Table)()
        self._c(self._L.mox_count(self._h, buf, len(buf), ctypes.byref(t)))
        return Table(t, self._L)

    def count_file(self, path):
        t = ctypes.POINTER(_Table)()
        self._c(self._L.mox_count_file(self._h, os.fsencode(path), ctypes.byref(t)))
        return Table(t, self._L)

    def run_file(self, path):
        """count_file without the fetch: the result stays on the device (mox_run_file)."""
        self._c(self._L.mox_run_file(self._h, os.fsencode(path)))

    # -- device-resident path
    def run_device(self, d_ptr, n):
        self._c(self._L.mox_run_device(self._h, ctypes.c_void_p(d_ptr), n))

    def run_range(self, d_ptr, buf_len, own_begin, own_end, at_end):
        self._c(self._L.mox_run_range(self._h, ctypes.c_void_p(d_ptr), buf_len, own_begin, own_end, 1 if at_end else 0))

    def run_range_async(self, d_ptr, buf_len, own_begin, own_end, at_end):
        """Enqueue a pass; completes the previously enqueued one (include/mox.h)."""
        self._c(self._L.mox_run_range_async(self._h, ctypes.c_void_p(d_ptr), buf_len, own_begin, own_end, 1 if at_end else 0))

    def run_wait(self):
        self._c(self._L.mox_run_wait(self._h))

    def fetch(self):
        t = ctypes.POINTER(_Table)()
        self._c(self._L.mox_fetch_table(self._h, ctypes.byref(t)))
        return Table(t, self._L)

    def sort_result(self):
        """Sort the device-resident result bytewise on the GPU (mox_sort_result)."""
        self._c(self._L.mox_sort_result(self._h))

    def top_words(self, k=10):
        """The k most frequent words of the device-resident result as a Table, count
        descending, ties in the resident table's order; selected on the GPU, only
        these words are copied (mox_top_words; k <= TOP_MAX)."""
        t = ctypes.POINTER(_Table)()
        self._c(self._L.mox_top_words(self._h, k, ctypes.byref(t)))
        return Table(t, self._L)

    def write_result(self, path):
        """The device-resident result as final_result.txt ("{word} {count}\\n" per
        word, in the resident table's order), formatted on the GPU and streamed to
        ``path``: what fetch().write_final_result(path) writes (mox_write_result)."""
        self._c(self._L.mox_write_result(self._h, os.fsencode(path)))

    def result_text(self):
        """The same text as bytes (mox_result_text)."""
        import numpy as np

        p, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
        self._c(self._L.mox_result_text(self._h, ctypes.byref(p), ctypes.byref(n)))
        try:
            # (ctypes.string_at takes a C int size: texts above 2 GiB need numpy)
            return np.ctypeslib.as_array(p, shape=(n.value,)).tobytes() if n.value else b""
        finally:
            self._L.mox_text_free(p)

    # -- accumulating results on the device (mox_accumulate*)
    def accumulate(self):
        """total += result: fold the device-resident result of the last run into the
        engine's accumulator on the GPU; the result is then the running total
        (mox_accumulate).  A result folds once: MOX_ESTATE the second time."""
        self._c(self._L.mox_accumulate(self._h))

    def accumulate_file(self, path, chunk_bytes=0):
        """Add a file's counts to the accumulator in passes of about chunk_bytes, cut
        at ASCII whitespace (0: the whole file in one pass; mox_accumulate_file)."""
        self._c(self._L.mox_accumulate_file(self._h, os.fsencode(path), chunk_bytes))

    def accumulate_reset(self):
        """Drop the accumulator and free its device memory (mox_accumulate_reset)."""
        self._c(self._L.mox_accumulate_reset(self._h))

    def accumulate_info(self):
        """{"passes", "words", "tokens", "device_bytes"} of the accumulator."""
        a = AccumInfo()
        self._c(self._L.mox_accumulate_info(self._h, ctypes.byref(a)))
        return _info_dict(a)

    # -- counts of given words (mox_lookup_words)
    def lookup(self, words, with_index=False, with_info=False):
        """The counts of ``words`` (an iterable of bytes; str is encoded as UTF-8) in
        the device-resident result, as a numpy uint64 array: 0 for a word the result
        does not hold.  Read on the GPU: only the words go up and the counts come
        back (mox_lookup_words; at most LOOKUP_MAX words).  Words are taken
        verbatim; a run's table holds lowercased words.  with_index adds the array
        of table positions (LOOKUP_NONE: absent), with_info the info dict
        {"queries", "distinct", "found", "tag_mismatch"}; with either the result
        is a tuple in that order."""
        from . import spill

        ws = [w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in words]
        data, offs, _ = spill.pack_pairs(ws, [])
        return self.lookup_packed(data, offs, with_index, with_info)

    def lookup_packed(self, data, offs, with_index=False, with_info=False):
        """lookup() over words already packed: word i is data[offs[i]:offs[i+1]]
        (data: bytes or a numpy uint8 array, offs: uint64[n + 1])."""
        import numpy as np

        buf, offs, n = _packed(data, offs, "words")
        counts = np.zeros(n, dtype=np.uint64)
        index = np.full(n, LOOKUP_NONE, dtype=np.uint64) if with_index else None
        info = LookupInfo()
        U64P = ctypes.POINTER(ctypes.c_uint64)
        self._c(self._L.mox_lookup_words(
            self._h, ctypes.c_void_p(buf.ctypes.data if buf.size else None), offs.ctypes.data_as(U64P), n,
            counts.ctypes.data_as(U64P), index.ctypes.data_as(U64P) if with_index else None, ctypes.byref(info)))
        out = (counts,)
        if with_index:
            out += (index,)
        if with_info:
            out += ({k: int(getattr(info, k)) for k in ("queries", "distinct", "found", "tag_mismatch")},)
        return out if len(out) > 1 else counts

    # -- the result made smaller on the device (mox_filter_result)
    def filter_result(self, min_count=0, max_count=None, min_len=0, max_len=None, prefix=b"", drop=None, keep=None,
                      count_only=False):
        """Keep the words of the device-resident result that satisfy every given
        term; they become the engine's result, in the order they had, and tokens
        the sum of their counts (mox_filter_result).  min_count <= count <=
        max_count and min_len <= byte length <= max_len (None: no upper bound);
        ``prefix``: the word's first bytes (at most FILTER_PREFIX_MAX); ``drop``: a
        list of words to remove (a stop list), ``keep``: the only words to let
        through (a vocabulary; [] keeps nothing) -- bytes, or str encoded as UTF-8,
        taken verbatim, at most LOOKUP_MAX, and mutually exclusive.  count_only:
        nothing changes, only the info is produced.  Returns the info dict
        {"words_in", "words_kept", "tokens_in", "tokens_kept", "bytes_kept",
        "list_found", "device_bytes", "ms"}."""
        from . import spill

        if drop is not None and keep is not None:
            raise ValueError("drop and keep are mutually exclusive")
        words = keep if keep is not None else drop
        data = offs = None
        if words is not None:
            ws = [w.encode("utf-8") if isinstance(w, str) else bytes(w) for w in words]
            data, offs, _ = spill.pack_pairs(ws, [])
        return self.filter_result_packed(data, offs, keep is not None, min_count, max_count, min_len, max_len, prefix, count_only)

    def filter_result_packed(self, data=None, offs=None, keep=False, min_count=0, max_count=None, min_len=0, max_len=None,
                             prefix=b"", count_only=False):
        """filter_result() with the word list already packed: word i is
        data[offs[i]:offs[i+1]] (data: bytes or a numpy uint8 array, offs:
        uint64[n + 1]; None: no list).  ``keep``: the list is a vocabulary, not a
        stop list."""
        f = Filter()
        f.min_count, f.max_count = min_count, max_count or 0  # (None, like the C struct's 0: no upper bound)
        f.min_len, f.max_len = min_len, max_len or 0
        pre = prefix.encode("utf-8") if isinstance(prefix, str) else bytes(prefix)
        pbuf = ctypes.create_string_buffer(pre, max(1, len(pre)))
        f.prefix, f.prefix_len = (ctypes.addressof(pbuf) if pre else None), len(pre)
        f.words_mode = FILTER_WORDS_KEEP if keep else FILTER_WORDS_DROP
        f.flags = FILTER_COUNT_ONLY if count_only else 0
        if offs is not None:
            buf, offs, n = _packed(data if data is not None else b"", offs, "words")  # (a list of empty words may come without bytes)
            f.words = buf.ctypes.data if buf.size else None
            f.word_offs = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            f.n_words = n
        info = FilterInfo()
        self._c(self._L.mox_filter_result(self._h, ctypes.byref(f), ctypes.byref(info)))
        return _info_dict(info)

    # -- the result joined against the accumulated total on the device (mox_join_total)
    def join_total(self, mode="semi", counts="result", count_only=False):
        """Keep the words of the device-resident result that the accumulator's
        total holds (``mode`` "semi") or lacks ("anti": the new words); they
        become the engine's result, in the order they had (mox_join_total).
        ``counts``: kept words keep their own count ("result"), take the total's
        ("total") or the smaller of both ("min"); the last two with "semi" only (with "anti": MOX_EINVAL).
        count_only: nothing changes, only the info is produced.  An empty
        accumulator is an empty total.  Returns the info dict {"words_in",
        "words_total", "words_matched", "words_kept", "tokens_in", "tokens_total",
        "tokens_matched_result", "tokens_matched_total", "tokens_min",
        "tokens_kept", "bytes_kept", "tag_mismatch", "device_bytes", "ms"}."""
        if mode not in _JOIN_MODES:
            raise ValueError("mode %r: one of %s" % (mode, sorted(_JOIN_MODES)))
        if counts not in _JOIN_COUNTS:
            raise ValueError("counts %r: one of %s" % (counts, sorted(_JOIN_COUNTS)))
        j = Join()
        j.mode, j.counts = _JOIN_MODES[mode], _JOIN_COUNTS[counts]
        j.flags = JOIN_COUNT_ONLY if count_only else 0
        info = JoinInfo()
        self._c(self._L.mox_join_total(self._h, ctypes.byref(j), ctypes.byref(info)))
        return _info_dict(info)

    # -- the result ordered by count on the device (mox_rank_result), and read by rows
    def rank_result(self, ascending=False):
        """Reorder the device-resident result by count on the GPU, most frequent
        first (``ascending``: least frequent first); words with equal counts keep
        the order they had, so sort_result() first gives "count, then bytewise"
        (mox_rank_result).  Returns the info dict {"words", "tokens", "max_count",
        "digit_passes", "device_bytes", "ms"}."""
        info = RankInfo()
        self._c(self._L.mox_rank_result(self._h, RANK_ASCENDING if ascending else 0, ctypes.byref(info)))
        return _info_dict(info)

    def fetch_rows(self, first, n):
        """Rows [first, first + n) of the device-resident result as a Table, in the
        order fetch() returns them; only these rows are copied (mox_fetch_rows).
        tokens is the whole result's."""
        t = ctypes.POINTER(_Table)()
        self._c(self._L.mox_fetch_rows(self._h, first, n, ctypes.byref(t)))
        return Table(t, self._L)

    # -- the result re-keyed on the device (mox_rekey_result)
    def rekey_result(self, trim=b"", punct=False, max_chars=0):
        """Strip the ASCII characters of ``trim`` (bytes; with ``punct`` also
        string.punctuation) from both ends of every word of the device-resident
        result, keep the first ``max_chars`` characters (0: all) and sum the rows
        that became equal, on the GPU; words left empty go (mox_rekey_result).
        A byte >= 128 in ``trim`` raises ValueError.  Returns the info dict
        {"words_in", "words_out", "words_changed", "words_dropped", "tokens_in",
        "tokens_out", "tokens_dropped", "bytes_out", "device_bytes", "ms"}."""
        k = Rekey()
        for b in bytes(trim):
            if b >= 128:
                raise ValueError("trim holds the byte 0x%02x: only ASCII characters can be stripped" % b)
            k.trim_set[b >> 6] |= 1 << (b & 63)
        k.max_chars = max_chars
        k.flags = REKEY_TRIM_ASCII_PUNCT if punct else 0
        info = RekeyInfo()
        self._c(self._L.mox_rekey_result(self._h, ctypes.byref(k), ctypes.byref(info)))
        return _info_dict(info)

    # -- row ranges in the sorted result (mox_find_ranges), and the top-k of a row range (mox_top_rows)
    def find(self, keys, mode="prefix", with_sums=True, with_info=False):
        """Row ranges of ``keys`` (an iterable of bytes; str is encoded as UTF-8) in
        the bytewise-sorted device-resident result, by binary search on the GPU
        (mox_find_ranges; at most FIND_MAX keys, taken verbatim).  ``mode``:
        "exact" (the row whose word equals the key), "prefix" (the rows whose word
        starts with it; b"" is every row) or "lower" (first = last = the rows below
        the key), or a FIND_* constant.  Returns (first, last[, sums][, info]) as
        numpy uint64 arrays: rows [first[i], last[i]) are what fetch_rows(first[i],
        last[i] - first[i]) returns, an absent key gives first == last == its
        insertion point, sums[i] is the wrapping sum of the range's counts; info is
        the dict {"queries", "matched", "rows", "tile_pass", "device_bytes", "ms"}.
        The result must be sorted (sort_result(); MOX_ESTATE otherwise)."""
        from . import spill

        ks = [k.encode("utf-8") if isinstance(k, str) else bytes(k) for k in keys]
        data, offs, _ = spill.pack_pairs(ks, [])
        return self.find_packed(data, offs, mode, with_sums, with_info)

    def find_packed(self, data, offs, mode="prefix", with_sums=True, with_info=False):
        """find() over keys already packed: key i is data[offs[i]:offs[i+1]]
        (data: bytes or a numpy uint8 array, offs: uint64[n + 1])."""
        import numpy as np

        buf, offs, n = _packed(data, offs, "keys")
        first = np.zeros(n, dtype=np.uint64)
        last = np.zeros(n, dtype=np.uint64)
        sums = np.zeros(n, dtype=np.uint64) if with_sums else None
        info = FindInfo()
        U64P = ctypes.POINTER(ctypes.c_uint64)
        self._c(self._L.mox_find_ranges(
            self._h, ctypes.c_void_p(buf.ctypes.data if buf.size else None), offs.ctypes.data_as(U64P), n,
            _FIND_MODES.get(mode, mode), first.ctypes.data_as(U64P), last.ctypes.data_as(U64P),
            sums.ctypes.data_as(U64P) if with_sums else None, ctypes.byref(info)))
        out = (first, last)
        if with_sums:
            out += (sums,)
        if with_info:
            out += (_info_dict(info),)
        return out

    def top_rows(self, first, n, k=10):
        """top_words(k) over rows [first, first + n) of the device-resident result:
        count descending, ties in table order, tokens the whole result's; works on
        any result, sorted or not (mox_top_rows; k <= TOP_MAX)."""
        t = ctypes.POINTER(_Table)()
        self._c(self._L.mox_top_rows(self._h, first, n, k, ctypes.byref(t)))
        return Table(t, self._L)

    def complete(self, prefix, k=10):
        """The k most frequent words of the sorted device-resident result that start
        with ``prefix``, as a Table: find(mode="prefix") + top_rows, no row outside
        the prefix is touched.  Raises what find raises on an unsorted result; it
        does not sort behind the caller's back."""
        first, last = self.find([prefix], "prefix", with_sums=False)
        return self.top_rows(int(first[0]), int(last[0] - first[0]), k)

    # -- histograms of the result on the device (mox_hist_result)
    def histogram(self, key="count", first=None, n=None, with_info=False):
        """Bin the rows of the device-resident result by a derived key on the GPU
        (mox_hist_result; the call only reads the result).  ``key``: "count" (the
        frequency spectrum), "bytes", "chars", "first" (the first character:
        hist_first_bytes decodes a key), or a HIST_* constant.  ``first`` / ``n``
        given: only rows [first, first + n), as top_rows takes them.  Returns
        (keys, bin_words, bin_tokens, first_row, words, tokens[, info]): four
        uint64 arrays of one entry per bin, keys ascending, first_row the lowest
        table index of a row with that key; words and tokens the rows binned and
        the wrapping u64 sum of their counts."""
        import numpy as np

        h = Hist()
        h.key = _HIST_KEYS.get(key, key)
        if first is not None or n is not None:
            h.flags = HIST_RANGE
            h.first = 0 if first is None else first
            h.rows = (1 << 64) - 1 if n is None else n
        info = HistInfo()
        t = ctypes.POINTER(_HistTable)()
        self._c(self._L.mox_hist_result(self._h, ctypes.byref(h), ctypes.byref(t), ctypes.byref(info)))
        try:
            c = t.contents
            g = int(c.n)
            out = tuple(np.ctypeslib.as_array(getattr(c, f), shape=(g,)).copy() if g else np.zeros(0, dtype=np.uint64)
                        for f in ("keys", "bin_words", "bin_tokens", "first_row")) + (int(c.words), int(c.tokens))
        finally:
            self._L.mox_hist_free(t)
        if with_info:
            out += (_info_dict(info),)
        return out

    def stats(self):
        s = Stats()
        self._c(self._L.mox_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def ms_map(self):
        """Map-kernel milliseconds of the last pass (cheap: for timed loops)."""
        if not hasattr(self, "_st"):
            self._st = Stats()
            self._st_ref = ctypes.byref(self._st)
        self._c(self._L.mox_get_stats(self._h, self._st_ref))
        return self._st.ms_map

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self._c(self._L.mox_device_alloc(self._h, nbytes, ctypes.byref(p)))
        return p.value

    def free(self, d_ptr):
        self._c(self._L.mox_device_free(self._h, ctypes.c_void_p(d_ptr)))

    def h2d(self, d_ptr, host_buf, nbytes=None):
        if nbytes is None:
            nbytes = len(host_buf)
        src = ctypes.c_char_p(host_buf) if isinstance(host_buf, bytes) else host_buf
        if hasattr(host_buf, "ctypes"):
            src = ctypes.c_void_p(host_buf.ctypes.data)
        self._c(self._L.mox_memcpy_h2d(self._h, ctypes.c_void_p(d_ptr), src, nbytes))

    def synchronize(self):
        self._c(self._L.mox_synchronize(self._h))

    # -- multi-GPU
    def comm_init(self, nranks, rank, uid):
        self._c(self._L.mox_comm_init(self._h, nranks, rank, uid))

    def exchange(self):
        """RCCL all-to-all exchange + final reduce (after run_range on every rank)."""
        self._c(self._L.mox_exchange(self._h))

    def exchange_host(self, nranks, rank, alltoallv):
        """The same exchange over a host transport.  ``alltoallv(send, send_sizes,
        recv_sizes)`` gets the send bytes (memoryview, blocks for ranks 0..n-1)
        and must return the received bytes (blocks from ranks 0..n-1)."""
        self._host_call(lambda fn: self._L.mox_exchange_host(self._h, nranks, rank, fn, None), nranks, alltoallv)

    def gather(self, root=0):
        """Gather every rank's final table into root's engine over RCCL (mox_gather)."""
        self._c(self._L.mox_gather(self._h, root))

    def gather_host(self, nranks, rank, alltoallv, root=0):
        """mox_gather over a host transport (same callback as exchange_host)."""
        self._host_call(lambda fn: self._L.mox_gather_host(self._h, nranks, rank, root, fn, None), nranks, alltoallv)

    def _host_call(self, call, nranks, alltoallv):
        err = []

        def cb(_user, send, send_bytes, recv, recv_bytes):
            try:
                ss = [int(send_bytes[i]) for i in range(nranks)]
                rs = [int(recv_bytes[i]) for i in range(nranks)]
                buf = (ctypes.c_uint8 * sum(ss)).from_address(send) if sum(ss) else bytearray()
                out = alltoallv(memoryview(buf), ss, rs)
                out = bytes(out)
                if len(out) != sum(rs):
                    raise ValueError("alltoallv returned %d bytes, expected %d" % (len(out), sum(rs)))
                if out:
                    ctypes.memmove(recv, out, len(out))
                return 0
            except Exception as ex:  # reported after the call returns
                err.append(ex)
                return 1

        fn = _A2A_FN(cb)
        rc = call(fn)
        if err:
            raise err[0]
        _check(rc)

    # -- spill files (mox/spill.py): reduce_phase over parsed map files
    def reduce_pairs(self, words, counts):
        """Sum counts by word (bytes, taken verbatim) on the GPU; returns the
        Table (main.rs:111-150 over read_map_result's maps)."""
        from . import spill

        data, offs, cnt = spill.pack_pairs(list(words), list(counts))
        if len(cnt) != len(offs) - 1:
            raise ValueError("words and counts differ in length")
        buf = ctypes.create_string_buffer(data, max(1, len(data)))
        self._c(self._L.mox_reduce_pairs(self._h, buf, ctypes.c_void_p(offs.ctypes.data),
                                      ctypes.c_void_p(cnt.ctypes.data), len(cnt)))
        return self.fetch()

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._L.mox_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    _check(lib().mox_comm_unique_id(buf))
    return buf.raw


def count_words(data, **kw):
    """One-shot: bytes -> {word(bytes): count} on the GPU."""
    e = Engine(**kw)
    try:
        t = e.count(data)
        try:
            return t.as_dict()
        finally:
            t.close()
    finally:
        e.close()


def count_files(paths, chunk_bytes=0, **kw):
    """One-shot: the word counts of several files together, as a Table.  Every
    file is added to one device-resident accumulator (Engine.accumulate_file, in
    passes of about chunk_bytes; 0: one pass per file), so the files need not fit
    in device memory together and only the final table is fetched.  Files are
    separate corpora: a token never continues from one file into the next."""
    e = Engine(**kw)
    try:
        for p in paths:
            e.accumulate_file(p, chunk_bytes)
        if e.accumulate_info()["passes"] == 0:  # no files: the empty table
            return e.count(b"")
        return e.fetch()
    finally:
        e.close()
