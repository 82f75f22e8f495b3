/* mox.h -- C ABI of the MI355X word-count engine (drop-in for the hot path of
 * AnarchistHoneybun/map-oxidize).
 *
 * The reference has no plugin / FFI API: the whole hot path is the private call
 * sequence in `main` (/root/reference/src/main.rs:16-22)
 *
 *     let chunks       = split_file("shakes.txt", 8).await?;                 // :16, fn :36-51
 *     let map_results  = map_phase(&chunks, 8).await?;                      // :19, fn :53-92
 *     let final_result = reduce_phase(map_results.clone(), 4).await?;       // :22, fn :111-150
 *
 * i.e. `path -> HashMap<String, usize>` consumed by write_final_result
 * (:170-182) and print_top_words (:184-192).  mox_count_file / mox_count
 * replace those three lines with one call that returns the same word -> count
 * table; mox_write_final_result / mox_print_top_words reproduce the L5 output.
 * INTEGRATION.md shows the Rust FFI binding a maintainer would add.
 *
 * Semantics (bit-exact with the reference): tokens are Rust
 * `str::split_whitespace` (Unicode White_Space delimiters) of the UTF-8 text,
 * each lowercased with Rust `str::to_lowercase` (full mapping + Final_Sigma),
 * counted with u64.  Invalid UTF-8 returns MOX_EUTF8 and no table, like the
 * reference's InvalidData abort at main.rs:44 -> :16.
 *
 * Conventions: every entry point returns an int status (0 = MOX_OK); no
 * exception crosses the ABI; mox_last_error() holds a thread-local message.
 * An engine is bound to one HIP device -- or, as an engine group
 * (mox_config.n_gpus > 1), drives several from the calling thread -- and is
 * not thread-safe (one host thread per engine).  Every call except mox_run_range_async is synchronous: it
 * returns after its work (and any pending asynchronous pass) is complete.
 * mox_run_range_async returns once its pass is queued; see its comment for
 * the lifetime rule of the device buffer it reads.
 */
#ifndef MOX_H
#define MOX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOX_ABI_VERSION 4

/* status codes */
#define MOX_OK 0
#define MOX_EINVAL (-1)  /* bad argument */
#define MOX_EUTF8 (-2)   /* input is not valid UTF-8 (reference: io::ErrorKind::InvalidData) */
#define MOX_ENOMEM (-3)  /* device or host allocation failed */
#define MOX_EHIP (-4)    /* HIP runtime error */
#define MOX_EIO (-5)     /* file I/O error (reference: io::Error from File::open / reads) */
#define MOX_ERCCL (-6)   /* RCCL error */
#define MOX_ESTATE (-7)  /* call out of order (e.g. fetch before run) */
#define MOX_EHALO (-8)   /* a shard's token ran past the end of its buffer: halo too small */

/* mox_config.flags */
#define MOX_F_NO_DICT 0x1u      /* disable the hot-word dictionary (all tokens take the cold path) */
#define MOX_F_SORT_BYTES 0x2u   /* the result table is sorted bytewise ascending (Rust String Ord) on the GPU
                                   (at mox_fetch_table; an engine group: right after its gather, inside the
                                   mox_count / mox_run_shards call) instead of engine order */
#define MOX_F_TIMING 0x4u       /* record per-kernel HIP-event timings into mox_stats */
#define MOX_F_TIMING_MAP 0x8u   /* HIP events around the map kernel only (ms_map): each event record idles
                                   the stream ~5.6 us, so timed loops bracket just the dominant kernel */

#define MOX_MAX_GPUS 16
/* mox_config.transport of an engine group */
#define MOX_XPORT_RCCL 0u  /* RCCL communicators (ncclCommInitAll) over xGMI, one ncclGroupStart/End per all-to-all */
#define MOX_XPORT_COPY 1u  /* device-to-device copies (hipMemcpyPeerAsync); members may share a GPU (tests) */

typedef struct mox_config {
  int device;             /* HIP device ordinal; -1 = current device */
  uint32_t flags;         /* MOX_F_* */
  uint32_t dict_words;    /* hot dictionary capacity; 0 = default (4096, also the maximum) */
  uint32_t sample_pieces; /* 4 KiB pieces sampled to build the dictionary; 0 = default (192), max 1024 */
  uint64_t reserve_bytes; /* pre-size device buffers for corpora of this size (per GPU); 0 = grow on demand */
  /* engine group: n_gpus > 1 makes ONE engine that
     drives n_gpus GPUs from the calling thread.  mox_count / mox_count_file
     split the input into byte ranges at whitespace, run the local passes on
     all GPUs at once, exchange the partial tables (hash-partitioned
     all-to-all), reduce per owner and gather the final table on member 0;
     mox_run_shards does the same over device-resident shards. */
  uint32_t n_gpus;        /* 0 or 1: a single-GPU engine on `device` */
  uint32_t transport;     /* MOX_XPORT_* (engine group) */
  uint32_t n_devices;     /* 0: member i runs on device i; else n_gpus: member i runs on devices[i] */
  int32_t devices[MOX_MAX_GPUS];
  uint32_t reserved[5];
} mox_config;

typedef struct mox_engine mox_engine;

/* One shard of a device-resident corpus for mox_run_shards: the buffer lives
 * on the member's GPU; tokens whose first byte lies in [own_begin, own_end)
 * belong to it (see mox_run_range for the context / look-ahead rules). */
typedef struct mox_shard {
  const void* d_buf;
  size_t buf_len, own_begin, own_end;
  int at_corpus_end;
} mox_shard;

/* Result table: one entry per distinct lowercased word.  Engine order: words
 * of at most 16 bytes without a NUL byte first, ascending by (32-bit key hash,
 * second 32-bit key hash, the word's 16-byte zero-padded key) -- the same
 * whichever reduce kernel grouped the word -- then longer words in long-table
 * slot order (which can vary from run to run when two long words race for a
 * slot).  With
 * MOX_F_SORT_BYTES (or after mox_table_sort_bytes): bytewise ascending, Rust
 * String Ord, sorted on the GPU).  The reference's own order is HashMap-random
 * (/root/reference/src/main.rs:177-179).  After mox_gather the root's table
 * is the ranks' tables one after another (rank order), each in engine order;
 * an engine group's gathered table likewise, unless MOX_F_SORT_BYTES.
 * Memory is owned by the library until mox_table_free. */
typedef struct mox_table {
  uint64_t n;              /* distinct words */
  uint64_t tokens;         /* total tokens counted (== sum of counts) */
  const uint64_t* counts;  /* [n] */
  const uint64_t* offs;    /* [n+1] byte offsets into bytes */
  const uint8_t* bytes;    /* concatenated UTF-8 words */
} mox_table;

typedef struct mox_stats {
  uint64_t bytes;          /* corpus bytes of the last run */
  uint64_t tokens;
  uint64_t uniques;
  uint64_t dict_words;     /* words in the hot dictionary */
  uint64_t cold_records;   /* tokens that took the cold (partitioned) path */
  uint64_t weighted_records;
  uint64_t unicode_tokens; /* tokens that went through the Unicode case lane */
  uint64_t long_tokens;    /* tokens longer than 16 bytes (hashed keys + byte compare) */
  uint64_t chunks;         /* cold-record chunks allocated */
  uint32_t retries;        /* buffer-growth reruns in the last call */
  uint32_t max_subpasses;  /* largest reduce sub-pass count of any bucket */
  /* device milliseconds (HIP events on the engine stream; MOX_F_TIMING) */
  double ms_run;           /* whole device pipeline: corpus in HBM -> table in HBM */
  double ms_dict;          /* sample + dictionary build */
  double ms_map;           /* map kernel (dominant kernel) */
  double ms_lanes;         /* unicode + long lanes */
  double ms_reduce;        /* directory + bucket reduce */
  double ms_finalize;      /* table materialisation */
  double ms_h2d;           /* host -> device corpus copy (mox_count / mox_count_file) */
  double ms_d2h;           /* table fetch */
  double ms_exchange;      /* multi-GPU all-to-all + final reduce (not the sorted exchange's sort: ms_sort) */
  uint64_t reduce_units;   /* reduce work units (partitions, or their sub-buckets when split) */
  uint32_t split_partitions; /* partitions split by the high-cardinality path */
  uint32_t async_reruns;   /* async passes re-run synchronously (overflow), cumulative over the engine */
  /* multi-GPU (last mox_exchange / mox_gather of this rank) */
  uint64_t x_bytes_sent;   /* exchange payload bytes this rank sent (records + long-word blobs, self included) */
  uint64_t x_bytes_recv;   /* exchange payload bytes this rank received */
  uint64_t gather_bytes;   /* table bytes this rank sent to the gather root (root: received) */
  double ms_gather;        /* wall time of the last mox_gather on this rank */
  /* exactness-fallback hit counters of the last pass (a local pass plus its
     exchange's reduce pass), counted only by the forced-collision check build
     (libmox_hc.so, -DMOX_HASH_COLLIDE); zero in production builds:
     [0] dictionary tag equal, key different   [1] long-word table: equal hash, different bytes
     [2] one-wave sort reduce re-sorted on 64-bit keys   [3] ... handed its unit to k_reduce
     [4] k_reduce table: equal tag, different key   [5] k_reduce_small: equal hash, different key */
  uint64_t path_hits[8];
  double ms_sort;          /* device bytewise table sort (MOX_F_SORT_BYTES), wall time */
  double ms_local;         /* engine group: local passes of all members (wall time) */
  uint32_t n_gpus;         /* engine group size (1 for a single-GPU engine) */
  uint32_t async_dropped;  /* overflowed async passes superseded by a later queued pass (never re-run) */
  uint32_t x_ranged;       /* the last exchange owned words by byte range (MOX_F_SORT_BYTES); 0: by hash
                              (no sort flag, or skewed 8-byte prefixes fell back to hash owners) */
  uint32_t x_pad;
} mox_stats;

const char* mox_last_error(void);
int mox_abi_version(void);

int mox_engine_create(const mox_config* cfg, mox_engine** out);
/* Replace the engine's MOX_F_* flags (e.g. switch timing modes between runs); an
 * engine group applies them to every member. */
int mox_set_flags(mox_engine* e, uint32_t flags);
void mox_engine_destroy(mox_engine* e);

/* ---- drop-in for main.rs:16-22 ---- */
/* Count words of a host buffer (copied to HBM first). */
int mox_count(mox_engine* e, const uint8_t* text, size_t len, mox_table** out);
/* Count words of a file (reference: split_file(path) .. reduce_phase):
 * mox_run_file + mox_fetch_table. */
int mox_count_file(mox_engine* e, const char* path, mox_table** out);
/* mox_count_file without the fetch: the result stays on the device (for
 * mox_write_result / mox_result_text, mox_top_words, mox_fetch_table). */
int mox_run_file(mox_engine* e, const char* path);
void mox_table_free(mox_table* t);
/* Reorder a fetched table bytewise ascending (Rust String Ord) in place. */
int mox_table_sort_bytes(mox_table* t);

/* ---- device-resident path (bench / pipelines): corpus already in HBM ---- */
/* One full pass: HBM corpus -> HBM table.  No host copy of the result. */
int mox_run_device(mox_engine* e, const void* d_text, size_t len);
/* Same over a shard window: count tokens whose first byte lies in
 * [own_begin, own_end) of the buffer d_buf[0, buf_len).  Bytes before own_begin
 * give the left context (own_begin == 0 means "corpus start"); bytes after
 * own_end are look-ahead for the last token.  at_corpus_end != 0 means the
 * buffer end is the end of the corpus; otherwise a token reaching the buffer
 * end is an error (MOX_EHALO).  A token reaches the end when no whole
 * whitespace character follows it inside the buffer: one ending exactly at the
 * end, or followed by a whitespace character that the end cuts, counts.  A
 * character whose first byte lies in [own_begin, own_end) and that the end of
 * a non-final buffer cuts is MOX_EHALO as well, whether or not its token is
 * owned (at the corpus end it is MOX_EUTF8). */
int mox_run_range(mox_engine* e, const void* d_buf, size_t buf_len, size_t own_begin, size_t own_end,
                  int at_corpus_end);
/* Asynchronous mox_run_range: enqueues the pass and returns; the pass queued
 * by the previous async call is completed (checked, and re-run synchronously
 * if a buffer overflowed) after this one is enqueued, so back-to-back passes
 * leave no host round trip between them on the GPU.  A pass's error is
 * returned by the call that completes it: the next mox_run_range_async, or
 * mox_run_wait.  Every other entry point completes pending passes first.
 * Buffer lifetime: an overflowed pass is re-run later from d_buf, so d_buf
 * must stay valid and unmodified until the call that completes the pass has
 * returned (the next mox_run_range_async, mox_run_wait, or any other entry
 * point of this engine).  An overflowed pass with a later pass already queued
 * behind it is not re-run: the later pass supersedes its table
 * (mox_stats.async_dropped). */
int mox_run_range_async(mox_engine* e, const void* d_buf, size_t buf_len, size_t own_begin, size_t own_end,
                        int at_corpus_end);
/* Complete every pending async pass; the last one's table is the result. */
int mox_run_wait(mox_engine* e);
/* Engine group: one call for n_gpus device-resident shards (shards[i] on
 * member i's GPU): local passes on every GPU at once, exchange, final
 * reduce, gather on member 0 (and the bytewise sort with MOX_F_SORT_BYTES).
 * A single-GPU engine takes one shard (= mox_run_range). */
int mox_run_shards(mox_engine* e, const mox_shard* shards);
/* Members of an engine group (1 for a single-GPU engine); member 0 is e
 * itself.  A member's engine serves device allocations and copies for its
 * shard (mox_device_alloc / mox_memcpy_h2d). */
int mox_group_size(const mox_engine* e);
mox_engine* mox_group_member(mox_engine* e, int i);
/* Copy the table of the last run (or of the last exchange) to the host.
 * (A row range of it: mox_fetch_rows, below.) */
int mox_fetch_table(mox_engine* e, mox_table** out);
/* Reorder the device-resident result table bytewise ascending (Rust String
 * Ord) on the GPU, without fetching it (e.g. the root's table after
 * mox_gather, inside a timed multi-GPU step).  MOX_ENOMEM when the sort's
 * device scratch cannot be allocated: the table then stays in engine order
 * (mox_fetch_table with MOX_F_SORT_BYTES still sorts it, on the host).
 * State: the result is marked sorted and a ranking (mox_rank_result) ends;
 * tokens, the folded state and the accumulator are unchanged.  A result that
 * is sorted already is not sorted again: only its ranked mark goes.  A table of at most one word is in every order: nothing moves, it
 * stays in the buffers it was in, and mox_find_ranges takes it whether it was
 * ever sorted or not. */
int mox_sort_result(mox_engine* e);
/* The k most frequent words of the device-resident result (after any run,
 * mox_reduce_pairs, mox_exchange, mox_gather, mox_run_shards, mox_sort_result),
 * selected on the GPU; only the selected words are copied to the host (the
 * full table does not cross PCIe and no host pass runs over it).  *out is a
 * normal mox_table (mox_table_free) of min(k, distinct words) entries, count
 * descending, equal counts by their index in the device-resident table
 * ascending -- mox_print_top_words' rule, so printing *out prints the lines
 * the fetched table would.  tokens is the result's total token count, not the
 * sum of the k counts.  Table order is the table as it lies in device memory
 * at the call: engine order, rank order after a gather, bytewise order once
 * the result is sorted (mox_sort_result, an earlier mox_fetch_table with
 * MOX_F_SORT_BYTES, a ranged engine-group result).  This call never sorts the
 * table itself, MOX_F_SORT_BYTES or not: engine order can differ from run to
 * run among words longer than 16 bytes, so a caller who wants deterministic
 * ties calls mox_sort_result first.  The result stays where it is (further
 * calls with another k, mox_fetch_table, an exchange all see it unchanged).
 * k == 0 or an empty result: an empty table.  MOX_EINVAL: k > MOX_TOP_MAX or a
 * NULL argument; MOX_ESTATE: no run yet.  An engine group: member 0's gathered
 * result.  Once the result is ranked (mox_rank_result), table order is count
 * order: the words this call selects are the ranked table's first rows, and
 * mox_fetch_rows reaches past MOX_TOP_MAX. */
#define MOX_TOP_MAX 4096
int mox_top_words(mox_engine* e, size_t k, mox_table** out);
/* The device-resident result as final_result.txt text, formatted on the GPU:
 * for each table entry i in the table's order in device memory, the word's
 * bytes, ' ', the count in decimal, '\n'.  Byte for byte what
 * mox_write_final_result writes from a mox_fetch_table of the same result, but
 * only the text crosses PCIe (no counts, no offsets) and no host pass runs
 * over the words.  mox_write_result streams the text to `path` in slices (the
 * file is truncated on open; the next slice is rendered and copied while one
 * is written; MOX_TEXT_SLICE=<bytes> overrides the slice size, at least 256,
 * rounded down to a multiple of 16); mox_result_text returns the whole text in
 * host memory (*text, *len; release it with mox_text_free; an empty result
 * gives *len == 0 and a pointer that is still valid to free).  Both complete a
 * pending asynchronous pass first.  Order is the table as it lies in device
 * memory at the call (see mox_top_words); with MOX_F_SORT_BYTES an unsorted
 * result is first sorted on the device, as mox_fetch_table does
 * (mox_stats.ms_sort).  If that sort returns MOX_ENOMEM so does the call: the
 * result stays in engine order and nothing is written -- fall back to
 * mox_fetch_table + mox_write_final_result, which sort on the host.  The
 * result stays where it is and unchanged (a later mox_fetch_table,
 * mox_top_words, exchange or a second rendering sees the same table).  A count
 * of 0 (mox_reduce_pairs lets one through) renders as "0".  MOX_ESTATE: no run
 * yet; MOX_EINVAL: a NULL argument; MOX_EIO: the file cannot be opened or
 * written.  An engine group: member 0's gathered result.  A ranked result
 * (mox_rank_result) is rendered in count order and is not re-sorted,
 * MOX_F_SORT_BYTES or not: an explicit ranking wins over the flag. */
int mox_write_result(mox_engine* e, const char* path);
int mox_result_text(mox_engine* e, uint8_t** text, uint64_t* len);
void mox_text_free(uint8_t* text);

/* ---- accumulating results on the device (windows, chunks, many files) ---- */
/* total += result.  Folds the device-resident result of the last run (any run,
 * mox_reduce_pairs, exchange, gather, mox_run_shards, sorted or not) into the
 * engine's accumulator, on the GPU; nothing is fetched.  Afterwards the engine's
 * result IS the running total: mox_top_words, mox_write_result, mox_result_text,
 * mox_sort_result, mox_fetch_table and (one process per rank) mox_exchange see it.
 * The merged table is what mox_reduce_pairs gives over the two tables' rows laid
 * end to end: words verbatim, counts summed as u64, a word of either table
 * present (a count of 0 included), tokens the sum of both.  Order is engine
 * order: the words of at most 16 bytes exactly as one pass over the whole input
 * orders them, then the longer words in long-table slot order.  The first call
 * after mox_engine_create or mox_accumulate_reset (an empty accumulator) runs no
 * reduce: the result is saved as the total and stays the table it was.  After a
 * merge the result is the merge pass's table, which an exchange can start from,
 * so "accumulate the local windows, then one mox_exchange + mox_gather" works.
 * A result is folded once: a second call without a run in between returns
 * MOX_ESTATE and changes nothing (it would double the counts), as does a call
 * with no result; MOX_EINVAL: a NULL engine.  The accumulator survives every
 * later run; only the result is replaced by them.  On any error the accumulator
 * is what it was before the call, the engine's result becomes that previous
 * total (with an empty accumulator it is left as it was) and the run's
 * contribution is lost: run it again and fold again.  That result is the
 * total's own table in the accumulator's buffers: its rows in the total's
 * order, sorted or ranked as the result was when the total was saved (a merged
 * total is neither), and folded.  Every call over the result works on it; the
 * ones that write a new table (filter, join, rank, sort, re-key) move it out of
 * the accumulator's buffers, mox_accumulate_reset before that takes it away.  A merge reduces the whole
 * total again, so it costs time in the total's distinct words, not the run's.
 * Completes pending asynchronous passes first.  An engine group folds member
 * 0's gathered result, on member 0.
 * MOX_TEST_FAIL_ACCUM=1 (tests; read at each call) makes a merge return
 * MOX_ENOMEM after both tables are packed and before the reduce pass. */
int mox_accumulate(mox_engine* e);
/* Adds a file's counts to the accumulator in passes of about chunk_bytes
 * (0 = the whole file in one pass, as mox_run_file; else >= 256, smaller is
 * MOX_EINVAL).  Cut k is the first file position >= k * chunk_bytes that follows
 * an ASCII whitespace byte (space, \t \n \v \f \r), so every chunk is a complete
 * corpus, no token is split, and a chunk grows past chunk_bytes where the text
 * has no ASCII whitespace; empty chunks are skipped.  Each chunk is read, run
 * and folded (mox_accumulate); an engine group splits each chunk over its
 * members as mox_run_file splits a file.  The call adds to whatever the
 * accumulator holds: loop over files, mox_accumulate_reset for a fresh total.
 * An empty file is one pass that adds nothing.  On an error the accumulator
 * holds the chunks before the failing one (mox_accum_info.passes counts them);
 * MOX_EUTF8 reports the byte offset in the file. */
int mox_accumulate_file(mox_engine* e, const char* path, uint64_t chunk_bytes);
/* Drop the accumulator and free its device memory.  The last run's result, if
 * there is one, can be folded again afterwards (into the empty accumulator).
 * A result that still is the total's own table (after a failed mox_accumulate)
 * goes with it: the engine then has no result, and every call over one returns
 * MOX_ESTATE until the next run. */
int mox_accumulate_reset(mox_engine* e);
typedef struct mox_accum_info {
  uint64_t passes;        /* results folded since create / reset */
  uint64_t words;         /* distinct words of the total */
  uint64_t tokens;        /* tokens of the total */
  uint64_t device_bytes;  /* device memory the accumulator holds (the saved table and the packer's scratch) */
} mox_accum_info;
int mox_accumulate_info(const mox_engine* e, mox_accum_info* out);

/* ---- looking words up in the device-resident result ---- */
/* The counts of n given words in the device-resident result, read on the GPU:
 * only the query words go to the device and only n counts (and n indices) come
 * back; the table is not fetched and no host pass runs over it.  Query word i
 * is bytes[offs[i], offs[i+1]) and is taken verbatim, as mox_reduce_pairs takes
 * its words: not lowercased, not validated as UTF-8.  A run's table holds
 * lowercased words (Rust str::to_lowercase), so a caller who asks about text
 * lowercases the word by Rust's rule first; "The" is not in a run's table.
 * counts[i]: the word's count, 0 when the result does not hold the word.
 * index[i] (index may be NULL): the word's position in the table as it lies in
 * device memory at the call -- table order as mox_top_words defines it: engine
 * order, rank order after a gather, bytewise order once sorted -- or
 * MOX_LOOKUP_NONE when the word is absent.  A word the result holds with count
 * 0 (only mox_reduce_pairs input produces one) gives counts[i] == 0 and a real
 * index: the index tells it from an absent word.  A word that occurs several
 * times among the queries gets the full count and the same index at every
 * position.  info may be NULL.  With n == 0 counts, bytes and offs may be NULL
 * too, and nothing runs on the device.
 * Works on every form of result: after any run, mox_reduce_pairs, mox_exchange
 * (this rank's words: ranks own disjoint words, so the ranks' counts add up to
 * the global ones without a gather), mox_gather, mox_run_shards,
 * mox_sort_result, mox_accumulate (the running total), a MOX_F_SORT_BYTES
 * fetch; an engine group: member 0's gathered result.  Completes pending
 * asynchronous passes first.  The call only reads: result, accumulator, folded
 * and sorted state are unchanged, and a later fetch, top-k, rendering,
 * accumulate or exchange sees what it would have seen without it.
 * Cost: one pass over the result's offsets, and over the bytes of the words
 * whose length some query has; device scratch is O(n + query bytes), lives in
 * the engine and is freed by mox_engine_destroy.
 * MOX_ESTATE: no result yet.  MOX_EINVAL: a NULL engine, a NULL required
 * pointer, n > MOX_LOOKUP_MAX, offsets that decrease, or offs[n] - offs[0] >=
 * 2^32 query bytes.  After any error the engine is usable and counts, index
 * and info are untouched: they are written only once the whole call has
 * succeeded, and then completely.
 * MOX_LOOKUP_GRID=<workgroups> (tests; read at each call) caps the grid of the
 * pass over the result, so that a small table runs several grid strides. */
#define MOX_LOOKUP_MAX (1u << 20)          /* query words per call */
#define MOX_LOOKUP_NONE (~0ull)            /* index of a word the result does not hold */
typedef struct mox_lookup_info {
  uint64_t queries;       /* n */
  uint64_t distinct;      /* distinct query words */
  uint64_t found;         /* query positions whose word the result holds */
  uint64_t tag_mismatch;  /* probes where the hash tag was equal and the bytes differed */
  uint64_t reserved[4];
} mox_lookup_info;
int mox_lookup_words(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, uint64_t n,
                     uint64_t* counts, uint64_t* index, mox_lookup_info* info);

/* ---- filtering the device-resident result ---- */
/* Makes the device-resident result smaller, on the GPU: the words that satisfy
 * the predicate *f, with their counts, become the engine's result.  Only the
 * word list goes to the device and four totals come back; the table is not
 * fetched and no host pass runs over it.  Afterwards mox_top_words,
 * mox_write_result / mox_result_text, mox_lookup_words, mox_accumulate,
 * mox_sort_result and mox_fetch_table work on the subset as on any result.
 * Predicate: a word is kept when every active term holds; a zeroed mox_filter
 * keeps everything.
 *  - count: min_count <= count <= max_count (max_count == 0: no upper bound).
 *    {0, 0} is "any count", so the zero-count words mox_reduce_pairs lets
 *    through cannot be selected alone (min_count = 1 drops them).
 *  - length in BYTES: min_len <= length <= max_len (max_len == 0: no bound).
 *  - prefix: the word's first prefix_len bytes equal prefix[0, prefix_len),
 *    compared bytewise; a word shorter than the prefix is dropped.
 *  - list: MOX_FILTER_WORDS_DROP removes the listed words (a stop list; with
 *    n_words == 0 there is no list term), MOX_FILTER_WORDS_KEEP keeps only
 *    listed words (a vocabulary; with n_words == 0 nothing is kept).  List
 *    words are taken verbatim, as mox_lookup_words takes its queries (not
 *    lowercased, duplicates allowed): a run's table holds words lowercased by
 *    Rust's rule, so lowercase the list the same way.
 * Result: the kept words in the order they had (engine, rank or bytewise
 * order), tokens = the sum of the kept counts.  Sorted and folded state are
 * the source's: a subset of a sorted table is sorted, a subset of a total
 * already folded is not folded again (mox_accumulate returns MOX_ESTATE until
 * a run or mox_accumulate_reset).  The new result is no pass's table and no
 * exchanged one, even when every word was kept: mox_exchange / mox_gather
 * after a filter return MOX_ESTATE.  The accumulator is untouched.  Zero kept
 * words give a valid empty result (n == 0), which every call accepts as it
 * accepts the empty corpus's.  The call never sorts, MOX_F_SORT_BYTES or not.
 * MOX_FILTER_COUNT_ONLY: only *info is produced; the result, its flags and its
 * buffers are exactly what they were ("how many hapaxes", "how many tokens do
 * the stop words carry").
 * Works on every form of result: a run's, mox_reduce_pairs, exchanged,
 * gathered, mox_run_shards, sorted, the accumulator's total, a filtered one
 * (filtering twice equals filtering by the conjunction).  Completes pending
 * asynchronous passes first.  An engine group: member 0's gathered result, on
 * member 0.
 * Distributed use: every term is per word, and after mox_exchange each word's
 * final count lives on one rank, so ranks filter their own exchanged result
 * and merge top lists or sum lookups as before.  A count term applied to a
 * local, un-exchanged table filters partial counts and is wrong.
 * info may be NULL.  Device memory: two sets of output buffers (a call writes
 * the set the result does not live in) and O(words / 8) scratch, held by the
 * engine until mox_engine_destroy.
 * MOX_ESTATE: no result yet.  MOX_EINVAL: a NULL engine or filter, a NULL
 * pointer that is needed, prefix_len > MOX_FILTER_PREFIX_MAX, n_words >
 * MOX_LOOKUP_MAX, offsets that decrease (or 2^32 list bytes and more), an
 * unknown mode or flag, a reserved word that is not 0.  After any error,
 * MOX_ENOMEM for the output buffers included, the result is exactly what it
 * was and *info is untouched.
 * MOX_FILTER_GRID=<workgroups> (tests; read at each call) caps the grid of the
 * two passes over the table; MOX_TEST_FAIL_FILTER=1 (tests; read at each call)
 * returns MOX_ENOMEM after the count pass and before the output is written. */
#define MOX_FILTER_PREFIX_MAX 16
#define MOX_FILTER_WORDS_DROP 0u   /* listed words are removed (stop list) */
#define MOX_FILTER_WORDS_KEEP 1u   /* only listed words survive (vocabulary) */
#define MOX_FILTER_COUNT_ONLY 0x1u /* flags: fill info, leave the result as it is */
typedef struct mox_filter {
  uint64_t min_count, max_count;   /* keep min_count <= count <= max_count; max_count == 0: no upper bound */
  uint64_t min_len, max_len;       /* word length in BYTES; max_len == 0: no upper bound */
  const uint8_t* prefix;           /* keep words whose first prefix_len bytes equal these; */
  uint64_t prefix_len;             /*   0: no prefix term; > MOX_FILTER_PREFIX_MAX: MOX_EINVAL */
  const uint8_t* words;            /* word list, word i = words[word_offs[i], word_offs[i+1]), verbatim */
  const uint64_t* word_offs;       /*   (as mox_lookup_words takes its queries; duplicates allowed) */
  uint64_t n_words;                /*   <= MOX_LOOKUP_MAX */
  uint32_t words_mode;             /* MOX_FILTER_WORDS_* ; DROP with n_words == 0 is "no list term" */
  uint32_t flags;                  /* MOX_FILTER_* */
  uint64_t reserved[4];            /* must be 0 */
} mox_filter;
typedef struct mox_filter_info {
  uint64_t words_in, words_kept;
  uint64_t tokens_in, tokens_kept; /* tokens_kept = sum of the kept counts */
  uint64_t bytes_kept;             /* word bytes of the kept table */
  uint64_t list_found;             /* distinct list words the result held */
  uint64_t device_bytes;           /* device memory the filter holds after the call */
  double ms;                       /* wall time of the call */
  uint64_t reserved[4];
} mox_filter_info;
int mox_filter_result(mox_engine* e, const mox_filter* f, mox_filter_info* info /* may be NULL */);

/* ---- joining the device-resident result against the accumulated total ---- */
/* Matches the device-resident result R against the accumulator's total T
 * (mox_accumulate), on the GPU, and keeps the rows of R the mode selects:
 * MOX_JOIN_SEMI the rows whose word T holds ("known words"), MOX_JOIN_ANTI the
 * rows whose word T lacks ("new words": the window minus the total's
 * vocabulary).  Neither table is fetched and no host pass runs over them; one
 * 64-byte block comes back.  *info also carries the overlap sums two corpora
 * are compared by: words_matched (vocabulary overlap), the tokens on shared
 * words on either side, and tokens_min = sum of min(a, b), the multiset
 * intersection that weighted Jaccard needs.
 * Operands: R is the result in any form: a run's, mox_reduce_pairs, exchanged,
 * gathered, mox_run_shards, sorted, ranked, filtered, re-keyed, joined, or a
 * total that is itself the result.  T is the accumulator's total.  An empty
 * accumulator (no fold since create or mox_accumulate_reset) is an empty T:
 * SEMI keeps nothing, ANTI keeps everything, no kernel reads T and the call is
 * not an error; an accumulator that holds an empty table behaves the same.
 * Matching: words match verbatim and bytewise, and the length is part of the
 * word ("ab" is not "ab\0").  A word T holds with count 0 is held: SEMI keeps
 * it, and MOX_JOIN_COUNTS_TOTAL gives it 0.
 * Counts: kept rows keep their own count (MOX_JOIN_COUNTS_RESULT), take T's
 * (MOX_JOIN_COUNTS_TOTAL: "seen before, and how often overall") or the smaller
 * of the two (MOX_JOIN_COUNTS_MIN); the last two with SEMI only.
 * The new result: the kept rows in the order they had in R; tokens = the sum
 * of the kept counts as written, substituted ones included, wrapping as
 * uint64_t.  Sorted and folded state are R's.  Ranked state is R's with
 * MOX_JOIN_COUNTS_RESULT; with _TOTAL or _MIN it is cleared, unless at most one
 * row is kept.  As after a filter the new result is no pass's table and no
 * exchanged one: mox_exchange / mox_gather afterwards return MOX_ESTATE.  It
 * lives where a filtered result lives, so joining or filtering it again works.
 * The accumulator is untouched in every case.  The call never sorts,
 * MOX_F_SORT_BYTES or not.
 * MOX_JOIN_COUNT_ONLY: only *info is produced; the result, its flags and its
 * buffers are exactly what they were.
 * Completes pending asynchronous passes first.  An engine group: member 0's
 * gathered result against member 0's accumulator, on member 0.
 * Distributed use: after a hash-owner mox_exchange (no MOX_F_SORT_BYTES) a
 * word's owner rank is the same in every window, so ranks that accumulate
 * their exchanged results join locally and add their infos
 * (mox.dist.sum_joins).  With ranged owners (MOX_F_SORT_BYTES) the splitters
 * move from exchange to exchange and a local join is wrong: gather first.
 * info may be NULL.  Device memory: a hash set over R of 32 to 64 bytes per row
 * of R (8-byte slots, the power of two >= 4 rows, load <= 1/4), 8 or 16 bytes
 * per row of R for the matched counts, and the filter's scratch and output
 * buffers; nothing is sized by T.  Held by the engine until mox_engine_destroy.
 * MOX_ESTATE: no result yet.  MOX_EINVAL: a NULL engine or spec, an unknown
 * mode, counts value or flag, ANTI with a counts value other than
 * MOX_JOIN_COUNTS_RESULT, a pad or reserved word that is not 0, a result of more
 * than MOX_JOIN_MAX_WORDS rows.  MOX_ENOMEM: the scratch or the output buffers
 * cannot be allocated.  After any error the result is exactly what it was and
 * *info is untouched.
 * MOX_JOIN_GRID=<workgroups> (tests; read at each call) caps every grid of the
 * call; MOX_TEST_FAIL_JOIN=1 (tests; read at each call) returns MOX_ENOMEM
 * after the stream pass and before any output buffer is written. */
#define MOX_JOIN_SEMI 0u          /* keep the result's rows whose word the total holds */
#define MOX_JOIN_ANTI 1u          /* keep the result's rows whose word the total lacks */
#define MOX_JOIN_COUNTS_RESULT 0u /* kept rows keep their own count */
#define MOX_JOIN_COUNTS_TOTAL  1u /* kept rows take the total's count        (SEMI only) */
#define MOX_JOIN_COUNTS_MIN    2u /* kept rows take min(own, total's) count  (SEMI only) */
#define MOX_JOIN_COUNT_ONLY 0x1u  /* flags: fill info, leave the result as it is */
#define MOX_JOIN_MAX_WORDS 0xFFFFFFFEull  /* rows of the RESULT: a slot holds row + 1 in 32 bits */
typedef struct mox_join {
  uint32_t mode, counts, flags, pad;   /* pad must be 0 */
  uint64_t reserved[4];                /* must be 0 */
} mox_join;                            /* 48 bytes */
typedef struct mox_join_info {
  uint64_t words_in, words_total;      /* rows of the result / of the total */
  uint64_t words_matched;              /* result words the total holds (whatever the mode) */
  uint64_t words_kept;
  uint64_t tokens_in, tokens_total;
  uint64_t tokens_matched_result;      /* sum of the result's counts over matched words */
  uint64_t tokens_matched_total;       /* sum of the total's counts over matched words */
  uint64_t tokens_min;                 /* sum of min(result's, total's) over matched words */
  uint64_t tokens_kept, bytes_kept;
  uint64_t tag_mismatch;               /* probes with an equal tag and different bytes */
  uint64_t device_bytes;
  double ms;
  uint64_t reserved[4];
} mox_join_info;
int mox_join_total(mox_engine* e, const mox_join* j, mox_join_info* info /* may be NULL */);

/* ---- ranking the device-resident result by count, fetching it by rows ---- */
/* Reorders the device-resident result by count, on the GPU: the same words
 * and counts, most frequent first, or least frequent first with
 * MOX_RANK_ASCENDING.  Nothing is fetched and no host pass runs over the
 * table.  Afterwards mox_fetch_table / mox_fetch_rows, mox_write_result /
 * mox_result_text, mox_top_words, mox_lookup_words (its indices are ranks),
 * mox_filter_result and mox_accumulate work on the ranked table as on any
 * result: "the first N rows by count", "page k of the ranked vocabulary" and
 * "final_result.txt sorted by count" need no full fetch.
 * Order: count descending (ascending with the flag); words with equal counts
 * keep the order they had in device memory at the call -- the sort is stable.
 * This is the tie rule of mox_top_words and mox_print_top_words, so
 * mox_top_words(k) taken before the call equals the first min(k, n) rows
 * after it, and mox_sort_result followed by mox_rank_result gives the
 * deterministic order "count descending, then bytewise" (engine order can
 * differ from run to run among words longer than 16 bytes).  Counts are
 * compared as full u64: 0 and 2^64 - 1 (mox_reduce_pairs lets both through)
 * sort like any other.  Ties keep table order in both directions, so the
 * ascending ranking is the descending one reversed only where counts are
 * distinct.
 * Works on every form of result: a run's, mox_reduce_pairs, exchanged,
 * gathered, mox_run_shards, sorted, filtered, the accumulator's total, a
 * ranked one (ranking twice, or ascending after descending, is legal).
 * Completes pending asynchronous passes first.  An engine group: member 0's
 * gathered result, on member 0.
 * State: tokens, the number of words, the byte total, the folded state and
 * the accumulator are unchanged.  As after a filter, the new result is no
 * pass's table and no exchanged one: mox_exchange / mox_gather afterwards
 * return MOX_ESTATE, so distributed callers gather first and rank at the
 * root.  The result is marked ranked and no longer counts as bytewise sorted
 * (unless it has at most one word): a ranked result is NOT re-sorted by the
 * implicit MOX_F_SORT_BYTES sort of mox_fetch_table, mox_fetch_rows,
 * mox_write_result and mox_result_text -- an explicit ranking wins over the
 * flag.  An explicit mox_sort_result sorts it bytewise and ends the ranking,
 * as does whatever replaces the result (a run, mox_reduce_pairs, an exchange,
 * a gather, an accumulate merge).  mox_filter_result keeps it (a subset of a
 * ranked table is ranked), and so does the first mox_accumulate into an empty
 * accumulator (the result stays the table it was).
 * info may be NULL.  digit_passes: only the bytes of the largest count are
 * sorted, ceil(bitlen(max_count) / 8) radix passes of 8 bits; max_count == 0
 * runs none (the order stays).  Empty and one-word tables succeed and launch
 * nothing that reads rows.  Device memory: two sets of output buffers (a call
 * writes the set the result does not live in) and 24 bytes of scratch per
 * word plus 1 KiB per 4096 words, held by the engine until mox_engine_destroy.
 * MOX_ESTATE: no result yet.  MOX_EINVAL: a NULL engine, unknown flag bits, or
 * a table of more than MOX_RANK_MAX_WORDS words (row indices travel as u32).
 * MOX_ENOMEM: the scratch or the output buffers cannot be allocated.  After
 * any error the result is exactly what it was and *info is untouched.
 * MOX_RANK_GRID=<workgroups> (tests; read at each call) caps the grid of every
 * pass over rows; MOX_TEST_FAIL_RANK=1 (tests; read at each call) returns
 * MOX_ENOMEM after the permutation is computed and before any output buffer is
 * written. */
#define MOX_RANK_ASCENDING 0x1u   /* least frequent first; default: most frequent first */
#define MOX_RANK_MAX_WORDS 0xFFFFFFFFull
typedef struct mox_rank_info {
  uint64_t words, tokens;      /* of the result (unchanged by the call) */
  uint64_t max_count;          /* largest count in the table (0 for an empty one) */
  uint64_t digit_passes;       /* radix passes that ran */
  uint64_t device_bytes;       /* device memory the ranking holds after the call */
  double ms;                   /* wall time of the call */
  uint64_t reserved[4];
} mox_rank_info;
int mox_rank_result(mox_engine* e, uint32_t flags, mox_rank_info* info /* may be NULL */);
/* Rows [first, min(first + n, N)) of the device-resident result (N words) as
 * a normal mox_table (mox_table_free), offs rebased to 0; tokens is the whole
 * result's total, as mox_top_words reports it.  The rows are taken in the
 * order mox_fetch_table would return them: the same implicit MOX_F_SORT_BYTES
 * sort runs first (flag set, result neither sorted nor ranked), so pages laid
 * end to end are byte for byte the fetched table.  Only the slice crosses
 * PCIe: its offsets first, then its counts and exactly its bytes; nothing
 * sized by the whole table is copied (one exception: where the implicit sort
 * finds no room for its device scratch the order exists only on the host, so
 * the whole table is fetched and sorted there, as mox_fetch_table does, for
 * every page).  first >= N or n == 0: an empty table.  The result stays where
 * it is.  Completes pending asynchronous passes first.  MOX_ESTATE: no result
 * yet; MOX_EINVAL: a NULL argument.  An engine group: member 0's gathered
 * result. */
int mox_fetch_rows(mox_engine* e, uint64_t first, uint64_t n, mox_table** out);

/* ---- re-keying the device-resident result ---- */
/* Replaces every word of the device-resident result by a byte window of
 * itself and sums the rows whose windows are equal, on the GPU: "the", "the,",
 * "(the)" and "the." become one row with the summed count.  The map's
 * tokenisation is unchanged (split_whitespace + to_lowercase, as the
 * reference); this call works on the table afterwards.  Nothing is fetched and
 * no host pass runs over the table: six totals come back.  Afterwards
 * mox_top_words, mox_write_result / mox_result_text, mox_lookup_words,
 * mox_filter_result, mox_rank_result, mox_sort_result, mox_fetch_table /
 * mox_fetch_rows and mox_accumulate work on the new table as on any result.
 * Every rule is per word, over its bytes, verbatim:
 *  1. Trim.  Leading bytes are dropped while the byte is < 128 and its bit is
 *     set in the effective set; then trailing bytes the same way.  Bytes >= 128
 *     are never stripped, so a UTF-8 sequence is never cut.  The effective set
 *     is trim_set, or'd with the punctuation set when
 *     MOX_REKEY_TRIM_ASCII_PUNCT is given: the 32 bytes of Rust's
 *     char::is_ascii_punctuation (Python's string.punctuation), as masks
 *     {MOX_REKEY_PUNCT_LO, MOX_REKEY_PUNCT_HI}.  Inner punctuation stays:
 *     "don't", "a.b".
 *  2. Cap (max_chars = K > 0).  A character start is a byte b with
 *     (b & 0xC0) != 0x80; the window ends before the (K+1)-th character start
 *     in the trimmed window.  Continuation bytes at the very front of the
 *     window are kept.  For valid UTF-8 this is the first K characters; it is
 *     defined for any bytes, as mox_reduce_pairs words may be anything.  No
 *     second trim follows the cap: "a.b.c" with K = 2 gives "a.".
 *  3. Drop.  An empty window drops the row; its count goes to tokens_dropped,
 *     and tokens_out = tokens_in - tokens_dropped is the new result's tokens.
 *  4. Reduce.  Rows with equal windows are summed as u64, wrapping as
 *     elsewhere; a word present with count 0 stays present.  The new table is
 *     what mox_reduce_pairs gives over the windowed rows, by the same
 *     classification rule (1..16 bytes without NUL: a 16-byte key; everything
 *     else: the long table), so a word may change class in either direction.
 *     Order is engine order.
 * State after a re-key that changed something: the result is a reduce pass's
 * table, as after an accumulate merge: a pass's own table, not exchanged, not
 * sorted, not ranked, so mox_exchange may start from it.  The folded state is
 * kept: a re-keyed total that was already folded is not folded again
 * (mox_accumulate returns MOX_ESTATE until a run or mox_accumulate_reset).
 * The accumulator is untouched.  Re-keying commutes with sums, so callers
 * re-key each run's result before mox_accumulate, or re-key once at the end;
 * a re-key of the total followed by another fold merges into the un-re-keyed
 * accumulator.
 * Nothing to do: when words_changed == 0 no reduce runs, and the result, its
 * order and all its flags (sorted, ranked, folded, pass, exchanged) are
 * exactly what they were; *info is still filled.  The call is therefore
 * idempotent at the cost of one pass over the table.  A spec with an empty
 * effective set and no cap is the same case.
 * Works on every form of result: a run's, mox_reduce_pairs, exchanged,
 * gathered, mox_run_shards, sorted, ranked, filtered, the accumulator's total,
 * a re-keyed one.  Completes pending asynchronous passes first.  An engine
 * group: member 0's gathered result, on member 0.
 * Distributed use: ranks re-key their local pass result and then
 * mox_exchange (or mox_exchange_host): owners are chosen from the new keys, so
 * the exchange sums the variants across ranks.
 * info may be NULL.  Device memory: 48 bytes of scratch per 1024 words and the
 * exchange's receive buffers (the windowed rows in wire form), held by the
 * engine until mox_engine_destroy.  A lane walks a run of stripped bytes
 * serially: a 100,000-byte word of dashes costs 100,000 steps on one lane.
 * MOX_ESTATE: no result yet.  MOX_EINVAL: a NULL engine or spec, an unknown
 * flag, a pad or reserved word that is not 0.  Any error before the reduce
 * pass -- MOX_ENOMEM for the scratch or the wire buffers included -- leaves
 * the result exactly as it was and *info untouched.  An error inside the
 * reduce pass leaves the engine with no result, as a failed mox_reduce_pairs
 * does (the source table's buffers are the pass's to overwrite; no copy is
 * kept to buy more); the accumulator is intact.
 * MOX_REKEY_GRID=<workgroups> (tests; read at each call) caps the grid of the
 * passes over rows; MOX_TEST_FAIL_REKEY=1 (tests; read at each call) returns
 * MOX_ENOMEM after the pack and before the reduce pass. */
#define MOX_REKEY_TRIM_ASCII_PUNCT 0x1u  /* or Rust's char::is_ascii_punctuation set into trim_set */
#define MOX_REKEY_PUNCT_LO 0xFC00FFFE00000000ull  /* the punctuation bytes below 64 */
#define MOX_REKEY_PUNCT_HI 0x78000001F8000001ull  /* ... and from 64 on */
typedef struct mox_rekey {
  uint64_t trim_set[2];   /* bit (b & 63) of trim_set[b >> 6]: ASCII byte b (< 128) is stripped from both ends */
  uint64_t max_chars;     /* then keep only the first max_chars characters; 0: no cap */
  uint32_t flags;         /* MOX_REKEY_* ; unknown bits: MOX_EINVAL */
  uint32_t pad;           /* must be 0 */
  uint64_t reserved[4];   /* must be 0 */
} mox_rekey;               /* 64 bytes */
typedef struct mox_rekey_info {
  uint64_t words_in, words_out;      /* rows before / after */
  uint64_t words_changed;            /* rows whose window is not the whole word (dropped ones included) */
  uint64_t words_dropped;            /* rows whose window is empty */
  uint64_t tokens_in, tokens_out, tokens_dropped;
  uint64_t bytes_out;                /* word bytes of the new table */
  uint64_t device_bytes;             /* device memory the call holds afterwards */
  double ms;                         /* wall time of the call */
  uint64_t reserved[4];
} mox_rekey_info;          /* 112 bytes */
int mox_rekey_result(mox_engine* e, const mox_rekey* k, mox_rekey_info* info /* may be NULL */);

/* ---- searching the sorted device-resident result ---- */
/* Row ranges of n keys in the bytewise-sorted device-resident result, by binary
 * search on the GPU: O(n log N) loads instead of a pass over the table.  Only
 * the keys go to the device and two (or three) numbers per key come back.  Key
 * i is bytes[offs[i], offs[i+1]), taken verbatim as mox_lookup_words takes its
 * queries (not lowercased, not validated; any byte, 0x00 and 0xFF included).
 * The order is the table's: Rust String Ord, bytes compared as unsigned, a
 * proper prefix before the longer word ("ab" < "ab\0").
 * first[i], last[i]: row indices into the table as it lies in device memory --
 * exactly the rows mox_fetch_rows(first[i], last[i] - first[i]) returns and
 * mox_top_rows selects from:
 *   MOX_FIND_EXACT   the row whose word equals the key (last = first + 1),
 *   MOX_FIND_PREFIX  the rows whose word starts with the key (an empty key:
 *                    every row),
 *   MOX_FIND_LOWER   first = last = the number of rows whose word is < key.
 * An absent key gives first == last == its insertion point, in every mode.
 * sums[i] (sums may be NULL): the wrapping u64 sum of counts[first, last) --
 * EXACT: the word's count, PREFIX: the tokens under the prefix, LOWER: 0.
 * With sums == NULL no kernel reads a count.  The sums are deterministic: no
 * atomic adds a count.  info may be NULL.  With n == 0 nothing runs on the
 * device and bytes, offs, first, last may be NULL.
 * Needs a result in bytewise order: after mox_sort_result, a MOX_F_SORT_BYTES
 * fetch, a ranged exchange or gather; a table of at most one word is in order
 * as it is.  With MOX_F_SORT_BYTES set and a result neither sorted nor ranked
 * the implicit device sort of mox_fetch_rows runs first; if that sort returns
 * MOX_ENOMEM so does the call.  Any other result that is not in bytewise order
 * (a ranked one included) is MOX_ESTATE: call mox_sort_result first.  Apart
 * from that implicit sort the call only reads: result, accumulator and every
 * state flag are unchanged.  Completes pending asynchronous passes first.  An
 * engine group: member 0's gathered result.  After an exchange each rank owns
 * a byte range of words, so the ranks' last - first and sums add up to the
 * global figures without a gather.
 * Cost: one lane per key, ceil(log2(N + 1)) steps of two offsets and the
 * word's bytes, compared 8 bytes at a time up to the first difference (a long
 * key against words that share its long prefix: O(len / 8) per step on that
 * lane).  The sums read at most 2 x 1,023 counts per key directly; one
 * streaming pass over the N counts (never over word bytes) is added only when
 * some range holds a whole aligned tile of 1,024 rows (mox_find_info.tile_pass).
 * Device scratch is O(n + key bytes + N / 1024), lives in the engine and is
 * freed by mox_engine_destroy.
 * MOX_ESTATE: no result yet, or a result not in bytewise order.  MOX_EINVAL: a
 * NULL engine or required pointer, n > MOX_FIND_MAX, an unknown mode, offsets
 * that decrease, or offs[n] - offs[0] >= 2^32 key bytes.  After any error the
 * engine is usable and first, last, sums and info are untouched: they are
 * written only after the last device check, and then completely.
 * MOX_FIND_GRID=<workgroups> (tests; read at each call) caps every grid of the
 * call, so that a small table and few keys run several grid strides. */
#define MOX_FIND_EXACT  0u  /* the row whose word equals the key */
#define MOX_FIND_PREFIX 1u  /* the rows whose word starts with the key (empty key: every row) */
#define MOX_FIND_LOWER  2u  /* first = last = number of rows whose word is bytewise < key */
#define MOX_FIND_MAX (1u << 20)
typedef struct mox_find_info {
  uint64_t queries, matched;   /* matched: queries with last > first */
  uint64_t rows;               /* sum over queries of last - first */
  uint64_t tile_pass;          /* 1: some range spanned a whole tile, the pass over the counts ran */
  uint64_t device_bytes;       /* device memory the search holds after the call */
  double ms;                   /* wall time of the call */
  uint64_t reserved[4];
} mox_find_info;
int mox_find_ranges(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, uint64_t n, uint32_t mode,
                    uint64_t* first, uint64_t* last, uint64_t* sums /* may be NULL */, mox_find_info* info /* may be NULL */);
/* mox_top_words over rows [first, min(first + n, N)) of the device-resident
 * result: the k most frequent words among those rows, count descending, equal
 * counts by table index ascending, tokens the whole result's total, k <=
 * MOX_TOP_MAX.  Works on any result, sorted or not; with a range from
 * mox_find_ranges(MOX_FIND_PREFIX) it is "the k most frequent words that start
 * with ..." and never touches a row outside the range.  first >= N, n == 0 or
 * k == 0: an empty table.  Errors as mox_top_words. */
int mox_top_rows(mox_engine* e, uint64_t first, uint64_t n, size_t k, mox_table** out);

/* ---- histograms of the device-resident result ---- */
/* Group-by with an aggregate over a derived key, on the GPU: the rows of the
 * device-resident result are binned by a u64 key derived from each row, and
 * per bin come back the key, the rows (bin_words), the wrapping u64 sum of
 * their counts (bin_tokens) and the lowest table index of a row with that key
 * (first_row).  ("Group" means an engine group in this interface, so the call
 * is a histogram with bins.)  The keys:
 *   MOX_HIST_COUNT  the row's count: the frequency spectrum (count of counts),
 *                   the input of Good-Turing smoothing and Zipf plots,
 *   MOX_HIST_BYTES  the word's length in bytes,
 *   MOX_HIST_CHARS  the word's character starts: bytes b with
 *                   (b & 0xC0) != 0x80, mox_rekey_result's rule; for valid
 *                   UTF-8 the word's characters,
 *   MOX_HIST_FIRST  the word's first character.  The window is the word's
 *                   first byte plus the continuation bytes ((b & 0xC0) == 0x80)
 *                   that follow it, at most 4 bytes in all; a word that opens
 *                   with continuation bytes keeps them, as the re-keying does.
 *                   key = the window's bytes packed big-endian into bits 39..8
 *                   (byte 0 in bits 39..32) and the window's length in bits
 *                   7..0, so ascending keys are the windows in bytewise order,
 *                   a proper prefix first.  For valid UTF-8 the window is the
 *                   first character's encoding.  An empty word's key is 0 (a
 *                   table holds no empty word today).
 * keys come out ascending and all distinct.  With MOX_HIST_RANGE only rows
 * [first, min(first + rows, N)) are binned, as mox_top_rows takes them (a
 * range from mox_find_ranges(MOX_FIND_PREFIX): the histogram of the words
 * under a prefix); first_row stays absolute, an index into the whole table.
 * The call only reads.  The result, its buffers, every state flag (pass,
 * exchanged, sorted, ranked, folded) and the accumulator are exactly what they
 * were.  It never sorts the table, MOX_F_SORT_BYTES or not: bins do not depend
 * on row order except first_row, which is an index into the table as it lies
 * in device memory at the call -- the row mox_fetch_rows(first_row, 1) returns.
 * Works on every form of result: a run's, mox_reduce_pairs, exchanged,
 * gathered, mox_run_shards, sorted, ranked, filtered, re-keyed, joined, the
 * accumulator's total.  Completes pending asynchronous passes first.  An engine
 * group: member 0's gathered result.
 * Only 4 x bins u64 values and a few totals come back: nothing sized by the
 * table crosses PCIe and no host pass runs over rows.
 * Small cases: an empty result or an empty range gives n == 0 with valid
 * pointers, and nothing runs on the device; one row gives one bin; when every
 * key is 0 there is one bin and no radix pass (digit_passes == 0).
 * Sums: bin_tokens and tokens wrap as u64, like every other sum here.  For
 * MOX_HIST_COUNT bin_tokens[i] == keys[i] * bin_words[i] mod 2^64.  The sum of
 * bin_words is words; the sum of bin_tokens is tokens, which equals the
 * result's tokens when no range is given.  These identities are checked on the
 * host before anything is handed out: a mismatch is MOX_EHIP ("inconsistent
 * totals"), as in mox_rank_result.  The sums are deterministic: no atomic adds
 * a count.
 * Ranked tables: on a result ranked by mox_rank_result the MOX_HIST_COUNT bins
 * are contiguous row ranges [first_row, first_row + bin_words), so
 * mox_fetch_rows(first_row[i], bin_words[i]) is "all words that occur keys[i]
 * times".
 * Distributed use: after mox_exchange the ranks own disjoint words, so the
 * ranks' bins merge by key and words and tokens add up without a gather;
 * first_row is per rank.
 * Cost: COUNT and BYTES never read a word byte, FIRST reads at most 4 bytes per
 * word, CHARS makes one pass over the word bytes.  Then come
 * ceil(bitlen(max key) / 8) radix passes over the rows (mox_rank_result's sort,
 * sharing its scratch) and one pass for the bins.  There is no cap on bins:
 * all-distinct counts give bins == rows.  Device scratch: 8 bytes per row for a
 * derived key, 24 bytes per row for the sort, 48 bytes per bin; it lives in the
 * engine and is freed by mox_engine_destroy.
 * The table is library-owned until mox_hist_free (NULL is fine).
 * MOX_ESTATE: no result yet.  MOX_EINVAL: a NULL engine, spec or out, an
 * unknown key or flag, a reserved word that is not 0, first or rows not 0
 * without MOX_HIST_RANGE, more than MOX_HIST_MAX_WORDS rows in the range.
 * MOX_ENOMEM: scratch or host memory cannot be allocated.  After any error
 * *out and *info are untouched and the engine is usable.
 * MOX_HIST_GRID=<workgroups> (tests; read at each call) caps every grid of the
 * call, the shared sort's grids included.  MOX_TEST_FAIL_HIST=1 (tests; read at
 * each call) returns MOX_ENOMEM after the bins are counted and before anything
 * is copied out. */
#define MOX_HIST_COUNT 0u  /* key = the row's count: the frequency spectrum */
#define MOX_HIST_BYTES 1u  /* key = the word's length in bytes */
#define MOX_HIST_CHARS 2u  /* key = the word's character starts: bytes b with (b & 0xC0) != 0x80
                              (mox_rekey_result's rule; for valid UTF-8: its characters) */
#define MOX_HIST_FIRST 3u  /* key = the word's first character (above) */
#define MOX_HIST_RANGE 0x1u /* flags: only rows [first, min(first + rows, N)), as mox_top_rows takes them */
#define MOX_HIST_MAX_WORDS 0xFFFFFFFFull   /* rows histogrammed per call: row indices travel as u32 */
typedef struct mox_hist {
  uint32_t key, flags;
  uint64_t first, rows;     /* both must be 0 without MOX_HIST_RANGE; with it rows == 0 is the empty range */
  uint64_t reserved[4];     /* must be 0 */
} mox_hist;                 /* 56 bytes */
typedef struct mox_hist_table {   /* library-owned until mox_hist_free */
  uint64_t n;                     /* bins: distinct keys among the rows */
  uint64_t words, tokens;         /* rows histogrammed, and the wrapping u64 sum of their counts */
  const uint64_t* keys;           /* [n] ascending, all distinct */
  const uint64_t* bin_words;      /* [n] rows with this key (>= 1) */
  const uint64_t* bin_tokens;     /* [n] wrapping u64 sum of their counts */
  const uint64_t* first_row;      /* [n] lowest table index (absolute, not range-relative) of a row with this key */
} mox_hist_table;
typedef struct mox_hist_info {
  uint64_t words, tokens, bins, max_key, digit_passes, device_bytes;
  double ms;
  uint64_t reserved[4];
} mox_hist_info;
int mox_hist_result(mox_engine* e, const mox_hist* h, mox_hist_table** out, mox_hist_info* info /* may be NULL */);
void mox_hist_free(mox_hist_table* t);

int mox_get_stats(const mox_engine* e, mox_stats* out);

/* device memory helpers so callers need no HIP headers */
int mox_device_alloc(mox_engine* e, size_t bytes, void** d_ptr);
int mox_device_free(mox_engine* e, void* d_ptr);
int mox_memcpy_h2d(mox_engine* e, void* d_dst, const void* h_src, size_t bytes);
int mox_memcpy_d2h(mox_engine* e, void* h_dst, const void* d_src, size_t bytes);
int mox_synchronize(mox_engine* e);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ---- */
#define MOX_UNIQUE_ID_BYTES 128
int mox_comm_unique_id(uint8_t id[MOX_UNIQUE_ID_BYTES]);
int mox_comm_init(mox_engine* e, int nranks, int rank, const uint8_t id[MOX_UNIQUE_ID_BYTES]);
/* After mox_run_range on every rank: hash-partition the local table, exchange
 * it with one RCCL all-to-all, and reduce the received partials.  Afterwards
 * this rank owns the final counts of its hash range (disjoint across ranks).
 * With MOX_F_SORT_BYTES the words are owned by byte range instead (splitters
 * from 1,024 sampled 8-byte prefixes per rank, exchanged first) and every rank
 * sorts its own range on its GPU, so mox_gather in rank order is the table in
 * bytewise order (no sort at the root). */
int mox_exchange(mox_engine* e);
/* Host-staged transport for the same exchange (several ranks sharing one GPU,
 * or no RCCL): the library calls fn once per all-to-all with pinned host
 * buffers; send holds nranks consecutive blocks of send_bytes[d] bytes for
 * rank d, recv must receive nranks consecutive blocks of recv_bytes[s] bytes
 * from rank s.  Return 0 on success. */
typedef int (*mox_alltoallv_fn)(void* user, const void* send, const uint64_t* send_bytes, void* recv,
                                const uint64_t* recv_bytes);
int mox_exchange_host(mox_engine* e, int nranks, int rank, mox_alltoallv_fn fn, void* user);
/* After mox_exchange on every rank: gather the ranks' final tables into the
 * root's engine (RCCL send/recv, device to device).  Ranks own disjoint words
 * after the exchange, so the root's table afterwards is the whole corpus's
 * table (fetch it with mox_fetch_table; MOX_F_SORT_BYTES gives bytewise order).
 * Other ranks keep their own table.  Replaces the reference's single-process
 * result (main.rs:22) for one process per GPU. */
int mox_gather(mox_engine* e, int root);
/* The same over the host-staged transport of mox_exchange_host. */
int mox_gather_host(mox_engine* e, int nranks, int rank, int root, mox_alltoallv_fn fn, void* user);

/* ---- output layer (reference L5: main.rs:170-192) ---- */
/* final_result.txt: one "{word} {count}\n" line per word.  Truncates on open
 * (the reference does not: SURVEY.md §0.2 quirk, not reproduced). */
int mox_write_final_result(const mox_table* t, const char* path);
/* "Top {n} words:" then up to n lines "{word}: {count}", count descending,
 * ties in table order (the reference's tie order is HashMap-random). */
int mox_print_top_words(const mox_table* t, size_t n);

/* ---- intermediate (spill) files, SURVEY.md §8(f) rank 4 ---- */
/* reduce_phase over parsed map files (replaces main.rs:111-150; the parse of
 * read_map_result main.rs:152-168 is host text work): n (word, count) pairs,
 * word i = bytes[offs[i], offs[i+1]) taken verbatim (not lowercased), are
 * summed by word with the GPU reduce; the result is then fetched with
 * mox_fetch_table like a run's.  Duplicate words are summed. */
int mox_reduce_pairs(mox_engine* e, const uint8_t* bytes, const uint64_t* offs, const uint64_t* counts, uint64_t n);

/* ---- test hook (no GPU needed) ---- */
/* The exchange's per-peer send / receive layout (mox_multi.hip x_layout) for
 * nranks ranks whose count rows are counts[i][d][0..2] = (short records, long
 * words, long-word bytes) that rank i sends to rank d, the count all-to-all
 * modelled as the device-copy transport does it.  out[i][k][d], k = 0..7:
 * short send offset / length, blob send offset / length, short receive offset /
 * length, blob receive offset / length of rank i for peer d (bytes). */
int mox_debug_exchange_layout(int nranks, const uint64_t* counts, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* MOX_H */
