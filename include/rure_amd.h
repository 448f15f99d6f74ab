/*
 * rure_amd.h — MI355X drop-in for the batched byte-regex scan path of the
 * reference `rure` C API (regex 0.2.5, regex-capi/include/rure.h).
 *
 * Part 1 re-declares the `rure` entry points a C caller of the reference
 * binds, with the same names, argument meaning, flag values and ownership
 * rules; each cites the reference declaration it replaces.  Every search
 * entry point runs on the GPU (HIP kernels for gfx950); there is no CPU
 * matching path inside this library.
 *
 * Part 2 adds the batched device-pointer entry points the hot path needs
 * (one call scans many haystacks resident in HBM).  Plain pointers and sizes
 * only; `stream` is a `hipStream_t` passed as `void *` (NULL = the null
 * stream).
 */
#ifndef RURE_AMD_H
#define RURE_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- Part 1 */

typedef struct rure rure;                  /* rure.h:29 */
typedef struct rure_set rure_set;          /* rure.h:36 */
typedef struct rure_options rure_options;  /* rure.h:47 */
typedef struct rure_iter rure_iter;        /* rure.h:106 */
typedef struct rure_error rure_error;      /* rure.h:130 */
typedef struct rure_captures rure_captures;                      /* rure.h:95 */
typedef struct rure_iter_capture_names rure_iter_capture_names;  /* rure.h:117 */

/* rure.h:56-68 */
#define RURE_FLAG_CASEI (1 << 0)
#define RURE_FLAG_MULTI (1 << 1)
#define RURE_FLAG_DOTNL (1 << 2)
#define RURE_FLAG_SWAP_GREED (1 << 3)
#define RURE_FLAG_SPACE (1 << 4)
#define RURE_FLAG_UNICODE (1 << 5)
#define RURE_DEFAULT_FLAGS RURE_FLAG_UNICODE

/* rure.h:73-78 */
typedef struct rure_match {
  size_t start;
  size_t end;
} rure_match;

/* rure.h:147 — aborts (after printing the error) if the pattern is invalid. */
rure *rure_compile_must(const char *pattern);
/* rure.h:168-169 — NULL on error (error filled if non-NULL). */
rure *rure_compile(const uint8_t *pattern, size_t length, uint32_t flags,
                   rure_options *options, rure_error *error);
/* rure.h:177 */
void rure_free(rure *re);
/* rure.h:197-198 */
bool rure_is_match(rure *re, const uint8_t *haystack, size_t length, size_t start);
/* rure.h:220-221 — `match` may be NULL. */
bool rure_find(rure *re, const uint8_t *haystack, size_t length, size_t start,
               rure_match *match);
/* rure.h:273-274 */
bool rure_shortest_match(rure *re, const uint8_t *haystack, size_t length,
                         size_t start, size_t *end);
/* rure.h:317-345 — iterator over successive non-overlapping matches. */
rure_iter *rure_iter_new(rure *re);
void rure_iter_free(rure_iter *it);
bool rure_iter_next(rure_iter *it, const uint8_t *haystack, size_t length,
                    rure_match *match);
/* rure.h:248-249 — leftmost-first match with every capture group's location
 * (exec.rs:524-596 dispatch: DFA bounds, then the Pike VM for the groups). */
bool rure_find_captures(rure *re, const uint8_t *haystack, size_t length,
                        size_t start, rure_captures *captures);
/* rure.h:285 — index of the named group, -1 if none. */
int32_t rure_capture_name_index(rure *re, const char *name);
/* rure.h:292-307 — group names in index order ("" for unnamed groups). */
rure_iter_capture_names *rure_iter_capture_names_new(rure *re);
void rure_iter_capture_names_free(rure_iter_capture_names *it);
bool rure_iter_capture_names_next(rure_iter_capture_names *it, char **name);
/* rure.h:369-371 */
bool rure_iter_next_captures(rure_iter *it, const uint8_t *haystack, size_t length,
                             rure_captures *captures);
/* rure.h:385-411 */
rure_captures *rure_captures_new(rure *re);
void rure_captures_free(rure_captures *captures);
bool rure_captures_at(rure_captures *captures, size_t i, rure_match *match);
size_t rure_captures_len(rure_captures *captures);
/* rure.h:423-454 */
rure_options *rure_options_new(void);
void rure_options_free(rure_options *options);
void rure_options_size_limit(rure_options *options, size_t limit);
void rure_options_dfa_size_limit(rure_options *options, size_t limit);
/* rure.h:476-538 */
rure_set *rure_compile_set(const uint8_t **patterns, const size_t *patterns_lengths,
                           size_t patterns_count, uint32_t flags,
                           rure_options *options, rure_error *error);
void rure_set_free(rure_set *re);
bool rure_set_is_match(rure_set *re, const uint8_t *haystack, size_t length, size_t start);
bool rure_set_matches(rure_set *re, const uint8_t *haystack, size_t length, size_t start,
                      bool *matches);
size_t rure_set_len(rure_set *re);
/* rure.h:551-568 */
rure_error *rure_error_new(void);
void rure_error_free(rure_error *err);
const char *rure_error_message(rure_error *err);

/* ---------------------------------------------------------------- Part 2 */

/* Status codes of the batched calls. */
#define RURE_AMD_OK 0
#define RURE_AMD_ERR_ARG (-1)        /* bad argument */
#define RURE_AMD_ERR_HIP (-2)        /* HIP runtime error (no device, launch failure) */
#define RURE_AMD_ERR_DFA (-3)        /* automaton could not be materialized */

/* A batch of haystacks resident in device memory.  Haystack i is
 *   bytes [offsets[i], offsets[i+1])            when offsets != NULL, else
 *   bytes [i*stride, i*stride + length)         (fixed stride).
 * The search in every haystack starts at `start` (with look-behind context,
 * like rure_find's `start`, rure.h:186-192).  Offsets in results are relative
 * to the haystack's first byte.
 * The kernels load whole aligned 16-byte blocks: the buffer must be readable
 * up to the 16-byte-rounded end of its last haystack (device allocations of
 * the HIP runtime and torch are); bytes outside a haystack never influence
 * its results.  `haystack` may have any alignment and `stride` any value:
 * some engines need a 16-byte-aligned base and stride, and a batch that is not
 * so placed takes another kernel with the same results.
 *
 * Outputs.  Record outputs (`rure_match *`, the uint64_t / size_t arrays:
 * out, end, mask, counts, matches, pieces, slots, records, total) need the
 * alignment of their element type, 8 bytes; no call needs more of them.  The
 * byte output `out` of rure_amd_replace_batch must be 16-byte aligned, that
 * of rure_amd_replace_expand_batch may have any alignment.  An output with a
 * `capacity` receives at most that many records (bytes for `out_capacity`):
 * nothing at or past it is written, so the buffer needs no slack, and the
 * counts, offsets and totals reported are exact whatever the capacity is
 * (it never changes the records that are written either).  With capacity 0
 * the output pointer may be NULL. */
typedef struct rure_amd_batch {
  const uint8_t *haystack;
  const uint64_t *offsets;
  size_t stride;
  size_t length;
  size_t count;
  size_t start;
} rure_amd_batch;

/* The three calls below, for a regex whose DFA kernels answer: they only
 * enqueue work on `stream`, never wait for it and read nothing back.  Few
 * long fixed-stride haystacks (256 KiB or more to search) are scanned in
 * parallel chunks.  So are, still without a wait, the long haystacks of an
 * offset batch (documents of their own lengths): the one-lane-per-haystack
 * kernel leaves every haystack with 256 KiB or more to search on a device
 * list, and a chunked scan of the listed haystacks follows on the device (a
 * few launches that return at once when nothing was listed;
 * rure_amd_last_long_units tells).  That holds for a regex whose forward DFA
 * answers the search and cannot quit; RegexSets, regexes with a Unicode word
 * boundary, of the DfaSuffix or anchored-start Literal match types, or
 * anchored at the start keep one lane per haystack of an offset batch
 * (end-anchored ones read only the match from the end).
 * A regex whose forward DFA does not materialise (past the eager state
 * budgets) runs on its on-demand DFA (RURE_AMD_PATH_LAZY_DFA), and these
 * calls are then synchronous: the host builds the rows the text needs between
 * rounds of the kernel and waits for each round.  Batches of at least 64
 * haystacks per compute unit run one lane per haystack; fixed-stride batches
 * of fewer than 128 haystacks per compute unit with 256 KiB or more to search
 * in each (a log buffer, one document; rure_is_match, rure_find and
 * rure_shortest_match on such a host buffer too) are cut into units as
 * above, which step into a state's twin without the unanchored prefix at
 * their cut (rure_amd_last_lazy_long tells).  Past the automaton's memory
 * budget, or after 256 rounds, the Pike VM answers the whole batch.  Other
 * batches of such a regex (offset batches, a regex anchored at the start)
 * run on the Pike VM, a wave per haystack. */
/* Batched rure_find: out[i] = leftmost-first match, or {SIZE_MAX, SIZE_MAX}. */
int rure_amd_find_batch(rure *re, const rure_amd_batch *batch, rure_match *out, void *stream);
/* Batched rure_is_match: out[i] in {0, 1}. */
int rure_amd_is_match_batch(rure *re, const rure_amd_batch *batch, uint8_t *out, void *stream);
/* Batched rure_shortest_match: end[i] or SIZE_MAX. */
int rure_amd_shortest_match_batch(rure *re, const rure_amd_batch *batch, size_t *end, void *stream);
/* Batched rure_set_matches (rure.h:532-533): bit j of mask[i] set iff
 * pattern j matches; sets of at most 64 patterns (RURE_AMD_ERR_ARG above).
 * This call and the next, for a set whose DFA kernels answer: they only
 * enqueue work on `stream`, never wait for it and read nothing back.  Few
 * long fixed-stride haystacks (256 KiB or more to search, fewer than 128 per
 * compute unit) are scanned in parallel chunks whose patterns are ORed into
 * the mask word, the same mask as one lane per haystack gives
 * (rure_amd_last_set_units tells; rure_set_matches and rure_set_is_match on a
 * long host buffer take the same scan).  That holds for a set whose DFA
 * cannot quit and that is not anchored at the start in every pattern; sets
 * with a Unicode word boundary, such anchored sets and every offset batch
 * keep one lane per haystack.  A set whose automaton is past the eager state
 * budget (no DFA; no Unicode word boundary) answers batches that fill the
 * device from its on-demand DFA: rows are built on the host as the text
 * needs them, so such a call synchronises `stream` between rounds, and the
 * first call on new text pays the construction.  Few long fixed-stride
 * haystacks of such a set (the thresholds above; not every pattern anchored
 * at the start) are cut into the same units, which run on that automaton and
 * step into a state's twin without the unanchored prefix at their cut: the
 * call is synchronous likewise, reports RURE_AMD_PATH_LAZY_DFA, and
 * rure_amd_last_set_units gives its units (rure_set_matches and
 * rure_set_is_match on a long host buffer take it too).  Past the automaton's
 * memory budget, or after 256 rounds, the Pike VM answers the whole batch; it
 * also keeps the other batches of such a set (offset batches, sets anchored
 * at the start, a Unicode word boundary).  Each 64-pattern group of a larger
 * set takes these decisions for itself. */
int rure_amd_set_matches_batch(rure_set *re, const rure_amd_batch *batch, uint64_t *mask,
                               void *stream);
/* The same for any number of patterns: `words` >= ceil(rure_set_len / 64)
 * u64 per haystack; bit (j % 64) of mask[i * words + j / 64] set iff pattern j
 * matches haystack i (unused bits and words are zero). */
int rure_amd_set_matches_batch_words(rure_set *re, const rure_amd_batch *batch, uint64_t *mask,
                                     size_t words, void *stream);

/* Batched find_iter (bytes::Regex::find_iter, re_trait.rs:197-221): every
 * successive non-overlapping leftmost-first match of every haystack.
 * counts[i] (device) = number of matches in haystack i; `matches` (device)
 * receives them concatenated in haystack order, at most `capacity` records;
 * *total (device) = the number of matches (rerun with a larger buffer if it
 * exceeds `capacity`).  Long haystacks are scanned in parallel chunks with
 * exact boundary repair: fixed-stride batches by their length, and offset
 * batches (documents of their own lengths) when a haystack has 256 KiB or
 * more to search, each haystack then cut by its own length.  An offset batch
 * synchronises the stream once to read the longest and the total length back
 * (16 bytes), and once more when it is chunked (the number of chunks).  A
 * regex whose forward DFA does not materialise runs, on batches of at least
 * 64 haystacks per compute unit, one lane per haystack on its on-demand DFA
 * (RURE_AMD_PATH_LAZY_DFA): synchronous, the host building the rows the text
 * needs between rounds; past its memory budget the Pike VM answers. */
int rure_amd_find_iter_batch(rure *re, const rure_amd_batch *batch, uint64_t *counts, rure_match *matches,
                             size_t capacity, uint64_t *total, void *stream);

/* Device grep: the matching records (lines) of one raw text buffer.  `text`
 * (device; alignment and readability as rure_amd_batch.haystack) holds
 * `length` bytes with the byte `delim` between records: a record starts at
 * offset 0 and after every `delim`, provided that start is < length, and ends
 * before the next `delim` or at `length` ("a\nb" and "a\nb\n" hold 2 records,
 * "\n" one empty record, an empty text none).  The delimiter is never part of
 * a record and the bytes around a record never influence its answer: record r
 * is selected iff rure_is_match(re, its bytes, its length, 0) is true (false
 * with RURE_AMD_RECORDS_INVERT), for every regex, with `^`, `$` and `\b`
 * evaluated at the record's edges.
 * Outputs (device; the record-output rules above): *nrecords = the records of
 * the text, *total = the selected ones (exact whatever `capacity` is),
 * records[j] = (start, end) in text offsets of the j-th selected record in
 * text order, numbers[j] (may be NULL) = its 0-based record index,
 * *pike_served (may be NULL) = the records the Pike VM answered (where the
 * DFA quit on a Unicode word boundary next to a non-ASCII byte; every record
 * of a regex without an eager DFA).  At most `capacity` entries of records
 * and numbers are written.
 * The text is cut into units of the long scan's size, and a unit's lane
 * answers the records that start in it (kernels/records_device.hpp;
 * rure_amd_last_records tells): a search never crosses a delimiter, so the
 * units need no repair.  The call only enqueues work on `stream`: it never
 * waits and reads nothing back (the first call of a regex on a device uploads
 * its tables, as for every batched call).  Bad arguments (a NULL regex, text
 * with a length, nrecords or total, records with a capacity; an unknown flag):
 * RURE_AMD_ERR_ARG, nothing launched.  rure_amd_last_fwd_path is left alone. */
#define RURE_AMD_RECORDS_INVERT (1u << 0)   /* select the records that do NOT match (grep -v) */
int rure_amd_match_records(rure *re, const uint8_t *text, size_t length, uint8_t delim, uint32_t flags,
                           uint64_t *nrecords, uint64_t *total, rure_match *records, uint64_t *numbers,
                           size_t capacity, uint64_t *pike_served, void *stream);

/* find_iter over one span [lo, hi) of a long haystack (sharded or streamed
 * iteration): the iteration of re_trait.rs:197-221 restricted to
 * the matches that START in [lo, hi) (a match may end past hi; the haystack
 * bytes after hi and before lo are read as context).  entry (device, may be
 * NULL) = the state the previous span's call left in its `exit`; NULL or
 * entry->fresh != 0 starts afresh at lo (no previous match).  *count
 * (device) = matches owned, the first `capacity` written to `matches`
 * (device).  *exit (device) = the state at hi: fresh != 0 when it is
 * equivalent to a fresh start at hi (the next span's speculative result
 * stands), else the next span must be recomputed with it as entry.  A span
 * with hi == length also owns an empty match at the very end.  Concatenating
 * the spans' matches in order equals rure_amd_find_iter_batch over the whole
 * haystack from lo of the first span. */
typedef struct rure_amd_iter_state {
  uint64_t next;        /* where the next search starts */
  uint64_t last_match;  /* end of the previous match, SIZE_MAX if none */
  uint64_t fresh;       /* 1: same as a fresh iteration from the span end */
} rure_amd_iter_state;
int rure_amd_find_iter_span(rure *re, const uint8_t *haystack, size_t length, size_t lo, size_t hi,
                            const rure_amd_iter_state *entry, uint64_t *count, rure_match *matches,
                            size_t capacity, rure_amd_iter_state *exit, void *stream);
/* rure_amd_find_iter_span for n regexes over the same span [lo, hi) of one
 * haystack: regex i's results go to count[i], matches[i] (capacity[i]
 * records) and exit[i], entered with entry[i] (NULL entry array or element:
 * a fresh start) — host arrays of device pointers; each regex's output is
 * exactly its own rure_amd_find_iter_span's.  Regexes that are finite sets of
 * strings of one common length (the regex-dna variants) are scanned together
 * in one pass over the text; otherwise each runs its own pass. */
int rure_amd_find_iter_span_multi(rure *const *res, size_t n, const uint8_t *haystack, size_t length, size_t lo,
                                  size_t hi, const rure_amd_iter_state *const *entry, uint64_t *const *count,
                                  rure_match *const *matches, const size_t *capacity,
                                  rure_amd_iter_state *const *exit, void *stream);

/* Batched replacen with a literal replacement (bytes::Regex::replacen's
 * no-expansion path, re_bytes.rs:489-512): in every haystack the first
 * `limit` matches (0 = all) of the batched find_iter are replaced by
 * rep[0..rep_len) (host memory; `$` is not expanded, as with NoExpand).
 * out_offsets (device, n + 1) = the output layout (exclusive sums of the
 * output lengths); out (device, 16-byte aligned: RURE_AMD_ERR_ARG otherwise,
 * nothing launched) receives the concatenated outputs, at most out_capacity
 * bytes: no byte at or past out_capacity is written; *total (device) = the
 * bytes needed (call again with a larger buffer if it exceeds
 * out_capacity).  Synchronises the stream once
 * to size the match buffer (twice if the first guess was short), except for
 * replace_all (limit 0) of a regex whose matches are single bytes of one
 * class over one fixed-stride haystack, which only enqueues. */
int rure_amd_replace_batch(rure *re, const rure_amd_batch *batch, const uint8_t *rep, size_t rep_len,
                           size_t limit, uint8_t *out, uint64_t *out_offsets, size_t out_capacity,
                           uint64_t *total, void *stream);
/* Batched replacen with a `$`-expanding template (bytes::Regex::replacen's
 * captures path, re_bytes.rs:513-535): as rure_amd_replace_batch (out,
 * out_offsets, out_capacity, total, limit: the same contract, except that
 * out may have any alignment; batch->start must be 0), but rep[0..rep_len)
 * is expanded per match as expand.rs:50-110 does: `$N`, `$name`, `${...}`
 * name a group (the longest run of [0-9A-Za-z_] after the `$`: `$1a` is the
 * group named "1a"), `$$` is a `$`, an unknown group or one that did not
 * participate expands to nothing.
 * diverged (device, n bytes) as for rure_amd_captures_iter_batch, over the
 * first `limit` matches of each haystack only: the output range
 * [out_offsets[i], out_offsets[i + 1]) of a haystack with diverged[i] != 0 is
 * not the reference's and must be recomputed by the caller from its
 * sequential captures (see there).  A template that names no group but 0
 * over a regex without look-around, and any template over a regex without
 * groups, skip the captures pass (diverged stays 0).  Synchronises the stream
 * to size the match buffer and once more before it returns.
 * rure_amd_last_fwd_path: RURE_AMD_PATH_REPLACE_EXPAND. */
int rure_amd_replace_expand_batch(rure *re, const rure_amd_batch *batch, const uint8_t *rep, size_t rep_len,
                                  size_t limit, uint8_t *out, uint64_t *out_offsets, size_t out_capacity,
                                  uint64_t *total, uint8_t *diverged, void *stream);
/* The compiled template of rure_amd_replace_expand_batch (host only, no
 * GPU): pieces[3 * i ..] = (0, offset into lits, length) for a literal piece,
 * (1, group, 0) for a group piece; references that expand to nothing for
 * every match (an unknown name, a number >= the group count) are dropped and
 * adjacent literals merged.  Returns the number of pieces (negative on
 * error) and copies at most `cap` of them and at most `lits_cap` bytes of the
 * literal pool, which is never longer than rep_len (NULL arrays: count
 * only). */
long rure_amd_expand_template_export(rure *re, const uint8_t *rep, size_t rep_len, uint32_t *pieces, size_t cap,
                                     uint8_t *lits, size_t lits_cap);
/* A chain of replace_all calls over one haystack, step i on step i - 1's
 * output: the regex-dna shootout's IUB substitutions
 * (examples/shootout-regex-dna-bytes.rs:44-60, each a bytes::Regex::
 * replace_all with NoExpand, re_bytes.rs:489-512).  Step i replaces every
 * match of res[i] by reps[i][0..rep_lens[i]) (host memory, no `$`
 * expansion).  Every res[i] must be a regex whose matches are single bytes of
 * one class (a literal byte, a byte class: rure_amd_class_one_export) and
 * 1 <= rep_lens[i] <= 64, else RURE_AMD_ERR_ARG.  haystack (device, 16-byte
 * aligned) holds `length` bytes; step i writes out0 if i is even, else out1
 * (device, 16-byte aligned, `capacity` bytes each; readable 16 bytes past
 * capacity); the result is in out0 if n is odd, else out1.  lengths (device,
 * n + 1 uint64) = length, then each step's output length.  An output longer
 * than capacity is cut and no byte at or past capacity is written.  A chain
 * that runs as one byte map (RURE_AMD_PATH_REPLACE_HMAP: every byte's image
 * under the whole chain is at most 64 bytes, the 256 images are at most 4096
 * bytes together and fewer than 256 byte values change) reports every length
 * exactly, cut or not.  Step by step (RURE_AMD_PATH_REPLACE_CLASS) the first
 * step whose output is cut reports its length exactly, and each step after
 * it reads exactly the `capacity` bytes its input buffer holds and reports
 * the length of what it makes of them: a lower bound of its true length and
 * at least capacity (a step never shortens its text), equal to capacity only
 * if it replaced nothing.  So the result is whole if and only if no lengths[i]
 * exceeds capacity; otherwise retry with capacity = the largest lengths[i]
 * (each retry fits at least one more step).  Only enqueues: each step's
 * match count per 4 KiB is counted by the previous step's kernel as it writes
 * the text, and nothing is read back. */
int rure_amd_replace_all_chain(rure *const *res, const uint8_t *const *reps, const size_t *rep_lens, size_t n,
                               const uint8_t *haystack, size_t length, uint8_t *out0, uint8_t *out1,
                               size_t capacity, uint64_t *lengths, void *stream);
/* Batched split / splitn (re_bytes.rs:699-749): the fields between matches
 * as (start, end) records relative to each haystack, concatenated;
 * counts[i] (device) = fields of haystack i; at most `limit` fields per
 * haystack with SplitN's rule (the last is the rest of the haystack);
 * limit = SIZE_MAX for split.  *total (device) = number of fields.
 * Synchronises the stream once (twice if the first guess of the match
 * buffer was short) to size the match buffer. */
int rure_amd_split_batch(rure *re, const rure_amd_batch *batch, size_t limit, uint64_t *counts,
                         rure_match *pieces, size_t capacity, uint64_t *total, void *stream);

/* Match records of a batched find for the multi-GPU gather (the
 * path's only exchange): records[3*j .. 3*j+2] (device) = (base + i, start,
 * end) of the j-th haystack i, in haystack order, whose found[i] (device,
 * the output of rure_amd_find_batch over n haystacks) holds a match; at most
 * `capacity` records are written; *count (device) = the number of matches
 * (may exceed capacity).  No host synchronisation. */
int rure_amd_compact_matches(const rure_match *found, size_t n, uint64_t base, uint64_t *records,
                             size_t capacity, uint64_t *count, void *stream);

/* Batched rure_find_captures: slots[i * 2 * ngroups + 2 * g + {0, 1}]
 * (device, size_t) = start / end of group g in haystack i, SIZE_MAX where the
 * group did not participate or the haystack has no match.  ngroups =
 * rure_amd_captures_len(re). */
int rure_amd_captures_batch(rure *re, const rure_amd_batch *batch, size_t *slots, void *stream);
/* Number of capture groups including group 0 (= rure_captures_len). */
size_t rure_amd_captures_len(rure *re);
/* Batched captures_iter (bytes::Regex::captures_iter, re_trait.rs:243-273):
 * the groups of every successive match of every haystack.  batch->start must
 * be 0 (RURE_AMD_ERR_ARG).  counts[i] (device) and *total (device) as for
 * rure_amd_find_iter_batch; slots (device) receives min(total, capacity) rows
 * of 2 * rure_amd_captures_len(re) entries, row j = the groups of the j-th
 * match in haystack order as (start, end) relative to the haystack, SIZE_MAX
 * where a group did not participate.
 * The rows are computed in parallel over the batched find_iter's match list:
 * the captures Pike VM runs from each match's start over the reference's cut
 * window (exec.rs:555-567).  The reference iterates on the Pike VM's group 0
 * instead; with a look-ahead at the cut (`(a..$)|(a)`) that can differ from
 * the find_iter match, and then the rest of that haystack's sequence differs
 * too.  diverged[i] (device, n bytes) is non-zero for such a haystack: its
 * counts[i] and rows are NOT the reference's.  The caller redoes it alone:
 * loop rure_find_captures(re, hay, len, last_end, caps) with CaptureMatches'
 * rule (re_trait.rs:243-273: after an empty match (s == e) last_end = e + 1
 * and the match is skipped if e == the previous match's end, else last_end =
 * e; not rure_iter_next_captures' rule, which restarts one past the previous
 * search start, regex-capi/src/rure.rs:363-397).  A regex without look-around
 * or without groups never diverges.  (Where the reference's DFA quits, a
 * Unicode \b next to a non-ASCII byte, its captures come from the whole text
 * and the check is made against those.  As in rure_find_captures, the quit
 * is decided with the reference's start-state prefix skip, dfa.rs:700-711: a
 * non-ASCII byte that its DFA jumps over on the way to a prefix literal does
 * not make it quit.)
 * Synchronisation as for
 * rure_amd_find_iter_batch's internal use by rure_amd_replace_batch: once to
 * size the match buffer (twice if the first guess was short).
 * rure_amd_last_fwd_path: RURE_AMD_PATH_CAPTURES_ITER. */
int rure_amd_captures_iter_batch(rure *re, const rure_amd_batch *batch, uint64_t *counts, size_t *slots,
                                 size_t capacity, uint64_t *total, uint8_t *diverged, void *stream);

/* Returns the device scratch this library keeps cached for reuse (blocks
 * of the stream-ordered allocator freed by earlier batched calls; at most
 * max(256 MiB, 2 x the peak of live scratch) are kept) to the allocator.
 * Also done when the last rure / rure_set is freed.  Safe at any time: each
 * block is freed after the kernels that last used it. */
void rure_amd_release_scratch(void);
// Scratch bookkeeping: bytes cached for reuse, bytes held by calls in
// flight, and the number of rure / rure_set handles alive.
void rure_amd_scratch_stats(size_t *cached, size_t *live, long *handles);

/* Diagnostics (host only, no GPU needed). */
typedef struct rure_amd_dfa_info {
  int32_t ok;            /* 1 if the automaton was materialized */
  int32_t states;        /* minimised states incl. dead/quit */
  int32_t raw_states;    /* lazy-DFA states before minimisation */
  int32_t normal;        /* [0, normal) carry no match flag */
  int32_t match_end;     /* [normal, match_end) carry the match flag */
  int32_t dead;
  int32_t quit;          /* -1 if none */
  int32_t hot;           /* states held in the LDS fast table */
  int32_t byte_classes;
  int32_t insts;
  int32_t fast_stride;   /* bytes per dependent LDS lookup in the tile kernel (1, 2, 4) */
  int32_t fast_classes;  /* local byte classes of the multi-byte table (K) */
} rure_amd_dfa_info;
/* which: 0 = forward DFA, 1 = reverse DFA, 2 = find_iter forward DFA,
 * 3 / 4 = the forward / reverse automata past the u16 tables (u32 column
 * form, built when 0 / 1 exceed 65535 states; byte_classes = columns),
 * 5 = the find_iter forward DFA's ASCII shadow (bytes >= 0x80 quit; built
 * where 2 is too big for the all-rows LDS table, else RURE_AMD_ERR_DFA). */
int rure_amd_dfa_info_get(rure *re, int which, rure_amd_dfa_info *info);
int rure_amd_set_dfa_info_get(rure_set *re, rure_amd_dfa_info *info);

/* Export of the compiled byte programs (the reference's Program/Inst
 * contract, prog.rs:18-75, 261-425) as flat 12-byte records, for the CPU
 * oracle and tests.  which: 0 = forward DFA program (with `.*?`),
 * 1 = reverse DFA program, 2 = NFA program (with capture saves).
 * Returns the number of instructions; copies at most `cap` records. */
typedef struct rure_amd_inst {
  uint8_t op, look, lo, hi;
  uint32_t x, y;
} rure_amd_inst;
typedef struct rure_amd_prog_info {
  uint32_t ninsts, start, nmatches, ncaptures;
  uint8_t anchored_start, anchored_end, has_unicode_word_boundary, is_reverse;
  uint8_t byte_classes[256];
} rure_amd_prog_info;
int64_t rure_amd_program_export(rure *re, int which, rure_amd_prog_info *info,
                                rure_amd_inst *insts, size_t cap);
int64_t rure_amd_set_program_export(rure_set *re, int which, rure_amd_prog_info *info,
                                    rure_amd_inst *insts, size_t cap);
/* Export of a materialized DFA: trans = states*256 u32, eof_match = states
 * bytes, start = 128 u32.  which: 0 forward, 1 reverse, 2 the forward DFA
 * of the chunked find_iter (with stripped states, see _strip_export), 5 its
 * ASCII shadow.  1 (and its rure_amd_dfa_info_get) also answers for a regex
 * whose forward DFA did not materialise while the reverse one did. */
int rure_amd_dfa_export(rure *re, int which, uint32_t *trans, uint8_t *eof_match,
                        uint32_t *start);
/* Export of a set's DFA (rure_amd_set_dfa_info_get gives the sizes): trans =
 * states*256 u32, eof_mask / now_mask = states u64 (patterns matched at the
 * end of the text / reported on entering the state), start = 128 u32. */
int rure_amd_set_dfa_export(rure_set *re, uint32_t *trans, uint64_t *eof_mask, uint64_t *now_mask,
                            uint32_t *start);
/* Export of the set DFA built with stripped states, which the chunked scan
 * of long haystacks walks (host only, for tests): sizes in info (may be NULL);
 * trans, eof_mask, now_mask and start as rure_amd_set_dfa_export, strip =
 * states u32 (the state without the `.*?` prefix threads: no match starts
 * from there on), reach = states u64 (the patterns any walk from the state
 * can still report).  NULL arrays are skipped (query the sizes first).
 * RURE_AMD_ERR_DFA where the set has no such automaton: no DFA, a DFA that
 * can quit, more than 65535 states with the stripped ones, more than 64
 * patterns (built per group), or every pattern anchored at the start. */
int rure_amd_set_long_dfa_export(rure_set *re, rure_amd_dfa_info *info, uint32_t *trans, uint64_t *eof_mask,
                                 uint64_t *now_mask, uint32_t *start, uint32_t *strip, uint64_t *reach);
/* A set's on-demand DFA as it stands (host only, for tests): the automaton
 * that answers the batches of a set without an eager DFA, rows built as
 * batches (or rure_amd_set_lazy_build) need them.  Sizes in info (may be
 * NULL): states interned, columns, rows built, rows the kernel holds in LDS,
 * and of the last batched call that took it the rounds it ran and 1 if it
 * gave up (memory budget, too many rounds) and the Pike VM answered.  trans =
 * states x columns entries (next state, | 0x80000000 when entering it
 * reports matches; 0 = dead; 0x7FFFFFFF = the row is not built yet), now /
 * eof_mask = states u64 (patterns reported on entering the state / at the
 * end of the text from it), built = states bytes, start = 128 entries by
 * start-flag index, colmap = 256 bytes (byte -> column).  NULL arrays are
 * skipped (query the sizes first; they grow with every row built).
 * RURE_AMD_ERR_DFA where the set gets no such automaton: a member with a
 * Unicode word boundary, more than 64 patterns (searched per group). */
typedef struct rure_amd_lazy_info {
  uint32_t states, columns, rows_built, hot_rows, rounds, fell_back;
} rure_amd_lazy_info;
int rure_amd_set_lazy_export(rure_set *re, rure_amd_lazy_info *info, uint32_t *trans, uint64_t *now,
                             uint64_t *eof_mask, uint8_t *built, uint32_t *start, uint8_t *colmap);
/* Builds the rows of the n named states of that automaton, then `ahead` more
 * in discovery order: what one round of a batched call does between two
 * launches.  Returns 1, 0 when the memory budget is spent, or an error. */
int rure_amd_set_lazy_build(rure_set *re, const uint32_t *states, size_t n, size_t ahead);
/* The strip links of that automaton and what its states can still report
 * (host only, for tests), one entry per state (`states` of
 * rure_amd_set_lazy_export's info): strip as rure_amd_lazy_strip_export
 * below (a twin may have no thread left and only the patterns its entry
 * reported: a live id whose row is all dead); reach = u64, a superset of the
 * patterns a walk from the state reports (those the program reaches from the
 * state's threads whatever the bytes, plus those its entry reports; 0 for
 * the dead state).  The chunked scan of few long haystacks steps into the
 * twin at a unit's cut and leaves the unit once everything in reach is in the
 * haystack's mask.  NULL arrays are skipped.  RURE_AMD_ERR_DFA where the set
 * has no on-demand automaton or every pattern is anchored at the start. */
int rure_amd_set_lazy_strip_export(rure_set *re, uint32_t *strip, uint64_t *reach);
/* Makes the links of the n named states.  Returns 1, 0 when the memory
 * budget is spent, or an error. */
int rure_amd_set_lazy_strip_build(rure_set *re, const uint32_t *states, size_t n);
/* The same for a regex (host only, for tests): the on-demand forward DFA that
 * answers find, is_match, shortest_match and find_iter over batches of a
 * regex whose forward DFA does not materialise.  info as above, rounds and
 * fell_back being those of the last batched find_iter that took it
 * (fell_back: the other engines answered).  trans, built, start and colmap as
 * above; the match bit marks a state entered one byte after a match ended
 * (the reference's delayed match flag), eof = states bytes (1: the end of the
 * text from the state is a match).  Match starts come from the reverse DFA
 * (rure_amd_dfa_export, which = 1).  RURE_AMD_ERR_DFA where the regex gets no
 * such automaton: a Unicode word boundary, a regex anchored at the end only
 * (searched in reverse), no Pike VM tables, or no reverse DFA. */
int rure_amd_lazy_export(rure *re, rure_amd_lazy_info *info, uint32_t *trans, uint8_t *eof, uint8_t *built,
                         uint32_t *start, uint8_t *colmap);
int rure_amd_lazy_build(rure *re, const uint32_t *states, size_t n, size_t ahead);
/* The strip links of that automaton (host only, for tests): strip = one u32
 * per state (`states` entries of rure_amd_lazy_export's info), the id of the
 * state's twin without the threads of the unanchored prefix (no match bit),
 * 0 = dead, 0x7FFFFFFF = not computed yet.  A chunked scan of long haystacks
 * steps into the twin at a unit's cut, so that only matches started inside
 * the unit go on.  Links are made on demand: a new twin is numbered after
 * every existing state with its row not built, and is its own twin; states,
 * rows and flags that existed stay as they were.  RURE_AMD_ERR_DFA where the
 * regex has no on-demand automaton or is anchored at the start (no prefix). */
int rure_amd_lazy_strip_export(rure *re, uint32_t *strip);
/* Makes the links of the n named states.  Returns 1, 0 when the memory
 * budget is spent, or an error. */
int rure_amd_lazy_strip_build(rure *re, const uint32_t *states, size_t n);
/* Core form of a large set's DFA (used by the set kernel when the set DFA has
 * more than 255 ordinary or match-reporting states): sizes in info; lds =
 * 256-byte class map + (hot + 1) x K u16 entries (next core << 6 | output
 * code), gcore / gout = ncores x K next core (u16) / reported patterns (u64),
 * eof = ncores u64, start = 128 u16.  RURE_AMD_ERR_DFA if not in core form. */
typedef struct rure_amd_core_info {
  uint32_t K, ncores, hot, dead, quit, lds_bytes;
} rure_amd_core_info;
int rure_amd_set_core_export(rure_set *re, rure_amd_core_info *info, uint8_t *lds, uint16_t *gcore,
                             uint64_t *gout, uint64_t *eof, uint16_t *start);
/* strip[s] (states u32) of the find_iter forward DFA: s without the `.*?` prefix. */
int rure_amd_dfa_strip_export(rure *re, uint32_t *strip);
/* The first-byte start rule of the find_iter DFA (host only): returns |F|
 * (1..4, bytes[0..|F|) = F) when every match starts with a byte of F and an
 * anchored run from such a byte cannot die before matching — the chunked
 * find_iter then takes a match's start from the first F byte of its search
 * instead of a reverse scan — else 0; negative on error. */
int rure_amd_first_byte_export(rure *re, uint8_t *bytes);
/* The find_iter lexer table (host only; iter_spec_lex_tile_kernel): u8
 * entries e = 4 row + code; the next entry after byte b is table[76 e + b];
 * code (e & 3): 0 = an ordinary state, 1 = the start state (*s0 = its entry),
 * 2 = its twin, 3 = another restart twin (entering a twin = a match ended at
 * that byte).  Returns the table's size in bytes (0: no lexer table), copies
 * at most `cap`. */
int64_t rure_amd_lex_export(rure *re, uint8_t *table, size_t cap, uint32_t *s0);
/* The same lexer four bytes per step (host only): kLex4Bytes = 5120 bytes,
 * next row at [256 row + c] where c packs four byte classes (2 bits each,
 * byte j at bits 2j; class 3 = no byte), the four bytes' codes (2 bits each)
 * at [2048 + 256 row + c], byte -> class << 2j at [4096 + 256 j + b];
 * *s0 = the start row.  Returns the size (0: the lexer does not fit: more
 * than 8 rows or 3 ASCII byte classes, or no lexer table). */
int64_t rure_amd_lex4_export(rure *re, uint8_t *table, size_t cap, uint32_t *s0);
/* The lexer tables of the find_iter automaton's ASCII shadow (four = 0: the
 * byte table, 1: four bytes per step), as rure_amd_lex_export; 0 if the
 * shadow has none (its first-byte rule may have any number of first bytes:
 * \w+, \S+, \pL+). */
int64_t rure_amd_lex_ascii_export(rure *re, int four, uint8_t *table, size_t cap, uint32_t *s0);
/* 1 if the regex is one byte class repeated (C+, the find_iter run engine:
 * matches = the maximal runs of C bytes) on all bytes (ascii = 0) or on
 * ASCII text (ascii = 1, the ASCII shadow: bytes >= 0x80 quit), with cls[b]
 * bit 0 = b in C, bit 1 = b quits, bit 2 = b (>= 0x80) is read as UTF-8
 * (a Unicode class: rure_amd_run_cp_export); 0 if not. */
int rure_amd_run_class_export(rure *re, int ascii, uint8_t *cls);
/* The run engine's code point bitmap of a Unicode class C+ (\w+, \pL+,
 * \S+ in Unicode mode: bit c of bits[c / 32]), at most n words copied;
 * returns its size in words (0x110000 / 32) or 0 if the engine reads no
 * UTF-8 for this regex. */
int rure_amd_run_cp_export(rure *re, uint32_t *bits, size_t n);
/* 1 if every match of the regex is exactly one byte of a class (cls[b] = 1
 * for its bytes): its replace_all over one haystack then runs without a
 * match list (rure_amd_replace_batch, RURE_AMD_PATH_REPLACE_CLASS); 0 if
 * not. */
int rure_amd_class_one_export(rure *re, uint8_t *cls);
/* The byte map rure_amd_replace_all_chain composes for a chain (host only, no
 * GPU; res, reps, rep_lens, n as there, n >= 1): the chain sends each byte x
 * to a string F(x).  Returns 1 if the chain is mappable (runs as
 * RURE_AMD_PATH_REPLACE_HMAP): every F(x) is at most 64 bytes, their lengths
 * sum to at most 4096, and fewer than 256 byte values change; 0 if it runs
 * step by step; RURE_AMD_ERR_ARG as that call.  *nact = the byte values with
 * F(x) != x and *pool_len = the sum of the |F(x)| (both 0 when an image is
 * longer than 64 bytes).  Only when it returns 1: flen[256] = |F(x)|,
 * soff[256] = the offset of F(x) in the pool, aidx[256] = the index of x among
 * the changed bytes in byte order, 0xFF if F(x) = x; pool = the strings (at
 * most pool_cap bytes copied); dlen[i * 256 + x] = |F_i(x)| - 1, the image of
 * x after steps 0..i.  Any array may be NULL. */
int rure_amd_chain_map_export(rure *const *res, const uint8_t *const *reps, const size_t *rep_lens, size_t n,
                              uint8_t *flen, uint16_t *soff, uint8_t *aidx, uint32_t *nact, uint8_t *pool,
                              size_t pool_cap, size_t *pool_len, uint32_t *dlen);

/* Export of the Pike VM closure tables the NFA kernel runs (host only):
 * leaves = 3 u32 per leaf (kind | lo << 8 | hi << 16, closure, slot),
 * cl_off = closures + 1 u32, entries = 2 u32 per entry (leaf,
 * cond | (1 + previous same-leaf entry) << 8).  Pass NULL arrays to query
 * the sizes.  Returns RURE_AMD_OK or an error. */
typedef struct rure_amd_nfa_info {
  uint32_t leaves, closures, entries, root, nmatch, anchored, looks, unicode_wb;
} rure_amd_nfa_info;
int rure_amd_nfa_export(rure *re, rure_amd_nfa_info *info, uint32_t *leaves, uint32_t *cl_off,
                        uint32_t *entries);
int rure_amd_set_nfa_export(rure_set *re, rure_amd_nfa_info *info, uint32_t *leaves, uint32_t *cl_off,
                            uint32_t *entries);
/* Capture slots each closure entry sets (the Saves on its path): save_off =
 * entries + 1 u32 CSR offsets into save_slot (u16).  *n_slots receives the
 * length of save_slot; NULL arrays query it. */
int rure_amd_nfa_saves_export(rure *re, uint32_t *save_off, uint16_t *save_slot, size_t *n_slots);
/* The regex as a finite string set, as the literal find_iter engine uses it
 * (the GPU counterpart of the reference's complete-prefix Literal engine,
 * exec.rs:1148-1166): returns the number of literals (0 = not a string set:
 * the DFA kernels iterate), in leftmost-first priority order; lens[i] and
 * bytes[32 * i ...] receive the first `cap` of them (NULL arrays: count only).
 * Host only. */
int64_t rure_amd_literals_export(rure *re, uint32_t *lens, uint8_t *bytes, size_t cap);
/* Diagnostics (host only): the Shift-And image of the find_iter string set
 * (iter_spec_sa_kernel) — 256 u64 byte masks, the first / last bit of every
 * class sequence and the string length.  Returns the state width in bits, 0
 * when the regex is not a set of equal-length strings that fits 64 bits. */
int64_t rure_amd_shiftand_export(rure *re, uint64_t *mask, uint64_t *init, uint64_t *fin, uint32_t *len);
/* Literal sets and the reference's engine choice (host only).
 * rure_amd_literals_syntax: regex-syntax's Expr::prefixes (which 0) /
 * suffixes (which 1) of a pattern (regex-syntax/src/literals.rs:285-304)
 * with the given limits (the reference's defaults: 250 bytes, 10 class
 * members), serialized as records {u8 cut, u32 length, bytes}; returns the
 * serialized size (copied only when cap suffices).  rure_amd_literals_op on
 * such records: 0 unambiguous_prefixes, 1 longest_common_prefix (raw bytes),
 * 2 longest_common_suffix (raw bytes), 3 unambiguous_suffixes.
 * rure_amd_exec_literals_export: the unambiguous prefix (which 0) / suffix
 * (which 1) set the reference's Exec builds for this regex (exec.rs:308-321).
 * rure_amd_match_info_get: its MatchType (exec.rs:1130-1210; codes:
 * 0 Literal(Unanchored), 1 Literal(AnchoredStart), 2 Literal(AnchoredEnd),
 * 3 Dfa, 4 DfaAnchoredReverse, 5 DfaSuffix, 6 Nfa, 7 Nothing), the two
 * LiteralSearchers' matcher kind (0 Empty, 1 Bytes, 2 one literal,
 * 3 several), len(), complete(), lcp / lcs character lengths and the lcs. */
typedef struct rure_amd_match_info {
  int32_t match_type;
  int32_t prefix_matcher, suffix_matcher;
  uint32_t prefix_len, suffix_len;
  uint8_t prefix_complete, suffix_complete, pad[2];
  uint32_t lcp_chars, lcs_chars;
  uint32_t lcs_bytes;
  uint8_t lcs[256];
} rure_amd_match_info;
int64_t rure_amd_literals_syntax(const uint8_t *pattern, size_t length, uint32_t flags, int which,
                                 size_t limit_size, size_t limit_class, uint8_t *out, size_t cap);
int64_t rure_amd_literals_op(int op, const uint8_t *in, size_t in_len, uint8_t *out, size_t cap);
int64_t rure_amd_exec_literals_export(rure *re, int which, uint8_t *out, size_t cap);
int rure_amd_match_info_get(rure *re, rure_amd_match_info *info);
/* 1 if batched searches of this regex run the DFA kernels, 0 if only the
 * Pike VM kernel (automaton too large), negative on error. */
int rure_amd_uses_dfa(rure *re);
/* 1 if the regex is of the DfaSuffix match type and no match of it holds its
 * longest common suffix anywhere but at its end, so that its find_iter is
 * the forward DFA's (host only; an offset batch with a long haystack then
 * takes the chunked find_iter instead of one wavefront per haystack); 0 if
 * not, negative on error. */
int rure_amd_suffix_forward(rure *re);
int rure_amd_set_uses_dfa(rure_set *re);
/* Diagnostics (host only): the engine that answered a batched call.  The
 * values are frozen (recorded profiles hold them); a new engine takes a new
 * value. */
typedef enum rure_amd_path {
  RURE_AMD_PATH_NONE = -1,              /* before the first launch */
  RURE_AMD_PATH_LANE_STREAM = 0,        /* the per-lane streaming kernel */
  RURE_AMD_PATH_TILE1 = 1,              /* the coalesced-tile kernel, 1 byte per dependent table lookup */
  RURE_AMD_PATH_TILE2 = 2,              /* the coalesced-tile kernel, 2 bytes per lookup */
  RURE_AMD_PATH_TILE4 = 4,              /* the coalesced-tile kernel, 4 bytes per lookup */
  RURE_AMD_PATH_ANCHORED_REVERSE = -2,  /* the reverse DFA from the end (DfaAnchoredReverse) */
  RURE_AMD_PATH_LITERAL = -3,           /* the literal engine (MatchType::Literal) */
  RURE_AMD_PATH_LONG_SCAN = -4,         /* the chunked cut-bounded scan (long haystacks split into units) */
  RURE_AMD_PATH_LANE_SEARCH = -5,       /* the lane search of the Literal / DfaSuffix match types */
  RURE_AMD_PATH_BIG_DFA = -6,           /* the big (u32) DFA */
  RURE_AMD_PATH_LINES = -8,             /* the ragged line kernel */
  RURE_AMD_PATH_SUFFIX_LONG = -9,       /* the chunked DfaSuffix scan */
  RURE_AMD_PATH_LAZY_DFA = -10,         /* the on-demand DFA (a regex's searches or find_iter, or a set's) */
  RURE_AMD_PATH_SUFFIX_ITER = -11,      /* the DfaSuffix find_iter */
  RURE_AMD_PATH_ITER_LOOKS = -12,       /* the chunked find_iter of a look-around regex answered */
  RURE_AMD_PATH_ITER_LOOKS_QUIT = -13,  /* it quit: one haystack per wavefront answers */
  RURE_AMD_PATH_ITER_SHADOW = -14,      /* the find_iter ASCII shadow answered, its quit read back */
  RURE_AMD_PATH_ITER_SHADOW_QUIT = -15, /* it quit, and the full automaton re-ran the batch, chunked */
  RURE_AMD_PATH_PIKE_ONLY = -16,        /* the Pike VM alone (no DFA) */
  RURE_AMD_PATH_SET_CORE_OFFSETS = -17, /* the core-form set kernel over an offset batch */
  RURE_AMD_PATH_ITER_RUNS = -19,        /* the find_iter run engine of a C+ regex, its class over all bytes */
  RURE_AMD_PATH_ITER_RUNS_ASCII = -20,  /* the run engine with the ASCII shadow's class */
  RURE_AMD_PATH_ITER_CHUNKED = -21,     /* the chunked find_iter of the full automaton (no look-around) */
  RURE_AMD_PATH_ITER_WAVE = -22,        /* find_iter with one haystack per wavefront */
  RURE_AMD_PATH_REPLACE_CLASS = -23,    /* replace_all of a one-byte-class regex without a match list; a chain step by step */
  RURE_AMD_PATH_REPLACE_HMAP = -24,     /* a replace_all chain as one composed byte map */
  RURE_AMD_PATH_ITER_SHADOW_GATED = -25, /* shadow and full automaton both enqueued, the quit kept on the device */
  RURE_AMD_PATH_ITER_WAVE_SERVED = -27, /* chunked find_iter whose quitting units are served by waves */
  RURE_AMD_PATH_CAPTURES_ITER = -28,    /* the batched captures_iter (a wave per match) */
  RURE_AMD_PATH_REPLACE_EXPAND = -29    /* the batched replacen with a `$` template */
} rure_amd_path;
/* The rure_amd_path of the last batched launch of this process (one value
 * for the whole process, not per thread or stream). */
int rure_amd_last_fwd_path(void);
/* Diagnostics (host only, one value for the whole process likewise): the
 * number of units (chunks) the last chunked find_iter launch cut its batch
 * into; *haystacks (may be NULL) = that batch's haystack count.  One unit per
 * haystack means nothing was cut.  0 and *haystacks = 0 before the first such
 * launch. */
uint64_t rure_amd_last_iter_units(uint64_t *haystacks);
/* Diagnostics (host only, one value for the whole process likewise): the
 * units the last find / is_match / shortest_match call over an offset batch
 * cut its deferred long haystacks into; *haystacks (may be NULL) = how many
 * haystacks it deferred to the chunked scan, *chunk (may be NULL) = the unit
 * size in bytes.  All 0 before the first such call and when it deferred
 * nothing.  The figures are made on the device (a kernel of the batched call
 * writes them into a pinned host record): this call waits for the work that
 * the batched call enqueued on its stream. */
uint64_t rure_amd_last_long_units(uint64_t *haystacks, uint64_t *chunk);
/* Diagnostics (host only, one value for the whole process likewise): the
 * units the last chunked RegexSet call cut its batch into, on the set's DFA
 * or on its on-demand DFA (also where that one gave up and the Pike VM
 * answered); *haystacks (may be NULL) = that batch's haystack count, *chunk
 * (may be NULL) = the unit size in bytes.  All 0 before the first such launch and after a set call (a
 * 64-pattern group's, for larger sets) that did not chunk.  The host knows
 * the geometry: this call waits for nothing. */
uint64_t rure_amd_last_set_units(uint64_t *haystacks, uint64_t *chunk);
/* Diagnostics (host only, one value for the whole process likewise): the
 * units the last rure_amd_match_records call cut its text into; *chunk (may
 * be NULL) = the unit size in bytes.  0, 0 before the first such call and
 * after one over an empty text.  The host knows both: this call waits for
 * nothing. */
uint64_t rure_amd_last_records(uint64_t *chunk);
/* The ownership rule of that call (host only; kernels/records_device.hpp, the
 * code the device runs) over a host text: for each unit u of `chunk` bytes
 * (>= 1), first[u] = the first record start it owns (SIZE_MAX: none) and
 * count[u] = how many records it owns, for the units below `cap` (first and
 * count may be NULL).  Returns the number of units, ceil(length / chunk);
 * RURE_AMD_ERR_ARG for a NULL text with a length or a chunk of 0. */
int64_t rure_amd_records_units(const uint8_t *text, size_t length, uint8_t delim, size_t chunk,
                               uint64_t *first, uint64_t *count, size_t cap);
/* Diagnostics (host only, one value for the whole process likewise): the
 * units the last chunked find / is_match / shortest_match (or captures
 * bounds) call on a regex's on-demand DFA cut its batch into; *haystacks =
 * that batch's haystack count, *chunk = the unit size in bytes, *rounds = the
 * kernel rounds it ran, *fell_back = 1 when the Pike VM answered instead
 * (any may be NULL).  All 0 before the first such call and after a regex
 * search that did not take that path.  The host knows the figures: this call
 * waits for nothing. */
uint64_t rure_amd_last_lazy_long(uint64_t *haystacks, uint64_t *chunk, uint32_t *rounds, uint32_t *fell_back);
/* Diagnostics (host only, one value for the whole process likewise): the
 * last find_iter (or split, replace, captures_iter) call that was cut into
 * units on a regex's on-demand DFA: few long fixed-stride haystacks of a
 * regex past the eager state budgets and without look-around.  units and
 * haystacks of the batch, chunk = the unit size in bytes, rounds = the kernel
 * rounds summed over its passes, repaired = the units iterated again from
 * another entry than their own start, resume_passes = the extra passes the
 * resolve step asked for, fell_back = 1 when the call gave the batch up and
 * another engine answered.  All 0 before the first such call and after a
 * find_iter that took another path.  Waits for nothing. */
typedef struct rure_amd_lazy_iter_long {
  uint64_t units, haystacks, chunk;
  uint32_t rounds, resume_passes;
  uint64_t repaired;
  uint32_t fell_back, pad;
} rure_amd_lazy_iter_long;
void rure_amd_last_lazy_iter_long(rure_amd_lazy_iter_long *info);
/* The resolve rule of that chunked find_iter (host only;
 * kernels/lazy_iter_long_device.hpp, the code the device runs), over unit
 * records the caller supplies.  An iteration state is (p, lm): the next
 * search start and the end of the last match (~0: none); p = ~0 is the stop
 * state.  A record: the entry state, the exit state, the matches owned, and
 * flags (bit 0: the record exists, bit 1: its exit is clean, bits 4..: where
 * a final record came from: 0 the speculation, 1 the fix record, 2 skipped,
 * 3 a run the walker asked for).  haystacks * units_per records each in spec
 * (every unit from its own start), fix (from the predecessor's exit, where
 * that was not clean) and fin (out).  first != 0: the parallel pass fills
 * fin, changed (a byte per unit) and zeroes walk (an entry per haystack)
 * before the walkers run; first = 0: the walkers resume, after the caller
 * stored the runs asked for into fin (flags: 1 | clean | 3 << 4).  Returns
 * the number of units the walkers need run (todo, at most one per haystack,
 * in haystack order: unit index in the batch and entry state), 0 when fin is
 * final; RURE_AMD_ERR_ARG on a null array. */
typedef struct rure_amd_lil_rec {
  uint64_t entry_p, entry_lm, exit_p, exit_lm;
  uint32_t count, flags;
} rure_amd_lil_rec;
typedef struct rure_amd_lil_walk {
  uint64_t next, exit_p, exit_lm;
  uint32_t active, clean;
} rure_amd_lil_walk;
typedef struct rure_amd_lil_todo {
  uint64_t unit, p, lm;
} rure_amd_lil_todo;
int64_t rure_amd_lazy_iter_resolve(uint64_t haystacks, uint64_t units_per, uint64_t start, uint64_t chunk, int first,
                                   const rure_amd_lil_rec *spec, const rure_amd_lil_rec *fix, rure_amd_lil_rec *fin,
                                   uint8_t *changed, rure_amd_lil_walk *walk, rure_amd_lil_todo *todo);
/* The tile kernel's skip rule (host only; kernels/tile_skip_device.hpp): a
 * regex that is, over ASCII text, one fixed sequence of m byte classes, and
 * whose packed forward DFA the host proved to leave its hot rows only at a
 * window of that sequence, lets a wave leave out the walk of a 128-byte tile
 * in which no lane has a byte >= 0x80 or a window ending.  anchor_a <=
 * anchor_b: the positions whose byte ranges find the windows (equal: one
 * anchor; -1: not eligible).  used: the kernel applies the rule, which it
 * does only where the byte frequency table expects less than one anchor
 * candidate per wave and tile (verifying more costs more than the walk). */
typedef struct rure_amd_tile_skip {
  int32_t eligible;
  int32_t m;
  int32_t anchor_a, anchor_b;
  int32_t used;
} rure_amd_tile_skip;
int rure_amd_tile_skip_info(rure *re, rure_amd_tile_skip *info);
/* One haystack walked the way a lane of the tile kernel walks it under the
 * skip rule (a wave of one lane, find), and plainly (host only): the forward
 * DFA state after each whole 128-byte tile both ways (len / 128 entries each)
 * and whether the lane found the tile dirty.  Returns the number of tiles;
 * RURE_AMD_ERR_ARG for a regex that is not eligible. */
int64_t rure_amd_tile_skip_simulate(rure *re, const uint8_t *hay, size_t len, uint32_t *states_skip,
                                    uint32_t *states_exact, uint8_t *dirty);
/* Debug-only overrides of the engine dispatch and launch geometry
 * (regex_amd/csrc/host/knobs.hpp lists them): replaces the whole override
 * table, read once per process from RURE_AMD_DEBUG, by spec
 * ("name=value,..."; NULL or "" clears it).  For tests and A/B tools; no
 * production path needs an override.  Returns RURE_AMD_ERR_ARG (table
 * unchanged) on an unknown name or a malformed value.  Tables a regex has
 * already built for a device keep the overrides they were built under. */
int rure_amd_debug_set(const char *spec);
/* Diagnostics (bench): rure_amd_kernel_timer(1) resets and starts timing the
 * speculative kernel of every find_iter pass (the dominant kernel of a pass:
 * iter_spec_*; HIP events on the launch stream), (0) stops;
 * rure_amd_kernel_timer_read waits for the timed launches and returns their
 * average duration in ms (*launches = how many; -1 on a HIP error). */
int rure_amd_kernel_timer(int on);
double rure_amd_kernel_timer_read(uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* RURE_AMD_H */
