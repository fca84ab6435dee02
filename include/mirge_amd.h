/*
 * mirge_amd.h -- C-ABI of the MI355X-native short-read annotation engine.
 *
 * This is the drop-in boundary for ONE path of miRge2.0's annotate mode: the
 * sequential bowtie cascade over collapsed unique reads plus the per-read
 * count tally.  The reference has no function ABI at this boundary -- it
 * shells out to the external `bowtie` / `bowtie-inspect` binaries and parses
 * their text output.  Each entry point below names the reference call site
 * (file:line under src/mirge/) whose work it replaces:
 *
 *   RAP = utils/runAnnotationPipeline.py   SUM = utils/summarize.py
 *   MAIN = __main__.py
 *
 * Conventions
 *   - plain C, no torch / C++ types in any signature;
 *   - every function returns 0 on success, <0 on error; the message is kept
 *     per-thread and read with mrg_last_error() (the Python host turns a
 *     non-zero status into the reference's "Alignment to library %s exited
 *     with none-zero status." + exit(1), RAP:661-663);
 *   - the caller allocates and owns every bulk buffer; the library owns only
 *     the opaque handles (mrg_index, mrg_ctx) and frees them in *_free/_destroy;
 *   - pointers named d_* are DEVICE (HBM) pointers, everything else is host
 *     memory; `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - there is no CPU fallback: every compute entry point fails with
 *     MRG_ERR_NO_DEVICE when no gfx950 device is usable.
 *
 * Read encoding: 2 bits per base, A=0 C=1 G=2 T=3, base i of a read in bits
 * [2i,2i+1] of word (i/32), words stored structure-of-arrays:
 * d_reads[w * n + r] is word w of read r (coalesced when a wave takes 64
 * consecutive reads).  Reads containing N carry an optional mask of the same
 * shape (bit 2i of the d_nmask word set = base i is N, its 2-bit code is then
 * 0; N always counts as a mismatch, as in bowtie 1).
 */
#ifndef MIRGE_AMD_H
#define MIRGE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MRG_OK 0
#define MRG_ERR_ARG (-1)
#define MRG_ERR_IO (-2)
#define MRG_ERR_NO_DEVICE (-3)
#define MRG_ERR_HIP (-4)
#define MRG_ERR_NOMEM (-5)
#define MRG_ERR_FORMAT (-6)

#define MRG_MAX_PASSES 16
#define MRG_MAX_WORDS 8 /* reads up to 255 nt (the length is one byte) */

typedef struct mrg_index mrg_index; /* host-side FM index of one library */
typedef struct mrg_ctx mrg_ctx;     /* one per GPU: HBM copies + workspaces */

int mrg_version(void);
const char *mrg_last_error(void);

/* ------------------------------------------------------------------ *
 * Index: replaces `bowtie-build` (offline) and `bowtie-inspect`
 * (SUM:6, RAP:610-611, RAP:630).  Host-only C++; no GPU needed.
 * ------------------------------------------------------------------ */

/* Build from in-memory entries (names[i], seqs[i] are NUL-terminated; seqs may
 * contain N/n, which splits an entry into un-alignable gaps as bowtie does). */
int mrg_index_build(const char *const *names, const char *const *seqs,
                    uint32_t n_ref, mrg_index **out);
/* Build from a FASTA file (multi-line records allowed; name = header up to
 * first whitespace, as bowtie-build records it). */
int mrg_index_build_fasta(const char *fasta_path, mrg_index **out);
/* The same two, with the suffix array, the BWT blocks and the suffix-array rows computed on GPU `device` (prefix
 * doubling over the library's radix sort; csrc/sa_build.hip).  The result is an ordinary host index, every array
 * identical to the host builder's.  MRG_ERR_NO_DEVICE without a usable gfx950 device (checked before anything is
 * read); MRG_ERR_NOMEM, with the bytes needed in the message, when the working set (about 33 bytes per base) does
 * not fit the free device memory.  There is no fallback to the host builder.  The calling thread's current HIP
 * device is the same after the call as before it. */
int mrg_index_build_device(int device, const char *const *names, const char *const *seqs,
                           uint32_t n_ref, mrg_index **out);
int mrg_index_build_fasta_device(int device, const char *fasta_path, mrg_index **out);
/* Sort rounds (the first-round sort of 30 bases included) of the device build this THREAD called last: never more
 * than ceil(log2((n_bases + 1) / 30)) + 1, and 0 when that call failed or the text was empty.  Every device build
 * resets it on entry, so a value is never left over from an earlier call. */
uint32_t mrg_index_build_device_rounds(void);
/* Build from the reference's own library file: `<prefix>.1.ebwt` (bowtie 1), the only form in which
 * miRge.Libs ships its libraries (MAIN:262-281).  Entry names and sequences are recovered from
 * the BWT as `bowtie-inspect` does (SUM:6, RAP:610-611,630, W2C:649) and indexed like a FASTA
 * file.  EXPERIMENTAL: the format is restated from bowtie 1.1.x without a bowtie-built sample at
 * hand and validated by round trip with an independent test writer only (tests/helpers/); the
 * reader therefore re-derives every redundant field of the file (side occurrence counts, fchr,
 * ftab order, fragment table) from the BWT it decoded and fails with MRG_ERR_IO on any mismatch. */
int mrg_index_build_ebwt(const char *prefix, mrg_index **out);
int mrg_index_save(const mrg_index *ix, const char *path);
int mrg_index_load(const char *path, mrg_index **out);
void mrg_index_free(mrg_index *ix);

typedef struct mrg_index_info {
  uint32_t n_ref;      /* library entries (histogram bins for the miRNA lib) */
  uint32_t n_seg;      /* N-free segments */
  uint32_t n_bases;    /* concatenated text length (without sentinel) */
  uint32_t n_blocks;   /* 16-byte occ blocks (32 BWT symbols each) */
  uint32_t n_super;    /* superblocks (65536 BWT symbols each), 4 words each */
  uint32_t primary;    /* BWT row holding the sentinel */
  uint32_t text_words; /* 2-bit packed text, 32-bit words incl. padding */
  uint8_t ftab_ks[4];  /* k of each k-mer jump table, largest first, 0 = absent: {big 12..14 or 0,
                        * main 8..11, 6, 4} */
  uint32_t C[4];       /* first BWT row of each symbol */
  uint64_t bytes_fm;   /* n_blocks * 16 + n_super * 16 */
  uint64_t bytes_sa;   /* (n_bases + 1) * 8 */
} mrg_index_info;

int mrg_index_get_info(const mrg_index *ix, mrg_index_info *info);
/* `bowtie-inspect -n`: name of entry i, valid for the index lifetime (SUM:6-9). */
int mrg_index_name(const mrg_index *ix, uint32_t i, const char **name);
/* `bowtie-inspect`: sequence of entry i (N restored) into buf (cap bytes incl. NUL). */
int mrg_index_seq(const mrg_index *ix, uint32_t i, char *buf, uint32_t cap,
                  uint32_t *len);

/* Raw views for tests and the oracle's CPU port (read-only, index lifetime). */
typedef struct mrg_index_view {
  const uint32_t *blocks;    /* n_blocks * 4 words: cnt[4] as uint16, lo, hi */
  const uint32_t *super;     /* n_super * 4 words: C[c] + count before the superblock */
  const uint32_t *text;      /* text_words */
  const uint64_t *sa;        /* n_bases + 1 rows: pos | before<<32 | after<<40 | seg<<48 */
  const uint32_t *ftab;      /* jump tables of ftab_ks back to back, 4^k + 1 words each: the rows
                              * starting with k-mer c (numbered lexicographically, first base
                              * most significant) are [T[c], T[c+1]) */
  const uint32_t *seg_start; /* n_seg + 1 */
  const uint32_t *seg_ref;   /* n_seg */
  const uint32_t *seg_off;   /* n_seg */
  const uint32_t *chunk_seg; /* (n_bases >> 5) + 2 */
  const uint32_t *ctx;       /* NULL, or for libraries of >= 2^20 bases one word per suffix-array
                              * row: bits 0-15 the 8 bases left of the row's position (the nearest
                              * in the top two), bits 16-31 the bases 8..15 after it */
  const uint32_t *kbits;     /* NULL, or for libraries of at most 190 000 bases the presence bitmap of
                              * their 9-mers: 4^9 bits, bit c = 9-mer with code c (first base in
                              * the low two bits) occurs */
} mrg_index_view;
int mrg_index_get_view(const mrg_index *ix, mrg_index_view *view);

/* Exact-match dictionary of a library of at most 2^22 bases (read-only view, index lifetime; built on
 * the first request for a key length and uploaded by mrg_ctx_add_library): what answers the `-n 0` /
 * `-v 0` runs (RAP:577, :598, :688) for one-word reads in ONE 16-byte load.  Open addressing, 2^log2_slots
 * slots of two uint64:
 *   slots[2 i]      the 32 text bases from the slot's text position (2 bits per base, first base lowest)
 *   slots[2 i + 1]  low 32 bits: library entry; high 32 bits: bits 0-5 bases to the end of the
 *                   position's N-free segment (clamped to 63), bits 6-9 chain = how far behind its
 *                   home slot a key homed at slot i may sit (15 = overflowed: ask the FM index),
 *                   bit 10 occupied, bits 11-31 offset of the position in its entry
 * home slot of a key = ((uint32) of its first key_bases bases * 0x9E3779B1) >> (32 - log2_slots);
 * keys are inserted in text order, a position that an earlier one makes unreachable is left out, so
 * the first match along home, home + 1, ... home + chain is the lowest (entry, offset). */
typedef struct mrg_dict_view {
  const uint64_t *slots;
  uint32_t log2_slots;
  uint32_t key_bases;
  uint64_t n_keys;     /* positions stored */
  uint64_t n_overflow; /* HOME SLOTS whose chain overflowed (a count of homes: every further position of such a home is left to the FM index) */
} mrg_dict_view;
int mrg_index_get_dict(const mrg_index *ix, uint32_t key_bases, mrg_dict_view *view);

/* ------------------------------------------------------------------ *
 * Context: one per GPU.  Replaces the per-pass process spawn + .ebwt
 * load of RAP:643 / RAP:689 with libraries resident in HBM.
 * ------------------------------------------------------------------ */
int mrg_ctx_create(int device, mrg_ctx **out);
void mrg_ctx_destroy(mrg_ctx *ctx);
/* Upload one library; *lib_id is what mrg_pass_cfg.lib refers to. */
int mrg_ctx_add_library(mrg_ctx *ctx, const mrg_index *ix, int32_t *lib_id);
/* Tunables (all have defaults): "lds_budget" = most bytes of LDS a match
 * workgroup may spend on a staged library (occ blocks + packed text; 0 serves
 * every library from HBM/L2); "wstop" = interval width at which a seed search
 * stops narrowing and hands the occurrences to verification (0 = narrow to the
 * end of the piece; default 8); "ftab" = 1/0 use the k-mer jump table for the first k steps
 * of a seed search; "wide_rows" = seed intervals wider than this many rows are
 * verified cooperatively by the whole wave (default 64); "hint_min_len" / "hint_max_len" = the
 * caller's promise that every read of the NEXT mrg_cascade_run has a length in that range (defaults
 * 0 / 255 = unknown; reset to the defaults by every run): a pass whose length window excludes the
 * whole range is not launched, and a one-word batch that may hold reads under "split_min_len" is split
 * (below); the hints decide no result: every kernel reads d_lens; "kmer_filter" = 1/0 stage a small
 * library's 9-mer presence bitmap in LDS and skip the jump-table load of a seed piece whose
 * last 9 bases do not occur in the library (default 1); "ctx_wide_rows" = the same
 * threshold for libraries of >= 2^20 bases, whose cooperative path drops most rows by their
 * stored text context (default 32); "fuse" = 0 one launch per pass, 1 (default)
 * consecutive passes with at most one seed mismatch after the first launched pass share one
 * fused launch per run of small (bitmap-filtered) / large libraries, 2 = one group regardless of
 * library size, 3 = only the small-library runs are fused; "pair_seeds" = 1 (default) / 0: a pass
 * with two seed mismatches on a library of at most 4 Mbp searches reads of at least 15 nt (after
 * -5 / -3) through the six pairs of four anchors instead of three pigeonhole pieces (the pair tables
 * are built by mrg_ctx_add_library: set 0 BEFORE adding libraries to save their memory, or at any
 * time to run the piece search); "split_strata" = 1 (default) / 0: such a pass, when it does run the
 * piece search, is launched as strata 1-2 and stratum 3 separately; "stratum_rows" = 0 (default) /
 * 1 / 2: that piece search in stratum_kernel (rows compacted over the wave) for the last stratum /
 * every strata launch; "pair_big" = 5 (default) / 0 / 4..7: anchor length A of the pair tables of
 * libraries of >= 2^20 bases -- a one-mismatch pass inside a fused launch searches reads whose seed
 * region is 3A .. 4A - 1 bases through three anchor pairs instead of two short pigeonhole pieces
 * (tables built on the device the first time such reads are met; mrg_pass_stats.pair_anchor reports
 * A); "dict" = 1 (default) / 0: batches of one-word reads without an N mask run the dictionary
 * kernels for the passes that can (a pass without seed mismatches on a library of at most 4 Mbp: one
 * load of its exact-match dictionary per read, built by mrg_ctx_add_library while the option is 1);
 * "dict_key" = 16 (default) / 8..16: key length of those dictionaries (set BEFORE adding libraries;
 * reads shorter than the key take the FM index); "seed_units" = 1 (default) / 0: in such batches the runs
 * of passes with at most one seed mismatch after the first launch go through seed_kernel (libraries of at
 * most 4 Mbp searched with one policy as ONE index of their concatenation, built when a cascade first
 * plans it); "split_mixed" = 1 (default) / 0 and "split_min_len" = 16 (default: the reference's own length floor, trim_file.py:33; round 3: 20) / 0..32: a batch with more
 * than one word per read, an N mask, or (by the length hint) reads under split_min_len nt -- unless the hint
 * puts every read on one side: all longer than 32 nt, or all under split_min_len -- is split on the
 * device into the reads of split_min_len .. 32 nt without N, which run the cascade through the dictionary
 * kernels as the one-word batch they are, and the rest, which runs it through the FM kernels first -- two
 * cascades over disjoint lists adding to the same counters (mrg_pass_stats then names the kernels and times
 * of the second one, ms_rest the times of the first, n_launches counts both);
 * (round 4) "dict_max_bases" = 1 << 22 (default): libraries up to this size get an exact-match dictionary;
 * raise it (e.g. 1 << 30) BEFORE adding a large library that a pass searches without seed mismatch (mRNA
 * `-n 0`, runAnnotationPipeline.py:584/598) -- 16 B x 2..4 slots per base of HBM, skipped when less than that
 * + 8 GB is free -- and that pass becomes one 16-byte gather per read; "seed_impl" = -1 (default: seed_kernel
 * for a launch on small libraries, wave_seed_kernel with 96 registers for one on large libraries) / 0
 * seed_kernel / 1, 2 wave_seed_kernel (64-80 / 80-96 registers); "pair_impl" = 1 (default) / 0: the anchor-pair
 * search of one-word batches in pair_wave_kernel / stratum_kernel; "grid_pct" = 100 (default) / 1..100: every
 * cascade launch with this share of its workgroups (room for another cascade's launches on another stream);
 * (round 5) "fused_step" = 0 (default) / 1: for a caller that follows EVERY mrg_cascade_run* with an mrg_tally_run* on the
 * same stream: the cascade records no per-pass events (mrg_pass_stats.ms = 0: take the times from a run with the option
 * off) and d_pass_counts is written by the tally launch instead of by a launch of its own -- nothing then sits between
 * the launches of a step, which may be captured into a hipGraph;
 * "collapse_fast" = 1 (default) / 0: mrg_collapse_run takes its duplication-aware path for batches that fit it
 * (one-word reads without N, at most 29 nt) / always the general column-by-column sort;
 * "device_tables" = 1 (default) / 0: libraries added afterwards get the derived tables of a large library (>= 2^20
 * bases) filled on the device / built on the host and uploaded (mrg_ctx_library_check_tables);
 * (round 6) "pos_lists" = 1 (default) / 0, before mrg_ctx_add_library: a library with seed buckets also gets, for every
 * k-mer whose bucket overflows (an interspersed element, poly-A, a tandem motif: 10^2..10^5 rows), the k-mer's rows in
 * TEXT ORDER (fm_index.hpp: seed_pos_lists); "pos_scan" = 1 (default) / 0 at run time: a seed launch answers such a
 * seed by walking that list up to the first valid alignment (plus a 64-ary search of the suffix-sorted rows for an
 * exact occurrence) instead of verifying every row of the suffix interval -- same answers (runAnnotationPipeline.py:
 * 581-584 offers every read to every library, whatever the library holds);
 * "walk_cap" = 256 (default; 0..256): records a wave of wave_seed_kernel may leave behind its stream (reads whose seeds
 * meet repeats); beyond it such a seed is verified row by row as before round 6 (tests shrink it);
 * "long_lane" = 0 (default) / 1: in a batch of two words per read, the N-free reads of 33..63 nt take the FM kernels / go
 * with the one-word reads through the dictionary kernels' LONG instantiations (seeds from the first 32 bases, the second
 * word fetched where an alignment is verified; exact_dict_kernel and the FM kernels of that lane cannot see them: a length
 * is taken only when every pass either runs in a seed launch, keeps it out by its window, or -- pair_wave_kernel -- sees
 * at most 32 bases of it behind the trims or could not align it at all).  Same results (tests/test_gpu_split.py,
 * test_gpu_random_worlds.py); measured slower -- 1.10 against 0.67 ms for the 6.4 M reads of 33..40 nt of
 * `bench.py --workload varlen`: a long read's candidate costs two or three dependent text trips where a short one is
 * judged from its 16-byte row -- hence off;
 * "count_variants" = 1 (default) / 0 / 2: mrg_count_best with one seed mismatch on one-word reads without N answers the
 * reads that fit it (8 <= largest jump table k <= length <= min(seed_len, 32)) with count_variants_kernel and the rest
 * with count_kernel / everything with count_kernel / (tests) runs count_variants_kernel ALONE, so that the reads it left
 * come back with d_best_mm = 254 and an unwritten d_count: which kernel answered a read is then visible;
 * "wide_rows_16", "round_large": see DESIGN.md. */
int mrg_ctx_set_option(mrg_ctx *ctx, const char *key, int64_t value);
int mrg_ctx_device_info(const mrg_ctx *ctx, int32_t *n_cu, uint64_t *hbm_bytes,
                        char *arch, uint32_t arch_cap);
/* What a resident library's derived structures hold (round 5; the bench line of an unfriendly library set reports them):
 * out4 = { text positions stored in its exact-match dictionary, HOME SLOTS whose chain overflowed (a count of
 * homes, not of positions: every further position of such a home is left to the FM fallback), log2 of the
 * dictionary's slots (0: no dictionary), k of its seed buckets (0: none) }. */
int mrg_ctx_library_stats(const mrg_ctx *ctx, int32_t lib, uint64_t *out4);
/* Self-check of a resident library's derived tables (round 5).  With "device_tables" = 1 (default) a library of at
 * least 2^20 bases gets its jump tables, row context, wide rows, seed buckets (csrc/libtables.hip) and exact-match
 * dictionary (csrc/dictbuild.hip) filled ON THE DEVICE from the suffix-array rows and the packed text -- what replaces
 * the `.ebwt` load of runAnnotationPipeline.py:643 at the start of a run; the index file stores none of them.  This call
 * rebuilds the first four on the host (fm_index.cpp) and compares them with the device arrays word by word:
 * mismatches4 = { jump tables, row context, wide rows, seed buckets (round 6: with the headers and the position lists
 * of the overflowing k-mers) }, UINT64_MAX for a table the library does not have.  (The dictionary's layout depends on who fills it; what a lookup finds does not: tests/test_gpu_dictbuild.py.)
 * Slow -- seconds of host time for a 137 Mbp library: tests and bench gates call it, a run does not. */
int mrg_ctx_library_check_tables(mrg_ctx *ctx, int32_t lib, const mrg_index *index, uint64_t *mismatches4);
/* A context is used by one host thread at a time (calls on it are serialised by the caller).  It keeps
 * one device scratch arena, grown on demand by mrg_collapse_run (40 B per raw read + 64 MB) and
 * mrg_list_best_count and reused by later calls; this frees it (after synchronising the device), e.g.
 * once the one collapse of a run is done. */
int mrg_ctx_release_scratch(mrg_ctx *ctx);

/* One alignment pass = one bowtie command line of RAP:577-599 / RAP:688. */
typedef struct mrg_pass_cfg {
  int32_t lib;          /* library id from mrg_ctx_add_library */
  int32_t seed_len;     /* -l (28) for -n mode; >= MRG_MAX_WORDS*32 for -v mode */
  int32_t max_mm_seed;  /* -n N, or V for -v mode */
  int32_t max_mm_total; /* 2 for -n mode (-e 70 at Q40), V for -v mode */
  int32_t trim5;        /* -5 */
  int32_t trim3;        /* -3 */
  int32_t min_len;      /* length filter of RAP:543-554: process min_len<=len<=max_len */
  int32_t max_len;      /* (255 = no upper bound: the reference's filters are `< 26`, `> 25` or none) */
  int32_t poly_t;       /* 1 = pass 3 (RAP:664-686): need T{3,}$, strip all 3' T, >=11 nt */
  int32_t reserved;
} mrg_pass_cfg;

typedef struct mrg_pass_stats {
  uint64_t processed;  /* "# reads processed" (RAP:9-18) */
  uint64_t aligned;    /* "# reads with at least one reported alignment" */
  uint64_t steps;      /* FM backward-extension (LF) steps executed */
  uint64_t candidates; /* seed occurrences verified against the text */
  uint64_t lookups;    /* k-mer jump-table loads (each replaces k LF steps) */
  float ms;            /* device time of the pass (the reference's cpuTime); a fused launch is
                          charged to its first pass, the other passes of the group report 0 */
  uint32_t lds_bytes;  /* library bytes staged in LDS for this pass (0 = served from HBM/L2) */
  uint32_t lds_mode;   /* 0 nothing, 1 occ blocks, 2 occ blocks + text, 3 text only: names the
                          match_kernel<W, blocks, text> instantiation that ran; 4 = the pass ran
                          inside a fused launch (fused_kernel<W>, only its 9-mer bitmap in LDS);
                          5 / 6 = stratum_kernel<W> with / without the packed text in LDS;
                          7 = exact_dict_kernel (one slot load of the library's exact-match
                          dictionary per read: steps = 0, lookups = slot / table loads, candidates =
                          slots / rows compared); 8 / 9 = seed_kernel<false, 8> / seed_kernel<true, 6>
                          (the pass rode, as a unit or a member of a unit, in the seed launch of its
                          group's first pass -- 9: a launch with a library that has seed buckets; steps = 0,
                          lookups = jump-table / bucket / slot loads and candidates = rows of the unit,
                          reported with the unit's first pass) */
  uint32_t group;      /* index of the first pass of the launch this pass ran in (itself when it
                          had a launch of its own) */
  uint32_t n_launches; /* kernel launches that carried this pass: 1, or 2 for a 2-mismatch pass split
                          into strata 1-2 and stratum 3; 0 for a pass that was not launched or rode
                          in the fused launch of its group's first pass; a split batch ("split_mixed")
                          counts the launches of both of its cascades */
  uint32_t kbits_log2; /* log2 of the bits of the 9-mer presence bitmap the pass filtered seed
                          pieces with (18 = the library's full bitmap, 13..17 = folded for a
                          fused launch, 0 = no filter) */
  uint32_t pair_anchor; /* != 0, pass with ONE seed mismatch (fused launch, or seed launch in wave_seed_kernel with seed
                          buckets; large library): reads of
                          3 x pair_anchor .. 4 x pair_anchor - 1 seed bases were searched through the
                          three pairs of three anchors, the others through the pigeonhole pieces.
                          != 0, TWO seed mismatches: reads of at least 4 x pair_anchor seed bases
                          were searched through the six pairs of four anchors of that many bases
                          (lookups = pair lookups, candidates = their rows, no LF steps), reads
                          of at least 4 x (pair_anchor - 1) through anchors one base shorter;
                          still shorter reads went through the stratum-first pigeonhole pieces */
  float ms_rest;       /* a split batch ("split_mixed"): device time of this pass in the FIRST cascade (the
                          long reads, reads with N, very short reads: FM kernels); ms and the kernel fields
                          above describe the second one (the one-word reads); 0 when the batch was not split */
  uint32_t variant;    /* which instantiation behind lds_mode 8 / 9 (round 4): 0 = seed_kernel (tiles of 256 reads,
                          three barriers per tile), 1 = wave_seed_kernel<false, 8> / <true, 6> (every wave on its
                          own: a read with nothing left to look up is finished on the spot, the others are parked
                          and worked off 64 at a time), 2 = wave_seed_kernel<false, 6> / <true, 5> (more registers);
                          + 4 = the launch's input list carried its reads (16-byte entries written by the seed
                          launch in front of it: seed_kernel<.., .., true>);
                          + 8 (round 6) = the LONG instantiation: the batch's reads of 33..63 nt ride this launch too
                          (seeds from their first 32 bases, the second word compared where an alignment is verified).
                          lds_mode 7 (exact_dict_kernel): 16 (round 6) = the streaming launch gave every workgroup one
                          contiguous stretch of the batch instead of every gridDim-th chunk of 4096 reads (taken when
                          more than 2 % of the (workgroup, trip) slots of the chunked run would stay empty).
                          lds_mode 11 (round 4) = pair_wave_kernel: the anchor-pair search of a 2-mismatch pass for
                          one-word reads without N, items and rows compacted over the wave */
  uint32_t reserved;
} mrg_pass_stats;

/* Bytes of device workspace mrg_cascade_run needs for n reads (three survivor lists of n + 2^23 entries of 16 bytes --
 * the seed launches' lists carry their reads --, segment counts, counters, and since round 6 the 67 MB of records of the
 * reads wave_seed_kernel answers behind its stream: 48 B per read + 470 MB).  A workspace belongs to ONE cascade at a
 * time: cascades of one context on several streams each bring their own. */
int mrg_cascade_workspace_bytes(uint64_t n, uint64_t *bytes);

/*
 * The cascade (RAP:636-705): passes run in order; a read is offered to pass i
 * only if no earlier pass claimed it (writeSeqToAnnot RAP:543-554 +
 * updateAnnotDic RAP:341-345).  Outputs, one entry per read:
 *   d_pass_id  -1 = unannotated, else index of the claiming pass
 *   d_ref_id   library entry index (order of mrg_index_name), -1 if unannotated
 *   d_pos      0-based offset in the entry of the first untrimmed base
 *              (SAM POS-1), -1 if unannotated
 *   d_mm       mismatches of the reported alignment (0 if unannotated)
 * Tie rule (bowtie's own choice is RNG-driven): fewest mismatches, then lowest
 * entry index, then lowest offset.
 * d_pass_counts: 2*n_pass uint64 (processed, aligned per pass) written on
 * device so a sharded run can all-reduce them without a host round trip.
 * Asynchronous on `stream`; call mrg_cascade_stats after synchronising.
 */
int mrg_cascade_run(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read,
                    const uint8_t *d_lens, const uint64_t *d_nmask, uint64_t n,
                    const mrg_pass_cfg *passes, uint32_t n_pass, int8_t *d_pass_id,
                    int32_t *d_ref_id, int32_t *d_pos, uint8_t *d_mm,
                    uint64_t *d_pass_counts, void *d_workspace,
                    uint64_t workspace_bytes, void *stream);
/*
 * The four assignment arrays of mrg_cascade_run as ONE 32-bit word per read ("4 B packed
 * assignment out"), for callers that move assignments over PCIe: 4 bytes per read instead of 10.
 *   bits 28-31  claiming pass + 1 (0 = unannotated)
 *   bits 26-27  mismatches, saturating at 3
 *   bits  8-25  library entry, saturating at MRG_PACKED_REF_SAT (2^18 - 1)
 *   bits  0-7   offset of the alignment in the entry, saturating at MRG_PACKED_POS_SAT (255)
 * Every miRNA / hairpin / tRNA alignment fits (what the isomiR, A-to-I, GFF and tRF consumers read);
 * a saturated field says "ask the full arrays" (an mRNA entry past the 262143rd, an offset deep inside
 * a transcript).  n_pass must be at most 15.  Asynchronous on `stream`.
 */
#define MRG_PACKED_REF_SAT 0x3FFFFu
#define MRG_PACKED_POS_SAT 0xFFu
int mrg_pack_assignments(mrg_ctx *ctx, const int8_t *d_pass_id, const int32_t *d_ref_id, const int32_t *d_pos,
                         const uint8_t *d_mm, uint64_t n, uint32_t *d_packed, void *stream);
/* The cascade with the packed word as its ONLY per-read output (every kernel writes d_packed[r]
 * instead of the four arrays: 4 bytes out per read, what SURVEY.md 8d's byte accounting assumes), and
 * the two tallies reading it.  Same semantics otherwise; the saturation rules above apply (the count
 * tally needs entries of the miRNA library only, the edit tally their offsets too: always exact). */
int mrg_cascade_run_packed(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read, const uint8_t *d_lens,
                           const uint64_t *d_nmask, uint64_t n, const mrg_pass_cfg *passes, uint32_t n_pass,
                           uint32_t *d_packed, uint64_t *d_pass_counts, void *d_workspace, uint64_t workspace_bytes,
                           void *stream);
int mrg_tally_run_packed(mrg_ctx *ctx, const uint32_t *d_packed, const uint32_t *d_quant, uint64_t n, uint32_t n_samples,
                         uint32_t n_mirna, uint32_t n_pass, int32_t canon_pass, int32_t isomir_pass, uint64_t *d_counts,
                         void *stream);
int mrg_edit_tally_run_packed(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read, const uint8_t *d_lens,
                              const uint64_t *d_nmask, const uint32_t *d_packed, const uint32_t *d_quant,
                              const uint8_t *d_keep, const uint32_t *d_remap, uint64_t n, uint32_t n_samples,
                              uint32_t n_bins, int32_t lib, int32_t canon_pass, int32_t isomir_pass, int32_t isomir_trim5,
                              uint32_t flank5, uint32_t flank3, uint32_t from_base, uint32_t to_base, uint64_t *d_counts,
                              void *stream);
/*
 * The cascade for reads of ANY length (round 5).  writeSeqToAnnot (RAP:543-554) writes every unannotated read
 * into a pass's FASTA whatever its length -- the length filters of RAP:574 are `< 26`, `> 25` or none -- and bowtie
 * aligns it end to end; the batches of mrg_cascade_run describe a length in one byte.  A host sends the reads
 * beyond 255 nt (an untrimmed long-cycle run, a read-through: a handful per sample) here, in the RAGGED form:
 *   d_words     read r = d_words[d_word_off[r] .. d_word_off[r + 1]), ceil(len / 32) words, 32 bases per word,
 *               base i of the read in bits [2 (i % 32), 2 (i % 32) + 1] of word i / 32 (as in the packed batches)
 *   d_nmask     the same shape, or NULL when no read has an N
 *   d_word_off  n + 1 offsets in words;  d_lens  n lengths in bases (any length < 2^31; short reads are fine too)
 * Same passes, same policy fields and the same outputs as mrg_cascade_run -- fewest mismatches, then lowest entry,
 * then lowest offset; -1 / -1 / -1 / 0 for an unannotated read -- with two differences: a pass's max_len of 255 or
 * more means "no upper bound" (the reference has none), and trim5 may be any non-negative number.  One wave per read
 * over the library's FM index (csrc/long_reads.hip): written for any length, not for speed.
 *   d_pass_counts  NULL, or the 2 * n_pass uint64 (processed, aligned per pass) of the batch's mrg_cascade_run:
 *                  the long reads' counts are ADDED to them (run it after that call, on the same stream)
 *   stats          NULL, or n_pass host entries: processed / aligned / steps / candidates / lookups / ms are ADDED
 *                  to what they hold (hand in mrg_cascade_stats' array, or a zeroed one)
 * Synchronises `stream`.
 */
int mrg_cascade_run_long(mrg_ctx *ctx, const uint64_t *d_words, const uint64_t *d_nmask, const uint64_t *d_word_off,
                         const uint32_t *d_lens, uint64_t n, const mrg_pass_cfg *passes, uint32_t n_pass,
                         int8_t *d_pass_id, int32_t *d_ref_id, int32_t *d_pos, uint8_t *d_mm, uint64_t *d_pass_counts,
                         mrg_pass_stats *stats, void *stream);
/* Number of cascade runs this context has launched (a caller that reads statistics later can tell
 * whether they are still those of its own run). */
int mrg_cascade_run_id(const mrg_ctx *ctx, uint64_t *run_id);
/* Synchronises `stream` of the LAST run and returns its per-pass statistics. */
int mrg_cascade_stats(mrg_ctx *ctx, mrg_pass_stats *stats, uint32_t n_pass);

/*
 * The tally (SUM:34-66): per sample s and read r with quant[r][s] != 0:
 *   trimmedUniq[s]++ ; cat[pass][s] += quant ; cat[n_pass][s] (remReads) for -1
 *   pass == canon_pass : mir_quant[ref][s] += q ; mir_iscan[ref][s] += q
 *   pass == isomir_pass: mir_quant[ref][s] += q
 * d_counts layout (uint64, caller zeroes it):
 *   [0, M*S) mir_quant | [M*S, 2*M*S) mir_iscan |
 *   [2*M*S, 2*M*S + (n_pass+1)*S) category totals | then S trimmedUniq
 */
int mrg_tally_counts_len(uint32_t n_mirna, uint32_t n_samples, uint32_t n_pass,
                         uint64_t *len);
int mrg_tally_run(mrg_ctx *ctx, const int8_t *d_pass_id, const int32_t *d_ref_id,
                  const uint32_t *d_quant, uint64_t n, uint32_t n_samples,
                  uint32_t n_mirna, uint32_t n_pass, int32_t canon_pass,
                  int32_t isomir_pass, uint64_t *d_counts, void *stream);

/* ------------------------------------------------------------------ *
 * Multi-GPU: one process per GPU, the globally collapsed read set cut into contiguous shards,
 * every library replicated, and ONE collective per batch: the sum over ranks of the fused count
 * vector [mir_quant | mir_iscan | category totals | trimmedUniq | per-pass processed, aligned]
 * (mrg_tally_run's d_counts followed by mrg_cascade_run's d_pass_counts, all uint64).  The
 * reference has no counterpart (it is a single process); `filter` (utils/filter.py:7-13) is
 * non-linear and must run on the reduced vector.  RCCL over xGMI, bound at run time (dlopen): a
 * host that already has an RCCL mapped (PyTorch) shares it.
 *   mrg_comm_unique_id  rank 0 fills 128 bytes and hands them to the other ranks out of band
 *                       (a file, a pipe, an environment variable)
 *   mrg_comm_init       collective over the `world` processes, each with its own context / GPU
 *   mrg_allreduce       in place, uint64 sum, asynchronous on `stream`; a no-op for world == 1
 * ------------------------------------------------------------------ */
#define MRG_COMM_ID_BYTES 128
int mrg_comm_unique_id(void *id128);
int mrg_comm_init(mrg_ctx *ctx, const void *id128, int32_t rank, int32_t world);
int mrg_allreduce(mrg_ctx *ctx, uint64_t *d_buf, uint64_t n, void *stream);
int mrg_comm_destroy(mrg_ctx *ctx);

/*
 * A-to-I position tally: the per-read part of A2IEditing (utils/writeDataToCSV.py:145-229) and
 * judgeAllign (:35-69) on the alignments the cascade already produced, for the reads claimed by
 * the exact-miRNA pass (canon_pass) or the isomiR pass (isomir_pass, whose reported position is
 * that of the first base after its `-5` trim: isomir_trim5).  A library entry is flank5 + mature
 * + flank3 bases (runAnnotationPipeline.py:413: 2 and 6); a read is kept when judgeAllign keeps
 * it -- starts at most 1 nt after the mature sequence, at most 1 mismatch and enough matches over
 * the window that function compares -- and, if d_keep is given, d_keep[r] != 0 (the host's
 * genome-uniqueness / RPM selection, :1251-1287, :1293-1300).  Per output bin b (= entry, or
 * d_remap[entry] for merged miRNA names; n_bins of them) and sample s, uint64, caller zeroes:
 *   d_counts[(b * S + s) * 3 + 0]  count_true: summed counts of the kept reads
 *   d_counts[(b * S + s) * 3 + 1]  seq_true:   number of kept reads with a non-zero count
 *   d_counts[(b * S + s) * 3 + 2]  canonical:  counts of kept reads that are substrings of the mature sequence
 *   d_counts[n_bins * S * 3 + (b * 32 + i) * S + s]  counts of kept reads showing `to_base` where
 *       the mature sequence has `from_base` at (0-based) position i < mature length - 5 (:147,:168)
 * Bases: A=0 C=1 G=2 T=3 (A-to-I reads as A -> G: from_base 0, to_base 2).
 */
int mrg_edit_counts_len(uint32_t n_bins, uint32_t n_samples, uint64_t *len);
int mrg_edit_tally_run(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read,
                       const uint8_t *d_lens, const uint64_t *d_nmask, const int8_t *d_pass_id,
                       const int32_t *d_ref_id, const int32_t *d_pos, const uint32_t *d_quant,
                       const uint8_t *d_keep, const uint32_t *d_remap, uint64_t n, uint32_t n_samples,
                       uint32_t n_bins, int32_t lib, int32_t canon_pass, int32_t isomir_pass,
                       int32_t isomir_trim5, uint32_t flank5, uint32_t flank3, uint32_t from_base,
                       uint32_t to_base, uint64_t *d_counts, void *stream);
/*
 * What the context's last tally launch was (tests and diagnostics; read-only, no device work): both tallies
 * choose among instantiations of their kernel from the "lds_budget" option, the bin count and the pointers'
 * alignment, and all of them must count alike.  which = MRG_TALLY_LAUNCH_COUNTS (mrg_tally_run*) or
 * MRG_TALLY_LAUNCH_EDIT (mrg_edit_tally_run*); a call with n = 0 launches nothing and leaves the record alone, and
 * so does a call whose launch fails.
 *   out4[0]  flags: MRG_TALLY_LDS_HIST  the per-entry bins are privatised in LDS (else: global atomics)
 *                   MRG_TALLY_LDS_LIB   edit tally only: the library's text and entry starts are staged in LDS
 *                   MRG_TALLY_VEC4      one sample (edit tally: and one-word reads), every array aligned for
 *                                       16-byte loads: four reads per lane and trip, the rest one by one
 *   out4[1]  workgroups launched      out4[2]  dynamic LDS bytes      out4[3]  0 (reserved)
 */
#define MRG_TALLY_LAUNCH_COUNTS 0
#define MRG_TALLY_LAUNCH_EDIT 1
#define MRG_TALLY_LDS_HIST 1u
#define MRG_TALLY_LDS_LIB 2u
#define MRG_TALLY_VEC4 4u
int mrg_ctx_last_tally_launch(const mrg_ctx *ctx, int32_t which, uint32_t *out4);

/*
 * Best stratum of every read against ONE library, forward strand only: d_best_mm[r] = fewest
 * mismatches of a valid alignment (255 = the read does not align), d_count[r] = number of
 * alignments reaching it (saturates at 255; also 255 when a seed is too repetitive to be
 * walked: more than 4096 suffix-array rows, of which only the first 4096 are looked at).  Such a
 * read's d_best_mm is what the walked rows gave and may be too high; (255, 255) -- none of them
 * aligned -- means UNDECIDED, too repetitive, and not "does not align" (255, 0): a caller that
 * combines libraries must not let another library's answer make such a read unique.
 * Replaces the genome bowtie runs of the -ai path (utils/writeDataToCSV.py:1263
 * `-n 1 -f -a -3 2` and :1488 `-n 0 -f -a -3 2`), which only ask "is the best hit unique"
 * (:1277-1287) and "does it align" (:1491-1496); the host trims the 3' 2 nt, submits each
 * read and its reverse complement, and sums over the chromosome libraries.
 */
int mrg_count_best(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read,
                   const uint8_t *d_lens, const uint64_t *d_nmask, uint64_t n, int32_t lib,
                   int32_t seed_len, int32_t max_mm_seed, int32_t max_mm_total,
                   uint8_t *d_best_mm, uint8_t *d_count, void *stream);

/*
 * Every alignment of each read's best stratum against one library: what `bowtie -a --best
 * --strata` prints (flags of every cascade command line, runAnnotationPipeline.py:577-599) and
 * parseAlignment3 (RAP:41-52) collects for the tRF tables (RAP:657-660, :698-701).  Two sweeps so
 * the caller owns the output buffers:
 *   mrg_list_best_count  d_best_mm[n] (255 = unaligned), d_offsets[n+1] = exclusive prefix of
 *                        the stratum sizes, *total = d_offsets[n]; synchronises the stream;
 *   mrg_list_best_fill   alignment k of read r at d_ref/d_pos[d_offsets[r] + k] (entry index,
 *                        0-based offset in the entry; order within a read unspecified); slots
 *                        >= cap are not written.
 */
int mrg_list_best_count(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read,
                        const uint8_t *d_lens, const uint64_t *d_nmask, uint64_t n, int32_t lib,
                        int32_t seed_len, int32_t max_mm_seed, int32_t max_mm_total,
                        uint8_t *d_best_mm, uint64_t *d_offsets, uint64_t *total, void *stream);
int mrg_list_best_fill(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read,
                       const uint8_t *d_lens, const uint64_t *d_nmask, uint64_t n, int32_t lib,
                       int32_t seed_len, int32_t max_mm_seed, int32_t max_mm_total,
                       const uint8_t *d_best_mm, const uint64_t *d_offsets, uint64_t cap,
                       int32_t *d_ref, int32_t *d_pos, void *stream);

/*
 * Every valid alignment of each read against one library, on the forward strand (strands = 1,
 * bowtie's --norc) or on both (strands = 2: the reverse complement is searched in the same launch,
 * from the same packed reads): the listing behind the bowtie front end (mirge_amd/bowtie.py),
 * whose `-a` runs without --strata need every stratum on both strands -- the -ai genome runs
 * (utils/writeDataToCSV.py:1263 `-n 1 -f -a -3 2`, :1488) and predict mode's genome mapping
 * (miRge2.0.py:538 `-n 0 -m 3 -l 25 -a --best`).  Validity: <= max_mm_seed mismatches in the
 * seed (the read's first seed_len bases -- its 5' end on either strand), <= max_mm_total (<= 3)
 * overall, an N mismatches everything.  No seed interval is cut short: a 10^4-copy element lists
 * every copy.  Two sweeps, so that a caller can sum the counts of several libraries (the parts of
 * one genome) before it decides what is written:
 *   mrg_list_valid_count  d_counts[mm * n + r] (uint32, 4 * n) = exact number of valid alignments
 *                         of read r with exactly mm = 0..3 mismatches, both strands summed;
 *                         asynchronous;
 *   mrg_list_valid_fill   for every read with d_best_mm[r] != 255: its alignments with exactly
 *                         d_best_mm[r] mismatches (MRG_STRATUM_BEST, `--best --strata`) or all of
 *                         them (MRG_STRATUM_ALL, `-a`) at d_offsets[r] + k: entry index, 0-based
 *                         offset in the entry, strand (0 = +, 1 = -), mismatches; order within a
 *                         read unspecified; slots >= cap are not written.  d_best_mm[r] = 255 (no
 *                         alignment, or suppressed by -m) writes nothing.  Asynchronous.
 */
#define MRG_STRATUM_BEST 0
#define MRG_STRATUM_ALL 1
int mrg_list_valid_count(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read,
                         const uint8_t *d_lens, const uint64_t *d_nmask, uint64_t n, int32_t lib,
                         int32_t strands, int32_t seed_len, int32_t max_mm_seed,
                         int32_t max_mm_total, uint32_t *d_counts, void *stream);
int mrg_list_valid_fill(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read,
                        const uint8_t *d_lens, const uint64_t *d_nmask, uint64_t n, int32_t lib,
                        int32_t strands, int32_t stratum_mode, int32_t seed_len,
                        int32_t max_mm_seed, int32_t max_mm_total, const uint8_t *d_best_mm,
                        const uint64_t *d_offsets, uint64_t cap, int32_t *d_ref, int32_t *d_pos,
                        uint8_t *d_strand, uint8_t *d_mm, void *stream);

/*
 * The same listing for reads of ANY length, in the ragged form of mrg_cascade_run_long (read r =
 * d_words[d_word_off[r] .. d_word_off[r + 1]), 32 bases per word; d_nmask the same shape or NULL;
 * d_lens uint32): what the bowtie front end lists the reads beyond 255 nt with.  One wave per read
 * and the library's superblock table from global memory, so no library is too large for it; meant
 * for the handful of such reads a sample holds.  Same rule, same two sweeps, same asynchrony and
 * the same refusals as mrg_list_valid_count / _fill; within a read the fill sweep writes in the
 * fixed order (strand, seed piece, suffix-array row).
 */
int mrg_list_valid_long_count(mrg_ctx *ctx, const uint64_t *d_words, const uint64_t *d_nmask,
                              const uint64_t *d_word_off, const uint32_t *d_lens, uint64_t n,
                              int32_t lib, int32_t strands, int32_t seed_len, int32_t max_mm_seed,
                              int32_t max_mm_total, uint32_t *d_counts, void *stream);
int mrg_list_valid_long_fill(mrg_ctx *ctx, const uint64_t *d_words, const uint64_t *d_nmask,
                             const uint64_t *d_word_off, const uint32_t *d_lens, uint64_t n,
                             int32_t lib, int32_t strands, int32_t seed_len, int32_t max_mm_seed,
                             int32_t max_mm_total, int32_t stratum_mode, const uint8_t *d_best_mm,
                             const uint64_t *d_offsets, uint64_t cap, int32_t *d_ref, int32_t *d_pos,
                             uint8_t *d_strand, uint8_t *d_mm, void *stream);

/*
 * Host-buffer convenience for a caller without its own device allocator (the
 * ctypes stub of INTEGRATION.md): H2D, cascade, tally, D2H in one call.
 * counts may be NULL (then quant/n_samples are ignored).
 */
int mrg_annotate_host(mrg_ctx *ctx, const uint64_t *reads, uint32_t words_per_read,
                      const uint8_t *lens, const uint64_t *nmask, uint64_t n,
                      const mrg_pass_cfg *passes, uint32_t n_pass, int8_t *pass_id,
                      int32_t *ref_id, int32_t *pos, uint8_t *mm,
                      mrg_pass_stats *stats, const uint32_t *quant,
                      uint32_t n_samples, uint32_t n_mirna, int32_t canon_pass,
                      int32_t isomir_pass, uint64_t *counts);

/* mrg_cascade_run_long with HOST buffers (same ragged form; stats may be NULL, else it is added to). */
int mrg_annotate_long_host(mrg_ctx *ctx, const uint64_t *words, const uint64_t *nmask, const uint64_t *word_off,
                           const uint32_t *lens, uint64_t n, const mrg_pass_cfg *passes, uint32_t n_pass,
                           int8_t *pass_id, int32_t *ref_id, int32_t *pos, uint8_t *mm, mrg_pass_stats *stats);

/* ------------------------------------------------------------------ *
 * Ingest: FASTQ -> packed reads (host), raw reads -> unique reads with
 * per-sample counts (device).  Replaces trim_file with `-ad none`
 * (utils/trim_file.py:89-134: 3' quality trimming at Q10, 16-nt minimum)
 * and quantReads (utils/quantReads.py:3-24).
 * ------------------------------------------------------------------ */
typedef struct mrg_fastq mrg_fastq;
typedef struct mrg_fastq_info {
  uint64_t n_total;        /* records read ("totalReads") */
  uint64_t n_kept;         /* records kept after trimming ("trimmedReads") */
  int32_t phred;           /* 33 or 64, as trim_file.py:104-106 reports it */
  uint32_t words_per_read; /* 1, 2, 4 or 8 */
  uint32_t max_len;
  int32_t has_n;
  uint64_t n_long;         /* kept reads longer than 255 nt (MRG_MAX_WORDS words, one length byte): not among n_kept, not
                              in the packed batch; read them with mrg_fastq_long_read / mrg_fastq_copy_long and annotate
                              them with mrg_cascade_run_long (the reference accepts any length) */
} mrg_fastq_info;
/* Plain or gzip FASTQ.  qual_cutoff 10 and min_len 16 are the reference's values
 * (trim_file.py:30,33).  adapter = the `-ad` value after __main__.py:123-127: NULL or "none",
 * "+N" (UnconditionalCutter, trim_file.py:34-35) or one or more comma-separated 3' adapter
 * sequences (AdapterCutter at error rate 0.12, trim_file.py:38-41).  threads = trimming worker
 * threads (the reference's `-cpu` worker processes, trim_file.py:93-98); <= 0 picks one per
 * hardware thread, at most 32.  One thread inflates and splits records, the workers trim. */
int mrg_fastq_load(const char *path, int32_t qual_cutoff, int32_t min_len, const char *adapter,
                   int32_t threads, mrg_fastq **out);
/* One sample read by SEVERAL readers (round 5: `--gpus N` on a single FASTQ file; the reference ingests a sample in one
 * process, __main__.py:289-314): reader `part` of `n_parts`.  A plain file is cut into n_parts byte ranges at record
 * starts (a line that starts with '@' whose line after next starts with '+': every reader finds the same cuts) and
 * each reader reads its own; a gzip file cannot be entered in the middle: every reader inflates all of it and takes
 * every n_parts-th block of records (trimming, adapter search and packing are shared out, the inflate is not).  The
 * handle's n_total / n_kept / long reads are those of the share (their sums over the parts are the file's); the
 * quality base is the one the FILE's first record decides, whatever the part; info.phred is 0 unless part == 0. */
int mrg_fastq_load_part(const char *path, int32_t qual_cutoff, int32_t min_len, const char *adapter,
                        int32_t threads, int32_t part, int32_t n_parts, mrg_fastq **out);
/* cutadapt's 3' adapter search on one upper-case read (the AdapterCutter step above, exposed
 * for callers that trim outside a FASTQ file and for the tests): out6 = found, read_start
 * (where the read is cut), read_stop, adapter_stop, matches, errors. */
int mrg_adapter_locate(const char *adapter, const char *read, double max_error_rate,
                       int32_t min_overlap, int32_t *out6);
int mrg_fastq_get_info(const mrg_fastq *fq, mrg_fastq_info *info);
/* i-th over-long read (upper-case ASCII, valid until mrg_fastq_free). */
int mrg_fastq_long_read(const mrg_fastq *fq, uint64_t i, const char **seq);
/* The info.n_long over-long reads packed into the ragged form of mrg_cascade_run_long (same two-call protocol as
 * mrg_pack_reads_ragged: words == NULL fills word_off[n_long + 1] and lens only).  In file order, duplicates included:
 * the host collapses them (by their text, mrg_fastq_long_read) before it annotates them. */
int mrg_fastq_copy_long(const mrg_fastq *fq, uint64_t *words, uint64_t *nmask, uint64_t *word_off, uint32_t *lens,
                        int *has_n);
/* Copy the packed reads out, widened to words_per_read words (>= the file's own);
 * nmask may be NULL when has_n is 0. */
int mrg_fastq_copy(const mrg_fastq *fq, uint32_t words_per_read, uint64_t *words, uint8_t *lens,
                   uint64_t *nmask);
void mrg_fastq_free(mrg_fastq *fq);

/*
 * The same ingest ON THE DEVICE for raw text (round 3): the host reads the file, cuts it into blocks
 * of whole records (mrg_fastq_block_cut gives the offset of the last record boundary of a buffer:
 * buf[0, cut) is a block, the rest is carried over; at_eof != 0 takes everything) and uploads them;
 * mrg_fastq_parse_device splits the records, applies the 3' quality rule (phred = 33 or 64, as the
 * first record's qualities decide: trim_file.py:104-110), the `-ad +N` cutter (cut > 0 drops the
 * first `cut` bases, cut < 0 the last -cut; 0 = `-ad none`), the minimum length and the 2-bit packing
 * -- the packed reads never exist on the host.  Kept reads come out in file order:
 * d_words[w * cap + i], d_lens[i], d_nmask[w * cap + i] (may be NULL; info.has_n then says whether
 * one was needed).  Strict four-line records only ('\n' or "\r\n", final newline optional):
 * info.status != 0 (1-3: record info.bad_record, 1-based, is ill-formed -- not a '@' header or a
 * blank line, no '+' line, sequence and quality of different length; 4: the line count is not a
 * multiple of four; 5: more kept reads than `cap`) means nothing was packed: use mrg_fastq_load,
 * which also accepts blank lines between records and words the errors as the reference's loader
 * does.  info.n_long = kept reads longer than min(32 * words_per_read, 255) bases (not packed: call again
 * with more words, up to MRG_MAX_WORDS).  Adapter SEQUENCES (`-ad illumina`): mrg_fastq_parse_device_ad below.
 * Synchronises `stream`; at most 2^31 - 2 bytes per call.
 */
typedef struct mrg_fastq_device_info {
  uint64_t n_records;  /* records in the block ("totalReads") */
  uint64_t n_kept;     /* reads packed */
  uint64_t n_long;     /* kept by the rules but longer than the words offered */
  uint64_t bad_record;
  uint32_t max_len;    /* longest packed read */
  int32_t has_n;
  int32_t status;
  int32_t reserved;
} mrg_fastq_device_info;
int mrg_fastq_block_cut(const char *buf, uint64_t len, int32_t at_eof, uint64_t *cut);
/* (round 4) mrg_fastq_parse_device_ad: the same with adapter SEQUENCES -- `adapters` = the `-ad` value after
 * __main__.py:123-127 resolved its aliases, "SEQ[,SEQ...]" (at most 4 of at most 64 bases; NULL or "" = none):
 * cutadapt's 3' search (`-a`, error rate 0.12, minimum overlap 3: trim_file.py:30-41), one thread per read,
 * after the quality trim and the cutter; the adapter with the most matched bases cuts the read. */
int mrg_fastq_parse_device_ad(mrg_ctx *ctx, const char *d_text, uint64_t n_bytes, int32_t phred, int32_t qual_cutoff,
                              int32_t min_len, int32_t cut, const char *adapters, uint32_t words_per_read, uint64_t cap,
                              uint64_t *d_words, uint8_t *d_lens, uint64_t *d_nmask, mrg_fastq_device_info *info, void *stream);
int mrg_fastq_parse_device(mrg_ctx *ctx, const char *d_text, uint64_t n_bytes, int32_t phred, int32_t qual_cutoff,
                           int32_t min_len, int32_t cut, uint32_t words_per_read, uint64_t cap, uint64_t *d_words,
                           uint8_t *d_lens, uint64_t *d_nmask, mrg_fastq_device_info *info, void *stream);

/*
 * Parallel inflate of a `.fastq.gz` sample (round 4): the reference reads gzip samples through ONE
 * inflate stream (parseArgument.py:32, __main__.py:289-314, trim_file.py:89-134).  mrg_gz_open maps the
 * file and inflates it with `threads` workers (block starts found by trial, the 32 KB window in front of
 * a chunk kept symbolic until the chunk in front is done: csrc/pgzip.cpp); mrg_gz_read returns the next
 * bytes of the text in order, exactly what gzread returns (*got == 0: end of file), checking every
 * member's CRC-32 and length.  threads <= 1, plain files and files too small to cut take zlib's own
 * reader.  mrg_fastq_load uses the same reader.  One reader per handle; not thread-safe.
 */
typedef struct mrg_gz mrg_gz;
int mrg_gz_open(const char *path, int32_t threads, mrg_gz **out);
int mrg_gz_read(mrg_gz *gz, void *buf, uint64_t len, uint64_t *got);
/* parallel != NULL: 1 when the parallel reader serves the file; merged != NULL: chunk starts dropped so far */
int mrg_gz_info(const mrg_gz *gz, int32_t *parallel, uint64_t *merged);
void mrg_gz_close(mrg_gz *gz);

/*
 * The compact wire form of a collapsed read set, for callers whose unique reads live on the HOST (the
 * reference's seqDic after quantReads.py:3-24): 6.5 bytes per 22-nt read over PCIe instead of the 13 of
 * the arrays (8-byte word + length + 32-bit count) -- what bounds a host-resident pipeline is the upload.
 *   runs       HOST array of n_runs (length, count) uint32 pairs: the reads come grouped by length
 *              (groups in any order, at most 64 of them; N-free reads of at most 32 nt) -- this replaces
 *              the length array
 *   d_bits     the reads as a bit stream of 64-bit words: read j of a run of L-base reads is the 2 L bits
 *              from bit 2 L j of the run's words (little-endian bit order: bit b of the run = bit b % 64 of
 *              word b / 64; base k of a read in its bits 2k, 2k+1 as in the packed word); every run starts
 *              a new word.  n_words = the words given: the runs' words + at least one of padding
 *   d_quant8   n x n_samples bytes, the per-sample counts; 255 = the count is in the escape list
 *              (NULL: no counts are expanded, d_quant is not written)
 *   d_esc      n_esc pairs of uint32: (flat index into the n x n_samples counts, count)
 * widened on the device into the arrays mrg_cascade_run / mrg_tally_run take: d_reads [1][n], d_lens [n],
 * d_quant [n][n_samples] (16-byte aligned).  Asynchronous on `stream`; the runs are read before the
 * call returns.
 */
int mrg_expand_compact(mrg_ctx *ctx, const uint64_t *d_bits, uint64_t n_words, const uint32_t *runs, uint32_t n_runs,
                       const uint8_t *d_quant8, const uint32_t *d_esc, uint64_t n_esc, uint64_t n,
                       uint32_t n_samples, uint64_t *d_reads, uint8_t *d_lens, uint32_t *d_quant, void *stream);

/*
 * Collapse n raw reads (device arrays, layout as for mrg_cascade_run; d_sample gives the
 * sample of each read or is NULL for one sample) into unique reads:
 *   d_u_reads [words_per_read][cap], d_u_lens [cap], d_u_nmask ([..][cap] or NULL),
 *   d_quant [n_unique][n_samples] (uint32), d_len_hist [256][n_samples] (uint64, the
 *   reference's readLengthDic), *n_unique on the host.  cap >= n is always enough.
 * max_len is a hint nobody needs any more (the call reads the lengths: its histogram is an output anyway); a batch
 * of one-word reads without N of at most 29 nt (2 max_len + sample bits <= 58, at most 16 distinct lengths) takes
 * the duplication-aware path (csrc/collapse.hip: copies of a sequence are merged in LDS before anything is
 * partitioned), everything else a stable radix sort of read ids column by column; a sample id >= n_samples is
 * MRG_ERR_ARG.  Uniques come out ordered by (length, bases); the call synchronises `stream`.
 */
int mrg_collapse_run(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read,
                     const uint8_t *d_lens, const uint64_t *d_nmask, const uint16_t *d_sample,
                     uint64_t n, uint32_t n_samples, uint32_t max_len, uint64_t cap,
                     uint64_t *d_u_reads, uint8_t *d_u_lens, uint64_t *d_u_nmask, uint32_t *d_quant,
                     uint64_t *d_len_hist, uint64_t *n_unique, void *stream);
/*
 * What the context's last mrg_collapse_run did (tests and diagnostics; read-only, no device work): the fast path hands
 * a batch it does not take to the general path silently, and both give the same arrays.  The record is of the last
 * call that succeeded (all 0 before the first, and after a call with n = 0); a call that failed leaves it alone.
 *   out8[0]  path      0 = general path, the fast path was not tried; 1 = the fast path answered; 2 = the fast path
 *                      declined the batch's shape after its prepass, the general path answered; 3 = a reduce table of
 *                      the fast path overflowed, the general path answered
 *   out8[1]  reason    paths 0 and 2: 1 = option "collapse_fast" is 0, 2 = more than one word per read, 3 = an N mask,
 *                      4 = more than 16 samples, 5 = a pointer not aligned for the wide loads (d_reads 16, d_lens 4,
 *                      d_sample 8 bytes), 6 = a read beyond 29 nt, 7 = more than 16 distinct lengths,
 *                      8 = 2 max_len + sample bits > 58; else 0
 *   out8[2]  n_chunks  workgroups of the prepass and the split      out8[3]  chunk  reads per workgroup
 *                      (both 0 when the prepass did not run)
 *   out8[4]  n_hot     keys in the split's LDS hot table            out8[5]  n_pairs  (rest of key, count) pairs the split left
 *   out8[6]  n_buckets non-empty final buckets the reduce walked    (4 to 6: 0 unless the fast path reached its reduce)
 *   out8[7]  n_unique  unique reads returned
 */
int mrg_ctx_last_collapse(const mrg_ctx *ctx, uint32_t *out8);

/*
 * mapped.csv / unmapped.csv (utils/writeDataToCSV.py:582-619, :1172-1188) streamed from the
 * columnar HOST arrays the cascade produced instead of the reference's dict of dicts:
 *   row = uniqueSequence,annotFlag,<slot 1>,...,<slot n_slots>,<count of sample 1>,...
 * mapped != 0: the reads with pass_id >= 0, annotFlag 1, slot pass_id + 1 = the entry's name
 * (names[names_off[pass] + ref_id], names_off has n_slots + 1 entries); mapped == 0: the reads
 * with pass_id < 0, annotFlag 0, all slots empty.  reads is SoA with `stride` elements between
 * the words of a read (a slice of a larger array is fine); header (may be NULL) is written first
 * unless append != 0.  Rows come out in array order.  *rows = rows written.
 */
int mrg_write_read_table(const char *path, int32_t mapped, const char *header, int32_t append,
                         const uint64_t *reads, uint32_t words_per_read, uint64_t stride,
                         const uint8_t *lens, const uint64_t *nmask, uint64_t n, const int8_t *pass_id,
                         const int32_t *ref_id, const uint32_t *quant, uint32_t n_samples,
                         uint32_t n_slots, const char *const *names, const uint64_t *names_off,
                         uint64_t *rows);

/*
 * bowtie 1.1.2's text output for the bowtie front end (mirge_amd/bowtie.py), from HOST arrays:
 * read r (input order) is names[names_off[r] .. names_off[r+1]) and its trimmed sequence
 * seqs[seqs_off[r] .. seqs_off[r+1]) (ASCII, as printed); its alignments are entries
 * offsets[r] .. offsets[r+1] of entry / offset / strand (0 = +, 1 = -) / mm, printed in that
 * order; entry numbers run over the parts in order (the parts of one genome are one index).
 * suppressed[r] != 0 (may be NULL): the read exceeded -m m.  sam != 0:
 *   @HD, one @SQ per entry (its full length), @PG with CL:"<cmdline>"; aligned lines FLAG 0 / 16,
 *   MAPQ 255, SEQ / QUAL in reference orientation, XA:i / MD:Z / NM:i (the reference bases come
 *   from the index text); unaligned FLAG 4 with XM:i:0, suppressed FLAG 4 with XM:i:<m+1>;
 * sam == 0: bowtie's default format, aligned reads only: name, strand, entry, 0-based offset,
 *   sequence and qualities in reference orientation, 0, mismatch descriptors offset:ref>read.
 * Formatted by worker threads in blocks of reads, written in order.  path NULL = standard output.
 * summary[4] = reads processed, reads with an alignment printed, reads suppressed, alignments printed.
 */
int mrg_write_bowtie(const char *path, int32_t sam, const char *cmdline, const mrg_index *const *parts,
                     uint32_t n_parts, uint64_t n_reads, const char *names, const uint64_t *names_off,
                     const char *seqs, const uint64_t *seqs_off, const uint64_t *offsets,
                     const int32_t *entry, const int32_t *offset, const uint8_t *strand,
                     const uint8_t *mm, const uint8_t *suppressed, int32_t m, uint64_t *summary);

/*
 * Predict mode's location clusters (reference utils/cluster_basedon_location.py, called at miRge2.0.py:538-548 on the
 * samtools-sorted SAM of the genome run) from the rows mrg_list_valid_fill left ON THE DEVICE: sorted by coordinate
 * and merged where they overlap, without the SAM text, samtools or a Python loop (mirge_amd/predict.py,
 * Engine.cluster_valid).  The rule, per (entry, strand) list in position order, rows at one position in read order:
 * an alignment [s, e] (1-based, e = s + read length - 1) joins the cluster [S, E] in front of it iff s <= E and
 * E - s + 1 >= threshold, else it opens a new one; a joining row with e > E appends SEQ[E - s + 1 :] (SEQ = the read,
 * reverse-complemented on the - strand, N kept) and sets E = e.  All buffers are the caller's; `rows` < 2^32 - 1,
 * positions < 2^pos_bits <= 2^31.
 *   mrg_cluster_workspace_bytes  scratch (d_tmp) and per-row work area (d_work) sizes for `rows` rows;
 *   mrg_cluster_keys    one call per genome part, after its mrg_list_valid_fill: 64-bit keys of the part's rows
 *                       (d_ref / d_pos / d_strand [rows], d_offsets [n_reads + 1] as given to the fill) at
 *                       row_base .. row_base + rows of d_keys, with the row number as value (d_vals) and the row's read
 *                       in d_owner.  Entry = entry_base + d_ref.  MRG_CLUSTER_ORDER: (entry, strand, position);
 *                       MRG_SAM_ORDER: (entry, position, strand) -- a coordinate-sorted SAM file, + before - at one
 *                       position.  d_entry_keep (may be NULL) [n_entries]: rows of an entry with 0 (a name without
 *                       "chr") get the entry number n_entries and sort behind all others.  Asynchronous;
 *   mrg_cluster_sort    the library's stable LSD radix sort of the pairs over the low `bits` key bits (pos_bits + 1 +
 *                       the bits of n_entries); *in_second = the result is in d_keys1 / d_vals1.  Equal keys keep row
 *                       order, which is read order.  Asynchronous;
 *   mrg_cluster_scan    over pairs sorted in MRG_CLUSTER_ORDER: a segmented inclusive max-scan of e over the lists,
 *                       the cluster heads, their prefix sum; d_member[i] = the read of sorted row i.  *n_valid = rows on
 *                       kept entries (the first n_valid), *n_clusters; synchronises the stream;
 *   mrg_cluster_bounds  per cluster: entry, strand, start, end, first sorted row (d_member_off [n_clusters + 1]),
 *                       sequence length (d_len [n_clusters + 1]) and its prefix sum (d_seq_off [n_clusters + 1]);
 *                       *total_len = d_seq_off[n_clusters]; synchronises the stream;
 *   mrg_cluster_assemble  every row writes the bases it contributes to d_seq [total_len] (ASCII) and adds its read's
 *                       d_counts[read] to d_sum [n_clusters] (64-bit).  Asynchronous;
 *   mrg_cluster_sorted_rows  sorted pairs of either order as columns: read, entry, 0-based offset, strand, and d_mm
 *                       [rows, unsorted] gathered.  Asynchronous.
 */
#define MRG_CLUSTER_ORDER 0
#define MRG_SAM_ORDER 1
int mrg_cluster_workspace_bytes(uint64_t rows, uint64_t *tmp_bytes, uint64_t *work_bytes);
int mrg_cluster_keys(mrg_ctx *ctx, const uint64_t *d_offsets, uint64_t n_reads, const int32_t *d_ref,
                     const int32_t *d_pos, const uint8_t *d_strand, uint64_t rows, uint64_t row_base,
                     uint64_t total_rows, uint32_t entry_base, uint32_t n_entries, uint32_t pos_bits,
                     int32_t order, const uint8_t *d_entry_keep, uint64_t *d_keys, uint32_t *d_vals,
                     uint32_t *d_owner, void *stream);
int mrg_cluster_sort(mrg_ctx *ctx, uint64_t *d_keys0, uint64_t *d_keys1, uint32_t *d_vals0,
                     uint32_t *d_vals1, uint64_t rows, uint32_t bits, void *d_tmp, uint64_t tmp_bytes,
                     int32_t *in_second, void *stream);
int mrg_cluster_scan(mrg_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_vals, uint64_t rows,
                     const uint32_t *d_owner, const uint8_t *d_lens, uint32_t n_entries,
                     uint32_t pos_bits, int32_t threshold, void *d_work, uint64_t work_bytes,
                     void *d_tmp, uint64_t tmp_bytes, uint32_t *d_member, uint64_t *n_valid,
                     uint64_t *n_clusters, void *stream);
int mrg_cluster_bounds(mrg_ctx *ctx, const uint64_t *d_keys, uint64_t rows, uint64_t n_valid,
                       uint64_t n_clusters, uint32_t pos_bits, void *d_work, uint64_t work_bytes,
                       void *d_tmp, uint64_t tmp_bytes, uint32_t *d_entry, uint8_t *d_strand,
                       uint32_t *d_start, uint32_t *d_end, uint32_t *d_member_off, uint32_t *d_len,
                       uint64_t *d_seq_off, uint64_t *total_len, void *stream);
int mrg_cluster_assemble(mrg_ctx *ctx, const uint64_t *d_keys, uint64_t rows, uint64_t n_valid,
                         uint64_t n_clusters, uint32_t pos_bits, void *d_work, uint64_t work_bytes,
                         const uint32_t *d_member, const uint64_t *d_reads, uint32_t words_per_read,
                         const uint8_t *d_lens, const uint64_t *d_nmask, uint64_t n_reads,
                         const uint32_t *d_counts, const uint32_t *d_start, const uint64_t *d_seq_off,
                         char *d_seq, uint64_t *d_sum, void *stream);
int mrg_cluster_sorted_rows(mrg_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_vals, uint64_t rows,
                            uint32_t pos_bits, int32_t order, const uint32_t *d_owner,
                            const uint8_t *d_mm, uint32_t *d_read, int32_t *d_entry, int32_t *d_pos,
                            uint8_t *d_strand, uint8_t *d_mm_out, void *stream);

/*
 * Direct access to the library's own device primitives (csrc/prims.hip), for tests and diagnostics: the prefix sums,
 * the segmented max-scan and the radix sort that the collapse, the pair and dictionary builders, the ingest, the
 * library tables, the suffix-array builder and the clustering above are made of.  Device pointers, asynchronous on
 * `stream`; n == 0 succeeds and touches nothing.  d_tmp: at least the bytes mrg_prims_temp_bytes reports for n.
 *   mrg_prims_temp_bytes     scratch of a scan or a segmented max-scan (MRG_PRIMS_SCAN) or of a sort (MRG_PRIMS_SORT)
 *                            of n elements;
 *   mrg_prims_scan           d_out[i] = d_in[0] + .. + d_in[i - 1] (MRG_SCAN_EXCLUSIVE_U32, modulo 2^32; _U64: d_out
 *                            is uint64 and exact) or .. + d_in[i] (MRG_SCAN_INCLUSIVE_U32).  d_in == d_out is allowed
 *                            for the 32-bit kinds;
 *   mrg_prims_segmented_max  d_out[i] = max of d_in[h .. i], h = the last index <= i with d_head[h] != 0 (0 when
 *                            there is none).  d_in == d_out is allowed;
 *   mrg_prims_radix_sort     stable sort of n < 2^32 - 1 keys of key_bytes (4 or 8) by their bits [0, bits), bits <=
 *                            8 * key_bytes; key bits at and above `bits` travel with the key and order nothing.  The
 *                            32-bit values follow their keys; d_vals0 == d_vals1 == NULL sorts keys alone.  The
 *                            passes ping-pong between the two buffer sets: *in_second = the result is in d_keys1 /
 *                            d_vals1 (n == 0 or bits == 0: nothing moves, *in_second = 0).
 */
#define MRG_PRIMS_SCAN 0
#define MRG_PRIMS_SORT 1
#define MRG_SCAN_EXCLUSIVE_U32 0
#define MRG_SCAN_INCLUSIVE_U32 1
#define MRG_SCAN_EXCLUSIVE_U64 2
int mrg_prims_temp_bytes(int32_t kind, uint64_t n, uint64_t *bytes);
int mrg_prims_scan(mrg_ctx *ctx, int32_t kind, const uint32_t *d_in, void *d_out, uint64_t n, void *d_tmp,
                   uint64_t tmp_bytes, void *stream);
int mrg_prims_segmented_max(mrg_ctx *ctx, const uint32_t *d_in, const uint8_t *d_head, uint32_t *d_out,
                            uint64_t n, void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_prims_radix_sort(mrg_ctx *ctx, uint32_t key_bytes, void *d_keys0, void *d_keys1, uint32_t *d_vals0,
                         uint32_t *d_vals1, uint64_t n, uint32_t bits, void *d_tmp, uint64_t tmp_bytes,
                         int32_t *in_second, void *stream);

/*
 * Predict mode's two files from HOST arrays (reads and index parts as for mrg_write_bowtie), formatted by worker
 * threads in blocks and written in order:
 *   mrg_write_sorted_sam  `@HD VN:1.0 SO:coordinate`, the @SQ lines of mrg_write_bowtie, then the n_rows aligned lines
 *                         in the order given (row k is read row_read[k]; the lines are mrg_write_bowtie's SAM lines),
 *                         then the FLAG 4 line of every read without a row, in input order.  summary as there;
 *   mrg_write_clusters    the header line and one line per cluster: <sample>:miRCluster_<i>_<len> (i from 1), entry
 *                         name, strand, start, end, sequence, length, summed read count, member count, and the
 *                         comma-joined names of reads members[member_off[c] .. member_off[c + 1]).  *rows = clusters;
 *   mrg_read_counts_from_names  counts[r] = the integer between the first and the second `_` of read r's name
 *                         (`mir<k>_<count>`, reference convert2Fasta.py:131); a name without one is MRG_ERR_FORMAT
 *                         with *bad_read = r (else -1).
 */
int mrg_write_sorted_sam(const char *path, const mrg_index *const *parts, uint32_t n_parts,
                         uint64_t n_reads, const char *names, const uint64_t *names_off, const char *seqs,
                         const uint64_t *seqs_off, uint64_t n_rows, const uint32_t *row_read,
                         const int32_t *entry, const int32_t *offset, const uint8_t *strand,
                         const uint8_t *mm, const uint8_t *suppressed, int32_t m, uint64_t *summary);
int mrg_write_clusters(const char *path, const char *sample, const mrg_index *const *parts,
                       uint32_t n_parts, uint64_t n_clusters, const uint32_t *entry, const uint8_t *strand,
                       const uint32_t *start, const uint32_t *end, const uint64_t *seq_off, const char *seq,
                       const uint64_t *count_sum, const uint32_t *member_off, const uint32_t *members,
                       uint64_t n_reads, const char *names, const uint64_t *names_off, uint64_t *rows);
int mrg_read_counts_from_names(uint64_t n_reads, const char *names, const uint64_t *names_off,
                               uint32_t *counts, int64_t *bad_read);

/*
 * Predict mode's preliminary trim of the location clusters (reference utils/preTrimClusteredSeq.py and generate_Seq.py,
 * miRge2.0.py:557-562) over the device arrays of mrg_cluster_bounds / mrg_cluster_assemble (csrc/predict_trim.hip).
 *
 *   mrg_predict_trim_temp_bytes  HOST: the bytes of device scratch mrg_predict_trim needs for n_clusters clusters.
 *   mrg_predict_trim  DEVICE.  d_entry / d_strand / d_start / d_end [n_clusters], d_seq_off [n_clusters + 1] ascending from
 *       0 to total_len, d_seq [total_len] ASCII.  The repeat table: d_rep_off [n_entries + 1] ascending into d_rep_start /
 *       d_rep_end [n_elements] (1-based inclusive), an entry's elements sorted stably by start; an entry without elements
 *       has an empty range.  Per cluster c:
 *         d_orig        its bytes of d_seq on `+`; on `-` their reverse complement (A<->T, C<->G, any other byte itself)
 *                       inside the same range [d_seq_off[c], d_seq_off[c + 1]);
 *         d_flag = 1    iff its length <= len_cutoff, d_orig does not end in six `A` nor begin with six `T`, and neither of
 *                       the two elements of its entry whose start is nearest d_start[c] shares a coordinate with
 *                       [d_start[c], d_end[c]] (an entry with one element: that one; with none: passes).  Nearest is by
 *                       |element start - d_start[c]|; at equal distance the lower element start goes first, then the lower
 *                       element index.  An element with end < start intersects nothing;
 *         d_rep         the nearer of the two elements if it intersects, else the other if it does, else -1.  The repeat
 *                       test is not reached (-1) when the length or the end test fails.
 *       The retained clusters (flag 1) in cluster order: d_kept [*n_kept of n_clusters] their numbers, d_kept_seq_off
 *       [*n_kept + 1 of n_clusters + 1] the offsets of their d_orig bytes in d_kept_orig [*kept_len of total_len].
 *       MRG_ERR_ARG when d_seq_off, d_entry or d_rep_off contradict the sizes given (the outputs are then undefined).
 *       Limits: n_clusters < 2^31, total_len < 2^38, n_elements < 2^32 - 1.  Synchronises the stream.
 *   mrg_write_trimmed_clusters  HOST: the three files from host arrays -- the cluster arrays, member lists and read names as
 *       mrg_write_clusters takes them, flag / rep / orig of mrg_predict_trim, and the repeat names (rep_name_id [n_elements]
 *       into the n_rep_names strings of rep_names / rep_names_off).  tsv_path: the header `miRClusterID OriginalSeq Flag
 *       repetitiveElementName` + columns 2.. of mrg_write_clusters' header, one line per cluster (the name is `*` for
 *       rep -1); fa_path / orig_fa_path: for the clusters with flag 1 `>` id `:` entry `:` start `_` end strand, then the
 *       sequence / its orig.  *rows = clusters, *kept = FASTA records.  Blocks are formatted in parallel, written in order.
 */
int mrg_predict_trim_temp_bytes(uint64_t n_clusters, uint64_t *bytes);
int mrg_predict_trim(mrg_ctx *ctx, uint64_t n_clusters, const uint32_t *d_entry, const uint8_t *d_strand,
                     const uint32_t *d_start, const uint32_t *d_end, const uint64_t *d_seq_off, const char *d_seq,
                     uint64_t total_len, uint32_t n_entries, const uint32_t *d_rep_off, const uint32_t *d_rep_start,
                     const uint32_t *d_rep_end, uint64_t n_elements, int32_t len_cutoff, uint8_t *d_flag,
                     int32_t *d_rep, char *d_orig, uint32_t *d_kept, uint64_t *d_kept_seq_off, char *d_kept_orig,
                     uint64_t *n_kept, uint64_t *kept_len, void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_write_trimmed_clusters(const char *tsv_path, const char *fa_path, const char *orig_fa_path, const char *sample,
                               const mrg_index *const *parts, uint32_t n_parts, uint64_t n_clusters,
                               const uint32_t *entry, const uint8_t *strand, const uint32_t *start,
                               const uint32_t *end, const uint64_t *seq_off, const char *seq,
                               const uint64_t *count_sum, const uint32_t *member_off, const uint32_t *members,
                               uint64_t n_reads, const char *names, const uint64_t *names_off, const uint8_t *flag,
                               const int32_t *rep, const char *orig, uint64_t n_elements,
                               const uint32_t *rep_name_id, uint64_t n_rep_names, const char *rep_names,
                               const uint64_t *rep_names_off, uint64_t *rows, uint64_t *kept);

/*
 * Predict mode's second mapping (reference miRge2.0.py:566-601: two bowtie passes of the sample's filtered reads against the
 * retained clusters, utils/processSam.py and `sort -k6,6 -k1,1`) around two listings of mrg_list_valid_count / _fill against
 * the cluster library, whose entry j is record j of `*_clusters_trimmed_orig.fa` (csrc/predict_remap.hip).
 *
 *   mrg_predict_remap_temp_bytes  HOST: the bytes of device scratch the two calls below need for n_reads reads and n_rows
 *       rows (pass 1 + pass 2).
 *   mrg_predict_trim_reads  DEVICE.  d_counts [4][n]: the per-stratum counts of mrg_list_valid_count for pass 1.  The reads
 *       with no alignment in any stratum, in read order: d_sel [*n_sel of n] their indices, and the reads themselves as a
 *       packed set of their own -- d_out_reads [words_per_read][*n_sel] (the stride is *n_sel; the buffers hold
 *       words_per_read * n words), d_out_lens [*n_sel of n], d_out_nmask like d_out_reads when d_nmask is given -- with
 *       trim5 bases cut at the 5' end and trim3 at the 3' end (bowtie's -5 / -3): the length is max(0, len - trim5 - trim3),
 *       the words and the N mask are shifted across the 64-bit word boundaries, every bit beyond the new length is zero.
 *       Synchronises the stream.
 *   mrg_predict_remap_rows  DEVICE.  Pass 1: d_off1 [n_reads + 1] ascending from 0 to rows1, d_ref1 / d_pos1 / d_mm1
 *       [rows1]; pass 2 likewise over the n_sel reads d_sel [n_sel] (d_off2 [n_sel + 1], rows2); a listing without rows is
 *       not read.  d_numbers [n_reads]: the n of `mir<n>_<count>`; d_kept [n_clusters]: entry j is cluster number
 *       d_kept[j] + 1.  Output, [rows1 + rows2] each: d_read, d_cluster (the entry), d_offset, d_mm, d_pass (0 / 1), ordered
 *       as `LC_ALL=C sort -k6,6 -k1,1` orders the lines: by the bytes of the cluster name, i.e. of the digits of its number
 *       followed by `_` (a 40-bit key: the digits left-aligned at 4 bits each, padded with 15), then likewise by the read
 *       name; rows equal in both keep the listing order (pass 1 before pass 2, rows of a listing in its order) and are put
 *       into the order of their lines by the writer.  MRG_ERR_ARG when offsets, entries or d_sel contradict the sizes given
 *       (the outputs are then undefined).  Limits: n_reads, n_clusters < 2^31, rows1 + rows2 < 2^32 - 1.  Synchronises.
 *   mrg_write_remapped_rows  HOST: `<sample>_vs_representative_seq_modified_selected_sorted.tsv` from host arrays: the
 *       packed reads, their numbers and counts, the cluster library (its entry names are printed), kept_seq_off /
 *       kept_orig of mrg_predict_trim and the rows above.  One line per row, 17 tab-separated fields: name, count, the whole
 *       read, the cluster's OriginalSeq, then FLAG (0) .. NM:i: exactly as mrg_write_bowtie's SAM lines have them; a pass-2
 *       row's sequence is the read without its first trim5 and last trim3 bases.  Rows that name no read or cluster, align
 *       an empty read or run past their cluster's end are MRG_ERR_ARG before the file is opened.  *rows = lines.
 */
int mrg_predict_remap_temp_bytes(uint64_t n_reads, uint64_t n_rows, uint64_t *bytes);
int mrg_predict_trim_reads(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read, uint64_t stride,
                           const uint8_t *d_lens, const uint64_t *d_nmask, uint64_t n, const uint32_t *d_counts,
                           uint32_t trim5, uint32_t trim3, uint32_t *d_sel, uint64_t *d_out_reads, uint8_t *d_out_lens,
                           uint64_t *d_out_nmask, uint64_t *n_sel, void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_predict_remap_rows(mrg_ctx *ctx, uint64_t n_reads, const uint32_t *d_numbers, uint64_t n_clusters,
                           const uint32_t *d_kept, const uint64_t *d_off1, uint64_t rows1, const int32_t *d_ref1,
                           const int32_t *d_pos1, const uint8_t *d_mm1, uint64_t n_sel, const uint32_t *d_sel,
                           const uint64_t *d_off2, uint64_t rows2, const int32_t *d_ref2, const int32_t *d_pos2,
                           const uint8_t *d_mm2, uint32_t *d_read, uint32_t *d_cluster, uint32_t *d_offset, uint8_t *d_mm,
                           uint8_t *d_pass, void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_write_remapped_rows(const char *path, const uint64_t *reads, uint32_t words_per_read, uint64_t stride,
                            const uint8_t *lens, const uint64_t *nmask, uint64_t n_reads, const uint32_t *numbers,
                            const uint32_t *counts, const mrg_index *clusters, uint64_t n_clusters,
                            const uint64_t *kept_seq_off, const char *kept_orig, uint64_t n_rows, const uint32_t *row_read,
                            const uint32_t *row_cluster, const uint32_t *row_offset, const uint8_t *row_mm,
                            const uint8_t *row_pass, uint32_t trim5, uint32_t trim3, uint64_t *rows);

/* Predict mode's cluster feature table (reference miRge2.0.py:604: utils/generate_featureFiles.py, classes/readCluster.py)
 * from the rows of mrg_predict_remap_rows (csrc/predict_features.hip; the rule: tests/predict_features_model.py).  The
 * retained clusters come as per-cluster arrays: d_cl_entry / _strand / _start / _end [n_clusters] (the location cluster's,
 * gathered by d_kept), d_kept, d_kept_seq_off / d_kept_orig of mrg_predict_trim.  Every call returns MRG_ERR_ARG when the
 * arrays contradict each other or the sizes given (the outputs are then undefined); no lane reads or writes beyond those
 * sizes.  Limits: rows < 2^32 - 1, reads, clusters, entries < 2^31.  All but _tally synchronise.
 *
 *   mrg_predict_feature_temp_bytes  HOST: the bytes of device scratch the calls below need for n_rows rows.
 *   mrg_predict_feature_groups  DEVICE.  The groups: consecutive rows of one cluster, in row order.  d_row_group [n_rows];
 *       d_group_off [n_rows + 1], d_group_cluster / d_group_sum / d_group_pass [n_rows], of which *n_groups (+ 1) are set.
 *       d_group_sum = the members' counts summed in 64 bits (a read listed twice counts twice); d_group_pass = 1 iff
 *       sum >= 10, members >= 3, start > 20 and end < d_entry_len[entry] - 20.  Nothing is compacted.
 *   mrg_predict_feature_align  DEVICE.  d_cl_word / d_cl_len [n_clusters]: the clusters packed two bits a base, length 255
 *       for one longer than 32 nt or with a letter other than A/C/G/T.  Per row of a passing group the first alignment
 *       pairwise2.align.localms(cluster, read, 2, -1, -20, -20) lists: d_row_status (0 = one ungapped diagonal, 1 = a tie
 *       settled on the device, 2 = row of a failing group, not aligned; 3 = not packable, 4 = N in the read, 5 = gapped,
 *       6 = tie left open, 7 = no score: left to the host), d_row_diag (read base 0 under cluster position d) and
 *       d_row_ident (equal columns over the whole overlap).  d_group_host [n_groups] = 1 for a group with a row >= 3.
 *   mrg_predict_feature_tally  DEVICE, asynchronous.  One wave per passing group that is not host-marked: d_frame
 *       [n_groups][4] = H, T (dashes before / behind the cluster), head, tail (first / last column whose majority base
 *       holds 5 c >= 4 sum; tail negative); d_valid = 1 iff such a column exists; d_exact = the summed counts of the
 *       members whose identity is their length; d_nine [n_groups][45] = the count-weighted A, T, C, G and dash of the nine
 *       feature columns of the re-padded frame.  Other groups get valid 0 and zeros.
 *   mrg_predict_feature_neighbors  DEVICE.  The groups with d_valid ordered by (d_entry_rank[entry], start, end, cluster
 *       number as text): d_order [n_groups], of which the first *n_sorted are those groups; per GROUP d_nb_t (its index on
 *       its chromosome), d_nb_up / d_nb_down (distance s2 - e1 - 1 between the intervals (start + head - H,
 *       end + 1 + tail + T)), d_nb_flags (bit 0: no upstream neighbour, bit 1: no downstream one, bits 2-3: 0 Null, 1 Good,
 *       2 Bad).  Groups the host worked out take part with their d_frame / d_valid patched in by the caller.
 *   mrg_write_predict_features  HOST: `_features.tsv` and `_cluster.txt` from host copies of the arrays above, for the
 *       groups order [n_order] in that order.  group_text: null, or per group null / its frame as text (the cluster's padded
 *       row and every member's, '\n' between) for a group whose rows have no diagonal.  mapped != 0: `-1\tNull` in front of
 *       every line, else `Null\tNull`.  The genome parts supply the chromosome names, lengths and template bases, the
 *       cluster library the cluster names.  Arrays that contradict each other, or a template range that leaves its
 *       chromosome, are MRG_ERR_ARG before a file is opened.  written[0] = blocks of `_cluster.txt`, written[1] = lines of
 *       `_features.tsv` below the header.  Worker threads: MIRGE_AMD_TABLE_THREADS.
 */
int mrg_predict_feature_temp_bytes(uint64_t n_rows, uint64_t *bytes);
int mrg_predict_feature_groups(mrg_ctx *ctx, uint64_t n_rows, const uint32_t *d_row_read, const uint32_t *d_row_cluster,
                               uint64_t n_reads, const uint32_t *d_counts, uint64_t n_clusters, const uint32_t *d_cl_entry,
                               const uint32_t *d_cl_start, const uint32_t *d_cl_end, const uint64_t *d_kept_seq_off,
                               uint64_t orig_len, uint64_t n_entries, const uint32_t *d_entry_len, uint32_t *d_row_group,
                               uint32_t *d_group_off, uint32_t *d_group_cluster, uint64_t *d_group_sum, uint8_t *d_group_pass,
                               uint64_t *n_groups, uint64_t *n_passed, void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_predict_feature_align(mrg_ctx *ctx, uint64_t n_rows, const uint32_t *d_row_read, const uint32_t *d_row_cluster,
                              const uint32_t *d_row_group, uint64_t n_groups, const uint8_t *d_group_pass,
                              const uint64_t *d_reads, const uint8_t *d_lens, const uint64_t *d_nmask, uint64_t n_reads,
                              uint64_t n_clusters, const uint64_t *d_kept_seq_off, const char *d_kept_orig, uint64_t orig_len,
                              uint64_t *d_cl_word, uint8_t *d_cl_len, uint8_t *d_row_status, int32_t *d_row_diag,
                              uint8_t *d_row_ident, uint8_t *d_group_host, void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_predict_feature_tally(mrg_ctx *ctx, uint64_t n_groups, const uint32_t *d_group_off, const uint32_t *d_group_cluster,
                              const uint8_t *d_group_pass, const uint8_t *d_group_host, uint64_t n_rows,
                              const uint32_t *d_row_read, const int32_t *d_row_diag, const uint8_t *d_row_ident,
                              const uint64_t *d_reads, const uint8_t *d_lens, uint64_t n_reads, const uint32_t *d_counts,
                              uint64_t n_clusters, const uint8_t *d_cl_len, uint8_t *d_valid, int32_t *d_frame,
                              uint64_t *d_exact, uint64_t *d_nine, void *stream);
int mrg_predict_feature_neighbors(mrg_ctx *ctx, uint64_t n_groups, const uint32_t *d_group_cluster, const uint8_t *d_valid,
                                  const int32_t *d_frame, uint64_t n_clusters, const uint32_t *d_cl_entry,
                                  const uint8_t *d_cl_strand, const uint32_t *d_cl_start, const uint32_t *d_cl_end,
                                  const uint32_t *d_kept, uint64_t n_entries, const uint32_t *d_entry_rank, uint32_t *d_order,
                                  uint32_t *d_nb_t, int64_t *d_nb_up, int64_t *d_nb_down, uint8_t *d_nb_flags,
                                  uint64_t *n_sorted, void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_write_predict_features(const char *features_path, const char *cluster_path, int mapped, const mrg_index *const *parts,
                               uint32_t n_parts, const mrg_index *clusters, uint64_t n_clusters, const uint32_t *cl_entry,
                               const uint8_t *cl_strand, const uint32_t *cl_start, const uint32_t *cl_end,
                               const uint64_t *kept_seq_off, const char *kept_orig, const uint64_t *reads,
                               uint32_t words_per_read, uint64_t stride, const uint8_t *lens, const uint64_t *nmask,
                               const uint32_t *counts, uint64_t n_reads, uint64_t n_rows, const uint32_t *row_read,
                               const int32_t *row_diag, uint64_t n_groups, const uint32_t *group_off,
                               const uint32_t *group_cluster, const int32_t *frame, const uint64_t *exact, const uint64_t *nine,
                               const uint32_t *nb_t, const int64_t *nb_up, const int64_t *nb_down, const uint8_t *nb_flags,
                               const char *const *group_text, uint64_t n_order, const uint32_t *order, uint64_t *written);

/* Predict mode's precursor candidates (reference miRge2.0.py:608: utils/get_precursors.py) from the groups of the feature
 * table and the resident genome libraries (csrc/predict_precursors.hip; the rule: tests/predict_precursors_model.py).  For
 * every group of d_order whose line `_features.tsv` holds -- (H + L + T) + max(0, 3 - head) + max(0, 6 - tailAdd) - head -
 * tailAdd >= 7, L = end - start + 1, tailAdd = -tail - 1 -- the stable part is s = start - H + head, e = end + T - tailAdd
 * on `+` and s = start - T + tailAdd, e = end + H - head on `-`; record 2 w is the bases [max(0, s - 71), e + 20) of the
 * cluster's entry (0-based, clipped at the entry's length), record 2 w + 1 is [max(0, s - 21), e + 70); on `-` the
 * reverse complement; as RNA (A C G U, N where the index holds no base).
 *
 *   mrg_predict_precursor_temp_bytes  HOST: the bytes of device scratch the two calls below need for n_order positions.
 *   mrg_predict_precursors  DEVICE, synchronises.  d_order [n_order]: the groups in file order (mrg_predict_feature_neighbors'
 *       first n_sorted), d_group_cluster / d_frame / d_valid [n_groups] as the feature calls left them; the retained clusters
 *       [n_clusters]; d_entry_len [n_entries].  d_written [n_order] = 1 for a group with a line; d_rec_group / d_rec_lo /
 *       d_rec_hi [2 n_order] and d_rec_off [2 n_order + 1], of which 2 *n_written (+ 1) are set: the record's group, its
 *       window [lo, hi) and the offset of its bytes; *seq_len = d_rec_off[2 *n_written].  MRG_ERR_ARG when d_order names
 *       no group or one with d_valid 0, a group names a cluster >= n_clusters, a cluster an entry >= n_entries, or a window
 *       ends at or before base 0 (the outputs are then undefined).  Limits: groups < 2^30, bytes < 2^38.
 *   mrg_predict_precursor_bases  DEVICE, synchronises.  d_seq [seq_len]: the bytes of the n_rec records.  libs [n_parts]: the
 *       genome's parts as libraries of ctx (mrg_ctx_add_library), entry_base [n_parts]: the global number of every part's
 *       first entry (host arrays; at most 32 parts; together they hold n_entries entries).  The records are checked first:
 *       offsets that do not ascend from 0 to seq_len by hi - lo, lo > hi, hi beyond the entry, a group, cluster or entry out
 *       of range are MRG_ERR_ARG and nothing is written.  A library's per-entry segment table is built at its first use.
 *   mrg_write_precursors  HOST: `<table>_features_precusor.fa` from host copies: `>` + the cluster library's name of the
 *       record's cluster + `:precusor_1` (even records) or `:precusor_2` (odd), the record's bytes.  Arrays that contradict
 *       each other (an odd record count, a pair of two groups, a group listed twice, offsets that do not close at seq_len or
 *       do not match hi - lo, a window beyond its entry) are MRG_ERR_ARG before the file is opened.  written[0] = records,
 *       written[1] = bytes.  Worker threads: MIRGE_AMD_TABLE_THREADS.
 */
int mrg_predict_precursor_temp_bytes(uint64_t n_order, uint64_t *bytes);
int mrg_predict_precursors(mrg_ctx *ctx, uint64_t n_order, const uint32_t *d_order, uint64_t n_groups,
                           const uint32_t *d_group_cluster, const int32_t *d_frame, const uint8_t *d_valid, uint64_t n_clusters,
                           const uint32_t *d_cl_entry, const uint8_t *d_cl_strand, const uint32_t *d_cl_start,
                           const uint32_t *d_cl_end, uint64_t n_entries, const uint32_t *d_entry_len, uint8_t *d_written,
                           uint32_t *d_rec_group, uint32_t *d_rec_lo, uint32_t *d_rec_hi, uint64_t *d_rec_off,
                           uint64_t *n_written, uint64_t *seq_len, void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_predict_precursor_bases(mrg_ctx *ctx, uint64_t n_rec, const uint32_t *d_rec_group, const uint32_t *d_rec_lo,
                                const uint32_t *d_rec_hi, const uint64_t *d_rec_off, uint64_t n_groups,
                                const uint32_t *d_group_cluster, uint64_t n_clusters, const uint32_t *d_cl_entry,
                                const uint8_t *d_cl_strand, uint64_t n_entries, const uint32_t *d_entry_len, uint32_t n_parts,
                                const int32_t *libs, const uint32_t *entry_base, char *d_seq, uint64_t seq_len, void *d_tmp,
                                uint64_t tmp_bytes, void *stream);
int mrg_write_precursors(const char *path, const mrg_index *const *parts, uint32_t n_parts, const mrg_index *clusters,
                         uint64_t n_clusters, const uint32_t *cl_entry, uint64_t n_groups, const uint32_t *group_cluster,
                         uint64_t n_rec, const uint32_t *rec_group, const uint32_t *rec_lo, const uint32_t *rec_hi,
                         const uint64_t *rec_off, const char *seq, uint64_t seq_len, uint64_t *written);

/* Predict mode's screening of the folded precursor candidates (reference miRge2.0.py:626: utils/screen_precusor_candidates.py
 * with classes/readPrecusor.py, prunedLength 15) around the two folds the caller runs (csrc/predict_screen.hip,
 * csrc/predict_screen_write.cpp; the rule: tests/predict_screen_model.py).  Strings travel as offsets
 * [n + 1] (uint64, ascending from 0 to the text's length) plus bytes; a record's sequence and structure share their offsets.
 * Line i of the feature file owns records 2 i (precusor_1) and 2 i + 1 (precusor_2) and miRNA i (its stableClusterSeq,
 * transcribed).  Candidates live in four slots a line: candidate c = 4 i + k.  Every DEVICE call synchronises and takes
 * mrg_predict_screen_temp_bytes(n_cand) bytes of scratch; arrays that contradict each other are MRG_ERR_ARG.
 *
 *   mrg_predict_screen_candidates  d_line_group [n_lines]: the lines' groups; d_nb_flags / d_nb_up / d_nb_down [n_groups] as
 *       mrg_predict_feature_neighbors left them (a `None` distance counts as 10000).  Not Good: the line's own two records,
 *       its own miRNA.  Good, with up = 9 <= upstreamDistance <= 44 and down likewise: down only -- records 2 i + 1, 2 i + 2,
 *       miRNAs (i, i + 1); both -- 2 i - 1 .. 2 i + 2, miRNAs (i, i - 1) for the first two and (i, i + 1) for the others; up
 *       only -- 2 i - 1, 2 i, miRNAs (i, i - 1).  d_cand_n [n_lines] = 2 or 4; d_cand_rec [4 n_lines] (0xffffffff: unused
 *       slot); d_cand_mir [8 n_lines] (0xffffffff: no second miRNA).  Where the reference dies of an IndexError (neither, or a
 *       neighbour before the first or behind the last line): MRG_ERR_ARG naming the line.
 *   mrg_predict_screen_prune  One wave per candidate: getPrunedPrecusor up to its fold.  d_status [n_cand]: 0 = None, 1 = cut,
 *       2 = left to the caller (a record beyond 256 or a miRNA beyond 255 characters), 3 = unused slot; d_lo / d_hi: the slice
 *       of the record (Python's slice semantics); d_pruned_off [n_cand + 1] and d_pruned (room for pruned_cap bytes): the
 *       slices' bytes, compacted; *pruned_len = their sum.  MRG_ERR_ARG naming the candidate for brackets that do not balance
 *       or an absent miRNA two or more longer than its record (the reference's IndexError).
 *   mrg_predict_screen_features  One wave per candidate with d_status 1, from the pruned sequence and its new structure
 *       (d_p_off [n_cand + 1], d_p_seq, d_p_str): d_feat [n_cand][16] int32 = state (0 the all-None row; 1 computed; 2 left
 *       to the caller: beyond 256 characters, or 10 or more stems or hairpins), hairpinCount, bindingCount,
 *       interiorLoopCount, the first miRNA's arm (0 loop, 1 arm5, 2 arm3, 3 unmatchedRegion), apicalLoopSize, its overlap and
 *       distanceToLoop, the second miRNA's arm (-1: none), overlap and distance, stemLen, the UGU flag, the brackets in the
 *       first miRNA's stretch, that stretch's length, the stems.  MRG_ERR_ARG naming the record for brackets that do not
 *       balance or a hairpin loop under 3.
 *   mrg_predict_screen_select  One lane per line: selcteOptimalPrecusor with `threshold` over the candidates of state 1 -- the
 *       retained ones, otherwise all; the lowest d_rec_mfe [n_rec] of the candidate's record, ties to the lower slot.  d_best
 *       [n_lines] = the slot or -1.  A row of state 2 is MRG_ERR_ARG: the caller fills those in first.
 *   mrg_read_str_file  HOST: RNAfold's output, three lines a record, into *handle: sequence, structure (the third line's
 *       first field) and the energy as the reference parses `(-12.30)` / `( -2.30)`, 0.0 where that fails.  MRG_ERR_ARG naming
 *       both counts when the records are not `expected`.  mrg_str_file_copy copies out off [n_rec + 1], seq and structure
 *       [text_len], mfe [n_rec]; mrg_str_file_free releases the handle.
 *   mrg_write_pruned_fasta  HOST: `>c<k>` and string k for every k with keep[k] != 0.
 *   mrg_write_screened_features  HOST: `<table>_features_updated_stableClusterSeq_15.tsv`: every line of the feature file
 *       stripped as line.strip() does, a tab, and the chosen candidate's 14 columns (best [n_lines], feat [4 n_lines][16],
 *       p_off [4 n_lines + 1] into p_seq / p_str, p_mfe [4 n_lines]) in the reference's format, or 14 x None.  Checked before
 *       the file is opened.  Worker threads: MIRGE_AMD_TABLE_THREADS.
 */
int mrg_predict_screen_temp_bytes(uint64_t n_cand, uint64_t *bytes);
int mrg_predict_screen_candidates(mrg_ctx *ctx, uint64_t n_lines, const uint32_t *d_line_group, uint64_t n_groups,
                                  const uint8_t *d_nb_flags, const int64_t *d_nb_up, const int64_t *d_nb_down,
                                  uint8_t *d_cand_n, uint32_t *d_cand_rec, uint32_t *d_cand_mir, void *d_tmp,
                                  uint64_t tmp_bytes, void *stream);
int mrg_predict_screen_prune(mrg_ctx *ctx, uint64_t n_cand, const uint32_t *d_cand_rec, const uint32_t *d_cand_mir,
                             uint64_t n_rec, const uint64_t *d_rec_off, const char *d_seq, const char *d_str, uint64_t seq_len,
                             uint64_t n_mir, const uint64_t *d_mir_off, const char *d_mir, uint64_t mir_len,
                             int32_t pruned_length, uint8_t *d_status, uint32_t *d_lo, uint32_t *d_hi, uint64_t *d_pruned_off,
                             char *d_pruned, uint64_t pruned_cap, uint64_t *pruned_len, void *d_tmp, uint64_t tmp_bytes,
                             void *stream);
int mrg_predict_screen_features(mrg_ctx *ctx, uint64_t n_cand, const uint8_t *d_status, const uint32_t *d_cand_mir,
                                const uint64_t *d_p_off, const char *d_p_seq, const char *d_p_str, uint64_t p_len,
                                uint64_t n_mir, const uint64_t *d_mir_off, const char *d_mir, uint64_t mir_len, int32_t *d_feat,
                                void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_predict_screen_select(mrg_ctx *ctx, uint64_t n_lines, const uint8_t *d_cand_n, const uint32_t *d_cand_rec,
                              uint64_t n_rec, const double *d_rec_mfe, const int32_t *d_feat, int32_t threshold,
                              int32_t *d_best, void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_read_str_file(const char *path, uint64_t expected, uint64_t *n_rec, uint64_t *text_len, void **handle);
int mrg_str_file_copy(void *handle, uint64_t *off, char *seq, char *structure, double *mfe);
void mrg_str_file_free(void *handle);
int mrg_write_pruned_fasta(const char *path, uint64_t n, const uint64_t *off, const char *seq, const uint8_t *keep,
                           uint64_t *written);
int mrg_write_screened_features(const char *features_path, const char *out_path, uint64_t n_lines, const int32_t *best,
                                const int32_t *feat, const uint64_t *p_off, const char *p_seq, const char *p_str,
                                const double *p_mfe, uint64_t *written);

/* Predict mode's classification (reference miRge2.0.py:647-648: utils/preprocess_featureFiles.py and utils/model_predict.py;
 * csrc/predict_svm.hip, csrc/predict_model_write.cpp; the rule: tests/predict_model_model.py).  The model's
 * arrays are the caller's (mirge_amd/svm_model.py reads them from the user's model file); everything is float64.
 *
 *   mrg_predict_model_filter  HOST: the screened table into the reference's three filter files, byte for byte -- dataset_path
 *       (`<tmp>.csv`: columns [0, 1, 5] + [10..]; rows with readCountSum >= 10, seqCount >= 3 and no cell from seqCount on
 *       that equals N), refined_tmp_path (rows whose pruned_precusor_str is not None) and refined_path (the columns `namelist`
 *       names, one a line) -- and into *handle: the refined rows' three leading cells and their raw feature rows [n][nf] for
 *       `features` (the model's selected names in its order, one a line; nf of them).  A selected name is a column in which
 *       every retained cell is a number; else `<column>_<value>` of a column that is not (1 where the cell equals the value);
 *       else 0 for every row.  counts [4]: the table's rows, the first filter's, the second's, and the selected names whose
 *       own column holds a cell that is no number (0 for every row, as pandas' get_dummies makes them).  A table without a
 *       header line, without the columns the filters name, or with a count that is no whole number is MRG_ERR_ARG; nothing is
 *       written then.  A table without retained rows gives header-only files (the reference raises there).
 *   mrg_predict_model_rows  copies the feature rows [n][nf] out of the handle.
 *   mrg_predict_svm  DEVICE, asynchronous on `stream`, no scratch: one lane per row of d_x [n_rows][nf] (raw rows).  The row is
 *       standardised ((x - d_mean) / d_scale, [nf]); the decision value is the sum of d_coef[i] exp(-gamma |z - d_sv[i]|^2)
 *       over the support vectors d_sv [n_sv][nf] IN THEIR STORED ORDER, each distance in the (z - sv)^2 form, plus intercept
 *       (sklearn's decision_function).  d_pred [n_rows] int8 = -1 where it is negative, else 1; d_dec [n_rows]; d_prob
 *       [n_rows][2] = libsvm's svm_predict_probability for the classes (-1, 1): sigmoid_predict with prob_a / prob_b, the clip
 *       to [1e-7, 1 - 1e-7] and multiclass_probability (eps 0.005 / 2, at most 100 rounds) per row.  No atomics: a row's
 *       results depend on the row and the model alone.  1 <= nf <= 64, n_sv >= 1, n_rows < 2^31; n_rows = 0 launches nothing.
 *   mrg_predict_model_write  HOST: detailed_path (`predictedValue,probability,` and the three leading columns: 1 or -1, the
 *       larger of the row's two probabilities as Python's repr prints it, the cells as text) and novel_path (the rows
 *       predicted 1 with a probability of at least 0.8, by (probability, line) descending).  pred [n], prob [n][2] on the
 *       host.  *predicted = rows predicted 1, *kept = rows of the novel list.  Worker threads: MIRGE_AMD_TABLE_THREADS.
 *   mrg_predict_model_free  releases the handle.
 *   mrg_format_repr  Python's repr of a double (the shortest digits that read back) into buf [cap], NUL-terminated.
 */
int mrg_predict_model_filter(const char *table_path, const char *dataset_path, const char *refined_tmp_path,
                             const char *refined_path, const char *namelist, const char *features, uint32_t nf,
                             uint64_t *counts, void **handle);
int mrg_predict_model_rows(void *handle, double *x);
int mrg_predict_svm(mrg_ctx *ctx, uint64_t n_rows, const double *d_x, uint32_t nf, const double *d_mean, const double *d_scale,
                    const double *d_sv, const double *d_coef, uint64_t n_sv, double intercept, double gamma, double prob_a,
                    double prob_b, int8_t *d_pred, double *d_dec, double *d_prob, void *stream);
int mrg_predict_model_write(void *handle, const int8_t *pred, const double *prob, const char *detailed_path,
                            const char *novel_path, uint64_t *predicted, uint64_t *kept);
void mrg_predict_model_free(void *handle);
int mrg_format_repr(double v, char *buf, uint32_t cap);

/* Predict mode's report (reference miRge2.0.py:652, utils/write_novel_report.py, without its drawing; csrc/predict_report.hip,
 * csrc/predict_report_write.cpp; the rule: tests/predict_report_model.py).
 *
 *   mrg_predict_report_read  HOST: the novel list (columns probability and clusterName; a name's first line counts), the
 *       screened table and the cluster file into *handle.  counts [3]: table lines, listed names, read rows.  Headers without
 *       the columns the report names, a line with fewer cells than the header, a clusterName that is not
 *       `<sample>:<cluster>:<chr>:<start>_<end><+|->` or repeated, a count that is no whole number and a listed name the table
 *       lacks are MRG_ERR_ARG.
 *   mrg_predict_report_array  a pointer into the handle (valid until mrg_predict_report_free) and its bytes, `which` one of
 *       MRG_REPORT_*: per line flags uint8 (1 listed, 2 pair_state Yes, 4 precursor None, arm code << 3: 0 arm5, 1 arm3, 2 loop,
 *       3 other; 32 minus strand), rank uint32 (in the novel list, 0xffffffff none), up / down int64 (INT64_MIN = None,
 *       INT64_MIN + 1 = no whole number), pos int64 [n][2] (start, end of the name), adj int32 [n][4] (head and tail dashes of
 *       alignedClusterSeq, headUnstableLength, tailUnstableLength), reads int64 (readCountSum), gid3 uint32 [n][3] (the interned
 *       group (precursor of line j - 1 / j / j + 1, chr, strand)), t_off uint64 [4 n + 1] into text (precursor, structure,
 *       clusterSeq, stableClusterSeq of every line); per block blk uint8 (0 missing, 1 read, 2 malformed), r_off uint64 [n + 1];
 *       per read row start / end / count int64, s_off uint64 [rows + 1] into the rows' text (RNA, dashes removed).
 *   mrg_predict_report_correct  DEVICE, synchronised on return, no scratch: one wave per line.  d_src [n] = the line whose
 *       precursor and structure the line ends up with (itself or a neighbour); d_state [n] = 1 touched by an offer | 2 re-typed
 *       to loop | 4 left to the host (a precursor or structure beyond 256 characters, a clusterSeq or stableClusterSeq beyond
 *       255: re-type and stable index are the caller's) | 8 precursor None | new arm code << 4; d_err [n] = where the reference
 *       raises (1 upstreamDistance no number, 2 downstreamDistance None behind an upstreamDistance above 44, 3 the last line
 *       offers downstream, 4 listed with precursor None, 8 offsets that do not ascend inside the text); d_pos_adj [n][2];
 *       d_stable_idx [n] = where the corrected precursor holds stableClusterSeq (T as U), -1 absent; d_gid [n] (0xffffffff none).
 *   mrg_predict_report_entries  DEVICE, synchronised on return: the project's radix sort over d_gid (file order inside a
 *       group), a group's chunks of two keyed by its first listed member's rank, a second sort, the three-way mature rule, the
 *       entry numbers by the project's prefix sum.  d_ent_m / d_ent_p [n] (entry e = novel_miRNA_<e + 1>: mature line,
 *       passenger line or -1), d_chunk_err / d_chunk_line [n] per visited chunk in visiting order (5 the chosen mature is not
 *       listed and not loop, 6 a stable sequence absent, 7 no block), d_row_off / d_prof_off [n + 1] (the entries' read rows and
 *       precursor lengths summed).  totals [3]: entries, rows, profile words.  Scratch: mrg_predict_report_temp_bytes(n_lines).
 *   mrg_predict_report_profile  DEVICE, synchronised on return, no scratch: one wave per entry; d_lead / d_trail [rows] (the
 *       dashes on either side of every padded row, never negative), d_prof [profile words] (per precursor position the summed
 *       count of the rows whose padded character there equals the precursor's; uint64), d_total [entries], d_flag [entries]
 *       (1 ragged: a padded row's length is not the precursor's; 2 left to the host: a precursor beyond 256, a read beyond 255
 *       or more than 65535 dashes on one side; 4 arrays that contradict each other).
 *   mrg_predict_report_write  HOST: `_corrected.tsv` and `_novel_miRNAs_report.csv` byte for byte as the reference writes
 *       them, and `_novel_miRNAs_report_profiles.tsv` (per entry `>novel_miRNA_<i>\t<L>\t<total>\t<rows>\t<ragged>`, the
 *       precursor, the structure, L sums, then `<padded row>\t<count>` for the mature's and the passenger's rows).  Worker
 *       threads: MIRGE_AMD_TABLE_THREADS.  Nothing is written when the arrays contradict the handle.
 *   mrg_predict_report_free  releases the handle.
 */
enum {
  MRG_REPORT_FLAGS = 0, MRG_REPORT_RANK, MRG_REPORT_UP, MRG_REPORT_DOWN, MRG_REPORT_POS, MRG_REPORT_ADJ, MRG_REPORT_READS,
  MRG_REPORT_GID3, MRG_REPORT_T_OFF, MRG_REPORT_TEXT, MRG_REPORT_BLK, MRG_REPORT_R_OFF, MRG_REPORT_ROW_START, MRG_REPORT_ROW_END,
  MRG_REPORT_ROW_COUNT, MRG_REPORT_ROW_SOFF, MRG_REPORT_ROW_TEXT
};
int mrg_predict_report_read(const char *novel_path, const char *table_path, const char *cluster_path, uint64_t *counts,
                            void **handle);
int mrg_predict_report_array(void *handle, uint32_t which, const void **data, uint64_t *bytes);
int mrg_predict_report_temp_bytes(uint64_t n_lines, uint64_t *bytes);
int mrg_predict_report_correct(mrg_ctx *ctx, uint64_t n_lines, const uint8_t *d_flags, const int64_t *d_up, const int64_t *d_down,
                               const int64_t *d_pos, const int32_t *d_adj, const uint32_t *d_gid3, const uint64_t *d_t_off,
                               const char *d_text, uint64_t text_len, uint32_t *d_src, uint8_t *d_state, uint8_t *d_err,
                               int64_t *d_pos_adj, int32_t *d_stable_idx, uint32_t *d_gid, void *stream);
int mrg_predict_report_entries(mrg_ctx *ctx, uint64_t n_lines, const uint8_t *d_flags, const uint32_t *d_rank,
                               const int64_t *d_reads, const uint64_t *d_t_off, const uint32_t *d_src, const uint8_t *d_state,
                               const int32_t *d_stable_idx, const uint32_t *d_gid, const uint8_t *d_blk, const uint64_t *d_r_off,
                               uint32_t *d_ent_m, int32_t *d_ent_p, uint8_t *d_chunk_err, uint32_t *d_chunk_line,
                               uint64_t *d_row_off, uint64_t *d_prof_off, uint64_t *totals, void *d_tmp, uint64_t tmp_bytes,
                               void *stream);
int mrg_predict_report_profile(mrg_ctx *ctx, uint64_t n_lines, const uint8_t *d_flags, const uint64_t *d_t_off, const char *d_text,
                               uint64_t text_len, const uint32_t *d_src, const int64_t *d_pos_adj, const int32_t *d_stable_idx,
                               const uint64_t *d_r_off, uint64_t n_rows, const int64_t *d_row_start, const int64_t *d_row_end,
                               const int64_t *d_row_count, const uint64_t *d_row_soff, const char *d_row_text,
                               uint64_t row_text_len, uint64_t n_entries, const uint32_t *d_ent_m, const int32_t *d_ent_p,
                               const uint64_t *d_row_off, const uint64_t *d_prof_off, int32_t *d_lead, int32_t *d_trail,
                               uint64_t *d_prof, uint64_t *d_total, uint8_t *d_flag, void *stream);
int mrg_predict_report_write(void *handle, const uint32_t *src, const uint8_t *state, const int64_t *pos_adj, uint64_t n_entries,
                             const uint32_t *ent_m, const int32_t *ent_p, const uint64_t *row_off, const int32_t *lead,
                             const int32_t *trail, const uint64_t *prof_off, const uint64_t *prof, const uint64_t *total,
                             const uint8_t *flag, const char *corrected_path, const char *report_path, const char *profiles_path);
void mrg_predict_report_free(void *handle);

/*
 * isomirs.csv and isomirs.samples.csv (utils/writeDataToCSV.py:1090-1170, over the grouping of :588-606) from the same
 * arrays (round 6): the reads claimed by canon_pass ("exact miRNA", slot 1) and isomir_pass ("isomiR miRNA", slot 9) are
 * grouped by group_of_entry[ref_id] -- the caller's map from a miRNA library entry to its name with the ".SNP..." suffix
 * stripped (:599-600), n_groups names in group_names --, groups in the order their first read appears, a group's isomiR
 * reads in array order.  filtered[s] = the sample's mirnaReadsFiltered (the RPM divisor).  Values are formatted as Python 2's
 * str(float) and the entropies are added in the reference's order: the files equal report.write_isomir_tables' byte for
 * byte (tests/test_report_tables.py).  header1 / header2: the two header lines.  *rows = rows of isomirs.csv.
 */
int mrg_write_isomir_tables(const char *isomirs_path, const char *samples_path, const char *header1, const char *header2,
                            const uint64_t *reads, uint32_t words_per_read, uint64_t stride, const uint8_t *lens,
                            const uint64_t *nmask, uint64_t n, const int8_t *pass_id, const int32_t *ref_id,
                            const uint32_t *quant, uint32_t n_samples, int32_t canon_pass, int32_t isomir_pass,
                            const int32_t *group_of_entry, uint64_t n_entries, const char *const *group_names,
                            uint32_t n_groups, const double *filtered, uint64_t *rows);

/*
 * `annotate -gff`: the per-sample <sample>_isomiRs.gff files from the arrays, without one Python record per read.  The two
 * calls replace updateIsomiRDic / updateIsomiRDic2 with fillTerminal, analyzeAlignment, make_cigar and make_id
 * (runAnnotationPipeline.py, RAP:86-446) and the writer loop of writeDataToCSV.py (W2C:621-646); mirge_amd/isomir.py holds
 * the Python model (classify_alignment, write_isomir_gff) whose results they reproduce exactly.
 *
 * mrg_isomir_classify   DEVICE arrays of a cascade (reads [W][stride], W in {1, 2, 4, 8}; d_nmask or NULL; pass_id, ref_id,
 *                       pos) and the HOST tables of mirge_amd.isomir.entry_table, which the call uploads:
 *                         desc    int32 [n_entries][5] per miRNA library entry: first word of its precursor in text /
 *                                 nplane, bases of the precursor, m0 = first occurrence of the mature sequence in it, bases
 *                                 of the mature sequence, status (0 = ok, 1 = mature not in the precursor: the read is
 *                                 dropped, 2 = unresolvable: the Python route raises for a read on this entry);
 *                         text    the precursors, 2 bits per base as the reads, each from a word boundary;
 *                         nplane  same shape, bit 2i set = base i is no ACGT: code 0 = N (equals a read's N), code 1 = any
 *                                 other character (equals nothing).
 *                       Rows: the reads with pass_id == canon_pass in array order, then those with pass_id == isomir_pass
 *                       in array order (flags, an exclusive prefix sum and a scatter on the device).  counts[0..1] (HOST)
 *                       = the two numbers of rows.  Capacity as for mrg_list_best_fill: rows >= cap are not written, so a
 *                       call with cap = 0 (output pointers may be NULL) only counts, and counts[0] + counts[1] > cap says
 *                       that the output is truncated.  Row k: d_idx[k] = the read, d_rec[k][8] =
 *                         [0] pre_start = r0 + 1, [1] pre_end = r1 (the read at [r0, r1) on the precursor's axis: r0 =
 *                             m0 - 2 + pos, one less for the isomiR pass; either may lie outside the precursor),
 *                         [2] iso_5p value m0 - r0 (0: none), [3] iso_3p or iso_add value r1 - m1 (0: none),
 *                         [4] kind | snp << 8 | add << 16: kind 0 = dropped, 1 = ref_miRNA, 2 = isomiR, 3 = the entry is
 *                             unresolvable, 4 = ref_id / pos / length out of range; snp 0 = none, 1 = iso_snp, 2 = _seed,
 *                             3 = _central_offset, 4 = _central, 5 = central_supp; add = [3] is an iso_add,
 *                         [5] leading | trailing << 16 read bases outside the precursor (the CIGAR's I columns),
 *                         [6] the entry, [7] 0,
 *                       d_mask[k][ceil(32 W / 64)]: bit i = read base i differs from the PRECURSOR at r0 + i (character
 *                       equality: N equals N, a position outside the precursor equals nothing).  kernel_ms (HOST, or NULL):
 *                       the time of the classification kernel alone, between two events.  Synchronises `stream`.
 * mrg_write_isomir_gff  HOST arrays: the reads and quant [n][n_samples], idx / rec / mask [k] as above, the entries' names
 *                       and precursor names.  Writes paths[s] for every sample: the four header lines (source; coldata[s]),
 *                       then one line per row with quant[idx][s] >= 1 and kind 1 or 2, in row order (kind 0 is skipped, any
 *                       other is MRG_ERR_ARG).  rows[s] (or NULL) = lines of sample s.  Blocks are formatted by worker
 *                       threads (MIRGE_AMD_TABLE_THREADS, as for the other writers; MIRGE_AMD_GFF_BLOCK_ROWS = rows per block,
 *                       default 32768, lowered by tests so that small inputs span several blocks); the bytes depend on neither.
 */
int mrg_isomir_classify(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read, uint64_t stride,
                        const uint8_t *d_lens, const uint64_t *d_nmask, uint64_t n, const int8_t *d_pass_id,
                        const int32_t *d_ref_id, const int32_t *d_pos, int32_t canon_pass, int32_t isomir_pass,
                        const int32_t *desc, uint64_t n_entries, const uint64_t *text, const uint64_t *nplane,
                        uint64_t text_words, uint64_t cap, uint32_t *d_idx, int32_t *d_rec, uint64_t *d_mask,
                        uint64_t *counts, float *kernel_ms, void *stream);
int mrg_write_isomir_gff(const char *const *paths, const char *const *coldata, uint32_t n_samples, const char *source,
                         const uint64_t *reads, uint32_t words_per_read, uint64_t stride, const uint8_t *lens,
                         const uint64_t *nmask, uint64_t n, const uint32_t *quant, const uint32_t *idx, const int32_t *rec,
                         const uint64_t *mask, uint64_t k, const char *const *entry_names, const char *const *pre_names,
                         uint64_t n_entries, uint64_t *rows);

/*
 * `annotate -trf`: tRFs.potential.report.tsv, discarded.reads.summary.assigningtRFs.csv, tRF.Counts.csv and tRF.RP100K.csv
 * from the arrays, without one Python record per read.  The two calls replace updatetrfContentDic2/3 with trfTypes
 * (runAnnotationPipeline.py, RAP:448-541) over the `-a --best --strata` listings and the first part of writeDataToCSV's
 * `if trf_output:` block with assign_cluster / getDistance2 (W2C:353-392, :546-564, :648-800); mirge_amd/trf.py holds the
 * Python model (collect_trf_content, write_trf_tables with choose = min) whose results they reproduce exactly.
 *
 * mrg_trf_classify      DEVICE arrays of a cascade (reads [W][stride], W in {1, 2, 4, 8}; d_nmask or NULL; pass_id), the two
 *                       tRNA libraries of the context and the HOST tables of mirge_amd.trf.entry_tables, which the call
 *                       uploads:
 *                         desc      int32 [n_entries][8] per entry of mature_lib, then of pre_lib: template length (-1: the
 *                                   Python lookup raises), len(trnaStruDic[name]["seq"]), anticodonStart - 1, flags (bit 0:
 *                                   "pre_" in name, bit 1: trfTypes raises), rank of the de-duplicated name in Python string
 *                                   order, the entry of the same library with that name (or -1), first and number of its
 *                                   predefined tRFs;
 *                         clusters  int32 [n_clusters][6] per predefined tRF: coordinate() of its dashed string (1-based
 *                                   first and last non-dash position), the string's length, its first word in text / plane,
 *                                   rank of the cluster name, index into trfMergedList (-1: none);
 *                         text      the dashed strings, 2 bits per character as the reads, each from a word boundary;
 *                         plane     same shape, bit 2i set = character i is no ACGT (code 0 = N, which equals a read's N,
 *                                   code 1 = any other character, which equals nothing), bit 2i + 1 set = it is a dash.
 *                       Rows: the reads with pass_id == mature_pass in array order, then those with pass_id ==
 *                       trailer_pass in array order (flags, an exclusive prefix sum and a scatter on the device), gathered
 *                       into two read sets on the device -- a trailer read without its trailing T's, or empty when fewer
 *                       than 3 T's would be cut or fewer than 11 nt left -- and listed with mrg_list_best_count / _fill: -v 1
 *                       against mature_lib, -v 0 against pre_lib.  The alignments are sorted by (row, entry, offset); the
 *                       lowest offset of each (row, entry) is kept.  counts[0..1] (HOST) = the two numbers of rows,
 *                       counts[2] = kept alignments of the rows processed.  Capacity as for mrg_list_best_fill: rows >=
 *                       cap_rows are neither listed nor written, kept alignments >= cap_hits are not written (the rows'
 *                       records are complete all the same), so a call with cap_rows = 0 (output pointers may be NULL) only
 *                       counts the rows.  Kept alignment j: d_hits[j][4] = entry (pre_lib's entries behind mature_lib's),
 *                       start (0-based), end = start + length - 1 - T tail, type (0 tRF-1, 1 tRF-whole, 2 5'-half, 3 5'-tRF,
 *                       4 3'-half, 5 3'-tRF, 6 i-tRF, 7 = trfTypes raises for the entry, 8 = entry / offset out of range).
 *                       Row r: d_rec[r][12] =
 *                         [0] the read, [1] the selected tRNA's entry (the smallest de-duplicated name among the read's
 *                             alignments; -1: none), [2] [3] [4] start, end and type of its alignment,
 *                         [5] the nearest predefined tRF by (get_distance2, name) or -1, [6] that distance (100: none),
 *                         [7] kind: 0 = assigned (distance <= 8), 1 = "Undef", 2 = "Dele" (the tRNA has no predefined
 *                             tRFs), 3 = unresolvable (the Python route raises: the de-duplicated name is no alignment of
 *                             the read, or a table lacks it), 4 = out of range (also a trailer read strip_poly_t rejects),
 *                             5 = no alignment,
 *                         [8] [9] first and number of the read's kept alignments (ascending entry), [10] its T tail, [11] 0.
 *                       kernel_ms (HOST float[2], or NULL): the times of trf_type_kernel and trf_assign_kernel alone, between
 *                       events.  Synchronises `stream`.
 * mrg_write_trf_tables  HOST arrays: the reads and quant [n][n_samples], rec [k] IN THE ORDER OF THE TSV (mature rows, then
 *                       the trailer rows grouped by stripped sequence: mirge_amd.trf.row_order), hits [h], desc and clusters
 *                       as above, per entry its name, aaType and anticodon (NULL where trnaAAanticodonDic lacks the name),
 *                       trfMergedList, denom[s] = maturetrnaReads + pretrnaReads of sample s.  paths[0..3] = the tsv, the
 *                       discarded-reads summary, tRF.Counts.csv, tRF.RP100K.csv.  A row of kind 5 is skipped, one of kind
 *                       3 or 4 (or one whose tables lack a name it needs) is MRG_ERR_ARG.  *rows (or NULL) = lines of the
 *                       tsv.  Blocks are formatted by worker threads (MIRGE_AMD_TABLE_THREADS; MIRGE_AMD_TRF_BLOCK_ROWS = rows
 *                       per block, default 16384, lowered by tests); the per-entity sums are added sequentially in row order
 *                       from the RP100K values re-read from their 3-decimal text; the bytes depend on neither setting.
 */
int mrg_trf_classify(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t *d_lens,
                     const uint64_t *d_nmask, uint64_t n, const int8_t *d_pass_id, int32_t mature_pass, int32_t trailer_pass,
                     int32_t mature_lib, int32_t pre_lib, const int32_t *desc, uint64_t n_entries, const int32_t *clusters,
                     uint64_t n_clusters, const uint64_t *text, const uint64_t *plane, uint64_t text_words, uint64_t cap_rows,
                     uint64_t cap_hits, int32_t *d_rec, int32_t *d_hits, uint64_t *counts, float *kernel_ms, void *stream);
int mrg_write_trf_tables(const char *const *paths, const char *const *samples, uint32_t n_samples, const uint64_t *denom,
                         const uint64_t *reads, uint32_t words_per_read, uint64_t stride, const uint8_t *lens,
                         const uint64_t *nmask, uint64_t n, const uint32_t *quant, const int32_t *rec, uint64_t k,
                         const int32_t *hits, uint64_t h, const int32_t *desc, const char *const *entry_names,
                         const char *const *aa_types, const char *const *anticodons, uint64_t n_entries,
                         const int32_t *clusters, uint64_t n_clusters, const char *const *merged_names, uint64_t n_merged,
                         uint64_t *rows);

/*
 * `annotate -trf`: the (sample, tRNA) blocks of tRFs.samples.tmp/ (W2C:802-874) from the arrays, without one Python object
 * per read: from the rows of mrg_trf_classify to the row arrays mrg_trf_rho takes, and the two report files of every sample.
 * mirge_amd/trf_samples.py holds the Python model (sample_trf_dic, sample_reports, load_data_new, Group, layout) whose
 * results they reproduce exactly.
 *
 * An ITEM is a pair (tsv row r, sample s) with kind <= 2 and quant[read][s] > 0; its block is (s, name of the selected
 * entry); it is a PRINTED ROW when start + length of the whole read <= the template's length (the others overhang: they
 * count in the block's sums only).  Blocks of a sample go by read count sum descending, then name descending; the printed
 * rows of a block by (count, start, read) descending, the read as a Python string.  A GROUP is a block with a printed row;
 * the k-th group of a sample is paired with the name of the sample's k-th block (load_data_new skips empty blocks).
 *
 * mrg_trf_rp100k_text    HOST: float("%.3f" % round(x, 3)) of x = 100000.0 * count / denom (0.0 for denom == 0), the RP100K
 *                        the density peaks see (load_data_new re-reads the report), computed in integers: x = m * 2^e, k =
 *                        m * 1000 * 2^e rounded to nearest, ties to even; the value is k / 1000.0.  The same function runs
 *                        on the device.
 * mrg_trf_sample_groups  DEVICE arrays: the reads [W][stride] (W in {1, 2, 4, 8}), d_lens, d_nmask or NULL, d_quant
 *                        [n][n_samples], d_rec [k][12] IN THE ORDER OF THE TSV.  HOST: denom[n_samples], entries int32
 *                        [n_entries][4] (mirge_amd.trf.sample_tables: rank of the entry's name among the distinct names in
 *                        Python string order, template length or -1, flags: bit 0 = "pre_" in name, bit 1 = "pre" in name,
 *                        0), n_names.  The call uploads the tables and validates them first (MRG_ERR_ARG).
 *                        Stages: flags of the printed rows, 64-bit atomic sums / printed counts / lowest entry per (sample,
 *                        name) cell, exclusive prefix sum and scatter; the dense cell tables are downloaded and ordered into
 *                        blocks ON THE HOST (n_samples x n_names cells, at most 2^22: MRG_ERR_ARG beyond; k x n_samples
 *                        must stay below 2^31, so that a row number fits the int32 block table); the rank of every selected read in Python string order by stable radix
 *                        sorts over 21-base chunks, last chunk first (3 bits per base: end 0, A 1, C 2, G 3, N 4, T 5), as
 *                        many as the longest selected read needs; the printed rows by two stable sorts, (start, read
 *                        rank) then (block, count); one lane per printed row writes the layout.
 *                        counts (HOST uint64[8]) = items, blocks, groups, printed rows, max_len (the longest template
 *                        among the groups, at least 1), 1 if a printed row holds an N, the first tsv row of an item whose
 *                        entry has no template (0xFFFFFFFF: none), the longest selected read.  A call with cap_blocks = 0
 *                        only counts (output pointers may be NULL).  A filling call needs cap_blocks >= blocks and
 *                        cap_rows >= printed rows, and is MRG_ERR_ARG when an item has no template or max_len > 255.
 *                        It writes, HOST: blocks int32 [B][6] = sample, representative entry, first and number of printed
 *                        rows, group or -1, 0; block_sums uint64 [B]; off uint32 [G + 1] (row offsets of the groups);
 *                        groups int32 [G][2] = its block, the block whose name it is paired with.  DEVICE, as mrg_trf_rho
 *                        takes them with row stride cap_rows: d_codes / d_nmask_out [ceil(max_len / 32)][cap_rows] (the
 *                        read shifted by `start` bases into the template frame, zeros elsewhere; d_nmask_out is written
 *                        only when counts[5] is set), d_span = (start + 1) | (start + length) << 8, d_rpm = the text value
 *                        above, d_rows uint32 [rows][3] = tsv row, count, type.  kernel_ms (HOST float[4], or NULL): items,
 *                        read order, row order, pack, between events.  Synchronises `stream`.
 * mrg_trf_rank           d_rank[off[g] + p] = the group-local row at position p of the stable sort of -rho within group g:
 *                        one radix sort of (group << 32 | ~bits of rho) over all rows (rho >= 0: the bit pattern is
 *                        monotone).  What mrg_trf_delta takes as d_rank.  off on the HOST.  Synchronises `stream`.
 * mrg_write_trf_sample_reports  HOST arrays: the reads, quant, rec and the tables as above, per entry its name, template and
 *                        aaType (NULL where a table lacks it; needed for representative entries only), the blocks, their
 *                        sums and the printed rows of mrg_trf_sample_groups.  paths[2 s] = <sample>.potential_tRFs.report,
 *                        paths[2 s + 1] = <sample>.potential_tRFs.summary.report.  A block's RP100K sum is added over the
 *                        tsv rows in order, overhanging items included; the summary in print order, from the exact RP100K.
 *                        Tables that contradict each other are MRG_ERR_ARG.  Runs of blocks are formatted by worker threads
 *                        (MIRGE_AMD_TABLE_THREADS; MIRGE_AMD_TRF_SAMPLE_BLOCK_ROWS = lines per run, default 16384, lowered
 *                        by tests); the bytes depend on neither setting.
 */
double mrg_trf_rp100k_text(uint64_t count, uint64_t denom);
int mrg_trf_sample_groups(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t *d_lens,
                          const uint64_t *d_nmask, uint64_t n, const uint32_t *d_quant, uint32_t n_samples, const int32_t *d_rec,
                          uint64_t k, const uint64_t *denom, const int32_t *entries, uint64_t n_entries, uint32_t n_names,
                          uint64_t cap_blocks, uint64_t cap_rows, int32_t *blocks, uint64_t *block_sums, uint32_t *off,
                          int32_t *groups, uint64_t *d_codes, uint64_t *d_nmask_out, uint16_t *d_span, double *d_rpm,
                          uint32_t *d_rows, uint64_t *counts, float *kernel_ms, void *stream);
int mrg_trf_rank(mrg_ctx *ctx, const uint32_t *off, uint32_t n_groups, const float *d_rho, uint32_t *d_rank, void *stream);
int mrg_write_trf_sample_reports(const char *const *paths, uint32_t n_samples, const uint64_t *denom, const uint64_t *reads,
                                 uint32_t words_per_read, uint64_t stride, const uint8_t *lens, const uint64_t *nmask, uint64_t n,
                                 const uint32_t *quant, const int32_t *rec, uint64_t k, const int32_t *entries,
                                 const char *const *entry_names, const char *const *templates, const char *const *aa_types,
                                 uint64_t n_entries, uint32_t n_names, const int32_t *blocks, const uint64_t *block_sums,
                                 uint64_t n_blocks, const uint32_t *rows, uint64_t n_rows);

/*
 * `annotate -tcf`: <sample>.trim.collapse.fa from the arrays.  The file holds every distinct read of the sample as
 * ">seq<i>_<count>\n<sequence>\n", i = 1.., by count and then by sequence, both descending (quantReads.py:26-44:
 * sorted((count, seq)) reversed); the sequence compares as a Python string: A < C < G < N < T, a proper prefix first.
 * DESIGN.md 8.9 holds the argument.
 *
 * mrg_collapsed_order_temp_bytes  HOST: the bytes of device scratch mrg_seq_rank (*rank_bytes) and mrg_collapsed_order
 *                       (*order_bytes) need for n reads (n < 2^31).
 * mrg_seq_rank          DEVICE arrays: the reads [W][stride] (W in {1, 2, 4, 8}), d_lens, d_nmask or NULL.  d_rank[u] = the
 *                       position of read u among the n reads in ascending string order (equal reads in either order: the
 *                       ranks are a permutation of 0 .. n - 1 all the same).  max_len <= min(255, 32 W) bounds the lengths:
 *                       a longer read is MRG_ERR_ARG (found on the device; d_rank is then undefined).  Stable radix sorts of
 *                       (key, read) over ceil(max_len / 21) chunks of 21 bases, the last chunk first (at least one), each
 *                       over the 3 x (bases of the chunk below max_len) bits it can occupy: 3 bits per base, end of read 0,
 *                       A 1, C 2, G 3, N 4, T 5, first base highest.  The number of launches depends on max_len and n only.
 *                       Bits of the words and of the mask at and beyond a read's length are not looked at.  n == 0 and null
 *                       pointers are MRG_ERR_ARG.  d_tmp: *rank_bytes bytes, 8-byte aligned.  Synchronises `stream`.
 * mrg_collapsed_order   DEVICE: d_quant [n][n_samples], d_rank of mrg_seq_rank.  d_order[j], j < *rows, = the read at line
 *                       pair j of sample `sample`: the reads with a count there by (count, rank) descending; *rows (HOST) =
 *                       their number, also when cap < *rows, which is MRG_ERR_ARG and writes no row.  Flags, exclusive prefix
 *                       sum, scatter of count << bits(n - 1) | rank, one radix sort over those bits and the bits of the
 *                       column's largest count (any uint32), delivered backwards.  n == 0, n_samples == 0, sample >=
 *                       n_samples and null pointers are MRG_ERR_ARG.  d_tmp: *order_bytes bytes, 8-byte aligned.
 *                       Synchronises `stream`.
 * mrg_write_collapsed_fasta  HOST arrays: the reads, lens, nmask or NULL, quant, and order [k] as above; extra rows
 *                       (extra_seqs[e], extra_counts[e]), e < n_extra, by (count, sequence) descending: the reads beyond 255 nt,
 *                       which the packed arrays do not hold, merged in by the same comparison.  Returns the rows written (k +
 *                       n_extra), or a negative error: order and the extra rows are checked before the file is opened, and an
 *                       entry >= n, a read without a count in the sample, an extra row without a count or out of order is
 *                       MRG_ERR_ARG and writes nothing.
 */
int mrg_collapsed_order_temp_bytes(uint64_t n, uint64_t *rank_bytes, uint64_t *order_bytes);
int mrg_seq_rank(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t *d_lens,
                 const uint64_t *d_nmask, uint64_t n, uint32_t max_len, uint32_t *d_rank, void *d_tmp, uint64_t tmp_bytes,
                 void *stream);
int mrg_collapsed_order(mrg_ctx *ctx, const uint32_t *d_quant, uint64_t n, uint32_t n_samples, uint32_t sample,
                        const uint32_t *d_rank, uint32_t *d_order, uint64_t cap, uint64_t *rows, void *d_tmp, uint64_t tmp_bytes,
                        void *stream);
int64_t mrg_write_collapsed_fasta(const char *path, const uint64_t *reads, uint32_t words_per_read, uint64_t stride,
                                  const uint8_t *lens, const uint64_t *nmask, uint64_t n, const uint32_t *quant,
                                  uint32_t n_samples, uint32_t sample, const uint32_t *order, uint64_t k,
                                  const char *const *extra_seqs, const uint64_t *extra_counts, uint64_t n_extra);

/*
 * Predict mode's candidate reads: what the reference's utils/convert2Fasta.py makes of unmapped.csv, from the arrays
 * `annotate` holds.  With the reads in array order (the row order of unmapped.csv), total = the sum of a read's sample
 * columns and len its length, the RAW list is the unmapped reads (pass_id < 0) with total >= 1, numbered 1, 2, .. in array
 * order, and the FILTERED list those with min_len <= len <= max_len and total >= count_cutoff, numbered likewise.  The
 * files hold ">mir<number>_<count>\n<sequence>\n" per row.  DESIGN.md 8.10 holds the rules.
 *
 * mrg_predict_reads_temp_bytes  HOST: the bytes of device scratch the three device calls need for n reads (n < 2^31).
 * mrg_predict_select    DEVICE arrays: d_pass_id [n], d_lens [n], d_quant [n][n_samples].  d_total[u] = the read's total
 *                       (every read, uint64); d_raw_no[u] / d_sel_no[u] = its number in the raw / filtered list, 0 when
 *                       it is not in it; *n_raw, *n_sel (HOST) = the lengths of the lists.  One lane per read sums the
 *                       columns of a row below 16 sample columns, 16 neighbouring lanes from 16 on; a flag pass, two
 *                       exclusive prefix sums, a numbering pass.  n == 0 gives two empty lists.  n_samples == 0,
 *                       min_len > max_len, count_cutoff == 0 and null pointers are MRG_ERR_ARG.  Synchronises `stream`.
 * mrg_predict_sample_reads  DEVICE: one sample column and one list (d_no = d_raw_no with threshold 1, or d_sel_no with
 *                       threshold count_cutoff): the reads u with d_no[u] != 0 and quant[u][sample] >= threshold in array
 *                       order as rows (d_idx = u, d_num = d_no[u], d_cnt = quant[u][sample]); *rows (HOST) = their number,
 *                       also when cap < *rows, which is MRG_ERR_ARG and writes no row.
 * mrg_predict_gather    DEVICE: the reads d_idx[j], j < k, as a compact packed set: d_out_reads [W][k], d_out_lens [k],
 *                       d_out_nmask [W][k] (or NULL; zeros where d_nmask is NULL) and d_out_counts[j] = the read's count in
 *                       `sample`, or its total for sample == 0xFFFFFFFF.  An index >= n, a read longer than its words hold
 *                       or a total of 2^32 and more is MRG_ERR_ARG (found on the device; the outputs are then undefined).
 * mrg_write_predict_fasta  HOST arrays: the reads, lens, nmask or NULL, and the rows (idx, num, counts) [k] of a list;
 *                       counts are uint32 (count_bytes 4) or uint64 (8).  Extra rows (extra_seqs, extra_nums, extra_counts),
 *                       in file order after the packed rows: the reads beyond 255 nt.  Returns the rows written, or a negative
 *                       error: the whole list is checked before the file is opened, and an index >= n, a number of 0,
 *                       numbers or indices that do not increase (the extra rows' numbers continue the packed ones) are
 *                       MRG_ERR_ARG and write nothing (an I/O error, MRG_ERR_IO, is met with the file open and can leave it
 *                       truncated).  Runs of rows are formatted by worker threads
 *                       (MIRGE_AMD_TABLE_THREADS, at most 16; MIRGE_AMD_PREDICT_BLOCK_ROWS = rows per run, lowered by tests).
 * mrg_predict_read_names  HOST: the names "mir<num>_<count>" of k rows, one after the other: name j is blob[offsets[j] ..
 *                       offsets[j + 1]) (offsets [k + 1]); *blob_bytes = the bytes of all names.  blob NULL sizes the buffer;
 *                       a blob smaller than that is MRG_ERR_ARG.
 */
int mrg_predict_reads_temp_bytes(uint64_t n, uint64_t *bytes);
int mrg_predict_select(mrg_ctx *ctx, const int8_t *d_pass_id, const uint8_t *d_lens, const uint32_t *d_quant, uint64_t n,
                       uint32_t n_samples, uint32_t min_len, uint32_t max_len, uint64_t count_cutoff, uint64_t *d_total,
                       uint32_t *d_raw_no, uint32_t *d_sel_no, uint64_t *n_raw, uint64_t *n_sel, void *d_tmp,
                       uint64_t tmp_bytes, void *stream);
int mrg_predict_sample_reads(mrg_ctx *ctx, const uint32_t *d_quant, uint64_t n, uint32_t n_samples, uint32_t sample,
                             const uint32_t *d_no, uint64_t threshold, uint32_t *d_idx, uint32_t *d_num, uint32_t *d_cnt,
                             uint64_t cap, uint64_t *rows, void *d_tmp, uint64_t tmp_bytes, void *stream);
int mrg_predict_gather(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t *d_lens,
                       const uint64_t *d_nmask, uint64_t n, const uint32_t *d_quant, uint32_t n_samples, uint32_t sample,
                       const uint32_t *d_idx, uint64_t k, uint64_t *d_out_reads, uint8_t *d_out_lens, uint64_t *d_out_nmask,
                       uint32_t *d_out_counts, void *d_tmp, uint64_t tmp_bytes, void *stream);
int64_t mrg_write_predict_fasta(const char *path, const uint64_t *reads, uint32_t words_per_read, uint64_t stride,
                                const uint8_t *lens, const uint64_t *nmask, uint64_t n, const uint32_t *idx,
                                const uint32_t *num, const void *counts, uint32_t count_bytes, uint64_t k,
                                const char *const *extra_seqs, const uint64_t *extra_nums, const uint64_t *extra_counts,
                                uint64_t n_extra);
int mrg_predict_read_names(const uint32_t *num, const void *counts, uint32_t count_bytes, uint64_t k, char *blob,
                           uint64_t blob_cap, uint64_t *offsets, uint64_t *blob_bytes);

/*
 * `annotate -ai`: every read claimed by the exact-miRNA or the isomiR pass aligned to the canonical sequence of its (merged)
 * miRNA, and a2IEditing.detail.txt, from the arrays.  mirge_amd/a2i.py holds the Python model (local_pair, judge_align,
 * a2i_editing) whose results the two calls reproduce exactly; DESIGN.md 8.6 holds the argument.
 *
 * mrg_a2i_align         DEVICE arrays of a cascade (reads [W][stride], W in {1, 2, 4, 8}; d_nmask or NULL; pass_id, ref_id;
 *                       d_keep: uint8 per read, 0 = leave the read out, or NULL) and the HOST tables of
 *                       mirge_amd.a2i.target_table, which the call checks and uploads:
 *                         canon_target / isomir_target  int32 per entry of the library the pass aligns to: its target id, -1
 *                                                       = none;
 *                         target_words / target_lens    per target its sequence, 2 bits per base as the reads, and its length:
 *                                                       1..32, or 0 for a target that cannot be aligned here (no sequence,
 *                                                       more than 32 bases, a character other than ACGT).
 *                       Rows: the selected reads in array order (flags, an exclusive prefix sum and a scatter on the device).
 *                       counts[0] (HOST) = their number.  Capacity as for mrg_isomir_classify: rows >= cap are not written, a
 *                       call with cap = 0 (output pointers may be NULL) only counts.  d_idx[row] = the read; d_rec[row] =
 *                       int32 [4] (16-byte aligned):
 *                         [0] status | verdict << 8 | substring << 9 | m << 16
 *                             status 0 = simple: `localms(target, read, 2, -1, -20, -20)` lists first the ungapped frame of
 *                                        diagonal d (the best ungapped local score m > 0 ends in one cell only and every path
 *                                        with a gap scores below m);
 *                                    1 = the best ungapped score ends in several cells, 2 = a path with a gap reaches m,
 *                                    3 = m == 0, 4 = unsupported (a read of 0 or more than 32 bases, no usable target),
 *                                    5 = a row of status 1 that mrg_a2i_settle settled (below);
 *                             verdict   = judge_align on the frame; substring = the read occurs in the target
 *                         [1] d = target position - read position
 *                         [2] bit k set: k < target length - 5, target[k] == from_base and read[k - d] == to_base (codes 0..3)
 *                         [3] the target id, -1 = none
 *                       Everything but status, m and the target id is 0 unless status is 0 (or 5).  A read's N equals nothing.
 *                       *kernel_ms (or NULL) = the alignment kernel alone, from device events.  Synchronises `stream`.
 * mrg_a2i_settle        The rows of status 1 among the k rows d_idx / d_rec (DEVICE) that a filling mrg_a2i_align call wrote,
 *                       walked once more: where every path with a gap scores below m, `localms` lists first the ungapped
 *                       frame of one of the tied cells, and the row is rewritten in place as
 *                         [0] status 5 | verdict << 8 | substring << 9 | m << 16   (m as it was)
 *                         [1] d   [2] the edit mask   [3] the target id (as it was)
 *                       exactly as a row of status 0 is filled.  The cell: a best cell is eligible iff no cell above it in
 *                       the positive run of its diagonal holds m; pairwise2 passes the best score along the last row and
 *                       the last column and stops listing at the first passed-along cell X whose upper-left neighbour is a
 *                       best cell; the answer is the last eligible cell before X in (target position, read position) order
 *                       (DESIGN.md 8.6).  A row of status 1 with a gapped path that reaches m keeps every byte, as does every
 *                       row of another status, so a second call examines the rows still of status 1 and changes nothing.
 *                       Reads, lens, nmask, the HOST tables and from_base / to_base as given to mrg_a2i_align (the tables are
 *                       checked in the same way before any launch; the target of a row is the id in its record; a record
 *                       whose read or target id is out of range is left as it is).  counts (HOST, 2 values): [0] rows
 *                       examined (status 1), [1] rows settled.  *kernel_ms (or NULL) = the settling kernel alone.
 *                       Synchronises `stream`.  The arguments are checked before the context, so a machine without a device
 *                       names a bad table; a NULL context is an error (there is no host route).
 * mrg_write_a2i_detail  HOST arrays.  Block b = one (miRNA, sample): rows [block_off[b], block_off[b + 1]), the miRNA
 *                       block_group[b] (its name and canonical sequence in group_names / group_targets), block_frame[b] =
 *                       {dashes in front of the target, dashes behind it}.  Row r: the read row_read[r] of the arrays, its
 *                       count, row_flags (bit 0 = verdict, bit 1 = retained by the genome filter) and its diagonal.  Writes the
 *                       blocks as a2i_editing does; a block with block_text[b] != NULL (block_text itself may be NULL) is that
 *                       text, written as it is.  *lines (or NULL) = lines written.  Runs of blocks are formatted by worker
 *                       threads (MIRGE_AMD_TABLE_THREADS, at most 16; MIRGE_AMD_A2I_RUN_BLOCKS = blocks per run, default 256,
 *                       lowered by tests); the bytes depend on neither.
 */
int mrg_a2i_align(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t *d_lens,
                  const uint64_t *d_nmask, uint64_t n, const int8_t *d_pass_id, const int32_t *d_ref_id,
                  const uint8_t *d_keep, int32_t canon_pass, int32_t isomir_pass, const int32_t *canon_target,
                  uint64_t n_canon, const int32_t *isomir_target, uint64_t n_isomir, const uint64_t *target_words,
                  const uint8_t *target_lens, uint64_t n_targets, uint32_t from_base, uint32_t to_base, uint64_t cap,
                  uint32_t *d_idx, int32_t *d_rec, uint64_t *counts, float *kernel_ms, void *stream);
int mrg_a2i_settle(mrg_ctx *ctx, const uint64_t *d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t *d_lens,
                   const uint64_t *d_nmask, uint64_t n, const int32_t *canon_target, uint64_t n_canon,
                   const int32_t *isomir_target, uint64_t n_isomir, const uint64_t *target_words, const uint8_t *target_lens,
                   uint64_t n_targets, uint32_t from_base, uint32_t to_base, uint64_t k, const uint32_t *d_idx, int32_t *d_rec,
                   uint64_t *counts, float *kernel_ms, void *stream);
int mrg_write_a2i_detail(const char *path, const uint64_t *reads, uint32_t words_per_read, uint64_t stride,
                         const uint8_t *lens, const uint64_t *nmask, uint64_t n, uint64_t n_blocks, const uint64_t *block_off,
                         const int32_t *block_group, const int32_t *block_frame, const char *const *block_text,
                         const char *const *group_names, const char *const *group_targets, uint64_t n_groups,
                         const uint32_t *row_read, const uint32_t *row_count, const uint8_t *row_flags, const int32_t *row_d,
                         uint64_t *lines);

/*
 * -trf: density-peak clustering (Rodriguez-Laio) of the per-sample tRF reports, the O(n^2) parts of
 * utils/writeDataToCSV.py (W2C) :802-1088 for every (sample, tRNA) group of one run at once.
 * Group g owns rows [off[g], off[g+1]) (off: HOST array of n_groups + 1, off[0] = 0), in the order of its
 * block of `<sample>.potential_tRFs.report`: row k is the reference's index k + 1.  A row is its read in
 * the template frame:
 *   d_span   uint16 per row: first | last << 8, 1-based template positions;
 *   d_codes  [W][n] uint64 (W = ceil(max_len / 32)): base at position p in bits 2(p-1), 2(p-1)+1 of word
 *            (p-1) / 32, A=0 C=1 G=2 T=3 (N = 0), as the read encoding above;
 *   d_nmask  same shape, bit 2(p-1) set = N, or NULL when no row has an N.
 * max_len is the longest template of the batch, 1..255 (a longer one is MRG_ERR_ARG).  The distance of two
 * rows is getDistance's (W2C:417-449): |first_i - first_j| + |last_i - last_j| + overlapping positions whose
 * characters differ (N = N, N != base); no n^2 matrix is stored.  Each call synchronises `stream`.
 *
 * mrg_trf_rho     local_density (W2C:470-499, gaussian): d_rho[i] = float32 of the left-to-right double sum
 *                 over j != i in row order of ktab[d_ij] * d_rpm[j] (each product rounded), plus d_rpm[i];
 *                 ktab = HOST table of K[d] = exp(-(d / dc)^2) for d < n_ktab (1..256; K = 0 beyond).
 *                 d_max_dis[g] = the group's largest pairwise distance (getDistance's max_dis; 0 for one row).
 * mrg_trf_delta   min_distance (W2C:509-533): d_rank lists each group's rows (group-local, 0-based) in rank
 *                 order (d_rank[off[g] + p] = row at position p).  For the row at position p > 0: d_delta =
 *                 min(max_dis, distance to any row at a position q < p), d_nneigh = that row (group-local), of
 *                 equally near rows the one at the largest q; the top row gets -1 in both.
 * mrg_trf_border  the border densities (W2C:951-961): d_label = each row's cluster label (-1 or 1..NCLUST);
 *                 bord_off = HOST array of n_groups + 1 offsets into d_bord, NCLUST + 1 slots per group (groups
 *                 with fewer than 3 slots, NCLUST <= 1, are skipped).  d_bord[bord_off[g] + c] = max over pairs
 *                 of rows with different labels and distance <= 3 of float32 (rho_i + rho_j) / 2 with label c
 *                 among them, 0 if none; label -1 is slot NCLUST (Python's bord_rho[-1]).  d_bord is zeroed first.
 */
int mrg_trf_rho(mrg_ctx *ctx, const uint32_t *off, uint32_t n_groups, uint32_t max_len, const uint64_t *d_codes,
                const uint64_t *d_nmask, const uint16_t *d_span, const double *d_rpm, const double *ktab, uint32_t n_ktab,
                float *d_rho, uint32_t *d_max_dis, void *stream);
int mrg_trf_delta(mrg_ctx *ctx, const uint32_t *off, uint32_t n_groups, uint32_t max_len, const uint64_t *d_codes,
                  const uint64_t *d_nmask, const uint16_t *d_span, const uint32_t *d_rank, const uint32_t *d_max_dis,
                  int32_t *d_delta, int32_t *d_nneigh, void *stream);
int mrg_trf_border(mrg_ctx *ctx, const uint32_t *off, uint32_t n_groups, uint32_t max_len, const uint64_t *d_codes,
                   const uint64_t *d_nmask, const uint16_t *d_span, const float *d_rho, const int32_t *d_label,
                   const uint32_t *bord_off, float *d_bord, void *stream);

/*
 * -trf: what follows the three passes above -- cluster centres, every row's label, core and halo, and the two files that
 * list the clusters -- from the arrays (the label pass of peaks_results, cluster_text and _write_clusters of
 * mirge_amd/trf_samples.py, whose results the calls reproduce exactly).  off as above, on the HOST.
 *
 * mrg_trf_assign  d_rho, d_rank, d_delta, d_nneigh as mrg_trf_rho / mrg_trf_rank / mrg_trf_delta left them (read only).
 *                 Per group: top = d_rank[off[g]]; the top's delta counts as max(0, delta of every other row) (0 in a
 *                 one-row group) and it has no neighbour.  CENTRES are the rows with rho >= 5.0f and delta >= 8, numbered
 *                 1..NCLUST in ROW order; a group without centre whose largest delta is <= 8 and largest rho >= 5.0f takes
 *                 its first row of maximal rho as cluster 1 (W2C:895-908).  d_label[i] (int32) = the number of the first
 *                 centre on the chain i, nneigh[i], nneigh[nneigh[i]], ...; -1 when the chain ends in a top row that is no
 *                 centre.  (The reference assigns in rank order; nneigh always ranks above its row, so the result is a
 *                 function of the forest alone.)  Found by pointer doubling over the rows of all groups at once, in
 *                 ceil(log2(largest group)) + 1 rounds fixed on the host, every index checked against its group before it
 *                 is followed.  A first rank entry or a nneigh outside its group, a row that names itself, and rows still
 *                 open after the last round (a cycle) are MRG_ERR_ARG: the host arrays are left alone and d_label is zeroed
 *                 (0 is no label).  HOST outputs: nclust[n_groups]; cen_off[n_groups + 1] (cen_off[n_groups] = all centres);
 *                 centers[] = the group-local row of every centre, cluster 1 first, written when cap_centers >=
 *                 cen_off[n_groups] (a call with cap_centers = 0 only counts; off[n_groups] always suffices).
 * mrg_trf_halo    after mrg_trf_border (d_label may be passed to it as it is).  cen_off / centers as above, bord_off / d_bord
 *                 as given to and left by mrg_trf_border (groups with NCLUST > 1 need NCLUST + 1 slots), all checked on the
 *                 host first.  d_counts[i * count_stride] = the read count of row i (uint32; the d_rows of
 *                 mrg_trf_sample_groups with d_rows + 1 and stride 3).  Row i of label c >= 1 is CORE unless NCLUST > 1 and
 *                 rho[i] < d_bord[bord_off[g] + c], or its getDistance to the centre of c exceeds 8; a row of label -1 is
 *                 never core and belongs to no cluster.  d_core[i] (uint8).  tallies (HOST uint64 [cen_off[n_groups]][4], by
 *                 64-bit atomic adds) = members, core rows, read count in the core, read count in the halo of every cluster.
 *                 d_order (uint32 [n]) = the rows sorted by (group, label - 1; label -1 last), stable: a cluster's members
 *                 are contiguous and in row order.  The RP100K sums are floating point and are NOT taken here.  A label
 *                 that names no cluster of its group is MRG_ERR_ARG.
 * mrg_write_trf_cluster_reports  HOST arrays: the row layout (codes / nmask [W][stride], span, rpm, rows [n][3] = tsv row,
 *                 count, type), off, and per group its sample (ascending), the bases of its own template, the name it is
 *                 paired with, the tRNA it is reported under (the name, or "_".join(name.split("_")[1:-1]) when "pre" is in
 *                 the name), trnaStruDic[name]["seq"] and pretrnaNameSeqDic[name] (NULL where the table lacks the name);
 *                 labels, core, order, nclust, cen_off, centers, tallies as above.  paths[2 s] =
 *                 <sample>.potential_tRFs.clusters.detail, paths[2 s + 1] = <sample>.tRFs.report.tsv.  Every RP100K sum is
 *                 added in the Python's order by the one thread that owns the group; the integer tallies are added again and
 *                 compared (a mismatch, or tables that contradict each other, is MRG_ERR_ARG).  status (HOST int64[2]):
 *                 {0, 0} = written; {1, g} = the record route's KeyError, {2, g} = its IndexError (detect_mismatch on a
 *                 template shorter than the tRF) at group g: the call returns MRG_OK and has written nothing.  Runs of
 *                 groups are formatted by worker threads (MIRGE_AMD_TABLE_THREADS, at most 16;
 *                 MIRGE_AMD_TRF_SAMPLE_BLOCK_ROWS = rows per run); the bytes depend on neither.
 * mrg_py3_float_repr  Python 3's repr(value) (shortest digits that read back, ".0" on whole numbers, exponent form below
 *                 1e-4 and from 1e16) into out[cap], cap >= 32, NUL-terminated: what "+".join(str(x) ...) prints.
 */
int mrg_trf_assign(mrg_ctx *ctx, const uint32_t *off, uint32_t n_groups, const float *d_rho, const uint32_t *d_rank,
                   const int32_t *d_delta, const int32_t *d_nneigh, int32_t *d_label, uint32_t *nclust, uint64_t cap_centers,
                   uint32_t *cen_off, uint32_t *centers, void *stream);
int mrg_trf_halo(mrg_ctx *ctx, const uint32_t *off, uint32_t n_groups, uint32_t max_len, const uint64_t *d_codes,
                 const uint64_t *d_nmask, const uint16_t *d_span, const float *d_rho, const int32_t *d_label,
                 const uint32_t *d_counts, uint32_t count_stride, const uint32_t *cen_off, const uint32_t *centers,
                 const uint32_t *bord_off, const float *d_bord, uint8_t *d_core, uint32_t *d_order, uint64_t *tallies,
                 void *stream);
int mrg_write_trf_cluster_reports(const char *const *paths, uint32_t n_samples, const uint64_t *codes, const uint64_t *nmask,
                                  uint32_t max_len, uint64_t stride, const uint16_t *span, const double *rpm,
                                  const uint32_t *rows, uint64_t n_rows, const uint32_t *off, uint32_t n_groups,
                                  const int32_t *group_sample, const int32_t *group_len, const char *const *group_names,
                                  const char *const *group_keys, const char *const *group_mature,
                                  const char *const *group_trailer, const int32_t *labels, const uint8_t *core,
                                  const uint32_t *order, const uint32_t *nclust, const uint32_t *cen_off,
                                  const uint32_t *centers, const uint64_t *tallies, int64_t *status);
int mrg_py3_float_repr(double value, char *out, uint64_t cap);

/* Packing helper used by hosts without numpy: ASCII reads -> SoA words. */
int mrg_pack_reads(const char *const *seqs, uint64_t n, uint32_t words_per_read,
                   uint64_t *reads, uint8_t *lens, uint64_t *nmask, int *has_n);
/* ... and -> the ragged form of mrg_cascade_run_long.  Two calls: with words == NULL only word_off[n + 1] (and lens,
 * if given) are filled -- word_off[n] is the number of words to allocate --, then with the buffers. */
int mrg_pack_reads_ragged(const char *const *seqs, uint64_t n, uint64_t *words, uint64_t *nmask, uint64_t *word_off,
                          uint32_t *lens, int *has_n);

#ifdef __cplusplus
}
#endif
#endif /* MIRGE_AMD_H */
