// seed_kernels.h -- launch interface between seed_api.hip and seed_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/diamond_hip.h"
#include "seed_core.h"
#include "seed_chain.h"
#include "seed_slices_core.h"
#include "length_ratio_core.h"
#include "linsearch_core.h"

namespace dmnd {

static const uint64_t SEED_EMPTY = ~0ull;
static const uint32_t LIST_END = 0xffffffffu;
// head = start of the seed's query-position list in SeedArgs::qlist -- or, for a list of ONE, the query position itself;
// flags = state (low byte) | list size << 8.
// A free slot is all ones (one memset initialises the table); the state of an occupied slot is written explicitly, and no
// kernel bit-tests the state of a free slot.
// LOWC: the seed of the group's first query position is not complex (written with the lists; spaced seeds only) -- if the seed
// joins, seed_mask_kernel turns it into ERASED.
enum : uint32_t { SLOT_JOINED = 1, SLOT_ERASED = 2, SLOT_LOWC = 8 };

// One entry of the open-addressing query seed table: key, head of the list of query positions, join state -- 16 bytes, so
// that the probe of the reference stream and the pair filter touch ONE cache line per seed instead of three arrays.
struct SeedSlot { uint64_t key; uint32_t head; uint32_t flags; };

// A (joined reference position, query position) pair whose stage-2 score exceeds 255: whether it saturates depends on the
// reference's SIMD batch it would have been scored in (simd_batch_size_sorted), resolved in a second pass.
struct SeedDeferred { int64_t sloc; uint32_t slot, x; int32_t score, pad; };

// A (joined reference position sloc of the seed in `slot`, query position x) pair that passed the Hamming filter
struct SeedSurvivor { uint32_t slot, x; int64_t sloc; };

// Mutual-coverage search (length_ratio_core.h): the query positions [first, end), counted from q_begin, of the queries whose
// length passes the ratio test against one target -- one range, since both blocks are length-sorted (seed_qwin_kernel)
struct SeedQueryWindow { uint32_t first, end; };

// A survivor whose stage-2 ungapped score passed the cutoff: input of the left-most rule (seed_leftmost_kernel)
struct SeedScored { uint32_t slot, x; int64_t sloc; int32_t score, chunk; };

struct SeedArgs {
	SeedParams params;
	const int8_t* qdata; const int8_t* tdata;     // block letters (HBM)
	const int8_t* qseed; const int8_t* tseed;     // the letters seeds are generated from: the blocks, or their motif-soft-masked views
	const int64_t* qlimits;                       // query block limits (HBM)
	int64_t q_begin, q_end, t_begin, t_end;       // letter ranges [limits[0], limits[n])
	const uint32_t* qid_of;                       // query position -> query id
	// mutual-coverage search: reference block limits (HBM) and per target its window of admissible query positions; qwin = NULL: ratio off,
	// and then every launch takes the kernel instance that holds no length test at all
	const int64_t* tlimits; int64_t n_targets;
	const SeedQueryWindow* qwin;
	// linearised search (linsearch_core.h): per slot of the shape's table the smallest joined reference position (launch_seed_lin_first, one
	// array for all shapes: a shape's reduction re-initialises the slots of its own records); NULL: switch off, and then every launch takes
	// the kernel instance that holds no selection test
	int64_t* lin_first;
	uint8_t* mask_time;                          // per query letter: (shape, chunk) time of its SEED_MASK bit
	// per-shape query seed table
	SeedSlot* slots;              // 16-byte slots: key, list start (or the seed's one query position), state | list size
	int slot_shift;               // log2 of the slot stride in bytes (4). Tried and dropped in round 3: 64-byte slots carrying the folded
	                              // 48-letter window of single-position seeds, so that the fused Hamming pre-filter needs no second random
	                              // read -- the 512 MB table no longer fits the 256 MB Infinity Cache and the stream + filter kernel of C3
	                              // went from 124 to 137 ms per 16 shapes (L2 misses 3.15e8 -> 4.05e8 per launch)
	__host__ __device__ SeedSlot& slot(uint64_t i) const { return *reinterpret_cast<SeedSlot*>(reinterpret_cast<char*>(slots) + (i << slot_shift)); }
	const uint32_t* qlist;                        // query positions grouped by seed, ascending in each group (SeedSlot::head = start, count in flags >> 8)
	uint64_t slot_mask;
	int classes;                                  // 8: slots and level-1 words are partitioned by seed_class(key) (always when fused); 0: one range
	// ... and then the reference letters as the stream wants them, made once per search by seed_codes_kernel: per group of 16
	// letters (from t_begin rounded down to 16) their class nibbles, and delimiter / no-class maps (low / high 16 bits)
	const uint64_t* tcodes; const uint32_t* tflags;
	const uint64_t* tplanes;                      // the same class nibbles bit-sliced: bits [16 b, 16 b + 16) = bit b of the group's 16 nibbles (seed_classify_kernel)
	const uint16_t* tclass; int64_t tclass_stride;  // per shape (seed_classify_kernel): plane c = the valid windows of class c, 16 per entry; plane 8 (hashed seeds): the special ones
	unsigned long long* phase_ticks;              // DMND_SEED_PHASES=1: 8 counters (seed_stream_fast_kernel PHASE_MARK), else NULL
	// Layout of the query side (seed_core.h seed_order). Every key has a 32-bit order value u = seed_hash_a(key), or
	// class << 29 | a >> 3 with classes; its top slot_bits bits t are the sort key of the build (launch_seed_build), and the home
	// slot, the level-1 word and the level-2 word are all non-decreasing functions of t -- so that ONE sort of the query positions
	// by t lays out the table, the filters and the lists in the same order, and the build writes them with plain stores. Class c
	// owns the c-th eighth of the slots and of both filters. The level-1 bits stay the low bits of a, the level-2 bit comes from
	// seed_hash_b.
	int slot_bits;                                // log2(slot_mask + 1)
	uint32_t bm1_hmask;                           // bits of hash a that choose the level-1 word (bm1_hmask_of)
	int bitmap_log2;                              // log2 of the level-2 word count
	__host__ __device__ uint32_t order(uint32_t h, uint64_t key) const { return seed_order(h, key, classes); }
	// home slot of a key (hh = seed_hash(key)) and word of its level-1 bits (h = seed_hash_a(key))
	__host__ __device__ uint64_t home(uint64_t hh, uint64_t key) const { return order((uint32_t)hh, key) >> (32 - slot_bits); }
	__host__ __device__ uint32_t bm1_index(uint32_t h, uint64_t key) const { return bm1_word_of_key(h, key, classes, bm1_hmask, bitmap1_words); }
	__host__ __device__ uint32_t bm1_of_top(uint32_t t) const { return bm1_word_of_top(t, slot_bits, bitmap1_words); }
	__host__ __device__ uint32_t bm2_of_top(uint32_t t) const { return bm2_word_of_top(t, slot_bits, bitmap_log2); }
	__host__ __device__ uint32_t bm2_index(uint32_t h, uint64_t key) const { return bm2_of_top(order(h, key) >> (32 - slot_bits)); }
	// two one-hash bitmaps of the query seeds: level 1 is sized to stay resident in every XCD's 4 MB L2 (the reference
	// stream probes it once per position), level 2 (>= 16 bits per query seed) filters level-1 false positives before
	// the open-addressing table is touched
	uint32_t* bitmap1; uint32_t bitmap1_words, bitmap1_k3;      // level-1 filter (seed_core.h bm1_word / bm1_bits)
	uint32_t* bitmap;                                           // level 2: word bm2_index, bit seed_hash_b >> 27
	// joined reference positions of this shape
	uint32_t* matched_slot; int64_t* matched_loc; unsigned long long* matched_count; int64_t matched_cap;
	SeedDeferred* deferred; unsigned long long* deferred_count; int64_t deferred_cap;
	SeedSurvivor* survivors; unsigned long long* survivor_count; int64_t survivor_cap;
	SeedScored* scored; unsigned long long* scored_count;      // as many entries as survivors are scored (launch_seed_post)
	// need_bits: one bit per slot, set for the seeds that have a deferred pair (1 MB for the 10k-query table: the scan over the
	// joined positions tests it in L2 instead of reading 16-byte slots all over the table); e_key: the joined positions of those
	// seeds, sorted by (slot, position) for the second pass
	uint32_t* need_bits;
	uint64_t* e_key; unsigned long long* e_count; int64_t e_n;     // key = slot << 40 | position
	const int8_t* matrix;                         // 32x32 int8 substitution matrix (HBM) for the stage-2 ungapped window score
	// output
	dmnd_seed_hit* hits; unsigned long long* hit_count; int64_t hit_cap;
	const uint8_t* qfold;                         // fused pipeline: the query block with 4 bits per letter (letter & 15), pre-filter of the Hamming test; else NULL
	const uint8_t* tfold;                         // fused pipeline: the reference block folded the same way; else NULL
	int level2;                                   // the level-2 bitmap is filled and consulted (long seeds: shape weight >= 10)
	int fused;                                    // short-seed pipeline: seed_build_kernel decides SLOT_LOWC for every group (the stream needs it)
};

// Up to 8 byte ranges set to a byte value each by ONE kernel launch. A search used to start with six hipMemsetAsync calls and add
// four to eight per shape (table, slots-of-positions, bitmaps, mask times, need map, five counters): every one is its own
// fillBufferAligned launch on the stream, ~5 us of launch floor each even for 8 bytes (profiles/r04_kernel_stats_C2.csv: 21 fills
// per C2 step, a tenth of it).
struct SeedClear {
	void* p[8]; uint64_t bytes[8]; uint32_t value[8];
	int n = 0;
	void add(void* ptr, uint64_t nbytes, uint32_t byte_value) { if (ptr && nbytes && n < 8) { p[n] = ptr; bytes[n] = nbytes; value[n] = byte_value; ++n; } }
};
hipError_t launch_seed_clear(const SeedClear& z, hipStream_t st);
hipError_t launch_seed_qid(const int64_t* limits, int64_t n_seqs, uint32_t* qid_of, hipStream_t st);
// qwin[t] for the n_targets targets of tlimits against the n_queries length-sorted queries of qlimits (both device arrays of n + 1 limits)
hipError_t launch_seed_qwin(const int64_t* qlimits, int64_t n_queries, const int64_t* tlimits, int64_t n_targets, double min_length_ratio, SeedQueryWindow* qwin, hipStream_t st);
// the folded need map that seed_collect's workgroups keep in LDS (2^13 words = 32 KB); it lies behind SeedArgs::need_bits
enum { SEED_NEED_FOLD_WORDS = 8192 };
// query seed positions whose shape window touches a soft-masked stretch get their mask time (MaskingTable::remove's bit mask)
hipError_t launch_seed_soft_time(const SeedArgs& a, hipStream_t st);
// Builds the query side of shape sid -- table, position lists (qlist_out, which a.qlist reads) and both filters -- from ONE stable radix sort of the
// query positions by their order value's top slot_bits bits. work: seed_build_work_words(n) words; sorted_top: n
// words; the table must be all ones and the filters zero.
inline int64_t seed_build_work_words(int64_t n) { return 5 * n + 66; }
hipError_t launch_seed_build(const SeedArgs& a, int sid, uint32_t* qlist_out, uint32_t* work, uint32_t* sorted_top, void** tmp, size_t* tmp_bytes, hipStream_t st);
// fused = true (short seeds, where a third of the reference positions join): the stream kernel also runs the Hamming filter on
// every joined pair while the reference letters are at hand, and fills a.survivors; a.matched_* then only serve the deferred pass
// a table kept from an earlier search of the same query block: clears the per-reference-block marks (joined, erased) of every slot
// and, for hashed seeds, repeats the masking of the non-complex query seeds that the index kernel does at enumeration
hipError_t launch_seed_reset(const SeedArgs& a, int sid, hipStream_t st);
// letters [0, n) of a block folded to 4 bits each, two per byte (out: (n + 1) / 2 bytes)
hipError_t launch_seed_fold(const int8_t* data, int64_t n, uint8_t* out, hipStream_t st);
// class nibbles + flag maps of the reference letters [t_begin & ~15, t_end + 32) (SeedArgs::tcodes / tflags); n_groups entries each
inline int64_t seed_code_groups(int64_t t_begin, int64_t t_end) { return (t_end - (t_begin & ~(int64_t)15) + 15) / 16 + 2; }
hipError_t launch_seed_codes(const SeedParams& c, const int8_t* tseed, int64_t t_begin, int64_t t_end, uint64_t* codes, uint32_t* flags, uint64_t* planes, hipStream_t st);
hipError_t launch_seed_stream(const SeedArgs& a, int sid, hipStream_t st, bool fused = false);
bool seed_stream_can_fuse(const SeedParams& c);
// Sliced long-seed stream (seed_slices_core.h). The routing of shape sid over the class nibbles / flags of launch_seed_codes: list
// receives the seed_ref_windows window offsets (from t_begin rounded down to 16) slice by slice, ascending in each, counts (64 words)
// the windows per slice; route / route_sorted: one byte per window each, scratch. Spaced nibble-mode shapes, fewer than 2^31 windows.
hipError_t launch_seed_route(const SeedParams& c, int sid, const uint64_t* codes, const uint32_t* flags, int64_t t_begin, int64_t t_end, int slice_bits,
	uint8_t* route, uint8_t* route_sorted, uint32_t* list, uint32_t* counts, void** tmp, size_t* tmp_bytes, hipStream_t st);
// ... and beside every list entry hash a of its window's key (seed_ref_hash_entry): hashes receives seed_ref_windows words, in list order
hipError_t launch_seed_ref_hashes(const SeedParams& c, int sid, const uint64_t* codes, const uint32_t* list, int64_t t_begin, int64_t t_end, uint32_t* hashes, hipStream_t st);
// launch_seed_stream's work for a search without key classes, from that routing: the same joined positions, in another order
hipError_t launch_seed_stream_slices(const SeedArgs& a, int sid, const uint64_t* codes, const uint32_t* list, const uint32_t* hashes, const uint32_t* counts, int slice_bits, hipStream_t st);
// n_matched >= 0: the number of joined positions in a.matched_* (few of them: the kernel walks that list instead of the table)
hipError_t launch_seed_mask(const SeedArgs& a, int sid, hipStream_t st, int64_t n_matched = -1);
// Linearised search: a.lin_first[slot] = the smallest of the n_matched positions in a.matched_* that carry `slot`, in two launches
// (initialise the slots that occur, then a 64-bit minimum per record) -- whatever the order of the records. launch_seed_pairs,
// launch_seed_pairs_tiled and launch_seed_chain_shape run it in front of their filter when a.lin_first is set.
hipError_t launch_seed_lin_first(const SeedArgs& a, int64_t n_matched, hipStream_t st);
hipError_t launch_seed_pairs(const SeedArgs& a, int sid, int64_t n_matched, hipStream_t st);
hipError_t launch_seed_pairs_tiled(const SeedArgs& a, int sid, int64_t n_matched, hipStream_t st);      // a.matched_* sorted by slot; fills a.survivors
hipError_t launch_seed_count_pairs(const SeedArgs& a, int64_t n_matched, unsigned long long* out, hipStream_t st);
// clear_scored = false: the caller has zeroed a.scored_count on the stream already (launch_seed_clear)
hipError_t launch_seed_post(const SeedArgs& a, int sid, int64_t n_survivors, hipStream_t st, bool clear_scored = true);
hipError_t sort_matched_by_slot(const uint32_t* slot_in, uint32_t* slot_out, const int64_t* loc_in, int64_t* loc_out, int64_t n, int slot_bits,
	void** tmp, size_t* tmp_bytes, hipStream_t st);
hipError_t launch_seed_collect(const SeedArgs& a, int64_t n_matched, hipStream_t st);
hipError_t launch_seed_deferred(const SeedArgs& a, int sid, int64_t n_deferred, hipStream_t st);
// ascending device sort of n 64-bit keys (rocPRIM radix sort); tmp is grown as needed
hipError_t sort_keys_u64(const uint64_t* in, uint64_t* out, int64_t n, void** tmp, size_t* tmp_bytes, hipStream_t st);
// Orders the n seed hits by (query, subject, seed_offset, score) on the device: three stable radix-sort passes over an index
// permutation (keys/idx: two buffers of n uint64 / uint32 each), then one gather into `out`.
hipError_t sort_seed_hits(const dmnd_seed_hit* hits, dmnd_seed_hit* out, int64_t n, uint64_t* keys[2], uint32_t* idx[2],
	void** tmp, size_t* tmp_bytes, hipStream_t st, int query_bits, int subject_bits, int off_bits, bool equal_scores = false);      // bits of the largest query id / subject position / seed offset; equal_scores: every hit carries the same score (no ungapped filter: --fast), the pass over the scores is left out

// ---- chain mode (seed_chain.h): the launches of the non-fused search whose sizes the host does not know. Every SeedArgs here
// addresses the WHOLE shared joined-position lists (matched_cap = their capacity); shape sid owns [ctr[sid - 1], ctr[sid]).
struct SeedChain {
	unsigned long long* ctr;      // the counter block (layout: seed_chain.h)
	int S;
	int64_t matched_cap, survivor_cap, hit_cap, tiled_from;      // capacities of matched_*, seed_survivors (= seed_scored), seed_hits; joined positions of a shape from which on its pair filter is the host's
};
// behind the stream kernel of shape sid: overflow flag, start of the next shape's range; behind the last one the gate of shape 0
hipError_t launch_seed_chain_streamed(const SeedChain& ch, int sid, hipStream_t st);
hipError_t launch_seed_chain_mask(const SeedArgs& a, const SeedChain& ch, int sid, hipStream_t st);
// pair filter, scoring and left-most rule of shape sid, then its flags and the gate of the next shape
hipError_t launch_seed_chain_shape(const SeedArgs& a, const SeedChain& ch, int sid, hipStream_t st);
inline bool sort_seed_hits_one_key(int query_bits, int subject_bits, int off_bits) { return off_bits >= 1 && off_bits <= 24 && query_bits + subject_bits + off_bits <= 64; }
// sort_seed_hits for a hit count that lies in ch.ctr[S]: the rocPRIM sorts run over sort_cap entries padded with keys that sort
// last (needs sort_seed_hits_one_key; sorted = false leaves the sort out). Then `ret` receives the counter block
// (chain_ret_header_bytes) and behind it the first ret_hits sorted hits.
hipError_t launch_seed_chain_sort(const SeedChain& ch, bool sorted, const dmnd_seed_hit* hits, dmnd_seed_hit* out, int64_t sort_cap, uint64_t* keys[2], uint32_t* idx[2],
	void** tmp, size_t* tmp_bytes, hipStream_t st, int query_bits, int subject_bits, int off_bits, bool equal_scores, char* ret, int64_t ret_hits);

}  // namespace dmnd
