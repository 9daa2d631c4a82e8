// seed_chain.h -- the chain mode of the long-seed (non-fused) seed search: what the device reports and what the host does with it.
// Host arithmetic only (no HIP): shared by seed_api.hip, seed_kernels.hip and the stand-alone check tests/host/seed_chain_check.cpp.
//
// In chain mode dmnd_seed_search enqueues everything from the first clear to the sorted hits on the context's stream without a
// host wait in between; the kernels take their element counts from the counter block in device memory. What the host would have
// decided between two launches (a buffer that overflowed, deferred pairs, the tiled pair filter) the kernels record as flags in a
// status word instead; a kernel that finds a flag set that voids its input does nothing. One copy at the end brings back the
// counter block, the status word and the leading sorted hits, and the host-driven code continues from the point the flags name.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define DMND_CHAIN_HD __host__ __device__ inline
#else
#define DMND_CHAIN_HD inline
#endif

namespace dmnd {

enum : unsigned long long {
	CHAIN_MATCHED_OVER = 1,       // joined positions over the capacity of matched_*: the lists are incomplete, nothing behind the stream ran
	CHAIN_SURVIVORS_OVER = 2,     // Hamming survivors of shape `done` over the capacity of seed_survivors: its scoring did not run
	CHAIN_HITS_OVER = 4,          // hits over the capacity of seed_hits
	CHAIN_DEFERRED = 8,           // shape `done` has pairs scoring above 255: its deferred pass is the host's
	CHAIN_TILED = 16,             // shape `done` reached the tiled-filter threshold: its pair filter did not run
	CHAIN_SORT_OVER = 32          // more hits than the fixed capacity of the device-sized sort: the hits are complete but unsorted
};

// Words of the counter block (unsigned long long each) for S shapes:
//   [0, S)   joined positions -- in chain mode CUMULATIVE over the shapes (shape s owns [ctr[s - 1], ctr[s]) of the shared lists)
//   [S]      hits   [S + 1] deferred pairs   [S + 2] collected positions   [S + 3] Hamming survivors   [S + 4] scored survivors
//   [S + 5]  chain status (flags above)      [S + 6] shapes whose pair filter, scoring and left-most rule are complete
//   [S + 8, S + 16)  DMND_SEED_PHASES ticks
//   [S + 16, 2 S + 16)  chain mode: Hamming survivors per shape
DMND_CHAIN_HD int chain_ctr_status(int S) { return S + 5; }
DMND_CHAIN_HD int chain_ctr_done(int S) { return S + 6; }
DMND_CHAIN_HD int chain_ctr_survivors_of(int S) { return S + 16; }
DMND_CHAIN_HD int chain_ctr_words(int S) { return 2 * S + 16; }

// The readback: the counter block, padded to a multiple of 64 bytes, then the leading sorted hits
inline size_t chain_ret_header_bytes(int S) { return ((size_t)chain_ctr_words(S) * sizeof(unsigned long long) + 63) & ~(size_t)63; }
// hits that travel with the readback: what the byte budget holds, never more than the sort's capacity
inline int64_t chain_ret_hits(int64_t budget_bytes, int64_t hit_bytes, int64_t sort_cap)
{
	if (budget_bytes < 0 || hit_bytes <= 0 || sort_cap <= 0) return 0;
	const int64_t n = budget_bytes / hit_bytes;
	return n < sort_cap ? n : sort_cap;
}

// Where the host-driven code takes over
enum ChainPoint {
	CHAIN_COMPLETE = 0,           // sorted hits are on the host
	CHAIN_FROM_PHASE1,            // joined positions over capacity: phase 1 again with grown lists
	CHAIN_FROM_PAIRS,             // pair filter of shape `shape` (tiled threshold, or survivors over capacity), then the following shapes
	CHAIN_FROM_DEFERRED,          // deferred pass of shape `shape`, then the following shapes
	CHAIN_FROM_PHASE2,            // hits over capacity: phase 2 again for every shape
	CHAIN_FROM_SORT               // every shape is complete, the hits are sorted by the host's launches
};
struct ChainPlan { ChainPoint point; int shape; };

// status / done: the words the chain left; S: shapes; sorted_on_device: the chain included the sort
inline ChainPlan chain_plan(unsigned long long status, unsigned long long done, int S, bool sorted_on_device)
{
	const int shape = done < (unsigned long long)S ? (int)done : S - 1;
	if (status & CHAIN_MATCHED_OVER) return ChainPlan{ CHAIN_FROM_PHASE1, 0 };
	if (status & CHAIN_HITS_OVER) return ChainPlan{ CHAIN_FROM_PHASE2, 0 };
	if (status & (CHAIN_TILED | CHAIN_SURVIVORS_OVER)) return ChainPlan{ CHAIN_FROM_PAIRS, shape };
	if (status & CHAIN_DEFERRED) return ChainPlan{ CHAIN_FROM_DEFERRED, shape };
	if ((status & CHAIN_SORT_OVER) || !sorted_on_device) return ChainPlan{ CHAIN_FROM_SORT, 0 };
	return ChainPlan{ CHAIN_COMPLETE, 0 };
}

// What the host-driven code does behind a chain; as constructed, what it does without one (everything, keeping nothing)
struct ChainResume {
	bool hits_done = false;              // the sorted hits are in place: neither phase 2 nor the hit sort is left
	bool phase1_again = true;            // phase 1 (index, stream and mask of every shape) is the host's ...
	bool dirty = false;                  // ... behind an abandoned chain that has used the counters, tables and filters
	int64_t cap_total = 0;               // capacity of the joined-position lists that phase 1 starts from
	int p2_first = 0;                    // phase 2: first shape whose pair filter is the host's ...
	bool p2_keep = false;                // ... the hits of the shapes before it are in seed_hits
	int deferred_sid = -1;               // shape whose deferred pass comes before that (-1: none) ...
	unsigned long long deferred_n = 0;   // ... and the deferred pairs the chain counted for it
	// p2_keep: the capacities under which the kept hits and deferred pairs were written. Otherwise the least capacity phase 2 starts
	// from: that of a list that overflowed, grown; 0 where phase 2's own starting capacity holds
	int64_t hit_cap = 0, def_cap = 0;
	bool discard_pairs_time = false;     // the chain's pair filters run again: their time does not count
};

// r: the counter block the chain left (r[S - 1] joined positions of all shapes, r[S] hits, r[S + 1] deferred pairs); cap_total,
// hit_cap, def_cap: the capacities the chain ran with
inline ChainResume chain_resume(const ChainPlan& plan, const unsigned long long* r, int S, int64_t cap_total, int64_t hit_cap, int64_t def_cap)
{
	ChainResume x;
	x.phase1_again = false;
	x.cap_total = cap_total;
	switch (plan.point) {
	case CHAIN_COMPLETE:
		x.hits_done = true;
		break;
	case CHAIN_FROM_PHASE1:
		x.phase1_again = x.dirty = x.discard_pairs_time = true;      // the abandoned attempt does not count
		x.cap_total = (int64_t)r[S - 1] + (int64_t)r[S - 1] / 8 + 1024;
		break;
	case CHAIN_FROM_PAIRS:
		x.p2_first = plan.shape; x.p2_keep = true;
		break;
	case CHAIN_FROM_DEFERRED:
		x.deferred_n = r[S + 1];
		if ((int64_t)x.deferred_n > def_cap) { x.def_cap = (int64_t)x.deferred_n + 1024; x.discard_pairs_time = true; return x; }      // an incomplete list: phase 2 again
		x.deferred_sid = plan.shape; x.p2_first = plan.shape + 1; x.p2_keep = true;
		break;
	case CHAIN_FROM_PHASE2:
		x.hit_cap = (int64_t)r[S] + 1024;
		x.discard_pairs_time = true;
		break;
	case CHAIN_FROM_SORT:
		x.p2_first = S; x.p2_keep = true;
		break;
	}
	if (x.p2_keep) { x.hit_cap = hit_cap; x.def_cap = def_cap; }
	return x;
}

// the DMND_TRACE summary's name of the path taken
inline void chain_path_name(char* out, size_t n, const ChainPlan& p, unsigned long long status)
{
	switch (p.point) {
	case CHAIN_COMPLETE: snprintf(out, n, "chain"); break;
	case CHAIN_FROM_PHASE1: snprintf(out, n, "chain, then host from phase 1 (joined positions over capacity)"); break;
	case CHAIN_FROM_PAIRS: snprintf(out, n, "chain, then host from the pair filter of shape %d (%s)", p.shape, (status & CHAIN_TILED) ? "tiled filter" : "survivors over capacity"); break;
	case CHAIN_FROM_DEFERRED: snprintf(out, n, "chain, then host from the deferred pass of shape %d", p.shape); break;
	case CHAIN_FROM_PHASE2: snprintf(out, n, "chain, then host from phase 2 (hits over capacity)"); break;
	case CHAIN_FROM_SORT: snprintf(out, n, "chain, then host from the hit sort"); break;
	}
}

}  // namespace dmnd
