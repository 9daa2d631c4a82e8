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
