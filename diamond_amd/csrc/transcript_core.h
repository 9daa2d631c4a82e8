// transcript_core.h -- the arithmetic of the transcripts the device half of the extension stage returns (extend_kernels.hip:
// ext_tr_* kernels; extend_device.hip), HIP-free: one statement of it for the kernels and for the CPU tests (tests/emu/
// transcript_emu.cpp). A transcript travels through three byte ranges, each one allocation addressed by non-negative offsets:
//   raw slots   one per entry of a walked piece, tr_slot_bytes wide, at the exclusive scan of the widths from the piece's first entry
//               (traceback_kernel writes the packed transcript and its 0 terminator at the front of the slot)
//   the store   dense and append-only: a piece's transcripts (tr_kept_bytes each) at the scan of their lengths behind what the
//               earlier pieces left -- the order of the walked list, no atomics, so the layout is the same in every run
//   the output  the records' transcripts in record order, at the scan of their lengths: what the caller's arena receives
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DMND_TR_HD __host__ __device__
#else
#define DMND_TR_HD
#endif

namespace dmnd {

enum { TR_LANES = 64 };

// width of a raw slot: no alignment of a query of query_len letters with a target of target_len has more packed operations than
// query_len + target_len, + the terminator, + the byte the walk leaves free at the back of the slot (the bound of dmnd_banded_swipe)
DMND_TR_HD inline int64_t tr_slot_bytes(int32_t query_len, int32_t target_len) { return (int64_t)query_len + (int64_t)target_len + 2; }

// bytes a transcript takes in the store and in the output: its operations and the terminator (an entry without a walk -- no
// score, or a saturated sweep, transcript_len -1 -- is the terminator alone)
DMND_TR_HD inline int64_t tr_kept_bytes(int32_t transcript_len) { return (int64_t)(transcript_len > 0 ? transcript_len : 0) + 1; }

// offset rule of the raw slots: entry's place in the piece's allocation, from the scan over the whole walked list
DMND_TR_HD inline int64_t tr_raw_off(int64_t scan_entry, int64_t scan_piece_first) { return scan_entry - scan_piece_first; }

// offset rule of the store (and, with base 0, of the output): the running base + the scan of the lengths inside the piece
DMND_TR_HD inline int64_t tr_dense_off(int64_t base, int64_t scan_entry) { return base + scan_entry; }

// The end of the piece that begins at entry s0 of a walked list of n entries: the most consecutive entries whose raw slots fit
// `limit` bytes, at least one. scan = the exclusive scan of the slot widths, n + 1 entries.
DMND_TR_HD inline uint32_t tr_piece_end(const int64_t* scan, uint32_t n, uint32_t s0, int64_t limit)
{
	// the last s1 in (s0, n] with scan[s1] - scan[s0] <= limit; scan is non-decreasing
	uint32_t lo = s0 + 1, hi = n;
	const int64_t top = scan[s0] + limit;
	if (scan[lo] > top) return lo;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo + 1) / 2;
		if (scan[mid] <= top) lo = mid; else hi = mid - 1;
	}
	return lo;
}

// the byte copy of one entry by TR_LANES lanes: lane L moves bytes L, L + 64, ... (neighbouring lanes, neighbouring bytes)
DMND_TR_HD inline void tr_copy_lane(uint8_t* dst, const uint8_t* src, int64_t bytes, int lane)
{
	for (int64_t x = lane; x < bytes; x += TR_LANES) dst[x] = src[x];
}

}  // namespace dmnd
