// tests/emu/transcript_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The transcript arrays' layout (diamond_amd/csrc/extend_core.h tr_layout, tr_regions) and the arithmetic of the keep and gather
// steps of the device half of the extension stage (diamond_amd/csrc/transcript_core.h) run lane by lane on the CPU, for
// tests/test_transcript_core.py: the same slot bound, offset rules, piece rule and byte copy the ext_tr_* kernels use.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../diamond_amd/csrc/extend_core.h"
#include "../../diamond_amd/csrc/transcript_core.h"

using namespace dmnd;

extern "C" int emu_tr_layout(uint64_t n_groups, uint64_t walk_cap, uint64_t record_cap, int cap, const char** names, uint64_t* off, uint64_t* used, uint64_t* bytes)
{
	const TrLayout T = tr_layout((size_t)n_groups, (size_t)walk_cap, (size_t)record_cap);
	ExtRegion r[TR_REGIONS];
	const int n = tr_regions(T, r);
	for (int i = 0; i < n && i < cap; ++i) { names[i] = r[i].name; off[i] = r[i].off; used[i] = r[i].used; }
	*bytes = T.bytes;
	return n;
}

extern "C" int64_t emu_tr_slot_bytes(int32_t query_len, int32_t target_len) { return tr_slot_bytes(query_len, target_len); }
extern "C" int64_t emu_tr_kept_bytes(int32_t transcript_len) { return tr_kept_bytes(transcript_len); }

// the piece bounds of a walked list of n entries with the given slot widths: bounds[0 .. return value], as ext_tr_pieces_kernel
extern "C" uint32_t emu_tr_pieces(const int64_t* widths, uint32_t n, int64_t limit, uint32_t* bounds, int64_t* scan)
{
	scan[0] = 0;
	for (uint32_t i = 0; i < n; ++i) scan[i + 1] = scan[i] + widths[i];
	uint32_t np = 0, s = 0;
	bounds[0] = 0;
	while (s < n) { s = tr_piece_end(scan, n, s, limit); bounds[++np] = s; }
	return np;
}

// One walked list through the whole path, as the kernels do it: n entries with query / target lengths and transcripts
// (tr[i]: len[i] bytes, none of them 0) in pieces of at most `limit` raw bytes -- per piece the transcripts are written to the front
// of their raw slots (with the terminator; the rest of the slot is filled with 0xEE), kept into the store behind the earlier
// pieces; then n_rec records, record r being entry slot_of[r], are gathered into `out`.
//   store_off[i]  where entry i lies in the store        rec_off[r]  where record r lies in out
//   sizes[0] pieces, [1] raw bytes of the largest piece, [2] bytes in the store, [3] bytes in out, [4] slot overlaps or
//   slots past their piece's raw bytes found
// returns 0, or -1 if store_cap / out_cap would be exceeded (nothing is written past them)
extern "C" int emu_tr_keep_gather(uint32_t n, const int32_t* qlen, const int32_t* tlen, const int32_t* len, const uint8_t* tr, const int64_t* tr_at,
	int64_t limit, uint32_t n_rec, const uint32_t* slot_of, uint8_t* store, int64_t store_cap, int64_t* store_off, uint8_t* out, int64_t out_cap,
	int64_t* rec_off, int64_t* sizes)
{
	std::vector<int64_t> scan((size_t)n + 1, 0);
	for (uint32_t i = 0; i < n; ++i) scan[i + 1] = scan[i] + tr_slot_bytes(qlen[i], tlen[i]);
	int64_t base = 0, raw_max = 0, bad = 0;
	uint32_t pieces = 0;
	for (uint32_t s0 = 0; s0 < n;) {
		const uint32_t s1 = tr_piece_end(scan.data(), n, s0, limit), m = s1 - s0;
		const int64_t raw_bytes = tr_raw_off(scan[s1], scan[s0]);
		raw_max = raw_bytes > raw_max ? raw_bytes : raw_max;
		std::vector<uint8_t> raw((size_t)raw_bytes, 0xEE);
		// the walk: each entry's transcript at the front of its slot
		for (uint32_t i = 0; i < m; ++i) {
			const int64_t o = tr_raw_off(scan[s0 + i], scan[s0]), w = scan[s0 + i + 1] - scan[s0 + i];
			if (o < 0 || o + w > raw_bytes || tr_kept_bytes(len[s0 + i]) > w) { ++bad; continue; }
			if (i > 0 && o < tr_raw_off(scan[s0 + i - 1], scan[s0]) + (scan[s0 + i] - scan[s0 + i - 1])) ++bad;
			std::memcpy(raw.data() + o, tr + tr_at[s0 + i], (size_t)len[s0 + i]);
			raw[(size_t)(o + len[s0 + i])] = 0;
		}
		// the keep step: lengths, their scan, one 64-lane copy per entry
		std::vector<int64_t> k_len((size_t)m + 1, 0), k_off((size_t)m + 1, 0);
		for (uint32_t i = 0; i < m; ++i) k_len[i] = tr_kept_bytes(len[s0 + i]);
		for (uint32_t i = 0; i < m; ++i) k_off[i + 1] = k_off[i] + k_len[i];
		if (base + k_off[m] > store_cap) return -1;
		for (uint32_t i = 0; i < m; ++i) {
			const int64_t dst = tr_dense_off(base, k_off[i]);
			for (int lane = 0; lane < TR_LANES; ++lane) tr_copy_lane(store + dst, raw.data() + tr_raw_off(scan[s0 + i], scan[s0]), k_len[i], lane);
			store_off[s0 + i] = dst;
		}
		base += k_off[m];
		++pieces;
		s0 = s1;
	}
	// the gather step: the records' lengths, their scan, one 64-lane copy per record
	std::vector<int64_t> r_len((size_t)n_rec + 1, 0), r_off((size_t)n_rec + 1, 0);
	for (uint32_t r = 0; r < n_rec; ++r) r_len[r] = tr_kept_bytes(len[slot_of[r]]);
	for (uint32_t r = 0; r < n_rec; ++r) r_off[r + 1] = r_off[r] + r_len[r];
	if (r_off[n_rec] > out_cap) return -1;
	for (uint32_t r = 0; r < n_rec; ++r) {
		const int64_t dst = tr_dense_off(0, r_off[r]);
		for (int lane = 0; lane < TR_LANES; ++lane) tr_copy_lane(out + dst, store + store_off[slot_of[r]], r_len[r], lane);
		rec_off[r] = dst;
	}
	sizes[0] = pieces; sizes[1] = raw_max; sizes[2] = base; sizes[3] = r_off[n_rec]; sizes[4] = bad;
	return 0;
}
