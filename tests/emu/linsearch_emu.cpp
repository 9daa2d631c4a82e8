// tests/emu/linsearch_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The rules of the linearised search (diamond_amd/csrc/linsearch_core.h) for tests/test_linsearch_core.py and the GPU tests of
// dmnd_set_linsearch: the selection of a seed's first joined reference position, and the seed stage's data flow with it at the
// places where the kernels of seed_kernels.hip apply the rules -- the reduction in front of the pair filter, the score that is
// never deferred, the left-most filter that is skipped. Built from the same per-thread code (seed_core.h) as
// tests/emu/seed_emu.cpp, without that file's soft-masking views.
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>
#include "../../diamond_amd/csrc/seed_core.h"
#include "../../diamond_amd/csrc/linsearch_core.h"

using namespace dmnd;

namespace {
struct LinHit { uint32_t query; int32_t seed_offset; int64_t subject; int32_t score; int32_t pad; };
}

// selected[i] = 1 iff record i (slot[i], position[i]) reaches the Hamming test: the two steps of the rule, as the kernels run them
extern "C" void emu_lin_select(const uint32_t* slot, const int64_t* position, int64_t n, int64_t n_slots, uint8_t* selected)
{
	std::vector<int64_t> first((size_t)n_slots, -12345);          // (any content: the reduction initialises what it reads)
	lin_first_positions(slot, position, n, first.data());
	for (int64_t i = 0; i < n; ++i) selected[i] = lin_record_selected(position[i], first[slot[i]]) ? 1 : 0;
}
extern "C" int emu_lin_score_is_deferred(int score, int lin) { return lin_score_is_deferred(score, lin != 0) ? 1 : 0; }
extern "C" int emu_lin_applies_left_most(int lin) { return lin_applies_left_most(lin != 0) ? 1 : 0; }
extern "C" int emu_lin_shape_weight_ok(int weight) { return lin_shape_weight_ok(weight) ? 1 : 0; }

// The linearised seed search of a query block against a (length-sorted) reference block. stats (6 words): joined reference positions
// of the seeds that are not erased (what the pair filter of a switch-off search walks), those of them the rule selects, pairs the
// Hamming filter saw, hits with a score above 255, dropped records that hold a query position whose pair passes the Hamming filter
// there while its pair with the seed's first position fails it, hits that the left-most filter would have dropped.
extern "C" int64_t emu_lin_seed_search(const SeedParams* cp, const int8_t* matrix, const int8_t* qdata, const int64_t* qlimits, int64_t nq,
	const int8_t* tdata, const int64_t* tlimits, int64_t nt, LinHit* hits, int64_t cap, int64_t* stats)
{
	const SeedParams& c = *cp;
	const int64_t qraw = qlimits[nq], traw = tlimits[nt];
	for (int i = 0; i < 6; ++i) stats[i] = 0;
	for (int sid = 0; sid < c.n_shapes; ++sid)
		if (!lin_shape_weight_ok(c.shape_weight[sid])) return -2;
	std::vector<uint8_t> mask_time((size_t)qraw + 256, SEED_NEVER);
	std::vector<uint32_t> qid_of((size_t)qraw, 0);
	for (int64_t i = 0; i < nq; ++i)
		for (int64_t p = qlimits[i]; p < qlimits[i + 1]; ++p) qid_of[(size_t)p] = (uint32_t)i;
	struct Group { std::vector<int64_t> q; uint32_t slot = 0; bool present = false, erased = false; };
	const bool hashed = c.seed_encoding == SEED_HASHED;
	int64_t n = 0;
	// (the masks of a shape depend on this and earlier shapes only, but the left-most statistic below reads all of them: two passes)
	std::vector<std::unordered_map<uint64_t, Group>> tables(c.n_shapes);
	std::vector<std::vector<std::pair<uint64_t, int64_t>>> matched(c.n_shapes);
	for (int sid = 0; sid < c.n_shapes; ++sid) {
		auto& tab = tables[sid];
		for (int64_t p = qlimits[0]; p < qraw; ++p) {
			uint64_t s;
			if (!(hashed ? seed_key_hashed(c, sid, qdata + p, s) : seed_at(c, sid, qdata + p, s))) continue;
			if (hashed && !seed_is_complex(c, sid, qdata + p)) {
				mask_time[(size_t)p] = (uint8_t)std::min<int>(mask_time[(size_t)p], sid * c.index_chunks);
				continue;
			}
			tab[s].q.push_back(p);
		}
		uint32_t n_slots = 0;
		for (auto& kv : tab) kv.second.slot = n_slots++;
		for (int64_t p = tlimits[0]; p < traw; ++p) {
			uint64_t s;
			if (!(hashed ? seed_key_hashed(c, sid, tdata + p, s) : seed_at(c, sid, tdata + p, s))) continue;
			auto it = tab.find(s);
			if (it == tab.end()) continue;
			it->second.present = true;
			matched[sid].push_back({ s, p });
		}
		for (auto& kv : tab) {
			Group& g = kv.second;
			if (!g.present || hashed) continue;
			const int64_t first = *std::min_element(g.q.begin(), g.q.end());
			if (!seed_is_complex(c, sid, qdata + first)) {
				g.erased = true;
				const int t = sid * c.index_chunks + seed_chunk(c, kv.first);
				for (int64_t p : g.q) mask_time[(size_t)p] = (uint8_t)std::min<int>(mask_time[(size_t)p], t);
			}
		}
	}
	for (int sid = 0; sid < c.n_shapes; ++sid) {
		auto& tab = tables[sid];
		const size_t nm = matched[sid].size();
		// the reduction over the shape's records, walked back to front: the result must not depend on their order
		std::vector<uint32_t> r_slot(nm);
		std::vector<int64_t> r_pos(nm);
		for (size_t i = 0; i < nm; ++i) { r_slot[i] = tab[matched[sid][nm - 1 - i].first].slot; r_pos[i] = matched[sid][nm - 1 - i].second; }
		std::vector<int64_t> first(tab.size() + 1, 0);
		lin_first_positions(r_slot.data(), r_pos.data(), (int64_t)nm, first.data());
		for (const auto& m : matched[sid]) {
			Group& g = tab[m.first];
			if (g.erased) continue;
			++stats[0];
			const bool selected = lin_record_selected(m.second, first[g.slot]);
			if (!selected) {
				// what the rule drops although it would pass: a later position whose pair passes where the first one's fails
				for (int64_t qp : g.q)
					if (fingerprint_id(qdata + qp, tdata + m.second) >= c.hamming_filter_id && fingerprint_id(qdata + qp, tdata + first[g.slot]) < c.hamming_filter_id) { ++stats[4]; break; }
				continue;
			}
			++stats[1];
			const int chunk = seed_chunk(c, m.first);
			for (int64_t qp : g.q) {
				++stats[2];
				if (fingerprint_id(qdata + qp, tdata + m.second) < c.hamming_filter_id) continue;
				const uint32_t qid = qid_of[(size_t)qp];
				const int seed_offset = (int)(qp - qlimits[qid]);
				int score = 0xFFFF;
				const int query_len = (int)(qlimits[qid + 1] - qlimits[qid] - 1);
				if (c.use_ungapped) {
					const int cutoff = ungapped_cutoff(c, query_len);
					if (cutoff) {
						const int window = stage2_window(c, query_len);
						int cb, ce;
						clip_window(qdata + qp - window, 2 * window, window, cb, ce);
						const int window_left = window - cb;
						score = ungapped_window_score(matrix, qdata + qp - window_left, tdata + m.second - window_left, ce - cb);
						if (lin_score_is_deferred(score, true)) return -3;      // (never: a batch of one keeps its scalar score)
						if (score <= cutoff) continue;
						stats[3] += score > 255;
					}
				}
				if (lin_applies_left_most(true)) return -3;
				if (!left_most_pair(c, qdata + qp, mask_time.data() + qp, tdata + m.second, seed_offset, sid, chunk, query_len)) ++stats[5];
				if (n >= cap) return -1;
				hits[n++] = LinHit{ qid, seed_offset, m.second, score, 0 };
			}
		}
	}
	return n;
}
