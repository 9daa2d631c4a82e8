// tests/emu/length_ratio_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The arithmetic of the mutual-coverage search (diamond_amd/csrc/length_ratio_core.h) for tests/test_length_ratio_core.py, and the
// seed stage's data flow with the length test at the places where the kernels of seed_kernels.hip apply it: the pair filter
// (next to the Hamming identity) and the batch count of the deferred pass (simd_batch_size_sorted with its admit predicate).
// Built from the same per-thread code (seed_core.h) as tests/emu/seed_emu.cpp, without that file's soft-masking views.
#include <algorithm>
#include <climits>
#include <cstdint>
#include <unordered_map>
#include <vector>
#include "../../diamond_amd/csrc/seed_core.h"
#include "../../diamond_amd/csrc/length_ratio_core.h"

using namespace dmnd;

namespace {
struct LrHit { uint32_t query; int32_t seed_offset; int64_t subject; int32_t score; int32_t pad; };
}

extern "C" int emu_length_ratio_passes(int64_t qlen, int64_t tlen, double mlr) { return length_ratio_passes(qlen, tlen, mlr) ? 1 : 0; }
extern "C" double emu_mutual_cover_ratio(double query_cover, double subject_cover, double given) { return mutual_cover_ratio(query_cover, subject_cover, given); }
extern "C" void emu_length_sort_order(const int64_t* limits, int64_t n, int64_t* order) { length_sort_order(limits, n, order); }
extern "C" void emu_length_window(const int64_t* lengths_desc, int64_t n, int64_t len, double mlr, int64_t* first, int64_t* end) { length_window(lengths_desc, n, len, mlr, first, end); }
extern "C" int emu_lengths_non_increasing(const int64_t* limits, int64_t n) { return lengths_non_increasing(limits, n) ? 1 : 0; }
// the window of query POSITIONS (from qlimits[0]) of target t, as seed_qwin_kernel writes it
extern "C" void emu_query_window(const int64_t* qlimits, int64_t nq, int64_t tlen, double mlr, uint32_t* out)
{
	int64_t first, end;
	length_window_of(LengthsOfLimits{ qlimits }, nq, tlen, mlr, &first, &end);
	out[0] = first < end ? (uint32_t)(qlimits[first] - qlimits[0]) : 0;
	out[1] = first < end ? (uint32_t)(qlimits[end] - qlimits[0]) : 0;
}

// The seed search of two length-sorted blocks with a minimum length ratio (mlr = 0: off). stats (5 words): pairs the length test
// removed before the Hamming filter, deferred pairs, deferred pairs whose batch count differs from the one without the length
// test (a batch mate failed it), of those the ones whose saturation decision (batch >= 4) differs, pairs the Hamming filter saw.
extern "C" int64_t emu_mutual_seed_search(const SeedParams* cp, const int8_t* matrix, const int8_t* qdata, const int64_t* qlimits, int64_t nq,
	const int8_t* tdata, const int64_t* tlimits, int64_t nt, double mlr, LrHit* hits, int64_t cap, int64_t* stats)
{
	const SeedParams& c = *cp;
	const int64_t qraw = qlimits[nq], traw = tlimits[nt];
	for (int i = 0; i < 5; ++i) stats[i] = 0;
	std::vector<uint8_t> mask_time((size_t)qraw + 256, SEED_NEVER);
	std::vector<uint32_t> qid_of((size_t)qraw, 0);
	for (int64_t i = 0; i < nq; ++i)
		for (int64_t p = qlimits[i]; p < qlimits[i + 1]; ++p) qid_of[(size_t)p] = (uint32_t)i;
	auto target_of = [&](int64_t loc) { return (int64_t)(std::upper_bound(tlimits, tlimits + nt + 1, loc) - tlimits) - 1; };
	auto admit = [&](int64_t qp, int64_t loc) {
		if (mlr <= 0.0) return true;
		const int64_t q = qid_of[(size_t)qp], t = target_of(loc);
		return length_ratio_passes(qlimits[q + 1] - qlimits[q] - 1, tlimits[t + 1] - tlimits[t] - 1, mlr);
	};
	struct Group { std::vector<int64_t> q; bool present = false, erased = false, need = false; };
	std::vector<std::unordered_map<uint64_t, Group>> tables(c.n_shapes);
	std::vector<std::vector<std::pair<uint64_t, int64_t>>> matched(c.n_shapes);
	const bool hashed = c.seed_encoding == SEED_HASHED;
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
	struct Deferred { size_t m; int64_t qp; int score; };
	int64_t n = 0;
	for (int sid = 0; sid < c.n_shapes; ++sid) {
		std::vector<Deferred> deferred;
		for (size_t mi = 0; mi < matched[sid].size(); ++mi) {
			const auto& m = matched[sid][mi];
			Group& g = tables[sid][m.first];
			if (g.erased) continue;
			const int chunk = seed_chunk(c, m.first);
			for (int64_t qp : g.q) {
				if (!admit(qp, m.second)) { ++stats[0]; continue; }
				++stats[4];
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
						if (score > 255) { deferred.push_back(Deferred{ mi, qp, score }); g.need = true; continue; }
						if (score <= cutoff) continue;
					}
				}
				if (!left_most_pair(c, qdata + qp, mask_time.data() + qp, tdata + m.second, seed_offset, sid, chunk, query_len)) continue;
				if (n >= cap) return -1;
				hits[n++] = LrHit{ qid, seed_offset, m.second, score, 0 };
			}
		}
		if (deferred.empty()) continue;
		std::vector<std::pair<uint64_t, int64_t>> e;
		for (const auto& m : matched[sid]) if (tables[sid][m.first].need) e.push_back(m);
		std::sort(e.begin(), e.end());
		std::vector<uint64_t> e_loc(e.size());
		for (size_t i = 0; i < e.size(); ++i) e_loc[i] = (uint64_t)e[i].second;
		for (const Deferred& d : deferred) {
			const auto& m = matched[sid][d.m];
			const size_t b = (size_t)(std::lower_bound(e.begin(), e.end(), std::make_pair(m.first, (int64_t)INT64_MIN)) - e.begin());
			const size_t en = (size_t)(std::upper_bound(e.begin(), e.end(), std::make_pair(m.first, (int64_t)INT64_MAX)) - e.begin());
			int score = d.score;
			const int64_t qp = d.qp;
			const int batch = simd_batch_size_sorted(c, e_loc.data() + b, (int64_t)(en - b), tdata, qdata + qp, m.second, [&](int64_t loc) { return admit(qp, loc); });
			const int batch_all = simd_batch_size_sorted(c, e_loc.data() + b, (int64_t)(en - b), tdata, qdata + qp, m.second);
			++stats[1];
			stats[2] += batch != batch_all;
			stats[3] += (batch >= 4) != (batch_all >= 4);
			if (batch >= 4) score = 255;
			const uint32_t qid = qid_of[(size_t)qp];
			const int seed_offset = (int)(qp - qlimits[qid]);
			const int query_len = (int)(qlimits[qid + 1] - qlimits[qid] - 1);
			if (score <= ungapped_cutoff(c, query_len)) continue;
			if (!left_most_pair(c, qdata + qp, mask_time.data() + qp, tdata + m.second, seed_offset, sid, seed_chunk(c, m.first), query_len)) continue;
			if (n >= cap) return -1;
			hits[n++] = LrHit{ qid, seed_offset, m.second, score, 0 };
		}
	}
	return n;
}
