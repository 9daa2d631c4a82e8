// CPU emulator of the SEG kernels (diamond_amd/csrc/seg_kernels.hip): the same arithmetic (seg_core.h) with the kernels' data flow --
// a byte of class per window centre, the raw segment's composition plus the prefix / suffix compositions of its ends, the trim's
// candidates 64 per round with a (value, order) minimum, seg_drive with its one saved frame -- next to the host statement
// (seg_mask.h) that it is compared with. Compile without FP contraction.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../diamond_amd/csrc/seg_core.h"
#include "../../diamond_amd/csrc/seg_mask.h"

using namespace dmnd;

namespace {

// every zero-terminated descending count vector with the sum n and parts <= max_part, in turn
template<typename F>
void partitions(int n, int max_part, int* sv, int depth, F& f)
{
	if (n == 0) { sv[depth] = 0; f(sv); return; }
	for (int k = n < max_part ? n : max_part; k >= 1; --k) { sv[depth] = k; partitions(n - k, k, sv, depth + 1, f); }
}

// the class table as the library builds it for a context: seg::entropy of every reachable count vector
int build_table(uint8_t* table)
{
	std::memset(table, SEG_BREAK, SEG_CLASS_TABLE);
	std::vector<char> set(SEG_CLASS_TABLE, 0);
	int n_states = 0, bad = 0;
	auto put = [&](const int* sv) {
		const int key = seg_class_key(sv);
		if (key < 0 || key >= SEG_CLASS_TABLE || set[(size_t)key]) { ++bad; return; }
		set[(size_t)key] = 1;
		table[key] = (uint8_t)seg_entropy_class(seg::entropy(sv));
		++n_states;
	};
	int sv[SEG_ALPHA + 1];
	for (int n = SEG_WINDOW - SEG_MAX_BOGUS; n <= SEG_WINDOW; ++n) partitions(n, n, sv, 0, put);
	return bad ? -bad : n_states;
}

struct Trim { int cut_left, cut_right; };

// the candidate form of seg::trim as the segments kernel runs it
Trim trim_candidates(const int8_t* s, int len, const double* F)
{
	int comp[SEG_ALPHA] = { 0 };
	for (int x = 0; x < len; ++x) { const int l = s[x] & 31; if (l < SEG_ALPHA) ++comp[l]; }
	const int dmax = len - 2 < SEG_MAX_TRIM - 1 ? len - 2 : SEG_MAX_TRIM - 1;
	uint8_t pre[SEG_MAX_TRIM][SEG_ALPHA] = {}, suf[SEG_MAX_TRIM][SEG_ALPHA] = {};
	for (int a = 0; a < SEG_ALPHA; ++a) {                  // one lane per residue, running counts
		int np = 0, ns = 0;
		for (int k = 0; k <= dmax; ++k) {
			pre[k][a] = (uint8_t)np; suf[k][a] = (uint8_t)ns;
			np += (s[k] & 31) == a; ns += (s[len - 1 - k] & 31) == a;
		}
	}
	const int n_cand = seg_candidates(len);
	double best_v = 1.0;
	int best_c = 0x7fffffff;
	for (int round = 0; round * 64 < n_cand; ++round) {
		double v[64]; int c[64];
		for (int lane = 0; lane < 64; ++lane) {
			c[lane] = round * 64 + lane;
			v[lane] = 1.0;
			if (c[lane] >= n_cand) { c[lane] = 0x7fffffff; continue; }
			int d, i, sv[SEG_ALPHA];
			seg_candidate(c[lane], d, i);
			for (int a = 0; a < SEG_ALPHA; ++a) sv[a] = comp[a] - pre[i][a] - suf[d - i][a];
			seg_sort_desc(sv);
			v[lane] = seg_ln_prob(sv, len - d, F);
		}
		for (int m = 32; m >= 1; m >>= 1)                  // the wave's butterfly
			for (int lane = 0; lane < 64; ++lane)
				if (seg_better(v[lane ^ m], c[lane ^ m], v[lane], c[lane]) && (lane & m) == 0) { v[lane] = v[lane ^ m]; c[lane] = c[lane ^ m]; }
		if (v[0] < 1.0 && seg_better(v[0], c[0], best_v, best_c)) { best_v = v[0]; best_c = c[0]; }
	}
	Trim t = { 0, 0 };
	if (best_v < 1.0) { int d, i; seg_candidate(best_c, d, i); t.cut_left = i; t.cut_right = d - i; }
	return t;
}

struct EmuOps {
	const int8_t* s;
	const uint8_t* cls;
	const double* F;
	std::vector<int32_t>* out;        // begin, end pairs
	std::vector<int32_t>* raw;        // left, len of every raw segment that was trimmed (may be NULL)
	int n_trims = 0, n_left = 0, max_child = 0;
	int next_trigger(int i, int last) { for (; i <= last; ++i) if (cls[i] == SEG_TRIGGER) return i; return -1; }
	int find_low(int i, int lowlim) { for (; i >= lowlim; --i) if (cls[i] != SEG_TRIGGER && cls[i] != SEG_EXTEND) break; return i + 1; }
	int find_high(int i, int last) { for (; i <= last; ++i) if (cls[i] != SEG_TRIGGER && cls[i] != SEG_EXTEND) break; return i - 1; }
	bool trim(int left, int len, int& cut_left, int& cut_right)
	{
		if (len > SEG_LNFACT_MAX) return false;
		++n_trims;
		if (raw) { raw->push_back(left); raw->push_back(len); }
		const Trim t = trim_candidates(s + left, len, F);
		cut_left = t.cut_left; cut_right = t.cut_right;
		return true;
	}
	void emit(int b, int e) { out->push_back(b); out->push_back(e); }
	void remainder_done(int found) { ++n_left; if (found > max_child) max_child = found; }
};

void classes(const int8_t* s, int len, const uint8_t* table, std::vector<uint8_t>& cls)
{
	cls.assign((size_t)len + 1, SEG_NONE);
	for (int x = SEG_DOWNSET; x <= len - SEG_UPSET; ++x) {
		int bogus;
		const int key = seg_window_key(s + x - SEG_DOWNSET, bogus);
		cls[(size_t)x] = (uint8_t)seg_window_class(table, key, bogus);
	}
}

}

// every count vector of 8 - 10 letters (11 ints each, zero-terminated) with its class through seg_core.h -- from the vector's key
// and from a window of letters that has these counts -- and the class that seg::entropy gives; returns their number, < 0 on a key clash
extern "C" int emu_seg_class_states(int32_t* states, uint8_t* by_key, uint8_t* by_window, uint8_t* by_entropy, int cap)
{
	uint8_t table[SEG_CLASS_TABLE];
	const int built = build_table(table);
	if (built < 0) return built;
	int n = 0;
	auto visit = [&](const int* sv) {
		if (n < cap) {
			int total = 0, bogus = 0, pos = 0;
			int8_t w[SEG_WINDOW];
			for (int i = 0; i <= SEG_WINDOW; ++i) states[n * (SEG_WINDOW + 1) + i] = 0;
			for (int i = 0; sv[i] != 0; ++i) {
				states[n * (SEG_WINDOW + 1) + i] = sv[i]; total += sv[i];
				for (int k = 0; k < sv[i]; ++k) w[pos++] = (int8_t)((i * 7 + 3) % SEG_ALPHA);      // 10 distinct residues for i < 10
			}
			for (; pos < SEG_WINDOW; ++pos) w[pos] = (int8_t)(pos & 1 ? 23 : 24 + 128);            // non-standard letters fill the rest
			for (int i = 0; i < SEG_WINDOW / 2; i += 2) { const int8_t t = w[i]; w[i] = w[SEG_WINDOW - 1 - i]; w[SEG_WINDOW - 1 - i] = t; }      // not sorted by residue
			by_key[n] = (uint8_t)seg_window_class(table, seg_class_key(sv), SEG_WINDOW - total);
			const int key = seg_window_key(w, bogus);
			by_window[n] = (uint8_t)seg_window_class(table, key, bogus);
			by_entropy[n] = (uint8_t)seg_entropy_class(seg::entropy(sv));
		}
		++n;
	};
	int sv[SEG_ALPHA + 1];
	for (int total = SEG_WINDOW - SEG_MAX_BOGUS; total <= SEG_WINDOW; ++total) partitions(total, total, sv, 0, visit);
	return n;
}

// the emulated driver over one sequence: ranges (begin, end pairs, ascending list order) into out, *n_ranges = their number;
// raw (may be NULL): left, len of every raw segment trimmed, *n_raw their number; stats: trims, left-remainder searches entered,
// most segments one such search found, 1 if the sequence is handed back. Returns 0, or -1 if a capacity is too small.
extern "C" int emu_seg_ranges(const int8_t* s, int len, int32_t* out, int cap, int32_t* n_ranges, int32_t* raw, int raw_cap, int32_t* n_raw, int32_t* stats)
{
	uint8_t table[SEG_CLASS_TABLE];
	if (build_table(table) < 0) return -2;
	std::vector<uint8_t> cls;
	classes(s, len, table, cls);
	std::vector<int32_t> ranges, raws;
	EmuOps ops;
	ops.s = s; ops.cls = cls.data(); ops.F = seg::lnfact().table.data(); ops.out = &ranges; ops.raw = &raws;
	const bool ok = seg_drive(ops, len);
	if (!ok) ranges.clear();
	if (stats) { stats[0] = ops.n_trims; stats[1] = ops.n_left; stats[2] = ops.max_child; stats[3] = ok ? 0 : 1; }
	*n_ranges = (int32_t)(ranges.size() / 2);
	if (n_raw) *n_raw = (int32_t)(raws.size() / 2);
	if ((int)ranges.size() / 2 > cap || (raw && (int)raws.size() / 2 > raw_cap)) return -1;
	if (!ranges.empty()) std::memcpy(out, ranges.data(), ranges.size() * sizeof(int32_t));
	if (raw && !raws.empty()) std::memcpy(raw, raws.data(), raws.size() * sizeof(int32_t));
	return 0;
}

// one raw segment through the candidate form and through seg::trim: out = cut_left, cut_right of each
extern "C" void emu_seg_trim_both(const int8_t* s, int len, int32_t* out)
{
	const Trim t = trim_candidates(s, len, seg::lnfact().table.data());
	out[0] = t.cut_left; out[1] = t.cut_right;
	int leftend = 0, rightend = len - 1;
	seg::trim(s, len, leftend, rightend);
	out[2] = leftend; out[3] = len - 1 - rightend;
}
