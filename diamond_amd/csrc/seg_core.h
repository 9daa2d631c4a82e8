// seg_core.h -- arithmetic of SEG low-complexity masking (`--masking seg`) in the form the device runs it, shared by the HIP kernels
// (seg_kernels.hip), the host side of the device call (mask_api.hip) and the CPU emulator (tests/emu/seg_emu.cpp). seg_mask.h stays
// the host statement of the reference (NCBI's SEG, blast_seg.cpp); everything here must give its numbers bit for bit.
//
//   window class   The K2 entropy of a 10-letter window depends only on the counts of its standard residues. A window's counts are
//                  folded into a key (sum of one weight per distinct residue, by its count; the weights make the key injective over
//                  all count vectors of 8 - 10 letters) and the key indexes a table of classes that the HOST fills by calling
//                  seg::entropy for every reachable count vector: no log on the device.
//   trim           seg::trim looks at every sub-window that is up to 49 letters shorter than the raw segment: candidates (d, i) =
//                  (letters cut, letters cut on the left). A candidate's composition is the raw segment's minus that of its first i
//                  and its last d - i letters; its ln P0 is seg::get_prob in the host's operation order -- counts sorted descending,
//                  ln_ass group by group, F(total) - F(sv[0]) - F(sv[1]) ..., then ans1 + ans2 - total * LN20 -- over the ln n!
//                  table (F), exact IEEE double arithmetic as long as nothing is contracted. The winner is the smallest value below
//                  1.0, ties to the smallest (d, i) in (d, i) order: what the host's strict `<` over its loop order yields.
//   driver         seg::seg_seq with its recursion unrolled (see seg_drive).
#pragma once
#include "swipe_core.h"      // DMND_HD

namespace dmnd {

enum { SEG_WINDOW = 10, SEG_DOWNSET = 4, SEG_UPSET = 6, SEG_MAX_TRIM = 50, SEG_MAX_BOGUS = 2, SEG_ALPHA = 20,
       SEG_LNFACT_MAX = 10000,         // raw segments above this need Stirling's formula (log): handed back to the host
       SEG_MAX_CANDIDATES = SEG_MAX_TRIM * (SEG_MAX_TRIM + 1) / 2,
       SEG_CLASS_TABLE = 324 };        // keys of all count vectors of 8 - 10 letters lie in [8, 322]
enum { SEG_NONE = 0, SEG_TRIGGER = 1, SEG_EXTEND = 2, SEG_BREAK = 3 };

// weight of a residue that occurs c times (1 <= c <= 10) in the window: 1, 11, 47, 121, 161, 64, 90, 29, 20, 32 -- found by a
// greedy search for the smallest weights under which no two multisets of counts with a sum <= 10 share a key
DMND_HD int seg_count_weight(int c)
{
	return (int)(((c <= 8 ? 0x1D5A40A1792F0B01ull : 0x2014ull) >> (8 * ((c - 1) & 7))) & 255);
}

// key of a zero-terminated count vector (any order)
DMND_HD int seg_class_key(const int* sv)
{
	int key = 0;
	for (int i = 0; sv[i] != 0; ++i) key += seg_count_weight(sv[i]);
	return key;
}

// key of the window w[0 .. 9] (letters taken & 31; 20 and above are non-standard and only counted)
DMND_HD int seg_window_key(const int8_t* w, int& bogus)
{
	int l[SEG_WINDOW], key = 0;
	bogus = 0;
#pragma unroll
	for (int j = 0; j < SEG_WINDOW; ++j) { l[j] = w[j] & 31; bogus += l[j] >= SEG_ALPHA; }
#pragma unroll
	for (int j = 0; j < SEG_WINDOW; ++j) {
		int count = 0, first = 1;
#pragma unroll
		for (int k = 0; k < SEG_WINDOW; ++k) { const int same = l[k] == l[j]; count += same; if (k < j && same) first = 0; }
		if (first && l[j] < SEG_ALPHA) key += seg_count_weight(count);
	}
	return key;
}

// class of an entropy value (seg_seq: H <= LOCUT triggers, H <= HICUT extends, above it breaks)
DMND_HD int seg_entropy_class(double H) { return H <= 1.8 ? SEG_TRIGGER : H <= 2.1 ? SEG_EXTEND : SEG_BREAK; }

DMND_HD int seg_window_class(const uint8_t* table, int key, int bogus) { return bogus > SEG_MAX_BOGUS ? SEG_NONE : (int)table[key]; }

// candidate c (0 .. 1274, the host's loop order) -> (d, i)
DMND_HD void seg_candidate(int c, int& d, int& i)
{
	int x = 0;
	while ((x + 1) * (x + 2) / 2 <= c) ++x;
	d = x;
	i = c - x * (x + 1) / 2;
}
DMND_HD int seg_candidates(int len) { const int dmax = len - 2 < SEG_MAX_TRIM - 1 ? len - 2 : SEG_MAX_TRIM - 1; return (dmax + 1) * (dmax + 2) / 2; }

// v[0 .. 19] descending (a fixed network: every index is known at compile time, the counts stay in registers)
DMND_HD void seg_sort_desc(int* v)
{
#pragma unroll
	for (int i = 1; i < SEG_ALPHA; ++i)
#pragma unroll
		for (int j = i; j >= 1; --j) {
			const int a = v[j - 1], b = v[j];
			v[j - 1] = a > b ? a : b;
			v[j] = a > b ? b : a;
		}
}

// seg::get_prob of a window of `total` letters (<= SEG_LNFACT_MAX; the non-standard ones count here, as in the reference) whose
// standard residues have the descending counts sv[0 .. 19]; F = the ln n! table
DMND_HD double seg_ln_prob(const int* sv, int total, const double* F)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
	// seg::ln_ass: 20! over the multiplicity! of every group of equal counts, the zero counts being one group
	double ans1 = F[SEG_ALPHA];
	if (sv[0] != 0) {
		int cl = 1, left = SEG_ALPHA;
		bool done = false;
#pragma unroll
		for (int i = 1; i < SEG_ALPHA; ++i) {
			if (done) continue;
			if (sv[i] == sv[i - 1]) ++cl;
			else {
				left -= cl;
				ans1 -= F[cl];
				if (sv[i] == 0) { ans1 -= F[left]; done = true; }
				cl = 1;
			}
		}
		if (!done) ans1 -= F[cl];
	}
	// s_LnPerm
	double ans2 = F[total];
#pragma unroll
	for (int i = 0; i < SEG_ALPHA; ++i) if (sv[i] != 0) ans2 -= F[sv[i]];
	const double totseq = ((double)total) * 2.9957322735539909;
	const double sum = ans1 + ans2;
	return sum - totseq;
}

// (value, candidate order): the host keeps the first of the smallest values
DMND_HD bool seg_better(double v, int c, double best_v, int best_c) { return v < best_v || (v == best_v && c < best_c); }

// seg::seg_seq over one sequence of `len` letters, wave-uniform on the device and scalar in the emulator. Ops supplies
//   int  next_trigger(int i, int last)           the first centre >= i, <= last of class TRIGGER, or -1
//   int  find_low(int i, int lowlim)             seg_seq's loi: down from i while the class is TRIGGER / EXTEND and the centre >= lowlim
//   int  find_high(int i, int last)              hii likewise, up to last
//   bool trim(int left, int len, int& cut_left, int& cut_right)      false: the raw segment cannot be trimmed here (too long)
//   void emit(int begin, int end)                the next segment of the sequence in ascending list order
//   void remainder_done(int found)               a left remainder was searched and held `found` segments (statistics only)
// and the function returns false when the sequence has to be handed back to the host.
//
// The recursion of seg_seq needs ONE level here, and that is exact: the search of a left remainder contributes only its list head
// (`out.insert(out.begin(), left.front())`), and a list's head is the segment of the LAST trigger of that call's own loop -- what a
// call's own recursions find is inserted before that segment is, so it never becomes the head, and it does not steer the loop either
// (i and lowlim follow from hii and the trim alone). So a remainder's own remainders are never searched: the explicit stack is the
// one saved parent frame below, for any input, and no sequence is handed back for its nesting.
template<typename Ops>
DMND_HD bool seg_drive(Ops& ops, int len)
{
	if (len < SEG_WINDOW) return true;
	int last = len - SEG_UPSET, lowlim = SEG_DOWNSET, i = SEG_DOWNSET;
	// the saved parent frame while a left remainder is searched, and that search's last segment
	bool in_child = false;
	int child_found = 0;
	int p_last = 0, p_hii = 0, p_left = 0, p_right = 0, c_left = 0, c_right = 0;
	for (;;) {
		const int t = ops.next_trigger(i, last);
		if (t < 0) {
			if (!in_child) return true;
			ops.remainder_done(child_found);
			if (child_found) ops.emit(c_left, c_right);
			ops.emit(p_left, p_right);
			in_child = false;
			last = p_last;
			i = p_hii < p_right + SEG_DOWNSET ? p_hii : p_right + SEG_DOWNSET;
			lowlim = i + 1;
			++i;
			continue;
		}
		i = t;
		const int loi = ops.find_low(i, lowlim), hii = ops.find_high(i, last);
		const int left0 = loi - SEG_DOWNSET, right0 = hii + SEG_UPSET - 1;
		int cut_left = 0, cut_right = 0;
		if (!ops.trim(left0, right0 - left0 + 1, cut_left, cut_right)) return false;
		const int left = left0 + cut_left, right = right0 - cut_right;
		if (!in_child) {
			if (i + SEG_UPSET - 1 < left && left - left0 >= SEG_WINDOW) {      // the trigger window lies in what the trim cut off on the left
				in_child = true; child_found = 0;
				p_last = last; p_hii = hii; p_left = left; p_right = right;
				last = left - SEG_UPSET;                                        // the remainder is [left0, left - 1]
				lowlim = i = left0 + SEG_DOWNSET;
				continue;
			}
			ops.emit(left, right);
		}
		else { ++child_found; c_left = left; c_right = right; }
		i = hii < right + SEG_DOWNSET ? hii : right + SEG_DOWNSET;
		lowlim = i + 1;
		++i;
	}
}

}  // namespace dmnd
