// tests/emu/chain_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// Runs the product's chaining (diamond_amd/csrc/chain_graph.h) and the retired round-1 restatement of the reference
// (oracle/chain_ref.h) on the same seed hits of one (query, target) pair and hands both results to the test.
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../diamond_amd/csrc/chain_graph.h"
#include "../../oracle/chain_ref.h"

namespace {

int g_last_links = 0;      // links the last emu_chain call's workspace held after chaining (a fixed instance stops counting at its capacity)

template<typename WsT, typename TableT, typename SeqT, typename SegT, typename ChainT>
bool run_chains(WsT& ws, const TableT& S, const SeqT& qs, const SeqT& ts, const std::vector<SegT>& segs, std::vector<ChainT>& chains)
{
	ws.run(S, qs, ts, segs, chains);
	return true;
}

bool run_chains(dmnd::ChainWorkspace& ws, const dmnd::ScoreTable& S, const dmnd::SeqRef& qs, const dmnd::SeqRef& ts, const std::vector<dmnd::Seg>& segs, std::vector<dmnd::Chain>& chains)
{
	ws.run(S, qs, ts, segs, chains);
	g_last_links = segs.size() > 1 ? (int)ws.links.size() : 0;
	return true;
}

// the device planner's instance of the chaining (fixed-capacity arrays, insertion sort), run on the host: false = a target that does
// not fit its arrays (the device hands those to the host)
typedef dmnd::ChainWorkspaceT<dmnd::FixedChainPolicy> FixedWs;
bool run_chains(FixedWs& ws, const dmnd::ScoreTable& S, const dmnd::SeqRef& qs, const dmnd::SeqRef& ts, const std::vector<dmnd::Seg>& segs, std::vector<dmnd::Chain>& chains)
{
	if (segs.size() > 16) return false;
	dmnd::FixedVec<dmnd::Chain, 16> out;
	ws.run_segs(S, qs, ts, segs.data(), segs.size(), out);
	g_last_links = segs.size() > 1 ? (int)ws.links.size() : 0;
	if (ws.overflowed() || out.overflow) return false;
	chains.assign(out.begin(), out.end());
	return true;
}

// the planner's small instance (plan_chain_kernel<4, 16, 4, true>: groups of two to four segments): false = it does not fit, the
// device lists the group again for the large instance
typedef dmnd::ChainWorkspaceT<dmnd::FixedChainPolicy, 4, 16, 4> SmallWs;
bool run_chains(SmallWs& ws, const dmnd::ScoreTable& S, const dmnd::SeqRef& qs, const dmnd::SeqRef& ts, const std::vector<dmnd::Seg>& segs, std::vector<dmnd::Chain>& chains)
{
	if (segs.size() > 4) return false;
	dmnd::FixedVec<dmnd::Chain, 4> out;
	ws.run_segs(S, qs, ts, segs.data(), segs.size(), out);
	g_last_links = segs.size() > 1 ? (int)ws.links.size() : 0;
	if (ws.overflowed() || out.overflow) return false;
	chains.assign(out.begin(), out.end());
	return true;
}

template<typename SegT, typename SeqT, typename TableT, typename WsT, typename ChainT, typename XdropF>
int run_one(const int8_t* q, int qlen, const int8_t* cbs, const int8_t* t, int tlen, const int8_t* matrix8, int gap_open, int gap_extend,
	const int* hi, const int* hj, int n_hits, int* seg_out, int seg_cap, int* n_segs, int* chain_out, int chain_cap, XdropF xdrop, bool resort)
{
	TableT S;
	for (int i = 0; i < 1024; ++i) S.m[i] = matrix8[i];
	S.gap_open = gap_open; S.gap_extend = gap_extend;
	const SeqT qs{ q, qlen }, ts{ t, tlen };
	WsT ws;
	std::vector<SegT> segs;
	// ungapped_stage: hits sorted by (diagonal, j); a hit inside the previous segment of its diagonal is skipped
	for (int x = 0; x < n_hits; ++x) {
		if (!segs.empty() && segs.back().diag() == hi[x] - hj[x] && segs.back().j_end() >= hj[x]) continue;
		const SegT d = xdrop(S, qs, cbs, ts, hi[x], hj[x], 20);      // config.raw_ungapped_xdrop = rawscore(12.3 bits) for BLOSUM62 11/1, config.cpp:428,853
		if (d.score > 0) segs.push_back(d);
	}
	// the extension stage's own order before chaining (extend_host.hip plan_groups, plan_kernels.hip plan_segments_kernel): stable by
	// (diagonal, segment start). It never moves anything (plan_kernels.hip says why); the tests compare the lists with and without it
	if (resort) std::stable_sort(segs.begin(), segs.end(), [](const SegT& a, const SegT& b) { return a.diag() < b.diag() || (a.diag() == b.diag() && a.j < b.j); });
	*n_segs = (int)segs.size();
	for (int x = 0; x < (int)segs.size() && x < seg_cap; ++x) { seg_out[4 * x] = segs[x].i; seg_out[4 * x + 1] = segs[x].j; seg_out[4 * x + 2] = segs[x].len; seg_out[4 * x + 3] = segs[x].score; }
	g_last_links = 0;
	if (segs.empty()) return 0;
	std::vector<ChainT> chains;
	if (!run_chains(ws, S, qs, ts, segs, chains)) return -1;
	for (int x = 0; x < (int)chains.size() && x < chain_cap; ++x) {
		const ChainT& c = chains[x];
		const int v[7] = { c.d_min, c.d_max, c.score, c.q0, c.q1, c.s0, c.s1 };
		std::memcpy(chain_out + 7 * x, v, sizeof v);
	}
	return (int)chains.size();
}

}

// q / t point INTO padded buffers (delimiter 31 before and after, as in a sequence block). Returns the number of chains, or -1 when a
// fixed-capacity instance (which = 2: 16 / 96 / 16, which = 3: 4 / 16 / 4) does not hold the target.
extern "C" int emu_chain(int which, const int8_t* q, int qlen, const int8_t* cbs, const int8_t* t, int tlen, const int8_t* matrix8, int gap_open, int gap_extend,
	const int* hi, const int* hj, int n_hits, int* seg_out, int seg_cap, int* n_segs, int* chain_out, int chain_cap)
{
	const bool resort = (which & 16) != 0;      // which | 16: the segments are sorted again before chaining, as the extension stage does
	which &= 15;
	if (which == 0)
		return run_one<dmnd::Seg, dmnd::SeqRef, dmnd::ScoreTable, dmnd::ChainWorkspace, dmnd::Chain>(q, qlen, cbs, t, tlen, matrix8, gap_open, gap_extend, hi, hj, n_hits,
			seg_out, seg_cap, n_segs, chain_out, chain_cap,
			[](const dmnd::ScoreTable& S, const dmnd::SeqRef& a, const int8_t* c, const dmnd::SeqRef& b, int i, int j, int x) { return dmnd::xdrop_ungapped(S, a, c, b, i, j, x); }, resort);
	if (which == 2)
		return run_one<dmnd::Seg, dmnd::SeqRef, dmnd::ScoreTable, FixedWs, dmnd::Chain>(q, qlen, cbs, t, tlen, matrix8, gap_open, gap_extend, hi, hj, n_hits,
			seg_out, seg_cap, n_segs, chain_out, chain_cap,
			[](const dmnd::ScoreTable& S, const dmnd::SeqRef& a, const int8_t* c, const dmnd::SeqRef& b, int i, int j, int x) { return dmnd::xdrop_ungapped(S, a, c, b, i, j, x); }, resort);
	if (which == 3)
		return run_one<dmnd::Seg, dmnd::SeqRef, dmnd::ScoreTable, SmallWs, dmnd::Chain>(q, qlen, cbs, t, tlen, matrix8, gap_open, gap_extend, hi, hj, n_hits,
			seg_out, seg_cap, n_segs, chain_out, chain_cap,
			[](const dmnd::ScoreTable& S, const dmnd::SeqRef& a, const int8_t* c, const dmnd::SeqRef& b, int i, int j, int x) { return dmnd::xdrop_ungapped(S, a, c, b, i, j, x); }, resort);
	return run_one<dmnd_ref::Seg, dmnd_ref::SeqRef, dmnd_ref::ScoreTable, dmnd_ref::ChainWorkspace, dmnd_ref::Chain>(q, qlen, cbs, t, tlen, matrix8, gap_open, gap_extend, hi, hj, n_hits,
		seg_out, seg_cap, n_segs, chain_out, chain_cap,
		[](const dmnd_ref::ScoreTable& S, const dmnd_ref::SeqRef& a, const int8_t* c, const dmnd_ref::SeqRef& b, int i, int j, int x) { return dmnd_ref::xdrop_ungapped(S, a, c, b, i, j, x); }, resort);
}

// links in the workspace after the last emu_chain call's chaining (which = 0: the host instance, the true number)
extern "C" int emu_chain_last_links() { return g_last_links; }

// lanes per workgroup of the planner's two chaining kernels (ChainLanes<...>::value): small = 1: the 4 / 16 / 4 instance
extern "C" int emu_chain_lanes(int small)
{
	return small ? (int)dmnd::ChainLanes<4, 16, 4>::value : (int)dmnd::ChainLanes<16, 96, 16>::value;
}
