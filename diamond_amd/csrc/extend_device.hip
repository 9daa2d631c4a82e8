// extend_device.hip -- the host side of the device half of dmnd_extend (round 6; split out of extend_host.hip): plan_on_device
// launches the planner (plan_kernels.hip: /root/reference/src/align/load_hits.h:44-127, ungapped.cpp:62-126, chaining/greedy_align.cpp,
// gapped_score.cpp:41-180) and reads its counters; extend_on_device drives the ranking iterations of the planned queries in HBM
// (extend_kernels.hip: /root/reference/src/align/extend.cpp:289-336, gapped_score.cpp:182-268, culling.cpp:97-113, gapped_final.cpp:66-160)
// -- per iteration one counter read-back, the sweeps of its band classes (api.hip dmnd_sweep_classes), append_hits on the device --
// then round 2, the records, the host's own e-value and bit score written back into the records where they stay for the join.
// A call with a transcript arena walks each list in pieces, keeps every piece's packed transcripts in a dense store and gathers the
// records' transcripts into the arena once the records exist (extend_kernels.h TrArgs, transcript_core.h).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "ctx.h"
#include "host_pool.h"
#include "bias_kernels.h"
#include "plan_kernels.h"
#include "extend_kernels.h"
#include "extend_device.h"
#include "match_order.h"
#include "cbs_adjust.h"
#include "cbs_model.h"

using namespace dmnd;

namespace {

// DMND_EXTEND_GUARD (a test hook, read per call): the bytes of a work buffer behind the call's layout, [used, cap), are filled with
// a pattern before its kernels run and read back once at its end; a kernel or a clear that wrote past the layout changed some of
// them, and the call fails with the extent. Off (the default): nothing is done.
struct Guard {
	enum { PATTERN = 0xA5 };
	const DevBuf& buf;
	size_t used;
	hipStream_t st;
	bool on;
	Guard(const DevBuf& b, size_t used_bytes, hipStream_t s) : buf(b), used(used_bytes), st(s), on(std::getenv("DMND_EXTEND_GUARD") != nullptr && b.cap > used_bytes) {}
	int arm() const
	{
		if (on) HIP_TRY(hipMemsetAsync(buf.as<char>() + used, PATTERN, buf.cap - used, st));
		return DMND_OK;
	}
	int check(const char* who) const
	{
		if (!on) return DMND_OK;
		std::vector<uint8_t> h(buf.cap - used);
		HIP_TRY(copy_now(st, h.data(), buf.as<char>() + used, h.size(), hipMemcpyDeviceToHost));
		size_t n_changed = 0, last = 0;
		for (size_t i = 0; i < h.size(); ++i) if (h[i] != PATTERN) { ++n_changed; last = i; }
		if (n_changed == 0) return DMND_OK;
		return fail(DMND_E_CAP, std::string(who) + ": " + std::to_string(n_changed) + " bytes past the end of the work arrays (" + std::to_string(used) +
			" bytes) were overwritten, up to " + std::to_string(last + 1) + " bytes past it");
	}
};

// DMND_EXTEND_MAX_CHUNKS (a test hook, read per call): ranking chunks a query may take on the device, 1 .. EXT_MAX_ITERATIONS
int ext_max_chunks()
{
	const char* e = std::getenv("DMND_EXTEND_MAX_CHUNKS");
	return e ? std::max(1, std::min(atoi(e), (int)EXT_MAX_ITERATIONS)) : (int)EXT_MAX_ITERATIONS;
}

// DMND_EXTEND_PIECE_KB (a capacity knob, read per call): with a transcript arena a walked list is walked in consecutive pieces whose
// raw transcript slots (query + target + 2 bytes per entry) come to at most this many KB -- at least one entry per piece; each
// piece's transcripts are kept in the dense store before the next piece is walked. Default 256 MB.
int64_t tr_piece_bytes()
{
	const char* e = std::getenv("DMND_EXTEND_PIECE_KB");
	return (e ? std::max<int64_t>(1, std::min<int64_t>(std::atoll(e), (int64_t)1 << 32)) : (int64_t)256 << 10) << 10;
}

// more room in a buffer whose first keep_bytes bytes stay (the store of the kept transcripts grows piece by piece)
int grow_keeping(DevBuf& b, size_t need, size_t keep_bytes, hipStream_t st)
{
	if (need <= b.cap && b.own) return DMND_OK;
	DevBuf nb;
	if (int rc = nb.ensure(std::max(need, 2 * b.cap))) return rc;
	if (keep_bytes > 0) {
		const hipError_t e = copy_now(st, nb.p, b.p, keep_bytes, hipMemcpyDeviceToDevice);
		if (e != hipSuccess) { nb.release(); return fail(DMND_E_DEVICE, std::string("the store of the kept transcripts: ") + hipGetErrorString(e)); }
	}
	else HIP_TRY(sync_stream(st));                      // (no kernel of the stream still reads the old one)
	b.release();
	b = nb;
	return DMND_OK;
}

// events of the transcript steps' kernel times (DMND_TRACE only)
struct TrEvents {
	hipEvent_t e[2] = { nullptr, nullptr };
	bool on = false;
	int init() { for (hipEvent_t& x : e) HIP_TRY(hipEventCreate(&x)); on = true; return DMND_OK; }
	~TrEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

// DMND_PLAN_SMALL_HITS (a test hook, read per call): a call of at least this many hits chains its groups of up to four segments
// with the small workspace first (the two-kernel form of plan_kernels.hip); 0 = every call
int64_t plan_small_hits()
{
	const char* e = std::getenv("DMND_PLAN_SMALL_HITS");
	return e ? std::max<int64_t>(0, std::atoll(e)) : (int64_t)1 << 18;
}

}  // namespace

// Runs the planner over the call's hits (in c->xd_hits, with their x-drop extensions in c->xd_out and -- gf_on -- their gapped
// filter flags in c->gf_flags), waits for it and copies its lists to the host. planned = false: the hits are not in
// (query, location, seed offset) order, the host has to plan.
int dmnd::plan_on_device(dmnd_ctx* c, const DeviceCfg& h, int64_t n_hits, bool gf_on, DevPlan& plan, bool& planned)
{
	planned = false;
	const size_t n = (size_t)n_hits;
	auto align = [](size_t x) { return (x + 63) & ~(size_t)63; };
	const size_t o_tgt = 0, o_heads = align(o_tgt + n * sizeof(uint32_t)), o_scan = align(o_heads + n * sizeof(uint64_t)),
		o_groups = align(o_scan + n * sizeof(uint64_t)), o_queries = align(o_groups + (n + 1) * sizeof(PlanGroup)),
		o_segs = align(o_queries + (n + 1) * sizeof(PlanQuery)), o_slots = align(o_segs + n * 4 * sizeof(int32_t)),
		o_count = align(o_slots + n * sizeof(PlanBand)), o_off = align(o_count + (n + 1) * sizeof(uint32_t)),
		o_bands = align(o_off + (n + 1) * sizeof(uint32_t)), o_counters = align(o_bands + n * sizeof(PlanBand)),
		o_chain = align(o_counters + sizeof(PlanCounters)), o_tr = align(o_chain + (n + 2) * sizeof(uint32_t));      // (both chaining lists, and a small group listed again)
	// translated queries: the sort, the permuted lists, the pairs (plan_kernels.h)
	const bool translated = h.contexts > 1;
	const size_t t_hits = o_tr, t_xd = align(t_hits + n * sizeof(dmnd_seed_hit)), t_gf = align(t_xd + n * sizeof(XdropSeg)), t_keys = align(t_gf + n),
		t_keys2 = align(t_keys + n * sizeof(uint64_t)), t_perm_in = align(t_keys2 + n * sizeof(uint64_t)), t_perm = align(t_perm_in + n * sizeof(uint32_t)),
		t_pheads = align(t_perm + n * sizeof(uint32_t)), t_pscan = align(t_pheads + n * sizeof(uint32_t)), t_pairs = align(t_pscan + n * sizeof(uint32_t)),
		t_pair_unit = align(t_pairs + (n + 1) * sizeof(PlanGroup)), t_unit_pair = align(t_pair_unit + (n + 1) * sizeof(uint32_t)),
		t_ungapped = align(t_unit_pair + n * sizeof(uint32_t)), t_band_query = align(t_ungapped + n * sizeof(uint16_t)), t_end = align(t_band_query + n * sizeof(uint32_t));
	const size_t bytes = translated ? t_end : o_tr;
	TraceLaps tr("dmnd_extend (planner)");
	if (int rc = c->plan_dev.ensure(bytes)) return rc;
	Guard guard(c->plan_dev, bytes, c->stream);
	if (int rc = guard.arm()) return rc;
	tr.lap("work arrays");
	char* d = c->plan_dev.as<char>();
	PlanArgs a;
	a.qblock = c->block[DMND_QUERY].as<int8_t>(); a.tblock = c->block[DMND_TARGET].as<int8_t>();
	a.qlimits = c->d_limits[DMND_QUERY].as<int64_t>(); a.tlimits = c->d_limits[DMND_TARGET].as<int64_t>();
	a.n_targets = (int64_t)c->limits[DMND_TARGET].size() - 1;
	a.matrix = c->matrix.as<int8_t>();
	a.hits = c->xd_hits.as<dmnd_seed_hit>(); a.n_hits = n_hits;
	a.gf_flags = gf_on ? c->gf_flags.as<uint8_t>() : nullptr;
	a.xd = h.ext_full ? nullptr : c->xd_out.as<XdropSeg>();      // (Mode::FULL has no x-drop stage: plan_full_kernel)
	a.ext_full = h.ext_full ? 1 : 0;
	a.gap_open = h.gap_open; a.gap_extend = h.gap_extend; a.band_fast = h.band_mode_fast;
	a.small_segs = n_hits >= plan_small_hits() ? 4 : 0;
	a.tgt = reinterpret_cast<uint32_t*>(d + o_tgt); a.heads = reinterpret_cast<uint64_t*>(d + o_heads); a.head_scan = reinterpret_cast<uint64_t*>(d + o_scan);
	a.groups = reinterpret_cast<PlanGroup*>(d + o_groups); a.queries = reinterpret_cast<PlanQuery*>(d + o_queries);
	a.segs = reinterpret_cast<int32_t*>(d + o_segs); a.band_slots = reinterpret_cast<PlanBand*>(d + o_slots);
	a.band_count = reinterpret_cast<uint32_t*>(d + o_count); a.band_off = reinterpret_cast<uint32_t*>(d + o_off);
	a.bands = reinterpret_cast<PlanBand*>(d + o_bands); a.counters = reinterpret_cast<PlanCounters*>(d + o_counters);
	a.chain_list = reinterpret_cast<uint32_t*>(d + o_chain); a.chain_cap = (uint32_t)(n + 2);
	a.scan_tmp = &c->plan_tmp; a.scan_tmp_bytes = &c->plan_tmp_bytes;
	a.contexts = h.contexts;
	a.hits_in = nullptr; a.gf_in = nullptr; a.xd_in = nullptr; a.hits_sorted = nullptr; a.gf_sorted = nullptr; a.xd_sorted = nullptr;
	a.keys = nullptr; a.keys_sorted = nullptr; a.perm_in = nullptr; a.perm = nullptr; a.target_bits = 0; a.key_bits = 0;
	a.pheads = nullptr; a.phead_scan = nullptr; a.pairs = nullptr; a.pair_unit = nullptr; a.unit_pair = nullptr; a.ungapped0 = nullptr; a.band_query = nullptr;
	if (translated) {
		a.hits_in = a.hits; a.gf_in = a.gf_flags; a.xd_in = a.xd;
		a.hits_sorted = reinterpret_cast<dmnd_seed_hit*>(d + t_hits); a.xd_sorted = reinterpret_cast<XdropSeg*>(d + t_xd); a.gf_sorted = reinterpret_cast<uint8_t*>(d + t_gf);
		a.hits = a.hits_sorted; a.xd = a.xd_sorted; a.gf_flags = gf_on ? a.gf_sorted : nullptr;
		a.keys = reinterpret_cast<uint64_t*>(d + t_keys); a.keys_sorted = reinterpret_cast<uint64_t*>(d + t_keys2);
		a.perm_in = reinterpret_cast<uint32_t*>(d + t_perm_in); a.perm = reinterpret_cast<uint32_t*>(d + t_perm);
		const PlanKeyBits kb = plan_key_bits((uint64_t)((c->limits[DMND_QUERY].size() - 1 + (size_t)h.contexts - 1) / (size_t)h.contexts), (uint64_t)a.n_targets);      // (extend_cfg refuses a block that is no multiple of the contexts; rounded up all the same)
		a.target_bits = kb.target_bits; a.key_bits = kb.target_bits + kb.read_bits;
		a.pheads = reinterpret_cast<uint32_t*>(d + t_pheads); a.phead_scan = reinterpret_cast<uint32_t*>(d + t_pscan);
		a.pairs = reinterpret_cast<PlanGroup*>(d + t_pairs); a.pair_unit = reinterpret_cast<uint32_t*>(d + t_pair_unit); a.unit_pair = reinterpret_cast<uint32_t*>(d + t_unit_pair);
		a.ungapped0 = reinterpret_cast<uint16_t*>(d + t_ungapped); a.band_query = reinterpret_cast<uint32_t*>(d + t_band_query);
	}
	HIP_TRY(launch_plan(a, c->stream));
	tr.lap("launched");
	if (int rc = c->plan_host.ensure(sizeof(PlanCounters))) return rc;
	tr.lap("host buffer");
	HIP_TRY(copy_now(c->stream, c->plan_host.p, a.counters, sizeof(PlanCounters), hipMemcpyDeviceToHost));
	tr.lap("counters back");
	const PlanCounters cn = *c->plan_host.as<PlanCounters>();
	if (int rc = guard.check("dmnd_extend (planner)")) return rc;
	plan.unsorted = cn.unsorted != 0;
	if (cn.unsorted || cn.n_groups == 0) return DMND_OK;
	plan.n_groups = cn.n_groups; plan.n_queries = cn.n_queries; plan.n_bands = cn.n_bands; plan.n_on_host = cn.n_on_host;
	plan.n_chain = cn.n_chain; plan.n_chain_big = cn.n_chain_big; plan.n_relisted = cn.n_relisted;
	plan.dev = a;
	if (translated) {
		// the device half and the callers see the pairs: what is ranked, extended and reported per read
		plan.n_groups = cn.n_pairs; plan.n_on_host = cn.n_pairs_on_host;
		plan.dev.groups = a.pairs;
	}
	planned = true;
	return DMND_OK;
}

// The planner's lists on the host (page-locked copies, valid until the context's next dmnd_extend): only the host path reads them
int dmnd::plan_fetch_lists(dmnd_ctx* c, DevPlan& plan)
{
	if (plan.groups) return DMND_OK;
	auto align = [](size_t x) { return (x + 63) & ~(size_t)63; };
	const size_t h_groups = align(sizeof(PlanCounters)), h_queries = align(h_groups + (size_t)plan.n_groups * sizeof(PlanGroup)),
		h_bands = align(h_queries + ((size_t)plan.n_queries + 1) * sizeof(PlanQuery)), h_bq = align(h_bands + (size_t)plan.n_bands * sizeof(PlanBand)),
		h_ug = align(h_bq + (plan.dev.band_query ? (size_t)plan.n_bands * sizeof(uint32_t) : 0)), h_bytes = h_ug + (plan.dev.ungapped0 ? (size_t)plan.n_groups * sizeof(uint16_t) : 0);
	if (int rc = c->plan_host.ensure(h_bytes)) return rc;
	char* hp = c->plan_host.as<char>();
	HIP_TRY(hipMemcpyAsync(hp + h_groups, plan.dev.groups, (size_t)plan.n_groups * sizeof(PlanGroup), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(hipMemcpyAsync(hp + h_queries, plan.dev.queries, ((size_t)plan.n_queries + 1) * sizeof(PlanQuery), hipMemcpyDeviceToHost, c->stream));
	if (plan.n_bands) HIP_TRY(hipMemcpyAsync(hp + h_bands, plan.dev.bands, (size_t)plan.n_bands * sizeof(PlanBand), hipMemcpyDeviceToHost, c->stream));
	if (plan.dev.band_query && plan.n_bands) HIP_TRY(hipMemcpyAsync(hp + h_bq, plan.dev.band_query, (size_t)plan.n_bands * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	if (plan.dev.ungapped0) HIP_TRY(hipMemcpyAsync(hp + h_ug, plan.dev.ungapped0, (size_t)plan.n_groups * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
	HIP_TRY(sync_stream(c->stream));
	if (plan.dev.band_query) plan.band_query = reinterpret_cast<const uint32_t*>(hp + h_bq);
	if (plan.dev.ungapped0) plan.ungapped0 = reinterpret_cast<const uint16_t*>(hp + h_ug);
	plan.groups = reinterpret_cast<const PlanGroup*>(hp + h_groups);
	plan.queries = reinterpret_cast<const PlanQuery*>(hp + h_queries);
	plan.bands = reinterpret_cast<const PlanBand*>(hp + h_bands);
	return DMND_OK;
}

// DMND_EXTEND_KEEP_TRACE=0 (read per call, like the hooks above: a test compares both forms in one process): round 1 keeps no trace rows
static bool keep_traces_dev() { const char* e = std::getenv("DMND_EXTEND_KEEP_TRACE"); return !e || e[0] != '0'; }

// The extension of the planned queries, ranking chunk by ranking chunk, in HBM from the planner's bands to the match records
// (extend_kernels.h): -k culling by e-value, or -- h.top >= 0 -- the --top culling by score, either with or without the HSP filters.
// records: those queries' matches in output order (query ascending; inside a query e-value, score, target, or under --top score,
// target) with the HOST's e-value and bit score; qstate[k] (k = index into plan.queries): EXT_Q_DEVICE = done here, anything else = the host path
// has to extend the query. done = false: nothing was done here (no eligible query, or the kept traces would not fit the context's
// trace budget), every query goes to the host path.
int dmnd::extend_on_device(dmnd_ctx* c, const DeviceCfg& h, const DevPlan& plan, int threads, std::vector<dmnd_match>& records, std::vector<uint8_t>& qstate, bool& done,
	uint8_t* transcript, int64_t transcript_cap, int64_t* transcript_used, const int8_t* qdata, const int8_t* tdata)
{
	done = false;
	if (transcript_used) *transcript_used = 0;
	TraceLaps tr("dmnd_extend (device half)");
	const int64_t chunk = h.ranking_chunk;
	if (chunk > EXT_MAX_CHUNK || plan.n_bands == 0) return DMND_OK;
	// --comp-based-stats 2 - 5: every group that is swept owns a 1 KB slot of the context's matrix store until the call ends (g_mat). A
	// call whose groups could ask for more than one pass of the host path may hold (DMND_CBS_PASS_HITS slots, 2 GB by default) is
	// left to the host path and its passes as a whole.
	const bool adjust = h.cbs_model != nullptr && cbs_matrix_adjust(h.cbs_mode);
	if (adjust && (h.ext_full || h.contexts > 1 || !qdata || !tdata || (int64_t)plan.n_groups > dmnd_cbs_pass_hits())) return DMND_OK;
	const bool top = h.top >= 0.0;                      // (--top: no LDS list, -k plays no part)
	if (!top && ((size_t)h.max_target_seqs + 2 * (size_t)chunk) * 24 > ((size_t)60 << 10)) return DMND_OK;      // (the LDS lists of ext_append_kernel)
	const bool filt = filters_on(h.filters);
	// (with filters: the aligned targets of a query and a chunk, and the matches of all rounds -- fewer than 2 k --, fit the LDS list)
	if (!top && filt && ((size_t)h.max_target_seqs + (size_t)chunk > EXT_FILTER_LIST || 2 * (size_t)h.max_target_seqs > EXT_FILTER_LIST)) return DMND_OK;
	const bool fchunk = filt && !top;                   // the chunk-by-chunk walk of the -k filter path (under --top the filters come after the one walk)
	// translated queries with filters: the filter kernel measures the query cover on the DNA read, one length per read of the block
	// (a call without them is not taken: dmnd_extend's gate; checked here again, the kernel indexes the array by read)
	const bool read_lens = filt && h.contexts > 1;
	const size_t n_reads = (c->limits[DMND_QUERY].size() - 1) / (size_t)h.contexts;
	if (read_lens && (n_reads == 0 || c->source_lens.size() != n_reads)) return DMND_OK;
	const ExtLayout L = ext_layout(plan.n_groups, plan.n_queries, plan.n_bands, h.max_target_seqs, filt, top);
	const size_t nQ = L.nQ, nR = L.nR;
	if (int rc = c->ext_dev.ensure(L.bytes)) return rc;
	Guard guard(c->ext_dev, L.bytes, c->stream);
	if (int rc = guard.arm()) return rc;
	// The read lengths in HBM: exactly one int32 per read, copied on the call's stream when the query block or the lengths themselves
	// have changed since the copy was made (dmnd_upload_block, dmnd_share_block and dmnd_set_query_source_lengths all void it)
	const size_t sl_bytes = read_lens ? n_reads * sizeof(int32_t) : 0;
	if (read_lens) {
		if (c->ext_source_lens.cap < sl_bytes || !c->ext_source_lens.own) c->source_lens_generation = ~(uint64_t)0;      // (the buffer is about to be replaced)
		if (int rc = c->ext_source_lens.ensure(sl_bytes)) return rc;
	}
	Guard guard_sl(c->ext_source_lens, sl_bytes, c->stream);
	if (read_lens) {
		if (int rc = guard_sl.arm()) return rc;
		if (c->source_lens_generation != c->query_generation) {
			HIP_TRY(copy_now(c->stream, c->ext_source_lens.p, c->source_lens.data(), sl_bytes, hipMemcpyHostToDevice));
			c->source_lens_generation = c->query_generation;
		}
	}
	// with a transcript arena: the arrays between the trace walk and the arena, in a buffer of their own (extend_core.h tr_layout)
	const bool with_tr = transcript != nullptr;
	const TrLayout T = tr_layout(L.nG, L.nS, nR);
	if (with_tr) if (int rc = c->ext_tr.ensure(T.bytes)) return rc;
	Guard guard_tr(c->ext_tr, T.bytes, c->stream);
	if (with_tr) if (int rc = guard_tr.arm()) return rc;
	TrArgs ta{};
	if (with_tr) {
		char* dt = c->ext_tr.as<char>();
		ta.g_store = reinterpret_cast<int64_t*>(dt + T.o_g_store); ta.k_len = reinterpret_cast<int64_t*>(dt + T.o_k_len); ta.k_off = reinterpret_cast<int64_t*>(dt + T.o_k_off);
		ta.r_len = reinterpret_cast<int64_t*>(dt + T.o_r_len); ta.r_off = reinterpret_cast<int64_t*>(dt + T.o_r_off);
		ta.pieces = reinterpret_cast<uint32_t*>(dt + T.o_pieces); ta.ctr = reinterpret_cast<TrCounters*>(dt + T.o_ctr);
		HIP_TRY(hipMemsetAsync(ta.g_store, 0xff, L.nG * sizeof(int64_t), c->stream));      // (-1: no transcript of the group in the store)
		HIP_TRY(hipMemsetAsync(ta.ctr, 0, sizeof(TrCounters), c->stream));
	}
	// with matrix adjustment: the arrays of that step in a buffer of their own (extend_cbs_core.h ext_cbs_layout); page-locked beside
	// them the step's counters, the kernel's model and what comes back of an iteration's pairs
	const ExtCbsLayout X = ext_cbs_layout(L.nG, nQ);
	if (adjust) if (int rc = c->ext_cbs.ensure(X.bytes)) return rc;
	Guard guard_cbs(c->ext_cbs, X.bytes, c->stream);
	if (adjust) if (int rc = guard_cbs.arm()) return rc;
	auto up64 = [](size_t x) { return (x + 63) & ~(size_t)63; };
	const size_t hx_ctr = 0, hx_model = up64(sizeof(ExtCbsCounters)), hx_rule = up64(hx_model + sizeof(CbsDevModel)), hx_status = up64(hx_rule + L.nG * 4),
		hx_qidx = up64(hx_status + L.nG), hx_toff = up64(hx_qidx + L.nG * 4), hx_tlen = up64(hx_toff + L.nG * 8), hx_qoff = up64(hx_tlen + L.nG * 4),
		hx_qlen = up64(hx_qoff + L.nG * 8), hx_keep = up64(hx_qlen + L.nG * 4), hx_bytes = up64(hx_keep + L.nG);
	if (adjust) if (int rc = c->cbs_host.ensure(hx_bytes)) return rc;
	char* const hx = adjust ? c->cbs_host.as<char>() : nullptr;
	const int64_t piece_limit = tr_piece_bytes();
	size_t tr_pieces = 0, tr_raw = 0, tr_kept = 0, tr_gathered = 0;      // of the call: pieces walked, raw-slot bytes, bytes in the store, bytes in the arena
	double ms_tr_walk = 0, ms_tr_keep = 0, ms_tr_gather = 0;
	TrEvents tev;
	if (with_tr && tr.on) if (int rc = tev.init()) return rc;
	tr.lap("work arrays");
	char* d = c->ext_dev.as<char>();
	ExtArgs a;
	a.tr_on = with_tr ? 1 : 0;
	a.groups = plan.dev.groups; a.queries = plan.dev.queries; a.bands = plan.dev.bands;
	a.n_groups = plan.n_groups; a.n_queries = plan.n_queries; a.n_bands = plan.n_bands;
	a.hits = plan.dev.hits; a.qlimits = plan.dev.qlimits; a.tlimits = plan.dev.tlimits;
	a.contexts = h.contexts; a.band_query = plan.dev.band_query; a.ungapped0 = plan.dev.ungapped0;
	a.source_lens = read_lens ? c->ext_source_lens.as<int32_t>() : nullptr;
	a.ext_full = h.ext_full ? 1 : 0;
	a.use_cbs = h.use_cbs ? 1 : 0; a.row_min_items = (uint32_t)std::min<int64_t>(sweep_rows_min_items(), 0xffffffffll); a.chunk_size = (uint32_t)chunk; a.k = h.max_target_seqs; a.max_swipe_dp = h.max_swipe_dp;
	const Evaluer& E = c->evaluer;
	a.min_bit_score = h.min_bit_score; a.filt = h.filters; a.filt_on = filt ? 1 : 0;
	a.top = top_cfg(top ? h.top : 0.0, E.lambda, E.ln_k); a.top_on = top ? 1 : 0;
	a.cand_score = reinterpret_cast<int32_t*>(d + L.o_cand_score); a.rperm = reinterpret_cast<uint32_t*>(d + L.o_rperm);
	a.ev = ExtEvalue{ E.lambda, E.K, E.ln_k, E.db_letters, E.a, E.b, E.alpha, E.beta, E.sigma, E.tau, E.v_thr, E.c_thr, h.max_evalue };
	a.qstate = reinterpret_cast<uint8_t*>(d + L.o_qstate); a.q_active = reinterpret_cast<uint8_t*>(d + L.o_qactive);
	a.q_i0 = reinterpret_cast<uint32_t*>(d + L.o_qi0); a.q_i1 = reinterpret_cast<uint32_t*>(d + L.o_qi1);
	a.q_tail = reinterpret_cast<int32_t*>(d + L.o_qtail); a.q_prev = reinterpret_cast<int32_t*>(d + L.o_qprev); a.q_swept = reinterpret_cast<uint32_t*>(d + L.o_qswept);
	a.okeys = reinterpret_cast<uint64_t*>(d + L.o_okeys); a.okeys_sorted = reinterpret_cast<uint64_t*>(d + L.o_okeys2);
	a.oidx = reinterpret_cast<uint32_t*>(d + L.o_oidx); a.gorder = reinterpret_cast<uint32_t*>(d + L.o_gorder);
	a.aligned = reinterpret_cast<uint8_t*>(d + L.o_aligned); a.g_first = reinterpret_cast<uint32_t*>(d + L.o_gfirst); a.g_cnt = reinterpret_cast<uint32_t*>(d + L.o_gcnt);
	a.cnt = reinterpret_cast<uint32_t*>(d + L.o_cnt); a.item_off = reinterpret_cast<uint32_t*>(d + L.o_item_off);
	a.kept = reinterpret_cast<uint32_t*>(d + L.o_kept); a.kept_pos = reinterpret_cast<uint32_t*>(d + L.o_kept_pos);
	a.cand_item = reinterpret_cast<uint32_t*>(d + L.o_cand_item); a.cand_ev = reinterpret_cast<double*>(d + L.o_cand_ev);
	a.fverdict = reinterpret_cast<uint8_t*>(d + L.o_fverdict); a.matched = reinterpret_cast<uint8_t*>(d + L.o_matched);
	a.q_matched = reinterpret_cast<uint32_t*>(d + L.o_qmatched); a.q_removed = reinterpret_cast<uint32_t*>(d + L.o_qremoved);
	a.item_base = 0; a.item_cap = (uint32_t)L.nI;
	a.items = reinterpret_cast<dmnd_dp_target*>(d + L.o_items); a.off_item = reinterpret_cast<int64_t*>(d + L.o_off_item);
	a.p_of_item = reinterpret_cast<int32_t*>(d + L.o_p); a.ends = reinterpret_cast<SwipeEnd*>(d + L.o_ends); a.hsps = reinterpret_cast<dmnd_hsp*>(d + L.o_hsps);
	a.keys = reinterpret_cast<uint32_t*>(d + L.o_keys); a.keys_sorted = reinterpret_cast<uint32_t*>(d + L.o_keys_sorted);
	a.idx = reinterpret_cast<uint32_t*>(d + L.o_idx); a.order = reinterpret_cast<uint32_t*>(d + L.o_order);
	a.rows = reinterpret_cast<int64_t*>(d + L.o_rows); a.rows_slot = reinterpret_cast<int64_t*>(d + L.o_rows_slot); a.off_slot = reinterpret_cast<int64_t*>(d + L.o_off_slot);
	a.pairs = reinterpret_cast<int32_t*>(d + L.o_pairs);
	a.r2_cap = (uint32_t)L.nS; a.r2_tr_clear = (uint32_t)L.r2_tr_clear;
	a.r2_order = reinterpret_cast<int32_t*>(d + L.o_r2_order); a.r2_p = reinterpret_cast<int32_t*>(d + L.o_r2_p);
	a.r2_off = reinterpret_cast<int64_t*>(d + L.o_r2_off); a.r2_tr = reinterpret_cast<int64_t*>(d + L.o_r2_tr); a.r2_group = reinterpret_cast<uint32_t*>(d + L.o_r2_group);
	a.records = reinterpret_cast<dmnd_match*>(d + L.o_records);
	a.ctr = reinterpret_cast<ExtCounters*>(d + L.o_ctr);
	a.scan_tmp = &c->plan_tmp; a.scan_tmp_bytes = &c->plan_tmp_bytes;
	a.g_mat = nullptr; a.g_row = nullptr; a.q_comp = nullptr; a.q_true_aa = nullptr; a.c_flag = nullptr; a.c_pos = nullptr;
	a.pair_group = nullptr; a.pair_qidx = nullptr; a.pair_toff = nullptr; a.pair_tlen = nullptr; a.pair_qoff = nullptr; a.pair_qlen = nullptr;
	a.pair_rule = nullptr; a.pair_status = nullptr; a.pair_keep = nullptr; a.cbs_ctr = nullptr;
	const CbsDevModel* cbs_model_dev = nullptr;
	if (adjust) {
		char* dx = c->ext_cbs.as<char>();
		a.g_mat = reinterpret_cast<int32_t*>(dx + X.o_g_mat); a.g_row = reinterpret_cast<uint32_t*>(dx + X.o_g_row);
		a.q_comp = reinterpret_cast<double*>(dx + X.o_comp); a.q_true_aa = reinterpret_cast<int32_t*>(dx + X.o_true_aa);
		a.c_flag = reinterpret_cast<uint32_t*>(dx + X.o_flag); a.c_pos = reinterpret_cast<uint32_t*>(dx + X.o_pos);
		a.pair_group = reinterpret_cast<uint32_t*>(dx + X.o_pair_group); a.pair_qidx = reinterpret_cast<int32_t*>(dx + X.o_qidx);
		a.pair_toff = reinterpret_cast<int64_t*>(dx + X.o_toff); a.pair_tlen = reinterpret_cast<int32_t*>(dx + X.o_tlen);
		a.pair_qoff = reinterpret_cast<int64_t*>(dx + X.o_qoff); a.pair_qlen = reinterpret_cast<int32_t*>(dx + X.o_qlen);
		a.pair_rule = reinterpret_cast<int32_t*>(dx + X.o_rule); a.pair_status = reinterpret_cast<uint8_t*>(dx + X.o_status);
		a.pair_keep = reinterpret_cast<uint8_t*>(dx + X.o_keep); a.cbs_ctr = reinterpret_cast<ExtCbsCounters*>(dx + X.o_ctr);
		cbs_model_dev = reinterpret_cast<const CbsDevModel*>(dx + X.o_model);
	}
	hipStream_t st = c->stream;
	// (page-locked, behind the counters: the transcript counters, one 64-bit value, the bounds of a walk's pieces)
	const size_t h_trc = (sizeof(ExtCounters) + 63) & ~(size_t)63, h_val = h_trc + ((sizeof(TrCounters) + 63) & ~(size_t)63), h_pieces = h_val + 64;
	if (int rc = c->ext_host.ensure(h_pieces + 64)) return rc;
	// Round 1 sweeps in traceback mode and keeps the trace rows (round 2 then only walks them) while the iterations' rows fit the
	// context's trace budget: the first iteration's in ext_trace, every later one's in an arena of its own, all addressed from
	// ext_trace's base (64-bit offsets). An iteration that does not fit is swept for scores only, and round 2 sweeps its survivors
	// again with traceback -- what the reference's round 2 does for every survivor.
	const size_t trace_budget = c->trace_arena_max;
	size_t trace_used = 0, n_more = 0;
	auto arena_for = [&](size_t bytes, DevBuf*& arena, int64_t& rel) -> int {
		arena = &c->ext_trace;
		if (trace_used > 0) {
			if (c->ext_trace_more.size() <= n_more) c->ext_trace_more.resize(n_more + 1);
			arena = &c->ext_trace_more[n_more++];
		}
		if (int rc = arena->ensure(bytes + 64)) return rc;
		if (!c->ext_trace.p) { if (int rc = c->ext_trace.ensure(64)) return rc; }
		rel = (int64_t)(arena->as<char>() - c->ext_trace.as<char>());
		trace_used += bytes;
		return DMND_OK;
	};
	HIP_TRY(launch_ext_begin(a, st));
	ExtCounters ctr;
	// the matrix adjustment step of a ranking iteration (extend_kernels.h): state of the call
	const int cbs_max_its = adjust ? dmnd_cbs_env_max_its() : 0;
	std::vector<uint32_t> cbs_tally;                      // per planned query: pairs by status (a query that goes back to the host path takes its pairs along)
	std::vector<int32_t> cbs_mat;
	std::vector<int64_t> cbs_handed;
	std::vector<uint8_t> cbs_kept;
	std::vector<int8_t> cbs_patch;
	std::vector<CbsPatchRun> cbs_runs;
	double cbs_ms = 0;
	if (adjust) {
		c->n_adj_matrices = 0;                              // (the store starts empty, as extend_range's does)
		cbs_dev_model(*reinterpret_cast<CbsDevModel*>(hx + hx_model), *h.cbs_model, h.cbs_mode, cbs_max_its);
		HIP_TRY(hipMemcpyAsync(const_cast<CbsDevModel*>(cbs_model_dev), hx + hx_model, sizeof(CbsDevModel), hipMemcpyHostToDevice, st));
		HIP_TRY(launch_ext_cbs_begin(a, c->block[DMND_QUERY].as<int8_t>(), st));
		cbs_tally.assign(nQ * 4, 0);
	}
	// the iteration's counters on the host; the launch classes as dmnd_sweep_classes takes them: with matrix adjustment the classes of
	// the own-matrix items behind the sixteen of the standard matrix
	uint32_t cls_count[EXT_ALL_CLASSES] = { 0 }, cls_steps[EXT_ALL_CLASSES] = { 0 };
	const int n_cls = adjust ? (int)EXT_ALL_CLASSES : (int)EXT_CLASSES;
	auto read_counters = [&]() -> int {
		HIP_TRY(hipMemcpyAsync(c->ext_host.p, a.ctr, sizeof(ExtCounters), hipMemcpyDeviceToHost, st));
		if (adjust) HIP_TRY(hipMemcpyAsync(hx + hx_ctr, a.cbs_ctr, sizeof(ExtCbsCounters), hipMemcpyDeviceToHost, st));
		HIP_TRY(sync_stream(st));
		ctr = *c->ext_host.as<ExtCounters>();
		std::memcpy(cls_count, ctr.class_count, sizeof ctr.class_count); std::memcpy(cls_steps, ctr.class_max_steps, sizeof ctr.class_max_steps);
		if (adjust) {
			const ExtCbsCounters& xc = *reinterpret_cast<const ExtCbsCounters*>(hx + hx_ctr);
			std::memcpy(cls_count + EXT_OWN_CLASS, xc.class_count, sizeof xc.class_count); std::memcpy(cls_steps + EXT_OWN_CLASS, xc.class_max_steps, sizeof xc.class_max_steps);
		}
		return DMND_OK;
	};
	// One iteration's new pairs, listed in HBM by launch_ext_cbs_window: the kernel fills their slots of the store, rule, status and
	// query row come back (9 bytes per pair), the host form computes the handed-back pairs from the caller's blocks and patches their
	// slots (cbs_slots_assign / cbs_patch_runs, as extend_range does), then every pair's group gets its matrix number.
	auto adjust_pairs = [&]() -> int {
		HIP_TRY(copy_now(st, hx + hx_ctr, a.cbs_ctr, sizeof(ExtCbsCounters), hipMemcpyDeviceToHost));
		const int64_t n_new = reinterpret_cast<const ExtCbsCounters*>(hx + hx_ctr)->n_pairs, before = c->n_adj_matrices;
		if (n_new == 0) return DMND_OK;
		if ((size_t)n_new > L.nG || before + n_new > (int64_t)L.nG) return fail(DMND_E_CAP, "dmnd_extend: more pairs to adjust than groups");
		if (int rc = dmnd_reserve_matrices(c, before, n_new)) return rc;
		if (int rc = dmnd_cbs_adjust_lists(c, cbs_model_dev, n_new, a.q_comp, a.q_true_aa, a.pair_qidx, a.pair_toff, a.pair_tlen, c->block[DMND_TARGET].as<int8_t>(),
			c->adj_matrices.as<int8_t>() + (size_t)before * 32 * 32, nullptr, a.pair_rule, a.pair_status)) return rc;
		const size_t n = (size_t)n_new;
		HIP_TRY(hipMemcpyAsync(hx + hx_rule, a.pair_rule, n * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(hx + hx_status, a.pair_status, n, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipMemcpyAsync(hx + hx_qidx, a.pair_qidx, n * 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(sync_stream(st));
		float ms = 0.f;
		HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
		cbs_ms += ms;
		const int32_t* rule = reinterpret_cast<const int32_t*>(hx + hx_rule);
		const uint8_t* status = reinterpret_cast<const uint8_t*>(hx + hx_status);
		const int32_t* qidx = reinterpret_cast<const int32_t*>(hx + hx_qidx);
		cbs_mat.resize(n); cbs_handed.resize(n);
		int64_t by_status[4];
		const int64_t n_handed = cbs_slots_assign(before, n_new, rule, status, cbs_mat.data(), cbs_handed.data(), by_status);
		for (size_t k = 0; k < n; ++k) {
			if ((size_t)qidx[k] >= nQ) return fail(DMND_E_DEVICE, "dmnd_extend: a pair of the matrix adjustment without a query");
			++cbs_tally[(size_t)qidx[k] * 4 + (status[k] < 4 ? status[k] : CBS_ST_ITERATIONS)];
		}
		if (n_handed > 0) {
			HIP_TRY(hipMemcpyAsync(hx + hx_toff, a.pair_toff, n * 8, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(hx + hx_tlen, a.pair_tlen, n * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(hx + hx_qoff, a.pair_qoff, n * 8, hipMemcpyDeviceToHost, st));
			HIP_TRY(hipMemcpyAsync(hx + hx_qlen, a.pair_qlen, n * 4, hipMemcpyDeviceToHost, st));
			HIP_TRY(sync_stream(st));
			const int64_t* toff = reinterpret_cast<const int64_t*>(hx + hx_toff);
			const int32_t* tlen = reinterpret_cast<const int32_t*>(hx + hx_tlen);
			const int64_t* qoff = reinterpret_cast<const int64_t*>(hx + hx_qoff);
			const int32_t* qlen = reinterpret_cast<const int32_t*>(hx + hx_qlen);
			uint8_t* keep = reinterpret_cast<uint8_t*>(hx + hx_keep);      // per pair, for ext_pair_matrix
			std::memset(keep, 1, n);
			cbs_patch.resize((size_t)n_handed * 32 * 32); cbs_kept.assign((size_t)n_handed, 0); cbs_runs.resize((size_t)n_handed);
			parallel_for((size_t)n_handed, std::max(1, std::min(threads, (int)((n_handed + 7) / 8))), [&](size_t x, int) {
				const size_t k = (size_t)cbs_handed[x];
				double comp[20];
				int true_aa = 0;
				cbs_composition(qdata + qoff[k], qlen[k], comp, &true_aa);
				const int8_t* tseq = tdata + toff[k];
				const int r = cbs_rule(*h.cbs_model, h.cbs_mode, comp, true_aa, tseq, tlen[k]);
				if (r == CBS_RULE_NONE) { keep[k] = 0; return; }
				cbs_kept[x] = 1;
				cbs_target_matrix(*h.cbs_model, r, comp, true_aa, tseq, tlen[k], cbs_patch.data() + x * 32 * 32);
			});
			const int64_t n_runs = cbs_patch_runs(before, cbs_handed.data(), cbs_kept.data(), n_handed, cbs_runs.data());
			for (int64_t r = 0; r < n_runs; ++r)
				HIP_TRY(hipMemcpyAsync(c->adj_matrices.as<int8_t>() + (size_t)cbs_runs[(size_t)r].first_slot * 32 * 32, cbs_patch.data() + (size_t)cbs_runs[(size_t)r].first_patch * 32 * 32,
					(size_t)cbs_runs[(size_t)r].n * 32 * 32, hipMemcpyHostToDevice, st));
			HIP_TRY(hipMemcpyAsync(a.pair_keep, keep, n, hipMemcpyHostToDevice, st));
			HIP_TRY(sync_stream(st));
		}
		HIP_TRY(launch_ext_cbs_matrices(a, before, (uint32_t)n_new, n_handed > 0, st));
		return DMND_OK;
	};
	// the trace walk over the first n entries of the round-2 list
	// (with a transcript arena: piece by piece, each piece's transcripts written into raw slots and kept in the store -- a chunk's
	// trace rows may be gone after the next sweep, so this is the one place where transcripts are made, in every mode)
	size_t store_used = 0;
	auto walk = [&](uint32_t n) -> int {
		TracebackArgs t;
		t.qblock = c->block[DMND_QUERY].as<int8_t>(); t.tblock = c->block[DMND_TARGET].as<int8_t>(); t.cbs = c->cbs_len > 0 ? c->cbs.as<int8_t>() : nullptr;
		t.matrix = c->matrix.as<int8_t>(); t.matrices = adjust ? c->adj_matrices.as<int8_t>() : nullptr;      // (an item with a matrix code is walked on its own matrix)
		t.items = a.items; t.order = a.r2_order; t.p_of_slot = a.r2_p; t.trace_off = a.r2_off; t.transcript_off = a.r2_tr;
		t.trace = c->ext_trace.as<uint8_t>(); t.transcript = nullptr; t.ends = a.ends; t.hsps = a.hsps; t.status = &a.ctr->tb_status;
		t.n = n; t.gap_open = c->params.gap_open; t.gap_extend = c->params.gap_extend;
		if (!with_tr) {
			HIP_TRY(launch_traceback(t, st));
			return DMND_OK;
		}
		// 1. the slots: r2_tr = scan of the entries' slot widths; the list cut into pieces of at most piece_limit raw bytes
		HIP_TRY(launch_tr_slots(a, ta, n, piece_limit, st));
		HIP_TRY(copy_now(st, c->ext_host.as<char>() + h_trc, ta.ctr, sizeof(TrCounters), hipMemcpyDeviceToHost));
		const TrCounters tc = *reinterpret_cast<const TrCounters*>(c->ext_host.as<char>() + h_trc);
		if (tc.n_pieces == 0 || tc.n_pieces > n || tc.raw_max <= 0 || tc.raw_max > tc.raw_total) return fail(DMND_E_DEVICE, "dmnd_extend: the pieces of the transcript walk are inconsistent");
		std::vector<uint32_t> bounds{ 0u, n };
		if (tc.n_pieces > 1) {
			const size_t bytes = ((size_t)tc.n_pieces + 1) * sizeof(uint32_t);
			if (int rc = c->ext_host.ensure(h_pieces + bytes)) return rc;
			HIP_TRY(copy_now(st, c->ext_host.as<char>() + h_pieces, ta.pieces, bytes, hipMemcpyDeviceToHost));
			const uint32_t* b = reinterpret_cast<const uint32_t*>(c->ext_host.as<char>() + h_pieces);
			bounds.assign(b, b + tc.n_pieces + 1);
		}
		if (int rc = c->ext_tr_raw.ensure((size_t)tc.raw_max)) return rc;
		Guard guard_raw(c->ext_tr_raw, (size_t)tc.raw_max, st);
		if (int rc = guard_raw.arm()) return rc;
		tr_raw += (size_t)tc.raw_total;
		for (uint32_t p = 0; p < tc.n_pieces; ++p) {
			const uint32_t s0 = bounds[p], s1 = bounds[p + 1];
			if (s1 <= s0 || s1 > n) return fail(DMND_E_DEVICE, "dmnd_extend: the pieces of the transcript walk are inconsistent");
			const uint32_t m = s1 - s0;
			// 2. the walk of the piece; its offsets count from the piece's first entry
			t.order = a.r2_order + s0; t.p_of_slot = a.r2_p + s0; t.trace_off = a.r2_off + s0; t.transcript_off = a.r2_tr + s0;
			t.transcript = c->ext_tr_raw.as<uint8_t>(); t.transcript_from_first = 1; t.n = m;
			if (tev.on) HIP_TRY(hipEventRecord(tev.e[0], st));
			HIP_TRY(launch_traceback(t, st));
			if (tev.on) HIP_TRY(hipEventRecord(tev.e[1], st));
			// 3. the keep step: lengths, their scan, the copy into the store behind the earlier pieces
			HIP_TRY(launch_tr_keep_sizes(a, ta, s0, m, st));
			HIP_TRY(copy_now(st, c->ext_host.as<char>() + h_val, ta.k_off + m, sizeof(int64_t), hipMemcpyDeviceToHost));
			const int64_t kept_bytes = *reinterpret_cast<const int64_t*>(c->ext_host.as<char>() + h_val);
			if (kept_bytes < (int64_t)m || kept_bytes > tc.raw_max) return fail(DMND_E_DEVICE, "dmnd_extend: the kept transcripts of a piece are inconsistent");
			if (tev.on) { float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, tev.e[0], tev.e[1])); ms_tr_walk += ms; }
			if (int rc = grow_keeping(c->ext_tr_store, store_used + (size_t)kept_bytes, store_used, st)) return rc;
			Guard guard_store(c->ext_tr_store, store_used + (size_t)kept_bytes, st);
			if (int rc = guard_store.arm()) return rc;
			if (tev.on) HIP_TRY(hipEventRecord(tev.e[0], st));
			HIP_TRY(launch_tr_keep(a, ta, s0, m, c->ext_tr_raw.as<uint8_t>(), c->ext_tr_store.as<uint8_t>(), (int64_t)store_used, st));
			if (tev.on) {
				HIP_TRY(hipEventRecord(tev.e[1], st));
				HIP_TRY(sync_stream(st));
				float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, tev.e[0], tev.e[1])); ms_tr_keep += ms;
			}
			if (int rc = guard_store.check("dmnd_extend (device half, transcript store)")) return rc;
			store_used += (size_t)kept_bytes;
			++tr_pieces;
		}
		tr_kept = store_used;
		return guard_raw.check("dmnd_extend (device half, raw transcript slots)");
	};
	// the list's entries whose round-1 sweep kept no trace rows, swept again with traceback as one more iteration (copies of their items)
	auto resweep = [&](uint32_t n_listed, double& ms) -> int {
		HIP_TRY(launch_ext_resweep(a, n_listed, st));
		if (int rc = read_counters()) return rc;
		// (these rows are not held against the budget of round 1, only against a hard limit)
		if ((size_t)ctr.total_rows > std::max(c->trace_arena_max * 4, (size_t)4 << 30)) return fail(DMND_E_NOMEM, "dmnd_extend: the trace rows of round 2 exceed the trace limit (4 x DMND_TRACE_ARENA_MB, at least 4 GB)");
		DevBuf* arena = nullptr;
		int64_t rel = 0;
		if (int rc = arena_for((size_t)ctr.total_rows, arena, rel)) return rc;
		HIP_TRY(hipEventRecord(c->ev0, st));
		if (int rc = dmnd_sweep_classes(c, c, a.items + a.item_base, cls_count, cls_steps, n_cls, reinterpret_cast<const int32_t*>(a.order), a.off_slot, a.pairs,
			a.off_item + a.item_base, arena->as<uint8_t>(), a.ends + a.item_base)) return rc;
		HIP_TRY(hipEventRecord(c->ev1, st));
		HIP_TRY(launch_ext_rewalk(a, ctr.n_items, n_listed, rel, st));
		HIP_TRY(sync_stream(st));
		float t_ms = 0.f;
		HIP_TRY(hipEventElapsedTime(&t_ms, c->ev0, c->ev1));
		ms += t_ms;
		return DMND_OK;
	};
	double ms_sweeps = 0, ms_sweeps2 = 0, ms_walk = 0;
	uint64_t items_total = 0, walked_filt = 0;
	unsigned long long cells2_filt = 0;
	const int max_chunks = ext_max_chunks();
	for (int iter = 0;; ++iter) {
		const bool last = iter + 1 >= max_chunks;      // (a query still ranking after this chunk goes back to the host)
		// with filters a chunk's targets are walked before the next chunk is swept: its trace rows are dead by now, and the arenas --
		// the kept rows' and the one of a chunk swept again -- are used again, so a call never holds more than one chunk's rows
		if (fchunk) { trace_used = 0; n_more = 0; }
		// 1. the chunk's items, launch order, trace offsets, pairs
		// (with matrix adjustment: the windows and the new pairs, their matrices, then the items with their matrix codes)
		if (adjust) {
			HIP_TRY(launch_ext_cbs_window(a, st));
			if (int rc = adjust_pairs()) return rc;
			HIP_TRY(launch_ext_cbs_items(a, st));
		}
		else HIP_TRY(launch_ext_prepare(a, st));
		if (int rc = read_counters()) return rc;
		if (iter == 0) tr.lap("items, launch order, trace offsets");
		if (iter == 0 && ctr.n_items == 0) return guard.check("dmnd_extend (device half)");
		// a call whose first ranking iteration took the row classes keeps them for its later, smaller iterations and for the copies
		// of round 2 (they are short next to the first one, and a row launch of 10^5 items still beats the wavefront classes)
		if (iter == 0 && ctr.n_items >= a.row_min_items && a.row_min_items > 4096) a.row_min_items = 4096;
		// 2. round 1 (one launch per band class)
		int64_t rel = 0;
		bool kept = false;
		if (ctr.n_items > 0) {
			// Trace rows are kept for the walk of round 2 -- unless they do not fit, or so few of the targets can survive the
			// culling (at most -k per query) that sweeping all of them for scores only (18 VALU instructions per packed cell
			// against 31 with trace bits) and the survivors a second time is less work: 18 + 31 f < 31 for a surviving fraction
			// f < 0.42 (C2skew: 125 targets per query, f <= 0.2; C2, C3: f = 0.8 / 0.56, rows kept)
			// (with filters every target past the report cutoff is walked, not the -k survivors: the rows are kept whenever they fit)
			// (--top: how many survive the cut is not known before the sweeps, the rows are kept whenever they fit)
			const bool few_survive = !filt && !top && ctr.window_bound * 100 < ctr.window_targets * (unsigned long long)tuning().extend_resweep_below_pct;
			kept = keep_traces_dev() && !few_survive && trace_used + (size_t)ctr.total_rows <= trace_budget;
			DevBuf* arena = nullptr;
			if (kept) if (int rc = arena_for((size_t)ctr.total_rows, arena, rel)) return rc;
			if (iter == 0) tr.lap("trace arena");
			HIP_TRY(hipEventRecord(c->ev0, st));
			if (int rc = dmnd_sweep_classes(c, c, a.items + a.item_base, cls_count, cls_steps, n_cls, reinterpret_cast<const int32_t*>(a.order), a.off_slot, a.pairs,
				a.off_item + a.item_base, kept ? arena->as<uint8_t>() : nullptr, a.ends + a.item_base)) return rc;
			HIP_TRY(hipEventRecord(c->ev1, st));
		}
		const uint32_t n_items_iter = ctr.n_items;
		if (!fchunk) {
			// 3. best HSP per target, append_hits, next window; and -- in case that was the last chunk of every query -- final culling + round-2 list
			if (top) HIP_TRY(launch_ext_top_append(a, ctr.n_items, kept, rel, last, st));
			else HIP_TRY(launch_ext_append(a, ctr.n_items, kept, rel, last, st));
			HIP_TRY(copy_now(st, c->ext_host.p, a.ctr, sizeof(ExtCounters), hipMemcpyDeviceToHost));
			ctr = *c->ext_host.as<ExtCounters>();
			if (n_items_iter > 0) { float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1)); ms_sweeps += ms; }
			a.item_base += n_items_iter;
		}
		else {
			// 3. with HSP filters: the chunk's targets past the report cutoff are walked now, before any culling; then the filters and
			// the ranking step read the walk's statistics (launch_ext_fcand .. launch_ext_fappend, extend_kernels.h)
			HIP_TRY(launch_ext_fcand(a, ctr.n_items, kept, rel, st));
			HIP_TRY(copy_now(st, c->ext_host.p, a.ctr, sizeof(ExtCounters), hipMemcpyDeviceToHost));
			ctr = *c->ext_host.as<ExtCounters>();
			if (n_items_iter > 0) { float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1)); ms_sweeps += ms; }
			a.item_base += n_items_iter;
			const uint32_t n_listed = ctr.n_kept, list_need = ctr.list_need;
			if (n_listed > L.nS) return fail(DMND_E_CAP, "dmnd_extend: more targets to walk than groups");
			cells2_filt += ctr.cells2; walked_filt += n_listed;
			if (ctr.n_resweep > 0) {
				if ((size_t)a.item_base + ctr.n_resweep > L.nI) return fail(DMND_E_CAP, "dmnd_extend: no room for the items swept again");
				if (int rc = resweep(n_listed, ms_sweeps2)) return rc;
				a.item_base += ctr.n_items;
			}
			if (n_listed > 0) if (int rc = walk(n_listed)) return rc;
			HIP_TRY(launch_ext_fappend(a, n_listed, list_need, last, st));
			HIP_TRY(copy_now(st, c->ext_host.p, a.ctr, sizeof(ExtCounters), hipMemcpyDeviceToHost));
			ctr = *c->ext_host.as<ExtCounters>();
			if (ctr.tb_status != 0) return fail(ctr.tb_status, ctr.tb_status == DMND_E_TRACEBACK ? "Traceback error." : "transcript slot too small");
		}
		items_total += n_items_iter;
		if (tr.on && (iter > 0 || ctr.n_active > 0)) std::fprintf(stderr, "dmnd_extend (device half): chunk %d: %u DpTargets%s, %.1f MB of trace rows kept so far, %u queries go on\n", iter, n_items_iter, kept ? "" : " (scores only)", (double)trace_used / 1048576.0, ctr.n_active);
		if (ctr.n_active == 0) break;
		if (last) return fail(DMND_E_CAP, "dmnd_extend: a query went on ranking past the last allowed chunk");
	}
	tr.lap("sweeps, culling");
	// 4. round 2: the survivors whose trace rows were not kept are swept again with traceback (copies of their items, one more
	// iteration), then one walk over all survivors' traces, then the records
	if (fchunk) {
		// every walk is done: the first -k of each query's matches and their record slots
		HIP_TRY(launch_ext_ffinal(a, st));
		HIP_TRY(copy_now(st, c->ext_host.p, a.ctr, sizeof(ExtCounters), hipMemcpyDeviceToHost));
		ctr = *c->ext_host.as<ExtCounters>();
		ctr.n_resweep = 0;
	}
	if (ctr.n_kept > nR) return fail(DMND_E_CAP, "dmnd_extend: more device records than -k allows");      // (--top: nR = the groups, the list has at most one entry per group)
	const uint32_t n_kept = ctr.n_kept;
	if (ctr.n_resweep > 0) {
		// (at most -k survivors per query)
		if (int rc = resweep(n_kept, ms_sweeps2)) return rc;
		tr.lap("round-2 sweeps");
	}
	ctr.n_kept = n_kept;
	HIP_TRY(hipEventRecord(c->ev1, st));
	if (ctr.n_kept > 0 && !fchunk) if (int rc = walk(ctr.n_kept)) return rc;
	HIP_TRY(hipEventRecord(c->ev2, st));
	// (--top: the filters' verdicts over the walked list, the cut against the best match that passed, the records in score order;
	// how many of the walked targets are records is known only now)
	uint32_t n_out = ctr.n_kept;
	if (top) {
		HIP_TRY(launch_ext_top_records(a, n_kept, st));
		HIP_TRY(copy_now(st, c->ext_host.p, a.ctr, sizeof(ExtCounters), hipMemcpyDeviceToHost));
		n_out = c->ext_host.as<ExtCounters>()->n_records;
		if (n_out > n_kept) return fail(DMND_E_CAP, "dmnd_extend: more device records than walked targets");
	}
	else HIP_TRY(launch_ext_records(a, ctr.n_kept, st));
	// 4b. the gather step: the records' transcripts from the store into one output buffer in record order, their offsets into the
	// records; then straight into the caller's arena
	if (with_tr && n_out > 0) {
		if (n_out > nR) return fail(DMND_E_CAP, "dmnd_extend: more device records than -k allows");
		HIP_TRY(launch_tr_gather_sizes(a, ta, n_out, st));
		HIP_TRY(copy_now(st, c->ext_host.as<char>() + h_val, ta.r_off + n_out, sizeof(int64_t), hipMemcpyDeviceToHost));
		const int64_t bytes = *reinterpret_cast<const int64_t*>(c->ext_host.as<char>() + h_val);
		if (bytes < (int64_t)n_out || (size_t)bytes > store_used) return fail(DMND_E_DEVICE, "dmnd_extend: the gathered transcripts are inconsistent");
		if (bytes > transcript_cap) return fail(DMND_E_CAP, "dmnd_banded_swipe: transcript arena too small");
		if (int rc = c->ext_tr_out.ensure((size_t)bytes)) return rc;
		Guard guard_out(c->ext_tr_out, (size_t)bytes, st);
		if (int rc = guard_out.arm()) return rc;
		if (tev.on) HIP_TRY(hipEventRecord(tev.e[0], st));
		HIP_TRY(launch_tr_gather(a, ta, n_out, c->ext_tr_store.as<uint8_t>(), c->ext_tr_out.as<uint8_t>(), st));
		if (tev.on) HIP_TRY(hipEventRecord(tev.e[1], st));
		HIP_TRY(copy_now(st, c->ext_host.as<char>() + h_trc, ta.ctr, sizeof(TrCounters), hipMemcpyDeviceToHost));
		if (reinterpret_cast<const TrCounters*>(c->ext_host.as<char>() + h_trc)->missing) return fail(DMND_E_DEVICE, "dmnd_extend: a device record without a kept transcript");
		if (tev.on) { float ms = 0.f; HIP_TRY(hipEventElapsedTime(&ms, tev.e[0], tev.e[1])); ms_tr_gather += ms; }
		if (int rc = guard_out.check("dmnd_extend (device half, gathered transcripts)")) return rc;
		if (int rc = download_bytes(c, transcript, c->ext_tr_out.p, (size_t)bytes)) return rc;
		tr_gathered = (size_t)bytes;
	}
	if (transcript_used) *transcript_used = (int64_t)tr_gathered;
	const size_t h_ctr = 0, h_qstate = (sizeof(ExtCounters) + 63) & ~(size_t)63, h_records = (h_qstate + nQ + 63) & ~(size_t)63,
		h_bytes = h_records + (size_t)n_out * sizeof(dmnd_match);
	if (int rc = c->ext_host.ensure(h_bytes)) return rc;
	char* hp = c->ext_host.as<char>();
	HIP_TRY(hipMemcpyAsync(hp + h_ctr, a.ctr, sizeof(ExtCounters), hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(hp + h_qstate, a.qstate, nQ, hipMemcpyDeviceToHost, st));
	if (n_out) HIP_TRY(hipMemcpyAsync(hp + h_records, a.records, (size_t)n_out * sizeof(dmnd_match), hipMemcpyDeviceToHost, st));
	HIP_TRY(sync_stream(st));
	ctr = *reinterpret_cast<const ExtCounters*>(hp + h_ctr);
	tr.lap("walk, records, copy");
	if (ctr.tb_status != 0) return fail(ctr.tb_status, ctr.tb_status == DMND_E_TRACEBACK ? "Traceback error." : "transcript slot too small");
	float ms2 = 0.f;
	HIP_TRY(hipEventElapsedTime(&ms2, c->ev1, c->ev2));
	ms_walk = ms2;
	qstate.assign(hp + h_qstate, hp + h_qstate + nQ);
	// 4. the host's own e-value and bit score in every record; the device ordered a query's records by ITS e-values -- checked,
	// and put right where the two disagree
	const dmnd_match* rec = reinterpret_cast<const dmnd_match*>(hp + h_records);
	records.assign(rec, rec + n_out);
	const std::vector<int64_t>& ql = c->limits[DMND_QUERY];
	const std::vector<int64_t>& tl = c->limits[DMND_TARGET];
	const size_t n = records.size(), per = 4096, n_chunks = (n + per - 1) / per;
	parallel_for(n_chunks, std::max(1, std::min(threads, (int)((n + 16383) / 16384))), [&](size_t ci, int) {
		for (size_t i = ci * per; i < std::min(n, (ci + 1) * per); ++i) {
			dmnd_match& m = records[i];
			const size_t qc = (size_t)m.query * (size_t)h.contexts + (size_t)m.frame;      // (the HSP's own context: extend_host.hip make())
			m.evalue = E.evalue(m.hsp.score, (unsigned)(ql[qc + 1] - ql[qc] - 1), (unsigned)(tl[m.target + 1] - tl[m.target] - 1));
			m.bit_score = E.bitscore(m.hsp.score);
		}
	});
	bool reordered = false;
	const auto less = top ? match_less_score : match_less;      // (Match::cmp_score under --top: exact on integers, so the check never fires there)
	for (size_t b = 0; b < n;) {
		size_t e = b + 1;
		bool sorted = true;
		while (e < n && records[e].query == records[b].query) { sorted &= !less(records[e], records[e - 1]); ++e; }
		if (!sorted) { std::sort(records.begin() + (ptrdiff_t)b, records.begin() + (ptrdiff_t)e, less); reordered = true; }
		b = e;
	}
	// 5. ... and back into the copy in HBM: the records stay there, complete, for a join on the device (dmnd_extend_records_device,
	// dmnd_join_contexts_device) -- 16 bytes per record up instead of 104 down and up again
	// (a call with a transcript arena is joined on the host: its records do not go back up)
	if (n > 0 && !with_tr) {
		if (reordered) HIP_TRY(hipMemcpyAsync(a.records, records.data(), n * sizeof(dmnd_match), hipMemcpyHostToDevice, st));
		else {
			if (int rc = c->ext_ev.ensure(n * 2 * sizeof(double))) return rc;
			if (int rc = c->ext_host.ensure(h_bytes + n * 2 * sizeof(double) + 64)) return rc;      // (the pairs go up from page-locked memory, behind the records)
			double* pairs = reinterpret_cast<double*>(c->ext_host.as<char>() + ((h_bytes + 63) & ~(size_t)63));
			for (size_t i = 0; i < n; ++i) { pairs[2 * i] = records[i].evalue; pairs[2 * i + 1] = records[i].bit_score; }
			HIP_TRY(hipMemcpyAsync(c->ext_ev.p, pairs, n * 2 * sizeof(double), hipMemcpyHostToDevice, st));
			HIP_TRY(launch_ext_patch(a.records, c->ext_ev.as<double>(), (uint32_t)n, st));
		}
		HIP_TRY(sync_stream(st));
	}
	if (!with_tr) { c->ext_records_dev = a.records; c->ext_records_n = (int64_t)n; }
	tr.lap("host e-values, order check");
	c->ext_stats[0] += (double)items_total; c->ext_stats[1] += (double)ctr.n_kept;
	c->ext_stats[2] += (double)ctr.cells1; c->ext_stats[3] += (double)ctr.cells2;
	c->ext_stats[9] += ms_sweeps; c->ext_stats[10] += ms_sweeps2; c->ext_stats[11] += ms_walk;
	size_t n_eligible = 0;
	for (uint8_t x : qstate) n_eligible += x != EXT_Q_HOST;
	c->ext_dev_stats[0] = (double)n_eligible; c->ext_dev_stats[1] = (double)(ctr.n_ambiguous + ctr.n_saturated); c->ext_dev_stats[2] = (double)items_total; c->ext_dev_stats[3] = (double)n_out;
	c->ext_dev_stats[4] = (double)ctr.diag_steps; c->ext_dev_stats[5] = (double)ctr.lane_steps;
	c->ext_dev_stats[6] = (double)ctr.cells2; c->ext_dev_stats[7] = (double)ctr.cells_again; c->ext_dev_stats[8] = ms_sweeps2;
	c->ext_dev_stats[1] += (double)ctr.n_capped; c->ext_dev_stats[9] = (double)ctr.n_capped;
	if (top && filt) { c->ext_dev_stats[1] += (double)ctr.n_threshold; c->ext_filter_stats[0] = (double)ctr.n_filtered; c->ext_filter_stats[1] = (double)ctr.n_threshold; }
	if (fchunk) {
		c->ext_stats[1] += (double)walked_filt - (double)ctr.n_kept; c->ext_stats[3] += (double)cells2_filt - (double)ctr.cells2;      // (every walked target is a round-2 target)
		c->ext_dev_stats[1] += (double)ctr.n_threshold; c->ext_dev_stats[6] = (double)cells2_filt;
		c->ext_filter_stats[0] = (double)ctr.n_filtered; c->ext_filter_stats[1] = (double)ctr.n_threshold;
	}
	if (tr.on) std::fprintf(stderr, "dmnd_extend (device half): %zu queries, %u handed back to the host (%u ambiguous, %u saturated, %u at the chunk cap of %d), %zu records; %u groups, %u bands, %zu bytes of work arrays\n",
		n_eligible, ctr.n_ambiguous + ctr.n_saturated + ctr.n_capped, ctr.n_ambiguous, ctr.n_saturated, ctr.n_capped, max_chunks, n, plan.n_groups, plan.n_bands, L.bytes);
	if (tr.on && with_tr) std::fprintf(stderr, "dmnd_extend (device half) transcripts: %zu pieces of at most %lld raw bytes, %zu raw bytes, %zu kept bytes, %zu gathered bytes; walk %.3f ms, keep %.3f ms, gather %.3f ms\n",
		tr_pieces, (long long)piece_limit, tr_raw, tr_kept, tr_gathered, ms_tr_walk, ms_tr_keep, ms_tr_gather);
	if (adjust) {
		// dmnd_cbs_device_stats: the pairs of the queries done here. A query that goes back takes its pairs out of these tallies -- the
		// host path lists and counts them again --, so a pair is counted once whichever half ends up with its query.
		double by_status[4] = { 0, 0, 0, 0 };
		for (size_t q = 0; q < nQ; ++q)
			if (qstate[q] == EXT_Q_DEVICE) for (int s = 0; s < 4; ++s) by_status[s] += (double)cbs_tally[q * 4 + (size_t)s];
		for (int s = 0; s < 4; ++s) { c->cbs_dev_stats[0] += by_status[s]; c->cbs_dev_stats[1 + s] += by_status[s]; }
		c->cbs_dev_stats[5] += cbs_ms;
		if (tr.on) std::fprintf(stderr, "dmnd_extend (device half) matrix adjustment: %lld slots of the store, %.0f pairs of the queries done here (%.0f handed back to the host form), kernel %.3f ms\n",
			(long long)c->n_adj_matrices, by_status[0] + by_status[1] + by_status[2] + by_status[3], by_status[1] + by_status[2] + by_status[3], cbs_ms);
		if (int rc = guard_cbs.check("dmnd_extend (device half, matrix adjustment arrays)")) return rc;
	}
	if (int rc = guard.check("dmnd_extend (device half)")) return rc;
	if (with_tr) if (int rc = guard_tr.check("dmnd_extend (device half, transcript arrays)")) return rc;
	if (read_lens) if (int rc = guard_sl.check("dmnd_extend (device half, read lengths)")) return rc;
	done = true;
	return DMND_OK;
}

