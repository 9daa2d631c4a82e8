// rank_api.hip -- the host side of the device form of the global ranking step (rank_kernels.h): dmnd_rank_targets_device lays the work
// arrays out in the context's rank_dev buffer, launches the x-drop walk of every hit, the grouping and the ranking kernels on the
// context's stream and reads back the count and the records -- the call's only readback.
#include <algorithm>
#include <string>
#include <vector>
#include "ctx.h"
#include "bias_kernels.h"
#include "rank_kernels.h"

using namespace dmnd;

extern "C" int dmnd_rank_targets_device(dmnd_ctx* c, const dmnd_seed_hit* hits, int64_t n_hits, int n_keep, uint32_t target_offset,
	dmnd_ranked_target* out, int64_t cap, int64_t* n_out)
{
	if (!c || !n_out || n_hits < 0 || n_keep < 0 || cap < 0 || (!out && cap)) return fail(DMND_E_ARG, "dmnd_rank_targets_device: bad argument");
	*n_out = 0;
	const std::vector<int64_t>& ql = c->limits[DMND_QUERY];
	const std::vector<int64_t>& tl = c->limits[DMND_TARGET];
	if (ql.size() < 2 || tl.size() < 2) return fail(DMND_E_ARG, "dmnd_rank_targets_device: blocks must be uploaded with limits");
	const int C = c->query_contexts;
	if ((ql.size() - 1) % (size_t)C != 0) return fail(DMND_E_ARG, "dmnd_rank_targets_device: the query block is no multiple of the query contexts");
	for (double& x : c->rank_stats) x = 0;
	c->rank_stats[3] = hits ? 0 : 1;
	if (!hits && n_hits != c->n_seed_hits) return fail(DMND_E_ARG, "dmnd_rank_targets_device: n_hits is not the count of the context's last seed search");
	if (n_hits == 0) return DMND_OK;
	if (n_hits >= 0xffffffffLL) return fail(DMND_E_CAP, "dmnd_rank_targets_device: more than 2^32 - 2 seed hits in one call");
	if (!hits && !c->seed_hits_sorted.p) return fail(DMND_E_ARG, "dmnd_rank_targets_device: the context holds no seed hits");
	if (hits)
		for (int64_t k = 0; k < n_hits; ++k) {
			const dmnd_seed_hit& h = hits[k];
			if ((size_t)h.query + 1 >= ql.size() || h.seed_offset < 0 || ql[h.query] + h.seed_offset >= ql[h.query + 1] - 1 || h.subject < tl.front() || h.subject >= tl.back())
				return fail(DMND_E_ARG, "dmnd_rank_targets_device: seed hit " + std::to_string(k) + " outside the blocks");
		}
	HIP_TRY(hipSetDevice(c->device));
	TraceLaps tr("dmnd_rank_targets_device");
	const size_t n = (size_t)n_hits;
	const dmnd_seed_hit* src = c->seed_hits_sorted.as<dmnd_seed_hit>();
	if (hits) {
		if (int rc = c->xd_hits.ensure(n * sizeof(dmnd_seed_hit))) return rc;
		HIP_TRY(hipMemcpyAsync(c->xd_hits.p, hits, n * sizeof(dmnd_seed_hit), hipMemcpyHostToDevice, c->stream));
		src = c->xd_hits.as<dmnd_seed_hit>();
	}
	if (int rc = c->xd_out.ensure(n * sizeof(XdropSeg))) return rc;
	// the work arrays: the planner's grouping arrays, then the ranking's own (rank_kernels.h)
	auto align = [](size_t x) { return (x + 63) & ~(size_t)63; };
	const bool translated = C > 1;
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t o = at; at = align(at + bytes); return o; };
	const size_t o_tgt = take(n * sizeof(uint32_t)), o_heads = take(n * sizeof(uint64_t)), o_scan = take(n * sizeof(uint64_t)), o_groups = take((n + 1) * sizeof(PlanGroup)),
		o_queries = take((n + 1) * sizeof(PlanQuery)), o_pcount = take(sizeof(PlanCounters)), o_keys = take(n * sizeof(uint64_t)), o_keys2 = take(n * sizeof(uint64_t)),
		o_idx_a = take(n * sizeof(uint32_t)), o_idx_b = take(n * sizeof(uint32_t)), o_sj = take(n * sizeof(int32_t)), o_send = take(n * sizeof(int32_t)), o_sscore = take(n * sizeof(int32_t)),
		o_best = take(n * sizeof(uint64_t)), o_recs = take(n * sizeof(dmnd_ranked_target)), o_keep = take((n + 1) * sizeof(uint32_t)), o_keep_off = take((n + 1) * sizeof(uint32_t)),
		o_recs_out = take(n * sizeof(dmnd_ranked_target)), o_count = take(sizeof(RankCounters));
	size_t t_hits = 0, t_xd = 0, t_keys = 0, t_keys2 = 0, t_perm_in = 0, t_perm = 0, t_pheads = 0, t_pscan = 0, t_pairs = 0, t_pair_unit = 0, t_unit_pair = 0;
	if (translated) {
		t_hits = take(n * sizeof(dmnd_seed_hit)); t_xd = take(n * sizeof(XdropSeg)); t_keys = take(n * sizeof(uint64_t)); t_keys2 = take(n * sizeof(uint64_t));
		t_perm_in = take(n * sizeof(uint32_t)); t_perm = take(n * sizeof(uint32_t)); t_pheads = take(n * sizeof(uint32_t)); t_pscan = take(n * sizeof(uint32_t));
		t_pairs = take((n + 1) * sizeof(PlanGroup)); t_pair_unit = take((n + 1) * sizeof(uint32_t)); t_unit_pair = take(n * sizeof(uint32_t));
	}
	if (int rc = c->rank_dev.ensure(at)) return rc;
	char* d = c->rank_dev.as<char>();
	tr.lap("work arrays");

	XdropArgs xa;
	xa.qblock = c->block[DMND_QUERY].as<int8_t>(); xa.tblock = c->block[DMND_TARGET].as<int8_t>(); xa.cbs = nullptr;
	xa.qlimits = c->d_limits[DMND_QUERY].as<int64_t>(); xa.matrix = c->matrix.as<int8_t>();
	xa.hits = src; xa.n_hits = n_hits; xa.xdrop = rank_xdrop(c->params.K, c->params.lambda); xa.out = c->xd_out.as<XdropSeg>();
	HIP_TRY(launch_xdrop_segs(xa, c->stream));

	RankArgs a;
	PlanArgs& p = a.plan;
	p = PlanArgs{};
	p.qblock = xa.qblock; p.tblock = xa.tblock; p.qlimits = xa.qlimits; p.tlimits = c->d_limits[DMND_TARGET].as<int64_t>();
	p.n_targets = (int64_t)tl.size() - 1; p.matrix = xa.matrix;
	p.hits = src; p.n_hits = n_hits; p.gf_flags = nullptr; p.xd = xa.out;
	p.tgt = reinterpret_cast<uint32_t*>(d + o_tgt); p.heads = reinterpret_cast<uint64_t*>(d + o_heads); p.head_scan = reinterpret_cast<uint64_t*>(d + o_scan);
	p.groups = reinterpret_cast<PlanGroup*>(d + o_groups); p.queries = reinterpret_cast<PlanQuery*>(d + o_queries); p.counters = reinterpret_cast<PlanCounters*>(d + o_pcount);
	p.scan_tmp = &c->plan_tmp; p.scan_tmp_bytes = &c->plan_tmp_bytes;
	p.contexts = C;
	if (translated) {
		p.hits_in = src; p.xd_in = xa.out; p.gf_in = nullptr;
		p.hits_sorted = reinterpret_cast<dmnd_seed_hit*>(d + t_hits); p.xd_sorted = reinterpret_cast<XdropSeg*>(d + t_xd);
		p.hits = p.hits_sorted; p.xd = p.xd_sorted;
		p.keys = reinterpret_cast<uint64_t*>(d + t_keys); p.keys_sorted = reinterpret_cast<uint64_t*>(d + t_keys2);
		p.perm_in = reinterpret_cast<uint32_t*>(d + t_perm_in); p.perm = reinterpret_cast<uint32_t*>(d + t_perm);
		const PlanKeyBits kb = plan_key_bits((uint64_t)((ql.size() - 1) / (size_t)C), (uint64_t)p.n_targets);
		p.target_bits = kb.target_bits; p.key_bits = kb.target_bits + kb.read_bits;
		p.pheads = reinterpret_cast<uint32_t*>(d + t_pheads); p.phead_scan = reinterpret_cast<uint32_t*>(d + t_pscan);
		p.pairs = reinterpret_cast<PlanGroup*>(d + t_pairs); p.pair_unit = reinterpret_cast<uint32_t*>(d + t_pair_unit); p.unit_pair = reinterpret_cast<uint32_t*>(d + t_unit_pair);
	}
	a.n_keep = n_keep; a.target_offset = target_offset;
	a.j_bits = std::min(32, plan_bits_below((uint64_t)c->block_len[DMND_TARGET] + 1));
	a.key_bits = 32 + plan_bits_below((uint64_t)n);
	a.cut_bits = 16 + plan_bits_below((uint64_t)n + 1);
	a.keys = reinterpret_cast<uint64_t*>(d + o_keys); a.keys_sorted = reinterpret_cast<uint64_t*>(d + o_keys2);
	a.idx_a = reinterpret_cast<uint32_t*>(d + o_idx_a); a.idx_b = reinterpret_cast<uint32_t*>(d + o_idx_b);
	a.sj = reinterpret_cast<int32_t*>(d + o_sj); a.sj_end = reinterpret_cast<int32_t*>(d + o_send); a.sscore = reinterpret_cast<int32_t*>(d + o_sscore);
	a.best = reinterpret_cast<uint64_t*>(d + o_best); a.recs = reinterpret_cast<dmnd_ranked_target*>(d + o_recs);
	a.keep = reinterpret_cast<uint32_t*>(d + o_keep); a.keep_off = reinterpret_cast<uint32_t*>(d + o_keep_off);
	a.recs_out = reinterpret_cast<dmnd_ranked_target*>(d + o_recs_out); a.counters = reinterpret_cast<RankCounters*>(d + o_count);
	HIP_TRY(launch_rank(a, c->stream));
	tr.lap("launched");
	RankCounters cn;
	HIP_TRY(copy_now(c->stream, &cn, a.counters, sizeof(cn), hipMemcpyDeviceToHost));
	tr.lap("count back");
	if (cn.unsorted) return fail(DMND_E_ARG, "dmnd_rank_targets_device: the hits are not in the order dmnd_seed_hits returns");
	*n_out = (int64_t)cn.n_records;
	c->rank_stats[0] = (double)cn.n_groups; c->rank_stats[1] = (double)cn.n_walked;
	if ((int64_t)cn.n_records > cap) return fail(DMND_E_CAP, "dmnd_rank_targets_device: record buffer too small");
	c->rank_stats[2] = (double)cn.n_records;
	if (cn.n_records > 0)
		if (int rc = download_bytes(c, out, n_keep > 0 ? a.recs_out : a.recs, (size_t)cn.n_records * sizeof(dmnd_ranked_target))) return rc;
	tr.lap("records back");
	return DMND_OK;
}

extern "C" int dmnd_rank_device_stats(const dmnd_ctx* c, double out[4])
{
	if (!c || !out) return fail(DMND_E_ARG, "dmnd_rank_device_stats: NULL argument");
	for (int i = 0; i < 4; ++i) out[i] = c->rank_stats[i];
	return DMND_OK;
}
