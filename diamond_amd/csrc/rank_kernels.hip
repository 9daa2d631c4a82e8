// rank_kernels.hip -- the device form of the global ranking step (rank_kernels.h has the steps and the argument for the cut).
// All kernels are one lane per hit, per run or per group over n_hits lanes: group and record counts are read on the device (groups <=
// hits), nothing comes back to the host between the launches. Bounds: every index below is a hit index < n_hits, a group index <
// n_groups <= n_hits, or a sorted position < n_hits; arrays with a sentinel have n_hits + 1 entries.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include "rank_kernels.h"

namespace dmnd {

namespace {

__device__ inline uint32_t rank_n_groups(const RankArgs& a) { return a.plan.contexts > 1 ? a.plan.counters->n_pairs : a.plan.counters->n_groups; }
__device__ inline uint32_t rank_group_of(const RankArgs& a, uint32_t k) { return (a.plan.contexts > 1 ? a.plan.phead_scan[k] : (uint32_t)a.plan.head_scan[k]) - 1; }
__device__ inline int32_t rank_j_of(const RankArgs& a, uint32_t k) { return (int32_t)(a.plan.hits[k].subject - a.plan.tlimits[a.plan.tgt[k]]); }

// six contexts, in front of the stable pass by j: j of every hit of the grouped list
__global__ __launch_bounds__(256) void rank_jkey_kernel(RankArgs a, uint32_t* jkeys, uint32_t* idx)
{
	const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= a.plan.n_hits) return;
	jkeys[k] = (uint32_t)rank_j_of(a, (uint32_t)k);
	idx[k] = (uint32_t)k;
}

// (group, diagonal) key of hit order[k] (order == NULL: of hit k, and idx_out[k] = k)
__global__ __launch_bounds__(256) void rank_key_kernel(RankArgs a, const uint32_t* order, uint32_t* idx_out)
{
	const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= a.plan.n_hits) return;
	const uint32_t src = order ? order[k] : (uint32_t)k;
	a.keys[k] = rank_key(rank_group_of(a, src), a.plan.hits[src].seed_offset - rank_j_of(a, src));
	if (!order) idx_out[k] = (uint32_t)k;
}

// behind the sort: what the walk reads, per sorted position; the groups' results cleared
__global__ __launch_bounds__(256) void rank_gather_kernel(RankArgs a, const uint32_t* sidx)
{
	const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= a.plan.n_hits) return;
	const uint32_t src = sidx[p];
	const int32_t j = rank_j_of(a, src);
	const RankSeg s = rank_seg(a.plan.hits[src].seed_offset, j, a.plan.xd[src]);
	a.sj[p] = j; a.sj_end[p] = s.j_end; a.sscore[p] = s.score;
	a.best[p] = 0;
}

__global__ __launch_bounds__(256) void rank_walk_kernel(RankArgs a)
{
	const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t n = (uint32_t)a.plan.n_hits;
	uint32_t counted = 0;
	if (p < (int64_t)n) {
		const uint64_t key = a.keys_sorted[p];
		if (p == 0 || a.keys_sorted[p - 1] != key) {
			// the run's end: doubling steps, then a binary search between the last two probes
			uint32_t lo = (uint32_t)p + 1, hi = n;                    // [p, lo) is of the run, nothing from hi on is
			for (uint64_t step = 1; lo < hi; step <<= 1) {
				const uint64_t probe = (uint64_t)lo + step - 1;
				if (probe >= hi) break;
				if (a.keys_sorted[probe] == key) lo = (uint32_t)probe + 1; else { hi = (uint32_t)probe; break; }
			}
			while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a.keys_sorted[mid] == key) lo = mid + 1; else hi = mid; }
			int32_t best; uint32_t best_pos;
			rank_walk_run(a.sj, a.sj_end, a.sscore, (uint32_t)p, lo, best, best_pos, counted);
			atomicMax(reinterpret_cast<unsigned long long*>(a.best + rank_key_group(key)), (unsigned long long)rank_pack_best(best, best_pos));
		}
	}
	// hits that were not skipped: summed over the wavefront, one atomic per wavefront
	for (int off = 32; off > 0; off >>= 1) counted += __shfl_down(counted, off, 64);
	if ((threadIdx.x & 63) == 0 && counted) atomicAdd(&a.counters->n_walked, (unsigned long long)counted);
}

// one record per group; n_keep > 0: the cut's key of the record (entries beyond the group count sort behind every record)
__global__ __launch_bounds__(256) void rank_records_kernel(RankArgs a, const uint32_t* sidx, uint32_t* cut_idx)
{
	const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= a.plan.n_hits) return;
	const uint32_t ng = rank_n_groups(a);
	if (g == 0) { a.counters->n_groups = ng; a.counters->unsorted = a.plan.counters->unsorted; if (a.n_keep == 0) a.counters->n_records = ng; }
	if (g >= (int64_t)ng) {
		if (a.n_keep > 0) { a.keys[g] = (uint64_t)a.plan.n_hits << 16; cut_idx[g] = (uint32_t)g; }
		return;
	}
	const PlanGroup& grp = a.plan.contexts > 1 ? a.plan.pairs[g] : a.plan.groups[g];
	const uint64_t b = a.best[g];
	const uint32_t src = sidx[rank_best_pos(b)];
	const uint32_t ctx = a.plan.hits[src].query, C = (uint32_t)a.plan.contexts;
	dmnd_ranked_target r;
	r.query = ctx / C; r.target = grp.target + a.target_offset; r.score = rank_record_score(rank_best_score(b)); r.context = (uint8_t)(ctx % C); r.pad = 0;
	a.recs[g] = r;
	if (a.n_keep > 0) {
		a.keys[g] = rank_cut_key((uint32_t)(a.plan.head_scan[grp.hit_begin] >> 32) - 1, r.score);
		cut_idx[g] = (uint32_t)g;
	}
}

// behind the cut's sort: a query's records lie where its groups lay, so the rank of a record in its query is its position minus the
// query's first group (PlanQuery::group_begin)
__global__ __launch_bounds__(256) void rank_keep_kernel(RankArgs a)
{
	const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p > a.plan.n_hits) return;
	uint32_t keep = 0;
	if (p < (int64_t)rank_n_groups(a)) keep = (uint32_t)p - a.plan.queries[rank_cut_query(a.keys_sorted[p])].group_begin < (uint32_t)a.n_keep;
	a.keep[p] = keep;
}

__global__ __launch_bounds__(256) void rank_compact_kernel(RankArgs a, const uint32_t* cut_sorted)
{
	const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= a.plan.n_hits) return;
	if (p == 0) a.counters->n_records = a.keep_off[a.plan.n_hits];
	if (a.keep[p]) a.recs_out[a.keep_off[p]] = a.recs[cut_sorted[p]];
}

}  // namespace

hipError_t launch_rank(const RankArgs& a, hipStream_t st)
{
	if (a.plan.n_hits <= 0) return hipSuccess;
	const size_t n = (size_t)a.plan.n_hits;
	const unsigned b256 = (unsigned)((n + 255) / 256), b256g = (unsigned)((n + 1 + 255) / 256);
	const bool translated = a.plan.contexts > 1;
	uint32_t* jk_in = reinterpret_cast<uint32_t*>(a.sj);
	uint32_t* jk_out = reinterpret_cast<uint32_t*>(a.sj_end);
	size_t need_j = 0, need_k = 0, need_c = 0, need_s = 0;
	hipError_t e;
	if (translated) {
		e = rocprim::radix_sort_pairs(nullptr, need_j, jk_in, jk_out, a.idx_a, a.idx_b, n, 0, a.j_bits, st);
		if (e != hipSuccess) return e;
	}
	e = rocprim::radix_sort_pairs(nullptr, need_k, a.keys, a.keys_sorted, a.idx_a, a.idx_b, n, 0, a.key_bits, st);
	if (e != hipSuccess) return e;
	if (a.n_keep > 0) {
		e = rocprim::radix_sort_pairs(nullptr, need_c, a.keys, a.keys_sorted, a.idx_a, a.idx_b, n, 0, a.cut_bits, st);
		if (e != hipSuccess) return e;
		e = rocprim::exclusive_scan(nullptr, need_s, a.keep, a.keep_off, 0u, n + 1, rocprim::plus<uint32_t>(), st);
		if (e != hipSuccess) return e;
	}
	size_t extra = need_j > need_k ? need_j : need_k;
	if (need_c > extra) extra = need_c;
	if (need_s > extra) extra = need_s;
	e = hipMemsetAsync(a.counters, 0, sizeof(RankCounters), st);
	if (e != hipSuccess) return e;
	e = launch_plan_groups(a.plan, st, extra);
	if (e != hipSuccess) return e;
	void* tmp = *a.plan.scan_tmp;
	// sidx: the hit indices in (group, diagonal, j) order; spare: the other index array
	uint32_t* sidx; uint32_t* spare;
	if (translated) {
		hipLaunchKernelGGL(rank_jkey_kernel, dim3(b256), dim3(256), 0, st, a, jk_in, a.idx_a);
		e = rocprim::radix_sort_pairs(tmp, need_j, jk_in, jk_out, a.idx_a, a.idx_b, n, 0, a.j_bits, st);
		if (e != hipSuccess) return e;
		hipLaunchKernelGGL(rank_key_kernel, dim3(b256), dim3(256), 0, st, a, (const uint32_t*)a.idx_b, (uint32_t*)nullptr);
		e = rocprim::radix_sort_pairs(tmp, need_k, a.keys, a.keys_sorted, a.idx_b, a.idx_a, n, 0, a.key_bits, st);
		if (e != hipSuccess) return e;
		sidx = a.idx_a; spare = a.idx_b;
	}
	else {
		hipLaunchKernelGGL(rank_key_kernel, dim3(b256), dim3(256), 0, st, a, (const uint32_t*)nullptr, a.idx_a);
		e = rocprim::radix_sort_pairs(tmp, need_k, a.keys, a.keys_sorted, a.idx_a, a.idx_b, n, 0, a.key_bits, st);
		if (e != hipSuccess) return e;
		sidx = a.idx_b; spare = a.idx_a;
	}
	hipLaunchKernelGGL(rank_gather_kernel, dim3(b256), dim3(256), 0, st, a, (const uint32_t*)sidx);
	hipLaunchKernelGGL(rank_walk_kernel, dim3(b256), dim3(256), 0, st, a);
	hipLaunchKernelGGL(rank_records_kernel, dim3(b256), dim3(256), 0, st, a, (const uint32_t*)sidx, spare);
	if (a.n_keep > 0) {
		// (the records kernel was the last reader of sidx: the cut's sorted indices go there)
		e = rocprim::radix_sort_pairs(tmp, need_c, a.keys, a.keys_sorted, spare, sidx, n, 0, a.cut_bits, st);
		if (e != hipSuccess) return e;
		hipLaunchKernelGGL(rank_keep_kernel, dim3(b256g), dim3(256), 0, st, a);
		e = rocprim::exclusive_scan(tmp, need_s, a.keep, a.keep_off, 0u, n + 1, rocprim::plus<uint32_t>(), st);
		if (e != hipSuccess) return e;
		hipLaunchKernelGGL(rank_compact_kernel, dim3(b256), dim3(256), 0, st, a, (const uint32_t*)sidx);
	}
	return hipGetLastError();
}

}  // namespace dmnd
