// extend_kernels.hip -- device half of the extension stage behind the planner (see extend_kernels.h; round 6, SURVEY.md 8 rows a14,
// a18 and the host preparation of a15 / a16 moved off the host for the queries whose targets fit one ranking chunk).
//
// Kernels, all latency-bound integer work on lists of 10^5 - 10^6 entries (a handful of bytes per entry, one pass each):
//   ext_mark_kernel      one wavefront per query: does the query run here? (no group left to the host by the planner, every band
//                        something the traceback-mode sweeps take); ranking state, sort keys of the ranking order
//   rocPRIM radix sort   -> every query's groups by (seed-hit score descending, load order)
//   per ranking-chunk iteration (most calls: one):
//     ext_window_kernel    item count of every group in an active query's current chunk; rocPRIM scan -> first item
//     ext_items_kernel     one thread per group: the DpTargets of its bands, band class, sweep steps, trace bytes, sort key; class
//                          histogram and DP cells (block-aggregated atomics)
//     rocPRIM radix sort (15 key bits) -> launch order: band class ascending, longest items first (api.hip order_slots)
//     ext_slots_kernel, rocPRIM scan, ext_offsets_kernel: trace offset of every item, item pairs of the packed 16-bit launches
//     (the sweeps: swipe16_kernels.hip / swipe_kernels.hip, launched by the host from the class histogram)
//     ext_append_kernel    one wavefront per query: best HSP per target past the report cutoff, append_hits (rank by counting when the
//                          aligned targets must be cut to k), next window, tail rule; ambiguity detection
//   ext_final_kernel     the first k of a query's aligned targets by (e-value, score desc, target); rocPRIM scan, ext_round2_kernel:
//                        the list the trace walk runs over (launched behind every iteration, used when no query is left ranking)
//   (traceback_kernel, swipe_kernels.hip)
//   ext_records_kernel   one wavefront per query: its match records in output order
//   --top (top_core.h): ext_top_append_kernel / ext_top_final_kernel in the place of ext_append_kernel / ext_final_kernel -- cuts by a
//                        threshold against the best bit score, wavefront reductions over the query's aligned flags, no LDS list;
//                        behind the walk ext_filter_kernel + ext_top_ffinal_kernel (with HSP filters), ext_top_keys_kernel, one
//                        rocPRIM radix sort by (query, 0xffffffff - score), ext_top_records_kernel
// Compiled with -ffp-contract=off like plan_kernels.hip (the e-value below follows evalue.h operation by operation).
#include <hip/hip_runtime.h>
#include <cfloat>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include "extend_kernels.h"
#include "swipe16_core.h"
#include "swipe_core.h"

namespace dmnd {

namespace {

__device__ inline double ext_normal_cdf(double x) { return 0.5 * erfc(-0.70710678118654752440 * x); }

// Evaluer::evalue (evalue.h:34-52) with the device's exp / erfc / sqrt
__device__ inline double ext_evalue(const ExtEvalue& p, int raw_score, int qlen, int slen)
{
	const double inv_sqrt_2pi = 1.0 / sqrt(2.0 * 3.1415926535897932384626433832795);
	const double y = (double)raw_score, len1 = (double)(unsigned)qlen, len2 = (double)(unsigned)slen;
	const double m_l = len2 - (p.a * y + p.b), n_l = len1 - (p.a * y + p.b);
	const double v = fmax(p.v_thr, p.alpha * y + p.beta), sv = sqrt(v);
	const double mF = sv == 0.0 ? 1e100 : m_l / sv, nF = sv == 0.0 ? 1e100 : n_l / sv;
	const double PmF = ext_normal_cdf(mF), PnF = ext_normal_cdf(nF);
	const double EmF = -inv_sqrt_2pi * exp(-0.5 * mF * mF), EnF = -inv_sqrt_2pi * exp(-0.5 * nF * nF);
	const double p1 = m_l * PmF - sv * EmF, p2 = n_l * PnF - sv * EnF;
	const double c = fmax(p.c_thr, p.sigma * y + p.tau);
	const double area = p1 * p2 + c * (PmF * PnF);
	return area * (p.K * exp(-p.lambda * y)) * p.db_letters / (double)slen;
}

// two device e-values whose order the host's own values could reverse (or a value that close to the cutoff)
__device__ inline bool ext_near(double x, double y) { return fabs(x - y) <= 1e-9 * fmax(fabs(x), fabs(y)); }

// Where K exp(-lambda y), the factor of the e-value that underflows, lies for a raw score y: 0 = a normal double on both sides; 2 =
// exp underflows to 0.0 on both sides (exp(-750) is 1/100 of the smallest subnormal), so the e-value is exactly 0.0 on the host and
// here; 1 = in between, where one side may round to 0.0 or to a subnormal (a few significant bits) that the other does not
__device__ inline int ext_underflow(const ExtEvalue& p, int raw_score)
{
	const double t = -p.lambda * (double)raw_score;
	return t < -750.0 ? 2 : (p.ln_k + t < -700.0 ? 1 : 0);
}

__device__ inline int64_t ext_cells(const dmnd_dp_target& d)       // DpTarget::cells of a banded target (dp/dp.h:47-52, 121-124)
{
	const int pos = imax(d.d_end - 1, 0) - (d.d_end - 1);
	const int j1 = imin(d.query_len - 1 - d.d_begin, d.target_len - 1) + 1;
	return (int64_t)(j1 - pos) * (int64_t)(d.d_end - d.d_begin);
}

// What config.max_swipe_dp is held against: the band's columns x width, or -- Mode::FULL, DP::Flags::FULL_MATRIX -- the whole matrix
// (dp/dp.h:121-124; extend_host.hip dp_size). The counters (cells1, cells2, the roofline statistics) count ext_cells in both modes, as
// the host path's do: the cells the band sweeps compute, corners outside the matrix included.
__device__ inline int64_t ext_dp_size(const ExtArgs& a, const dmnd_dp_target& d)
{
	return a.ext_full ? full_matrix_dp_size(d.query_len, d.target_len) : ext_cells(d);
}

// bit score of a raw score (Evaluer::bitscore, evalue.h): plain double arithmetic, no library function -- the host's value bit for bit
__device__ inline double ext_bitscore(const ExtEvalue& p, int raw_score) { return (p.lambda * (double)raw_score - p.ln_k) / 0.69314718055994530941723212145818; }

// the report cutoff (ScoreMatrix::report_cutoff): the e-value against --evalue, or -- --min-score -- the bit score against that; amb
// is set where the host's own value could decide the other way
__device__ inline bool ext_reported(const ExtArgs& a, int score, double ev, bool& amb)
{
	if (a.min_bit_score != 0.0) {
		const double bits = ext_bitscore(a.ev, score);
		if (ext_near(bits, a.min_bit_score)) amb = true;
		return bits >= a.min_bit_score;
	}
	if (ext_near(ev, a.ev.max_evalue)) amb = true;
	return ev <= a.ev.max_evalue;
}

__global__ __launch_bounds__(64) void ext_mark_kernel(ExtArgs a)
{
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin, ng = g1 - g0;
	const uint32_t query = a.queries[q].query;
	// (translated queries: every band is checked with the length of its own context, below)
	const int qlen1 = a.band_query ? 1 : (int)(a.qlimits[query + 1] - a.qlimits[query] - 1);
	// more groups than a chunk: ranked in chunks (extend.cpp:289-336). A first chunk smaller than -k would grow by the e-value of
	// the seed-hit scores (extend.cpp:262-268): those queries stay on the host
	// (--top: the chunk is 128 x block_mult whatever -k is, and the growth rule does not apply)
	bool bad = ng > EXT_MAX_GROUPS || qlen1 <= 0 || (!a.top_on && ng > a.chunk_size && (uint32_t)a.k > a.chunk_size);
	if (!bad)
		for (uint32_t g = g0 + lane; g < g1; g += 64) {
			const PlanGroup grp = a.groups[g];
			if (!grp.pass) continue;
			if (grp.n_bands == PLAN_ON_HOST) { bad = true; break; }
			const int tlen = (int)(a.tlimits[grp.target + 1] - a.tlimits[grp.target] - 1);
			if (tlen <= 0) { bad = true; break; }
			for (uint32_t k = 0; k < grp.n_bands; ++k) {
				const PlanBand b = a.bands[grp.band_begin + k];
				const int band = b.d_end - b.d_begin;
				int qlen = qlen1;
				if (a.band_query) { const uint32_t bq = a.band_query[grp.band_begin + k]; qlen = (int)(a.qlimits[bq + 1] - a.qlimits[bq] - 1); }
				const dmnd_dp_target d{ 0, 0, 0, qlen, tlen, b.d_begin, b.d_end };
				if (qlen <= 0 || band <= 0 || band_class(band) > 32 || ext_dp_size(a, d) > a.max_swipe_dp) bad = true;
			}
		}
	const bool ok = __ballot(bad) == 0;
	for (uint32_t g = g0 + lane; g < g1; g += 64) {
		// ranking order = (score descending, load order): a stable sort by (query, 0xffff - score) of the groups as they lie
		a.okeys[g] = ((uint64_t)q << 16) | (uint64_t)(0xffffu - (uint32_t)a.groups[g].score);
		a.oidx[g] = g;
		a.aligned[g] = 0; a.g_cnt[g] = 0; a.g_first[g] = 0;
		if (a.filt_on) { a.fverdict[g] = EXT_F_PASS; a.matched[g] = 0; }
		if (a.top_on) a.cand_score[g] = 0;
	}
	if (lane == 0) {
		a.qstate[q] = ok ? EXT_Q_DEVICE : EXT_Q_HOST;
		a.q_active[q] = ok ? 1 : 0;
		a.q_i0[q] = 0; a.q_i1[q] = ng < a.chunk_size ? ng : a.chunk_size;
		a.q_tail[q] = 0; a.q_prev[q] = 0;
		if (a.filt_on) { a.q_matched[q] = 0; a.q_removed[q] = 0; }
	}
}

// the items of the current iteration: the bands of the passing groups of every active query's window. Every group gets its count
// (0 outside the windows) and a cleared `kept` flag here, and workgroup 0 resets the iteration's counters -- seven memset launches per
// iteration otherwise (each a kernel of its own on the stream)
__global__ __launch_bounds__(64) void ext_window_kernel(ExtArgs a)
{
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin;
	const bool active = a.q_active[q] != 0;
	const uint32_t i0 = active ? a.q_i0[q] : 0, i1 = active ? a.q_i1[q] : 0;
	uint32_t swept = 0;                        // targets of the window that are swept (they passed the filters before)
	for (uint32_t w = lane; w < g1 - g0; w += 64) {
		const uint32_t g = a.gorder[g0 + w];
		uint32_t n = 0;
		if (w >= i0 && w < i1) { const PlanGroup grp = a.groups[g]; n = grp.pass ? grp.n_bands : 0u; }
		a.cnt[g] = n;
		a.kept[g] = 0;
		swept += n ? 1u : 0u;
	}
	for (int off = 32; off >= 1; off >>= 1) swept += __shfl_xor(swept, off);
	if (lane == 0) a.q_swept[q] = swept;       // summed by ext_items_kernel (an atomic per query here is 10 ns each, one after the other)
	if (q == 0 && lane < EXT_CLASSES) { a.ctr->class_count[lane] = 0; a.ctr->class_max_steps[lane] = 0; }
	if (q == 0 && lane == 0) {
		a.cnt[a.n_groups] = 0; a.kept[a.n_groups] = 0;
		a.ctr->n_items = 0; a.ctr->n_active = 0; a.ctr->n_resweep = 0; a.ctr->total_rows = 0; a.ctr->cells2 = 0;
		a.ctr->window_targets = 0; a.ctr->window_bound = 0; a.ctr->list_need = 0;
	}
}

__global__ __launch_bounds__(256) void ext_init_kernel(ExtArgs a)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = a.item_cap - a.item_base;
	if (i >= n) return;
	a.idx[i] = i; a.keys[i] = 0x7fffu; a.rows[i] = 0;
}

// launch class of an item (api.hip sweep_class: the row classes take what the packed 16-bit kernels take)
// (own: the item is scored with a matrix of its own -- 32-bit kernels only, extend_cbs_core.h)
__device__ inline int ext_class(bool rows, bool own, int band, int64_t steps)
{
	return ext_item_class(rows, own, band, steps, (int64_t)SW16_MAX_PAIRS);
}

// ---- matrix adjustment inside the device half (--comp-based-stats 2 - 5; extend_kernels.h, extend_cbs_core.h) ----
// One wavefront per planned query: its composition as cbs_composition (cbs_adjust.cpp) and the target side of cbsd_pair (cbs_core.h)
// compute it -- exact integer counts, one correctly rounded division each, so the doubles are the host's --, and its groups' rows.
__global__ __launch_bounds__(64) void ext_cbs_comp_kernel(ExtArgs a, const int8_t* qblock)
{
	__shared__ int cnt[CBSD_N];
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	const uint32_t query = a.queries[q].query;
	const int64_t q0 = a.qlimits[query];
	const int64_t len = a.qlimits[query + 1] - q0 - 1;
	if (lane < CBSD_N) cnt[lane] = 0;
	__syncthreads();
	for (int64_t p = lane; p < len; p += 64) { const int l = qblock[q0 + p] & 31; if (l < CBSD_N) atomicAdd(&cnt[l], 1); }
	__syncthreads();
	int n = 0;
	for (int i = 0; i < CBSD_N; ++i) n += cnt[i];
	if (lane < CBSD_N) a.q_comp[(size_t)q * CBSD_N + lane] = n == 0 ? 0.0 : (double)cnt[lane] / n;
	if (lane == 0) a.q_true_aa[q] = n;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin;
	for (uint32_t g = g0 + lane; g < g1; g += 64) { a.g_row[g] = q; a.g_mat[g] = EXT_MAT_UNSET; }
}

// the iteration's new pairs: groups of the windows that have items and no matrix number yet
__global__ __launch_bounds__(256) void ext_cbs_flag_kernel(ExtArgs a)
{
	const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g < a.n_groups) a.c_flag[g] = a.cnt[g] > 0 && a.g_mat[g] == EXT_MAT_UNSET ? 1u : 0u;
	else if (g == a.n_groups) a.c_flag[g] = 0;
}

__global__ __launch_bounds__(256) void ext_cbs_pairs_kernel(ExtArgs a)
{
	const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g == 0) {
		a.cbs_ctr->n_pairs = a.c_pos[a.n_groups];
		for (int c = 0; c < EXT_OWN_CLASS; ++c) { a.cbs_ctr->class_count[c] = 0; a.cbs_ctr->class_max_steps[c] = 0; }
	}
	if (g >= a.n_groups || !a.c_flag[g]) return;
	const uint32_t k = a.c_pos[g], row = a.g_row[g];
	const uint32_t target = a.groups[g].target, query = a.queries[row].query;
	const int64_t t0 = a.tlimits[target], q0 = a.qlimits[query];
	a.pair_group[k] = g; a.pair_qidx[k] = (int32_t)row;
	a.pair_toff[k] = t0; a.pair_tlen[k] = (int32_t)(a.tlimits[target + 1] - t0 - 1);
	a.pair_qoff[k] = q0; a.pair_qlen[k] = (int32_t)(a.qlimits[query + 1] - q0 - 1);
}

__global__ __launch_bounds__(256) void ext_cbs_matrices_kernel(ExtArgs a, int64_t before, uint32_t n_pairs, int keep)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < n_pairs) a.g_mat[a.pair_group[k]] = ext_pair_matrix(before, (int64_t)k, a.pair_rule[k], a.pair_status[k], keep ? a.pair_keep[k] : (uint8_t)1);
}

__global__ __launch_bounds__(256) void ext_items_kernel(ExtArgs a)
{
	__shared__ uint32_t h_count[EXT_CLASSES], h_steps[EXT_CLASSES];
	__shared__ unsigned long long h_cells, h_diag, h_lane;
	__shared__ uint32_t h_targets, h_bound;
	__shared__ uint32_t h_own_count[EXT_OWN_CLASS], h_own_steps[EXT_OWN_CLASS];      // items with a matrix of their own (a.g_mat)
	if (threadIdx.x < EXT_CLASSES) { h_count[threadIdx.x] = 0; h_steps[threadIdx.x] = 0; }
	if (threadIdx.x < EXT_OWN_CLASS) { h_own_count[threadIdx.x] = 0; h_own_steps[threadIdx.x] = 0; }
	if (threadIdx.x == 0) { h_cells = 0; h_diag = 0; h_lane = 0; h_targets = 0; h_bound = 0; }
	__syncthreads();
	const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
	for (uint32_t q = g; q < a.n_queries; q += gridDim.x * blockDim.x) {      // the windows' swept targets, and how many of them can survive the culling
		const uint32_t swept = a.q_swept[q];
		if (swept) { atomicAdd(&h_targets, swept); atomicAdd(&h_bound, swept < (uint32_t)a.k ? swept : (uint32_t)a.k); }
	}
	const bool rows = a.item_off[a.n_groups] >= a.row_min_items;      // by the items of the whole iteration
	if (g < a.n_groups) {
		const uint32_t n = a.cnt[g];
		if (n) {
			const PlanGroup grp = a.groups[g];
			const uint32_t query = a.hits[grp.hit_begin].query;
			int64_t q0 = a.qlimits[query];
			const int64_t t0 = a.tlimits[grp.target];
			int qlen = (int)(a.qlimits[query + 1] - q0 - 1);
			const int tlen = (int)(a.tlimits[grp.target + 1] - t0 - 1);
			const uint32_t local = a.item_off[g], first = a.item_base + local;
			a.g_first[g] = first; a.g_cnt[g] = n;
			unsigned long long cells = 0, diag = 0, lanes = 0;
			// the group's adjusted matrix, if it has one: its items are swept with it and without the bias (extend_host.hip item_of)
			const int32_t mat = a.g_mat ? a.g_mat[g] : (int32_t)EXT_MAT_STANDARD;
			const bool own = mat >= 0;
			for (uint32_t k = 0; k < n; ++k) {
				const PlanBand b = a.bands[grp.band_begin + k];
				if (a.band_query) {      // the item reads the sequence, bias and length of its band's context
					const uint32_t bq = a.band_query[grp.band_begin + k];
					q0 = a.qlimits[bq]; qlen = (int)(a.qlimits[bq + 1] - q0 - 1);
				}
				const dmnd_dp_target d{ q0, t0, ext_matrix_code(mat, a.use_cbs != 0, q0), qlen, tlen, b.d_begin, b.d_end };
				a.items[first + k] = d;
				const Geom geom = make_geom(qlen, tlen, b.d_begin, b.d_end);
				const int64_t steps = n_steps(geom);
				const int P = ext_class(rows, own, b.d_end - b.d_begin, steps);
				const int c = ext_class_slot(P, own);
				a.p_of_item[first + k] = P;
				a.rows[local + k] = trace_bytes(geom, P);
				const int64_t s16 = steps >> 4;
				a.keys[local + k] = ((uint32_t)c << 10) | (uint32_t)(1023 - (s16 < 1023 ? s16 : 1023));
				const uint32_t steps32 = (uint32_t)(steps < 0x7fffffff ? steps : 0x7fffffff);
				if (own) { atomicAdd(&h_own_count[c - EXT_OWN_CLASS], 1u); atomicMax(&h_own_steps[c - EXT_OWN_CLASS], steps32); }
				else { atomicAdd(&h_count[c], 1u); atomicMax(&h_steps[c], steps32); }
				cells += (unsigned long long)ext_cells(d);
				diag += (unsigned long long)(b.d_end - b.d_begin) * (unsigned long long)steps;
				lanes += (unsigned long long)(2 * P * class_lanes(P)) * (unsigned long long)steps;
			}
			atomicAdd(&h_cells, cells); atomicAdd(&h_diag, diag); atomicAdd(&h_lane, lanes);
		}
		if (g == 0) a.ctr->n_items = a.item_off[a.n_groups];
	}
	__syncthreads();
	if (threadIdx.x < EXT_CLASSES && h_count[threadIdx.x]) {
		atomicAdd(&a.ctr->class_count[threadIdx.x], h_count[threadIdx.x]);
		atomicMax(&a.ctr->class_max_steps[threadIdx.x], h_steps[threadIdx.x]);
	}
	if (a.g_mat && threadIdx.x < EXT_OWN_CLASS && h_own_count[threadIdx.x]) {
		atomicAdd(&a.cbs_ctr->class_count[threadIdx.x], h_own_count[threadIdx.x]);
		atomicMax(&a.cbs_ctr->class_max_steps[threadIdx.x], h_own_steps[threadIdx.x]);
	}
	if (threadIdx.x == 0 && h_cells) { atomicAdd(&a.ctr->cells1, h_cells); atomicAdd(&a.ctr->diag_steps, h_diag); atomicAdd(&a.ctr->lane_steps, h_lane); }
	if (threadIdx.x == 0 && h_targets) { atomicAdd(&a.ctr->window_targets, (unsigned long long)h_targets); atomicAdd(&a.ctr->window_bound, (unsigned long long)h_bound); }
}

__global__ __launch_bounds__(256) void ext_slots_kernel(ExtArgs a)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s > a.item_cap - a.item_base) return;
	a.rows_slot[s] = s < a.ctr->n_items ? a.rows[a.order[s]] : 0;
}

__global__ __launch_bounds__(256) void ext_offsets_kernel(ExtArgs a)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t n = a.ctr->n_items;
	if (s == 0) a.ctr->total_rows = (unsigned long long)a.off_slot[n];
	if (s >= n) return;
	const uint32_t item = a.order[s];                   // (relative to item_base, as the sweeps see the item arrays)
	a.off_item[a.item_base + item] = a.off_slot[s];
	// the packed 16-bit launches take their items in pairs (eights for a row class) of neighbours of the launch order; every class
	// starts a new wavefront, and the last wavefront of a class is filled up with -1 (dmnd_sweep_classes reads the same layout)
	const uint32_t c = a.keys_sorted[s] >> 10;
	if (c >= EXT_CLASSES) return;                        // (an own-matrix class: behind all others in the launch order, never in a packed launch)
	uint32_t s0 = 0, pair0 = 0;
	for (uint32_t x = 0; x < c; ++x) {
		const uint32_t per = (uint32_t)class_items_per_wave16(class_of_index((int)x));
		s0 += a.ctr->class_count[x]; pair0 += (a.ctr->class_count[x] + per - 1) / per * per;
	}
	const uint32_t count = a.ctr->class_count[c], per = (uint32_t)class_items_per_wave16(class_of_index((int)c));
	a.pairs[pair0 + (s - s0)] = (int32_t)item;
	if (s - s0 == count - 1)
		for (uint32_t x = count; x < (count + per - 1) / per * per; ++x) a.pairs[pair0 + x] = -1;
}

// behind an iteration's sweeps: its items' trace offsets from the first arena on (the walk of round 2 reads all arenas from one
// base), or -1 where the sweeps ran without keeping trace rows
__global__ __launch_bounds__(256) void ext_rebase_kernel(ExtArgs a, uint32_t n_items, int64_t rel, int kept)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n_items) a.off_item[a.item_base + i] = kept ? a.off_item[a.item_base + i] + rel : (int64_t)-1;
}

struct SelSlot { double ev; int score; uint32_t target; int tlen; uint32_t g; };

__device__ inline bool sel_less(const SelSlot& x, const SelSlot& y)      // Target::comp_evalue (target.h:123-129)
{
	return x.ev < y.ev || (x.ev == y.ev && (x.score > y.score || (x.score == y.score && x.target < y.target)));
}
// the host's own e-values could order the two the other way round (equal inputs give equal values on both sides). Two e-values
// that are 0.0 on both sides are ordered by score and target exactly, as the host orders them; next to the underflow the
// relative tolerance means nothing, and two tiny values are always flagged
// (translated queries: equal inputs also means contexts of equal length, read from the best items of the two groups)
__device__ inline bool sel_ambiguous(const ExtArgs& a, const SelSlot& x, const SelSlot& y)
{
	const ExtEvalue& p = a.ev;
	if (x.score == y.score && x.tlen == y.tlen && (a.contexts <= 1 || a.items[a.cand_item[x.g]].query_len == a.items[a.cand_item[y.g]].query_len)) return false;
	const int ux = ext_underflow(p, x.score), uy = ext_underflow(p, y.score);
	if (ux == 2 && uy == 2) return false;
	if ((ux == 1 || uy == 1) && fmax(x.ev, y.ev) < 1e-250) return true;
	return ext_near(x.ev, y.ev);
}

// the query's aligned targets into an LDS list (any order); returns their number (all lanes), cap + 1 if they do not fit
__device__ inline uint32_t gather_flagged(const ExtArgs& a, const uint8_t* flag8, const uint32_t* flag32, uint32_t g0, uint32_t ng, SelSlot* list, uint32_t cap, uint32_t* counter, uint32_t lane)
{
	if (lane == 0) *counter = 0;
	__syncthreads();
	for (uint32_t gi = lane; gi < ng; gi += 64) {
		const uint32_t g = g0 + gi;
		if (!(flag8 ? flag8[g] != 0 : flag32[g] != 0)) continue;
		const uint32_t x = atomicAdd(counter, 1u);
		if (x >= cap) continue;
		const uint32_t target = a.groups[g].target;
		list[x] = SelSlot{ a.cand_ev[g], a.ends[a.cand_item[g]].score, target, (int)(a.tlimits[target + 1] - a.tlimits[target] - 1), g };
	}
	__syncthreads();
	const uint32_t n = *counter;
	return n > cap ? cap + 1 : n;
}

// One ranking-chunk iteration of a query behind its sweeps (extend.cpp:289-336 with default options, one wavefront per query):
// the chunk's targets with a reported HSP (v), append_hits (culling.cpp:115-145) into the aligned targets, the next window, the
// tail rule (ranking_terminate, extend.cpp:111-119). last: no further chunk is allowed -- a query that would go on is handed back
// to the host like an ambiguous one (the reference goes on for as long as every chunk brings new hits)
__global__ __launch_bounds__(64) void ext_append_kernel(ExtArgs a, int last)
{
	extern __shared__ SelSlot lds[];
	__shared__ uint32_t n_v_sh, n_al_sh, flags_sh;
	__shared__ double kth_sh;
	__shared__ SelSlot kth_slot;
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	if (!a.q_active[q]) return;
	SelSlot* vs = lds;                                   // chunk_size entries
	SelSlot* al = lds + a.chunk_size;                    // k + chunk_size entries
	const uint32_t cap_al = (uint32_t)a.k + a.chunk_size;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin, ng = g1 - g0;
	const uint32_t i0 = a.q_i0[q], i1 = a.q_i1[q];
	if (lane == 0) { n_v_sh = 0; flags_sh = 0; }
	__syncthreads();
	bool amb = false, sat = false;
	for (uint32_t w = i0 + lane; w < i1; w += 64) {
		const uint32_t g = a.gorder[g0 + w], n = a.g_cnt[g], first = a.g_first[g];
		const uint32_t target = a.groups[g].target;
		const int tlen = (int)(a.tlimits[target + 1] - a.tlimits[target] - 1);
		// best HSP of the target among its bands that pass the report cutoff (gapped_score.cpp:182-268; Target::add_hit + inner_culling:
		// the highest score, of equal ones the band that starts first; over several contexts best_hsp_replaces, plan_core.h)
		bool have = false;
		int best = 0; uint32_t bi = 0; double bev = 0;
		for (uint32_t k = 0; k < n; ++k) {
			const SwipeEnd e = a.ends[first + k];
			if (e.pad[0]) sat = true;
			if (e.score <= 0) continue;
			const dmnd_dp_target it = a.items[first + k];      // (the e-value is that of the item's own context)
			const double ev = ext_evalue(a.ev, e.score, it.query_len, tlen);
			if (!ext_reported(a, e.score, ev, amb)) continue;
			if (!have || best_hsp_replaces(e.score, it.query_off, it.d_begin, best, a.items[bi].query_off, a.items[bi].d_begin)) { have = true; best = e.score; bi = first + k; bev = ev; }
		}
		a.cand_item[g] = bi;
		a.cand_ev[g] = bev;
		if (have) vs[atomicAdd(&n_v_sh, 1u)] = SelSlot{ bev, best, target, tlen, g };
	}
	__syncthreads();
	const uint32_t n_v = n_v_sh;
	bool new_hits = false;
	if (n_v > 0) {
		const uint32_t na = gather_flagged(a, a.aligned, nullptr, g0, ng, al, cap_al, &n_al_sh, lane);
		if (na > cap_al) amb = true;                       // (cannot happen: the list is cut to k before it grows by a chunk)
		new_hits = na < (uint32_t)a.k;
		const bool lost = __ballot(amb) != 0;              // (uniform: the branch below holds barriers)
		if (!new_hits && !lost) {
			// culling(targets, sort_only = false): the first k stay; the chunk is appended if its best e-value reaches the k-th's
			for (uint32_t x = lane; x < na; x += 64) {
				const SelSlot me = al[x];
				uint32_t rank = 0;
				for (uint32_t y = 0; y < na; ++y) {
					if (y == x) continue;
					if (sel_ambiguous(a, al[y], me)) amb = true;
					rank += sel_less(al[y], me) ? 1u : 0u;
				}
				if (rank >= (uint32_t)a.k) a.aligned[me.g] = 0;
				if (rank == (uint32_t)a.k - 1) { kth_sh = me.ev; kth_slot = me; }
			}
			__syncthreads();
			const double kth = kth_sh;
			const SelSlot ks = kth_slot;
			bool reach = false;
			for (uint32_t x = lane; x < n_v; x += 64) {
				if (sel_ambiguous(a, vs[x], ks)) amb = true;
				reach |= vs[x].ev <= kth;
			}
			if (__ballot(reach) != 0) new_hits = true;
		}
		if (new_hits) for (uint32_t x = lane; x < n_v; x += 64) a.aligned[vs[x].g] = 1;
	}
	const bool any_amb = __ballot(amb) != 0, any_sat = __ballot(sat) != 0;
	if (any_amb || any_sat) {
		// the host redoes the query: nothing of it stays here
		for (uint32_t gi = lane; gi < ng; gi += 64) a.aligned[g0 + gi] = 0;
		if (lane == 0) {
			a.qstate[q] = EXT_Q_AMBIGUOUS; a.q_active[q] = 0;
			if (any_amb) atomicAdd(&a.ctr->n_ambiguous, 1u);
			if (any_sat) atomicAdd(&a.ctr->n_saturated, 1u);
		}
		return;
	}
	// the next window and whether the ranking goes on (extend.cpp:325-336; uniform over the wavefront)
	const uint32_t n0 = i1, n1 = i1 + (a.chunk_size < ng - i1 ? a.chunk_size : ng - i1);
	const int prev = a.q_tail[q];
	const int next_tail = (int)a.groups[a.gorder[g0 + n1 - 1]].score;
	const bool terminate = !new_hits && (prev == 0 || (double)next_tail / (double)prev <= 0.95 || ext_bitscore(a.ev, next_tail) < 25.0);
	const bool go_on = n0 < ng && !terminate;
	if (go_on && last) {
		for (uint32_t gi = lane; gi < ng; gi += 64) a.aligned[g0 + gi] = 0;
		if (lane == 0) { a.qstate[q] = EXT_Q_CAPPED; a.q_active[q] = 0; atomicAdd(&a.ctr->n_capped, 1u); }
		return;
	}
	if (lane == 0) {
		a.q_prev[q] = prev;
		if (new_hits) a.q_tail[q] = next_tail;
		a.q_i0[q] = n0; a.q_i1[q] = n1;
		a.q_active[q] = go_on ? 1 : 0;
		if (go_on) atomicAdd(&a.ctr->n_active, 1u);
	}
}

// culling(aligned_targets) once the ranking is over (extend.cpp:331): sort by (e-value, score, target), the first k survive
__global__ __launch_bounds__(64) void ext_final_kernel(ExtArgs a)
{
	extern __shared__ SelSlot lds[];
	__shared__ uint32_t n_sh;
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	if (a.qstate[q] != EXT_Q_DEVICE || a.q_active[q]) return;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin, ng = g1 - g0;
	const uint32_t cap = (uint32_t)a.k + a.chunk_size;
	const uint32_t na = gather_flagged(a, a.aligned, nullptr, g0, ng, lds, cap, &n_sh, lane);
	bool amb = na > cap;
	if (!amb)
		for (uint32_t x = lane; x < na; x += 64) {
			const SelSlot me = lds[x];
			bool keep = true;
			if (na > (uint32_t)a.k) {
				uint32_t rank = 0;
				for (uint32_t y = 0; y < na; ++y) {
					if (y == x) continue;
					if (sel_ambiguous(a, lds[y], me)) amb = true;
					rank += sel_less(lds[y], me) ? 1u : 0u;
				}
				keep = rank < (uint32_t)a.k;
			}
			a.kept[me.g] = keep ? 1u : 0u;
		}
	if (__ballot(amb) != 0) {
		for (uint32_t gi = lane; gi < ng; gi += 64) { a.kept[g0 + gi] = 0; a.aligned[g0 + gi] = 0; }
		if (lane == 0) { a.qstate[q] = EXT_Q_AMBIGUOUS; atomicAdd(&a.ctr->n_ambiguous, 1u); }
	}
}

__global__ __launch_bounds__(256) void ext_round2_kernel(ExtArgs a)
{
	__shared__ unsigned long long h_cells;
	__shared__ uint32_t h_lost;
	if (threadIdx.x == 0) { h_cells = 0; h_lost = 0; }
	__syncthreads();
	const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g < a.n_groups) {
		if (g == 0) a.ctr->n_kept = a.kept_pos[a.n_groups];
		if (a.kept[g]) {
			const uint32_t k = a.kept_pos[g], item = a.cand_item[g];
			a.r2_order[k] = (int32_t)item;
			a.r2_p[k] = a.p_of_item[item];
			a.r2_off[k] = a.off_item[item];
			a.r2_group[k] = g;
			if (a.off_item[item] < 0) atomicAdd(&h_lost, 1u);
			atomicAdd(&h_cells, (unsigned long long)ext_cells(a.items[item]));
		}
	}
	__syncthreads();
	if (threadIdx.x == 0 && h_cells) atomicAdd(&a.ctr->cells2, h_cells);
	if (threadIdx.x == 0 && h_lost) atomicAdd(&a.ctr->n_resweep, h_lost);
}

// Round 2 for the survivors whose round-1 sweep kept no trace rows (the reference's round 2 sweeps every survivor again with
// traceback, gapped_final.cpp:66-160): a copy of the item behind all others, as one more iteration; the group's best item is the copy
__global__ __launch_bounds__(256) void ext_resweep_kernel(ExtArgs a, uint32_t n_kept)
{
	__shared__ uint32_t h_count[EXT_CLASSES], h_steps[EXT_CLASSES];
	__shared__ unsigned long long h_cells;
	__shared__ uint32_t h_own_count[EXT_OWN_CLASS], h_own_steps[EXT_OWN_CLASS];
	if (threadIdx.x < EXT_CLASSES) { h_count[threadIdx.x] = 0; h_steps[threadIdx.x] = 0; }
	if (threadIdx.x < EXT_OWN_CLASS) { h_own_count[threadIdx.x] = 0; h_own_steps[threadIdx.x] = 0; }
	if (threadIdx.x == 0) h_cells = 0;
	__syncthreads();
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < n_kept && a.r2_off[k] < 0) {
		const uint32_t local = atomicAdd(&a.ctr->n_items, 1u), copy = a.item_base + local;
		const dmnd_dp_target d = a.items[a.r2_order[k]];
		a.items[copy] = d;                        // (with its matrix code)
		const bool own = a.g_mat && d.cbs_off <= -2;
		const Geom geom = make_geom(d.query_len, d.target_len, d.d_begin, d.d_end);
		const int64_t steps = n_steps(geom);
		const int P = ext_class(a.ctr->n_resweep >= a.row_min_items, own, d.d_end - d.d_begin, steps);
		const int c = ext_class_slot(P, own);
		a.p_of_item[copy] = P;
		a.rows[local] = trace_bytes(geom, P);
		const int64_t s16 = steps >> 4;
		a.keys[local] = ((uint32_t)c << 10) | (uint32_t)(1023 - (s16 < 1023 ? s16 : 1023));
		const uint32_t steps32 = (uint32_t)(steps < 0x7fffffff ? steps : 0x7fffffff);
		if (own) { atomicAdd(&h_own_count[c - EXT_OWN_CLASS], 1u); atomicMax(&h_own_steps[c - EXT_OWN_CLASS], steps32); }
		else { atomicAdd(&h_count[c], 1u); atomicMax(&h_steps[c], steps32); }
		a.r2_order[k] = (int32_t)copy;
		a.r2_p[k] = P;                            // (the copy's class: the first sweep may have been in another one, ext_class)
		a.cand_item[a.r2_group[k]] = copy;
		atomicAdd(&h_cells, (unsigned long long)ext_cells(d));
	}
	__syncthreads();
	if (threadIdx.x < EXT_CLASSES && h_count[threadIdx.x]) {
		atomicAdd(&a.ctr->class_count[threadIdx.x], h_count[threadIdx.x]);
		atomicMax(&a.ctr->class_max_steps[threadIdx.x], h_steps[threadIdx.x]);
	}
	if (a.g_mat && threadIdx.x < EXT_OWN_CLASS && h_own_count[threadIdx.x]) {
		atomicAdd(&a.cbs_ctr->class_count[threadIdx.x], h_own_count[threadIdx.x]);
		atomicMax(&a.cbs_ctr->class_max_steps[threadIdx.x], h_own_steps[threadIdx.x]);
	}
	if (threadIdx.x == 0 && h_cells) atomicAdd(&a.ctr->cells_again, h_cells);
}

// ... and behind the sweeps of the copies: the walk's trace offsets of those slots
__global__ __launch_bounds__(256) void ext_rewalk_kernel(ExtArgs a, uint32_t n_kept)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k < n_kept && a.r2_off[k] < 0) a.r2_off[k] = a.off_item[a.r2_order[k]];
}

// the frame of a record: the context of the read whose sequence the winning item reads (0 for an untranslated query)
__device__ inline int32_t ext_frame(const ExtArgs& a, uint32_t read, const dmnd_dp_target& d)
{
	for (int f = a.contexts - 1; f > 0; --f)
		if (a.qlimits[(size_t)read * (size_t)a.contexts + (size_t)f] == d.query_off) return f;
	return 0;
}

__global__ __launch_bounds__(64) void ext_records_kernel(ExtArgs a)
{
	extern __shared__ SelSlot lds[];
	__shared__ uint32_t n_sh;
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	if (a.qstate[q] != EXT_Q_DEVICE) return;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin, ng = g1 - g0;
	const uint32_t first = a.kept_pos[g0];
	if (a.kept_pos[g1] == first) return;
	const uint32_t query = a.queries[q].query;
	const uint32_t nk = gather_flagged(a, nullptr, a.kept, g0, ng, lds, (uint32_t)a.k, &n_sh, lane);
	for (uint32_t x = lane; x < nk && x < (uint32_t)a.k; x += 64) {
		const SelSlot me = lds[x];
		uint32_t rank = 0;
		for (uint32_t y = 0; y < nk; ++y) rank += y != x && sel_less(lds[y], me) ? 1u : 0u;
		const uint32_t g = me.g, item = a.cand_item[g];
		const dmnd_dp_target d = a.items[item];
		dmnd_match& m = a.records[first + rank];             // (field by field into HBM: a local record would live in scratch memory)
		m.query = query; m.target = me.target;
		m.ungapped_score = a.ungapped0 ? (int32_t)a.ungapped0[g] : (int32_t)a.groups[g].score; m.d_begin = d.d_begin; m.d_end = d.d_end;
		m.frame = ext_frame(a, query, d); m.read_begin = 0; m.read_end = 0;
		m.evalue = me.ev; m.bit_score = 0.0;                  // the host writes its own e-value and the bit score
		const dmnd_hsp hsp = a.hsps[item];
		m.hsp.score = hsp.score; m.hsp.q_begin = hsp.q_begin; m.hsp.q_end = hsp.q_end; m.hsp.s_begin = hsp.s_begin; m.hsp.s_end = hsp.s_end;
		m.hsp.length = hsp.length; m.hsp.identities = hsp.identities; m.hsp.mismatches = hsp.mismatches; m.hsp.positives = hsp.positives;
		m.hsp.gap_openings = hsp.gap_openings; m.hsp.gaps = hsp.gaps; m.hsp.transcript_len = hsp.transcript_len;
		m.hsp.transcript_off = a.tr_on ? (int64_t)g : -1;      // (tr_on: its group, for launch_tr_gather)
	}
}

// ---- the ranking loop with HSP filters (a.filt_on) ----

// the query goes back to the host: nothing of it stays here
__device__ inline void ext_hand_back(const ExtArgs& a, uint32_t q, uint32_t g0, uint32_t ng, uint32_t lane, uint8_t state)
{
	for (uint32_t gi = lane; gi < ng; gi += 64) { a.aligned[g0 + gi] = 0; a.matched[g0 + gi] = 0; a.kept[g0 + gi] = 0; }
	if (lane == 0) { a.qstate[q] = state; a.q_active[q] = 0; }
}

// Behind a chunk's sweeps: best HSP per target past the report cutoff (the first loop of ext_append_kernel), flagged in `kept` --
// the list the trace walk runs over BEFORE any culling, so that the filters can read identities, length and coordinates of every
// target that a place among the -k could go to
__global__ __launch_bounds__(64) void ext_fcand_kernel(ExtArgs a)
{
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	if (!a.q_active[q]) return;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin, ng = g1 - g0;
	const uint32_t i0 = a.q_i0[q], i1 = a.q_i1[q];
	bool amb = false, sat = false;
	for (uint32_t w = i0 + lane; w < i1; w += 64) {
		const uint32_t g = a.gorder[g0 + w], n = a.g_cnt[g], first = a.g_first[g];
		const uint32_t target = a.groups[g].target;
		const int tlen = (int)(a.tlimits[target + 1] - a.tlimits[target] - 1);
		bool have = false;
		int best = 0; uint32_t bi = 0; double bev = 0;
		for (uint32_t k = 0; k < n; ++k) {
			const SwipeEnd e = a.ends[first + k];
			if (e.pad[0]) sat = true;
			if (e.score <= 0) continue;
			const dmnd_dp_target it = a.items[first + k];      // (the e-value is that of the item's own context)
			const double ev = ext_evalue(a.ev, e.score, it.query_len, tlen);
			if (!ext_reported(a, e.score, ev, amb)) continue;
			if (!have || best_hsp_replaces(e.score, it.query_off, it.d_begin, best, a.items[bi].query_off, a.items[bi].d_begin)) { have = true; best = e.score; bi = first + k; bev = ev; }
		}
		a.cand_item[g] = bi;
		a.cand_ev[g] = bev;
		a.kept[g] = have ? 1u : 0u;
	}
	const bool any_amb = __ballot(amb) != 0, any_sat = __ballot(sat) != 0;
	if (any_amb || any_sat) {
		ext_hand_back(a, q, g0, ng, lane, EXT_Q_AMBIGUOUS);
		if (lane == 0) { if (any_amb) atomicAdd(&a.ctr->n_ambiguous, 1u); if (any_sat) atomicAdd(&a.ctr->n_saturated, 1u); }
	}
	else if (lane == 0) atomicMax(&a.ctr->list_need, i1 < ng ? i1 : ng);      // (aligned targets + this chunk's <= targets swept so far)
}

// The HSP filters (filter_hsp, culling.cpp:147-170), one lane per target of the walked list: identity, approximate identity and the
// two covers of its HSP from what traceback_kernel left, with the arithmetic of the host path (filter_core.h) -- the verdict the
// ranking step below reads. A value on a threshold (within the tolerance of ext_near) is not decided here.
// Bound: n <= ctr->n_kept <= n_groups, the capacity of the round-2 arrays under filters (ExtLayout::nS); one byte per group written.
__global__ __launch_bounds__(256) void ext_filter_kernel(ExtArgs a, uint32_t n)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n) return;
	const uint32_t g = a.r2_group[k];
	const PlanGroup grp = a.groups[g];
	const uint32_t query = a.hits[grp.hit_begin].query, item = a.cand_item[g];
	const int tlen = (int)(a.tlimits[grp.target + 1] - a.tlimits[grp.target] - 1);
	// translated queries: a group is a (read, target) pair and `query` one of the read's contexts, not necessarily the one the best
	// HSP lies in -- the context's length is the walked item's, the read's length that of read query / contexts (< reads of the
	// block = the entries of source_lens, checked by the host before the call is taken)
	const int qlen = a.contexts > 1 ? a.items[item].query_len : (int)(a.qlimits[query + 1] - a.qlimits[query] - 1);
	const int rlen = a.contexts > 1 ? a.source_lens[query / (uint32_t)a.contexts] : 0;
	const dmnd_hsp h = a.hsps[item];
	const FilterValues v = filter_values_contexts(h.score, h.identities, h.length, h.q_begin, h.q_end, h.s_begin, h.s_end, a.contexts, qlen, rlen, tlen);
	a.fverdict[g] = filter_on_threshold(a.filt, v) ? EXT_F_THRESHOLD : filter_fails(a.filt, v) ? EXT_F_FAIL : EXT_F_PASS;
}

// ranks of the LDS list's entries [0, n) among themselves in Target::comp_evalue order; returns whether a pair's order is ambiguous
__device__ inline bool rank_list(const ExtArgs& a, const SelSlot* list, uint32_t n, uint16_t* rank_of, uint32_t lane)
{
	bool amb = false;
	for (uint32_t x = lane; x < n; x += 64) {
		const SelSlot me = list[x];
		uint32_t rank = 0;
		for (uint32_t y = 0; y < n; ++y) {
			if (y == x) continue;
			if (sel_ambiguous(a, list[y], me)) amb = true;
			rank += sel_less(list[y], me) ? 1u : 0u;
		}
		rank_of[x] = (uint16_t)rank;
	}
	return amb;
}

// One ranking step of a query with HSP filters, behind the walk and the filter kernel (one wavefront per query):
//   append_hits without culling (culling.cpp:115-145 with with_culling = false, extend.cpp:272): the chunk's targets always join the
//     aligned targets; new_hits = fewer than k were aligned, or the chunk's best e-value reaches the k-th best's
//   the next window and the tail rule, as ext_append_kernel
//   where the chunk loop ends: round 2 (gapped_final.cpp:105-152) over the aligned targets in e-value order, a step of
//     ceil16(max(k - passed, 16)) targets at a time until k matches (with those of earlier rounds) passed the filters or the list
//     ends -- a target that fails a filter takes no place; the first k that passed become matches
//   extend.cpp:336: fewer than k matches, targets left and the last chunk had hits -> the chunk loop starts again, no target aligned
// LDS (dynamic): cap slots -- the most any active query can need, at most EXT_FILTER_LIST --, their ranks, verdicts by rank,
// selection by rank: 28 bytes per slot. A query with more than EXT_FILTER_LIST aligned targets goes
// back to the host (counted with the capped ones).
__global__ __launch_bounds__(64) void ext_fappend_kernel(ExtArgs a, int last, uint32_t cap)
{
	extern __shared__ SelSlot lds[];
	SelSlot* list = lds;
	uint16_t* rank_of = reinterpret_cast<uint16_t*>(lds + cap);
	uint8_t* verdict = reinterpret_cast<uint8_t*>(rank_of + cap);
	uint8_t* sel = verdict + cap;
	__shared__ uint32_t n_sh, res_sh[4];
	__shared__ SelSlot kth_slot;
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	if (!a.q_active[q]) return;
	const uint32_t K = (uint32_t)a.k;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin, ng = g1 - g0;
	const uint32_t i1 = a.q_i1[q];
	const uint32_t na = gather_flagged(a, a.aligned, nullptr, g0, ng, list, cap, &n_sh, lane);
	uint32_t nv = 0;
	if (na <= cap) nv = gather_flagged(a, nullptr, a.kept, g0, ng, list + na, cap - na, &n_sh, lane);
	if (na > cap || nv > cap - na) {
		ext_hand_back(a, q, g0, ng, lane, EXT_Q_CAPPED);
		if (lane == 0) atomicAdd(&a.ctr->n_capped, 1u);
		return;
	}
	const uint32_t n = na + nv;
	bool amb = false;
	bool new_hits = nv > 0 && na < K;
	if (nv > 0 && !new_hits) {
		amb |= rank_list(a, list, na, rank_of, lane);
		__syncthreads();
		for (uint32_t x = lane; x < na; x += 64) if (rank_of[x] == K - 1) kth_slot = list[x];
		__syncthreads();
		const SelSlot ks = kth_slot;
		bool reach = false;
		for (uint32_t x = na + lane; x < n; x += 64) {
			if (sel_ambiguous(a, list[x], ks)) amb = true;
			reach |= list[x].ev <= ks.ev;
		}
		new_hits = __ballot(reach) != 0;
	}
	// the next window and whether the chunk loop goes on (extend.cpp:325-336)
	const uint32_t n0 = i1, n1 = i1 + (a.chunk_size < ng - i1 ? a.chunk_size : ng - i1);
	const int prev = a.q_tail[q];
	const int next_tail = (int)a.groups[a.gorder[g0 + n1 - 1]].score;
	const bool terminate = !new_hits && (prev == 0 || (double)next_tail / (double)prev <= 0.95 || ext_bitscore(a.ev, next_tail) < 25.0);
	bool go_on = n0 < ng && !terminate;
	uint32_t matched_now = a.q_matched[q];
	bool threshold = false;
	const bool round2 = !go_on;
	if (round2) {
		// round 2: the aligned targets in e-value order, a step at a time
		__syncthreads();
		amb |= rank_list(a, list, n, rank_of, lane);
		__syncthreads();
		for (uint32_t x = lane; x < n; x += 64) verdict[rank_of[x]] = a.fverdict[list[x].g];
		__syncthreads();
		if (lane == 0) {
			uint32_t pos = 0, passed = 0, removed = 0, thr = 0;
			for (;;) {
				const uint32_t left = n - pos, want = K - passed > 16 ? K - passed : 16;
				const uint32_t step = (want + 15) / 16 * 16 < left ? (want + 15) / 16 * 16 : left;
				uint32_t got = 0;
				for (uint32_t r = pos; r < pos + step; ++r) {
					const uint8_t v = verdict[r];
					sel[r] = v == EXT_F_PASS && passed + got < K ? 1 : 0;
					got += v == EXT_F_PASS ? 1u : 0u; removed += v == EXT_F_FAIL ? 1u : 0u; thr += v == EXT_F_THRESHOLD ? 1u : 0u;
				}
				passed = passed + got < K ? passed + got : K;      // culling(matches): the first k of the round stay
				pos += step;
				if (!(pos < n && passed + matched_now < K)) break;
			}
			for (uint32_t r = pos; r < n; ++r) sel[r] = 0;
			res_sh[0] = passed; res_sh[1] = removed; res_sh[2] = thr;
		}
		__syncthreads();
		threshold = res_sh[2] != 0;
	}
	const bool any_amb = __ballot(amb) != 0;
	if (any_amb || threshold) {
		ext_hand_back(a, q, g0, ng, lane, EXT_Q_AMBIGUOUS);
		if (lane == 0) { if (any_amb) atomicAdd(&a.ctr->n_ambiguous, 1u); else atomicAdd(&a.ctr->n_threshold, 1u); }
		return;
	}
	if (round2) {
		for (uint32_t x = lane; x < n; x += 64) {
			const uint32_t g = list[x].g;
			a.aligned[g] = 0;
			if (sel[rank_of[x]]) a.matched[g] = 1;
		}
		matched_now += res_sh[0];
		// extend.cpp:336: the chunk loop starts again
		go_on = matched_now < K && n0 < ng && nv > 0;
	}
	else for (uint32_t x = na + lane; x < n; x += 64) a.aligned[list[x].g] = 1;
	if (go_on && last) {
		ext_hand_back(a, q, g0, ng, lane, EXT_Q_CAPPED);
		if (lane == 0) atomicAdd(&a.ctr->n_capped, 1u);
		return;
	}
	if (lane == 0) {
		a.q_prev[q] = prev;
		if (new_hits) a.q_tail[q] = next_tail;
		a.q_i0[q] = n0; a.q_i1[q] = n1;
		a.q_matched[q] = matched_now;
		if (round2) a.q_removed[q] += res_sh[1];
		a.q_active[q] = go_on ? 1 : 0;
		if (go_on) atomicAdd(&a.ctr->n_active, 1u);
	}
}

// culling(matches) once every round is over (extend.cpp:341): the first k of the query's matches by (e-value, score, target)
__global__ __launch_bounds__(64) void ext_ffinal_kernel(ExtArgs a)
{
	extern __shared__ SelSlot list[];                      // 2 k slots
	__shared__ uint32_t n_sh;
	const uint32_t cap = 2 * (uint32_t)a.k;
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin, ng = g1 - g0;
	for (uint32_t gi = lane; gi < ng; gi += 64) a.kept[g0 + gi] = 0;
	if (q == 0 && lane == 0) { a.kept[a.n_groups] = 0; a.ctr->n_resweep = 0; }
	if (a.qstate[q] != EXT_Q_DEVICE) return;
	__syncthreads();
	const uint32_t nm = gather_flagged(a, a.matched, nullptr, g0, ng, list, cap, &n_sh, lane);
	bool amb = nm > cap;                                  // (cannot happen: fewer than 2 k matches)
	if (!amb)
		for (uint32_t x = lane; x < nm; x += 64) {
			const SelSlot me = list[x];
			bool keep = true;
			if (nm > (uint32_t)a.k) {
				uint32_t rank = 0;
				for (uint32_t y = 0; y < nm; ++y) {
					if (y == x) continue;
					if (sel_ambiguous(a, list[y], me)) amb = true;
					rank += sel_less(list[y], me) ? 1u : 0u;
				}
				keep = rank < (uint32_t)a.k;
			}
			a.kept[me.g] = keep ? 1u : 0u;
		}
	if (__ballot(amb) != 0) {
		for (uint32_t gi = lane; gi < ng; gi += 64) a.kept[g0 + gi] = 0;
		if (lane == 0) { a.qstate[q] = EXT_Q_AMBIGUOUS; atomicAdd(&a.ctr->n_ambiguous, 1u); }
	}
	else if (lane == 0 && a.q_removed[q]) atomicAdd(&a.ctr->n_filtered, a.q_removed[q]);
}

// ---- --top (a.top_on): culling by score against a threshold, top_core.h ----

__device__ inline int wave_max(int v) { for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off); v = o > v ? o : v; } return v; }
__device__ inline int wave_min(int v) { for (int off = 32; off >= 1; off >>= 1) { const int o = __shfl_xor(v, off); v = o < v ? o : v; } return v; }
__device__ inline uint32_t wave_sum(uint32_t v) { for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off); return v; }

// the query goes back to the host: nothing of it stays here
__device__ inline void ext_top_hand_back(const ExtArgs& a, uint32_t q, uint32_t g0, uint32_t ng, uint32_t lane, uint8_t state)
{
	for (uint32_t gi = lane; gi < ng; gi += 64) { a.aligned[g0 + gi] = 0; a.kept[g0 + gi] = 0; }
	if (lane == 0) { a.qstate[q] = state; a.q_active[q] = 0; }
}

// One ranking-chunk iteration of a query under --top behind its sweeps (one wavefront per query): the chunk's targets with a reported
// HSP (V), append_hits with culling (culling.cpp:115-145 with config.toppercent): the aligned targets A are cut to those whose bit
// score reaches max((1 - top/100) x bits(best of A), 1.0), V joins them if A is empty or V's best score reaches
// (int)((1 - top/100) x lowest score left in A), and that same condition is new_hits; then the next window and the tail rule as
// ext_append_kernel. A and its cut are two reductions over the query's `aligned` flags and scores in HBM (both loaded for every group,
// so a pass is one round trip per 64 groups): no list, no limit on |A|. Indices: groups g0 + gi < g1 <= n_groups, the per-group arrays'
// size; the window [i0, i1) lies inside [0, ng).
__global__ __launch_bounds__(64) void ext_top_append_kernel(ExtArgs a, int last)
{
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	if (!a.q_active[q]) return;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin, ng = g1 - g0;
	const uint32_t i0 = a.q_i0[q], i1 = a.q_i1[q];
	bool amb = false, sat = false;
	int max_v = 0;
	for (uint32_t w = i0 + lane; w < i1; w += 64) {
		const uint32_t g = a.gorder[g0 + w], n = a.g_cnt[g], first = a.g_first[g];
		const uint32_t target = a.groups[g].target;
		const int tlen = (int)(a.tlimits[target + 1] - a.tlimits[target] - 1);
		// best HSP of the target among its bands that pass the report cutoff, as ext_append_kernel
		bool have = false;
		int best = 0; uint32_t bi = 0; double bev = 0;
		for (uint32_t k = 0; k < n; ++k) {
			const SwipeEnd e = a.ends[first + k];
			if (e.pad[0]) sat = true;
			if (e.score <= 0) continue;
			const dmnd_dp_target it = a.items[first + k];      // (the e-value is that of the item's own context)
			const double ev = ext_evalue(a.ev, e.score, it.query_len, tlen);
			if (!ext_reported(a, e.score, ev, amb)) continue;
			if (!have || best_hsp_replaces(e.score, it.query_off, it.d_begin, best, a.items[bi].query_off, a.items[bi].d_begin)) { have = true; best = e.score; bi = first + k; bev = ev; }
		}
		a.cand_item[g] = bi;
		a.cand_ev[g] = bev;
		a.cand_score[g] = have ? best : 0;
		max_v = best > max_v ? best : max_v;
	}
	max_v = wave_max(max_v);
	bool new_hits = false;
	if (max_v > 0) {
		// (the scores read below are those of earlier chunks -- earlier launches --: the window's targets are not aligned yet)
		int max_a = 0;
		for (uint32_t gi = lane; gi < ng; gi += 64) {
			const uint8_t al = a.aligned[g0 + gi];
			const int s = a.cand_score[g0 + gi];
			if (al && s > max_a) max_a = s;
		}
		max_a = wave_max(max_a);
		int min_a = 0x7fffffff;
		if (max_a > 0)
			for (uint32_t gi = lane; gi < ng; gi += 64) {
				const uint8_t al = a.aligned[g0 + gi];
				const int s = a.cand_score[g0 + gi];
				if (!al) continue;
				if (top_near(a.top, s, max_a)) amb = true;
				if (top_pass(a.top, s, max_a)) min_a = s < min_a ? s : min_a;
				else a.aligned[g0 + gi] = 0;
			}
		min_a = wave_min(min_a);
		new_hits = min_a == 0x7fffffff || top_append(a.top, max_v, min_a);      // (nothing aligned, or nothing left of it)
		if (new_hits)
			for (uint32_t w = i0 + lane; w < i1; w += 64) {
				const uint32_t g = a.gorder[g0 + w];
				if (a.cand_score[g] > 0) a.aligned[g] = 1;               // (written by this lane above)
			}
	}
	const bool any_amb = __ballot(amb) != 0, any_sat = __ballot(sat) != 0;
	if (any_amb || any_sat) {
		ext_top_hand_back(a, q, g0, ng, lane, EXT_Q_AMBIGUOUS);
		if (lane == 0) { if (any_amb) atomicAdd(&a.ctr->n_ambiguous, 1u); if (any_sat) atomicAdd(&a.ctr->n_saturated, 1u); }
		return;
	}
	// the next window and whether the ranking goes on (extend.cpp:325-336; uniform over the wavefront)
	const uint32_t n0 = i1, n1 = i1 + (a.chunk_size < ng - i1 ? a.chunk_size : ng - i1);
	const int prev = a.q_tail[q];
	const int next_tail = (int)a.groups[a.gorder[g0 + n1 - 1]].score;
	const bool terminate = !new_hits && (prev == 0 || (double)next_tail / (double)prev <= 0.95 || ext_bitscore(a.ev, next_tail) < 25.0);
	const bool go_on = n0 < ng && !terminate;
	if (go_on && last) {
		ext_top_hand_back(a, q, g0, ng, lane, EXT_Q_CAPPED);
		if (lane == 0) atomicAdd(&a.ctr->n_capped, 1u);
		return;
	}
	if (lane == 0) {
		a.q_prev[q] = prev;
		if (new_hits) a.q_tail[q] = next_tail;
		a.q_i0[q] = n0; a.q_i1[q] = n1;
		a.q_active[q] = go_on ? 1 : 0;
		if (go_on) atomicAdd(&a.ctr->n_active, 1u);
	}
}

// culling(aligned_targets) once the ranking is over (extend.cpp:331) under --top: the same cut once more; what it leaves is walked.
// Every group of the query gets its `kept` flag (ext_window_kernel cleared them for this iteration).
__global__ __launch_bounds__(64) void ext_top_final_kernel(ExtArgs a)
{
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	if (a.qstate[q] != EXT_Q_DEVICE || a.q_active[q]) return;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin, ng = g1 - g0;
	int max_a = 0;
	for (uint32_t gi = lane; gi < ng; gi += 64) {
		const uint8_t al = a.aligned[g0 + gi];
		const int s = a.cand_score[g0 + gi];
		if (al && s > max_a) max_a = s;
	}
	max_a = wave_max(max_a);
	bool amb = false;
	for (uint32_t gi = lane; gi < ng; gi += 64) {
		const uint8_t al = a.aligned[g0 + gi];
		const int s = a.cand_score[g0 + gi];
		bool keep = false;
		if (al) { if (top_near(a.top, s, max_a)) amb = true; keep = top_pass(a.top, s, max_a); }
		a.kept[g0 + gi] = keep ? 1u : 0u;
	}
	if (__ballot(amb) != 0) {
		ext_top_hand_back(a, q, g0, ng, lane, EXT_Q_AMBIGUOUS);
		if (lane == 0) atomicAdd(&a.ctr->n_ambiguous, 1u);
	}
}

// --top with HSP filters, behind the walk of the survivors and ext_filter_kernel (gapped_final.cpp:103-154, culling.cpp:199-202):
// a match that a filter removed stays as a placeholder of score 0, the matches are cut against the best one that passed -- none
// passed: none is reported. A value on a filter threshold hands the query back; so does a cutoff so low that the placeholders
// themselves would pass it (bits(0) against max(f x bits(best), 1.0): --top near 100 only).
__global__ __launch_bounds__(64) void ext_top_ffinal_kernel(ExtArgs a)
{
	const uint32_t q = blockIdx.x, lane = threadIdx.x;
	if (a.qstate[q] != EXT_Q_DEVICE) return;
	const uint32_t g0 = a.queries[q].group_begin, g1 = a.queries[q + 1].group_begin, ng = g1 - g0;
	int best = 0;
	uint32_t n_fail = 0;
	bool thr = false;
	for (uint32_t gi = lane; gi < ng; gi += 64) {
		const uint32_t kp = a.kept[g0 + gi];
		const uint8_t v = a.fverdict[g0 + gi];
		const int s = a.cand_score[g0 + gi];
		if (!kp) continue;
		thr |= v == EXT_F_THRESHOLD;
		n_fail += v == EXT_F_FAIL ? 1u : 0u;
		if (v == EXT_F_PASS && s > best) best = s;
	}
	best = wave_max(best);
	n_fail = wave_sum(n_fail);
	if (__ballot(thr) != 0) {
		ext_top_hand_back(a, q, g0, ng, lane, EXT_Q_AMBIGUOUS);
		if (lane == 0) atomicAdd(&a.ctr->n_threshold, 1u);
		return;
	}
	bool amb = n_fail > 0 && best > 0 && (top_pass(a.top, 0, best) || top_near(a.top, 0, best));
	for (uint32_t gi = lane; gi < ng; gi += 64) {
		const uint32_t kp = a.kept[g0 + gi];
		const uint8_t v = a.fverdict[g0 + gi];
		const int s = a.cand_score[g0 + gi];
		if (!kp) continue;
		bool keep = false;
		if (v == EXT_F_PASS && best > 0) { if (top_near(a.top, s, best)) amb = true; keep = top_pass(a.top, s, best); }
		a.kept[g0 + gi] = keep ? 1u : 0u;
	}
	if (__ballot(amb) != 0) {
		ext_top_hand_back(a, q, g0, ng, lane, EXT_Q_AMBIGUOUS);
		if (lane == 0) atomicAdd(&a.ctr->n_ambiguous, 1u);
	}
	else if (lane == 0 && n_fail) atomicAdd(&a.ctr->n_filtered, n_fail);
}

// Record order under --top: a sort key per entry of the walked list (n <= r2_cap = n_groups entries, the size of okeys / oidx):
// (query, 0xffffffff - score) for an entry that is a record, all ones -- behind every record -- for one that is none (filtered, cut,
// or its query handed back). The list is in load order, so a stable sort by this key is Match::cmp_score order inside a query.
__global__ __launch_bounds__(256) void ext_top_keys_kernel(ExtArgs a, uint32_t n)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	bool rec = false;
	if (k < n) {
		const uint32_t g = a.r2_group[k];
		rec = a.kept[g] != 0;
		const uint32_t query = a.hits[a.groups[g].hit_begin].query / (uint32_t)a.contexts;      // (the read)
		a.okeys[k] = rec ? ((uint64_t)query << 32) | (uint64_t)(0xffffffffu - (uint32_t)a.cand_score[g]) : ~(uint64_t)0;
		a.oidx[k] = k;
	}
	const unsigned long long m = __ballot(rec);
	if ((threadIdx.x & 63) == 0 && m) atomicAdd(&a.ctr->n_records, (uint32_t)__popcll(m));
}

// ... and the records through the sorted permutation: record i < ctr->n_records <= n <= r2_cap, the size of `records` under --top
__global__ __launch_bounds__(256) void ext_top_records_kernel(ExtArgs a, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n || i >= a.ctr->n_records) return;
	const uint32_t g = a.r2_group[a.rperm[i]], item = a.cand_item[g];
	const PlanGroup grp = a.groups[g];
	const dmnd_dp_target d = a.items[item];
	dmnd_match& m = a.records[i];                            // (field by field into HBM: a local record would live in scratch memory)
	m.query = a.hits[grp.hit_begin].query / (uint32_t)a.contexts; m.target = grp.target;
	m.ungapped_score = a.ungapped0 ? (int32_t)a.ungapped0[g] : (int32_t)grp.score; m.d_begin = d.d_begin; m.d_end = d.d_end;
	m.frame = ext_frame(a, m.query, d); m.read_begin = 0; m.read_end = 0;
	m.evalue = a.cand_ev[g]; m.bit_score = 0.0;               // the host writes its own e-value and the bit score
	const dmnd_hsp hsp = a.hsps[item];
	m.hsp.score = hsp.score; m.hsp.q_begin = hsp.q_begin; m.hsp.q_end = hsp.q_end; m.hsp.s_begin = hsp.s_begin; m.hsp.s_end = hsp.s_end;
	m.hsp.length = hsp.length; m.hsp.identities = hsp.identities; m.hsp.mismatches = hsp.mismatches; m.hsp.positives = hsp.positives;
	m.hsp.gap_openings = hsp.gap_openings; m.hsp.gaps = hsp.gaps; m.hsp.transcript_len = hsp.transcript_len;
	m.hsp.transcript_off = a.tr_on ? (int64_t)g : -1;          // (tr_on: its group, for launch_tr_gather)
}

hipError_t ensure_tmp(void** tmp, size_t* have, size_t need)
{
	if (need <= *have) return hipSuccess;
	if (*tmp) (void)hipFree(*tmp);
	*tmp = nullptr; *have = 0;
	const hipError_t e = hipMalloc(tmp, need);
	if (e == hipSuccess) *have = need;
	return e;
}

int bits_for(uint32_t n) { int b = 1; while (b < 32 && ((uint32_t)1 << b) <= n) ++b; return b; }

}  // namespace

hipError_t launch_ext_begin(const ExtArgs& a, hipStream_t st)
{
	hipError_t e = hipMemsetAsync(a.ctr, 0, sizeof(ExtCounters), st);
	if (e != hipSuccess) return e;
	e = hipMemsetAsync(a.r2_tr, 0, (size_t)a.r2_tr_clear * sizeof(int64_t), st);
	if (e != hipSuccess) return e;
	const int key_bits = 16 + bits_for(a.n_queries);
	size_t need = 0;
	e = rocprim::radix_sort_pairs(nullptr, need, a.okeys, a.okeys_sorted, a.oidx, a.gorder, (size_t)a.n_groups, 0, key_bits, st);
	if (e != hipSuccess) return e;
	e = ensure_tmp(a.scan_tmp, a.scan_tmp_bytes, need);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_mark_kernel, dim3(a.n_queries), dim3(64), 0, st, a);
	e = rocprim::radix_sort_pairs(*a.scan_tmp, need, a.okeys, a.okeys_sorted, a.oidx, a.gorder, (size_t)a.n_groups, 0, key_bits, st);
	if (e != hipSuccess) return e;
	return hipGetLastError();
}

namespace {

// the iteration's counters (the cell counts and the flags of the call stay)
hipError_t reset_iteration(const ExtArgs& a, hipStream_t st)
{
	hipError_t e = hipMemsetAsync(&a.ctr->n_items, 0, 2 * sizeof(uint32_t), st);
	if (e != hipSuccess) return e;
	if (a.g_mat) {
		e = hipMemsetAsync(a.cbs_ctr->class_count, 0, 2 * EXT_OWN_CLASS * sizeof(uint32_t), st);
		if (e != hipSuccess) return e;
	}
	return hipMemsetAsync(a.ctr->class_count, 0, 2 * EXT_CLASSES * sizeof(uint32_t) + sizeof(unsigned long long), st);
}

// launch order, trace offsets and pairs of the items the iteration has written (keys, rows, class histogram)
hipError_t order_items(const ExtArgs& a, hipStream_t st)
{
	const uint32_t n_left = a.item_cap - a.item_base;
	const unsigned bB = (n_left + 1 + 255) / 256;
	size_t need_b = 0, need_c = 0;
	hipError_t e = rocprim::radix_sort_pairs(nullptr, need_b, a.keys, a.keys_sorted, a.idx, a.order, (size_t)n_left, 0, 15, st);
	if (e != hipSuccess) return e;
	e = rocprim::exclusive_scan(nullptr, need_c, a.rows_slot, a.off_slot, (int64_t)0, (size_t)n_left + 1, rocprim::plus<int64_t>(), st);
	if (e != hipSuccess) return e;
	e = ensure_tmp(a.scan_tmp, a.scan_tmp_bytes, need_b > need_c ? need_b : need_c);
	if (e != hipSuccess) return e;
	if (n_left > 0) {
		e = rocprim::radix_sort_pairs(*a.scan_tmp, need_b, a.keys, a.keys_sorted, a.idx, a.order, (size_t)n_left, 0, 15, st);
		if (e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(ext_slots_kernel, dim3(bB), dim3(256), 0, st, a);
	e = rocprim::exclusive_scan(*a.scan_tmp, need_c, a.rows_slot, a.off_slot, (int64_t)0, (size_t)n_left + 1, rocprim::plus<int64_t>(), st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_offsets_kernel, dim3(bB), dim3(256), 0, st, a);
	return hipGetLastError();
}

}  // namespace

hipError_t launch_ext_prepare(const ExtArgs& a, hipStream_t st)
{
	const uint32_t n_left = a.item_cap - a.item_base;
	size_t need_a = 0;
	hipError_t e = rocprim::exclusive_scan(nullptr, need_a, a.cnt, a.item_off, 0u, (size_t)a.n_groups + 1, rocprim::plus<uint32_t>(), st);
	if (e != hipSuccess) return e;
	e = ensure_tmp(a.scan_tmp, a.scan_tmp_bytes, need_a);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_window_kernel, dim3(a.n_queries), dim3(64), 0, st, a);
	if (n_left > 0) hipLaunchKernelGGL(ext_init_kernel, dim3((n_left + 255) / 256), dim3(256), 0, st, a);
	e = rocprim::exclusive_scan(*a.scan_tmp, need_a, a.cnt, a.item_off, 0u, (size_t)a.n_groups + 1, rocprim::plus<uint32_t>(), st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_items_kernel, dim3((a.n_groups + 255) / 256), dim3(256), 0, st, a);
	return order_items(a, st);
}

hipError_t launch_ext_cbs_begin(const ExtArgs& a, const int8_t* qblock, hipStream_t st)
{
	hipLaunchKernelGGL(ext_cbs_comp_kernel, dim3(a.n_queries), dim3(64), 0, st, a, qblock);
	return hipGetLastError();
}

hipError_t launch_ext_cbs_window(const ExtArgs& a, hipStream_t st)
{
	const uint32_t n_left = a.item_cap - a.item_base;
	size_t need = 0;
	hipError_t e = rocprim::exclusive_scan(nullptr, need, a.c_flag, a.c_pos, 0u, (size_t)a.n_groups + 1, rocprim::plus<uint32_t>(), st);
	if (e != hipSuccess) return e;
	e = ensure_tmp(a.scan_tmp, a.scan_tmp_bytes, need);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_window_kernel, dim3(a.n_queries), dim3(64), 0, st, a);
	if (n_left > 0) hipLaunchKernelGGL(ext_init_kernel, dim3((n_left + 255) / 256), dim3(256), 0, st, a);
	hipLaunchKernelGGL(ext_cbs_flag_kernel, dim3((a.n_groups + 1 + 255) / 256), dim3(256), 0, st, a);
	e = rocprim::exclusive_scan(*a.scan_tmp, need, a.c_flag, a.c_pos, 0u, (size_t)a.n_groups + 1, rocprim::plus<uint32_t>(), st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_cbs_pairs_kernel, dim3((a.n_groups + 255) / 256), dim3(256), 0, st, a);
	return hipGetLastError();
}

hipError_t launch_ext_cbs_matrices(const ExtArgs& a, int64_t before, uint32_t n_pairs, bool keep, hipStream_t st)
{
	if (n_pairs == 0) return hipSuccess;
	hipLaunchKernelGGL(ext_cbs_matrices_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, st, a, before, n_pairs, keep ? 1 : 0);
	return hipGetLastError();
}

hipError_t launch_ext_cbs_items(const ExtArgs& a, hipStream_t st)
{
	size_t need_a = 0;
	hipError_t e = rocprim::exclusive_scan(nullptr, need_a, a.cnt, a.item_off, 0u, (size_t)a.n_groups + 1, rocprim::plus<uint32_t>(), st);
	if (e != hipSuccess) return e;
	e = ensure_tmp(a.scan_tmp, a.scan_tmp_bytes, need_a);
	if (e != hipSuccess) return e;
	e = rocprim::exclusive_scan(*a.scan_tmp, need_a, a.cnt, a.item_off, 0u, (size_t)a.n_groups + 1, rocprim::plus<uint32_t>(), st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_items_kernel, dim3((a.n_groups + 255) / 256), dim3(256), 0, st, a);
	return order_items(a, st);
}

hipError_t launch_ext_append(const ExtArgs& a, uint32_t n_items, bool kept, int64_t rel, bool last, hipStream_t st)
{
	if (n_items > 0 && (!kept || rel != 0)) hipLaunchKernelGGL(ext_rebase_kernel, dim3((n_items + 255) / 256), dim3(256), 0, st, a, n_items, rel, kept ? 1 : 0);
	// (n_active, n_resweep, cells2 and the kept flags were cleared by this iteration's ext_window_kernel: the round-2 list below is
	// rebuilt behind every iteration)
	hipError_t e = hipSuccess;
	const size_t lds_append = ((size_t)a.k + 2 * (size_t)a.chunk_size) * sizeof(SelSlot), lds_final = ((size_t)a.k + (size_t)a.chunk_size) * sizeof(SelSlot);
	hipLaunchKernelGGL(ext_append_kernel, dim3(a.n_queries), dim3(64), lds_append, st, a, last ? 1 : 0);
	// speculatively (the host only uses it when no query is left ranking): final culling, record slots, the round-2 list
	size_t need = 0;
	e = rocprim::exclusive_scan(nullptr, need, a.kept, a.kept_pos, 0u, (size_t)a.n_groups + 1, rocprim::plus<uint32_t>(), st);
	if (e != hipSuccess) return e;
	e = ensure_tmp(a.scan_tmp, a.scan_tmp_bytes, need);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_final_kernel, dim3(a.n_queries), dim3(64), lds_final, st, a);
	e = rocprim::exclusive_scan(*a.scan_tmp, need, a.kept, a.kept_pos, 0u, (size_t)a.n_groups + 1, rocprim::plus<uint32_t>(), st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_round2_kernel, dim3((a.n_groups + 255) / 256), dim3(256), 0, st, a);
	return hipGetLastError();
}

namespace {
// record slots (exclusive scan of the kept flags) and the list the trace walk runs over
hipError_t list_kept(const ExtArgs& a, hipStream_t st)
{
	size_t need = 0;
	hipError_t e = rocprim::exclusive_scan(nullptr, need, a.kept, a.kept_pos, 0u, (size_t)a.n_groups + 1, rocprim::plus<uint32_t>(), st);
	if (e != hipSuccess) return e;
	e = ensure_tmp(a.scan_tmp, a.scan_tmp_bytes, need);
	if (e != hipSuccess) return e;
	e = rocprim::exclusive_scan(*a.scan_tmp, need, a.kept, a.kept_pos, 0u, (size_t)a.n_groups + 1, rocprim::plus<uint32_t>(), st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_round2_kernel, dim3((a.n_groups + 255) / 256), dim3(256), 0, st, a);
	return hipGetLastError();
}
}

hipError_t launch_ext_fcand(const ExtArgs& a, uint32_t n_items, bool kept, int64_t rel, hipStream_t st)
{
	if (n_items > 0 && (!kept || rel != 0)) hipLaunchKernelGGL(ext_rebase_kernel, dim3((n_items + 255) / 256), dim3(256), 0, st, a, n_items, rel, kept ? 1 : 0);
	hipLaunchKernelGGL(ext_fcand_kernel, dim3(a.n_queries), dim3(64), 0, st, a);
	return list_kept(a, st);
}

hipError_t launch_ext_fappend(const ExtArgs& a, uint32_t n_listed, uint32_t list_need, bool last, hipStream_t st)
{
	if (n_listed > 0) hipLaunchKernelGGL(ext_filter_kernel, dim3((n_listed + 255) / 256), dim3(256), 0, st, a, n_listed);
	// the LDS list: what the query with the most swept targets can need, in steps of 64 slots, at most EXT_FILTER_LIST (56 KB)
	uint32_t cap = (list_need + 63) / 64 * 64;
	cap = cap < 64 ? 64 : cap > EXT_FILTER_LIST ? EXT_FILTER_LIST : cap;
	hipLaunchKernelGGL(ext_fappend_kernel, dim3(a.n_queries), dim3(64), (size_t)cap * (sizeof(SelSlot) + 4), st, a, last ? 1 : 0, cap);
	return hipGetLastError();
}

hipError_t launch_ext_ffinal(const ExtArgs& a, hipStream_t st)
{
	hipLaunchKernelGGL(ext_ffinal_kernel, dim3(a.n_queries), dim3(64), 2 * (size_t)a.k * sizeof(SelSlot), st, a);
	return list_kept(a, st);
}

hipError_t launch_ext_resweep(const ExtArgs& a, uint32_t n_kept, hipStream_t st)
{
	hipError_t e = reset_iteration(a, st);
	if (e != hipSuccess) return e;
	const uint32_t n_left = a.item_cap - a.item_base;
	if (n_left > 0) hipLaunchKernelGGL(ext_init_kernel, dim3((n_left + 255) / 256), dim3(256), 0, st, a);
	hipLaunchKernelGGL(ext_resweep_kernel, dim3((n_kept + 255) / 256), dim3(256), 0, st, a, n_kept);
	return order_items(a, st);
}

hipError_t launch_ext_rewalk(const ExtArgs& a, uint32_t n_items, uint32_t n_kept, int64_t rel, hipStream_t st)
{
	if (n_items > 0 && rel != 0) hipLaunchKernelGGL(ext_rebase_kernel, dim3((n_items + 255) / 256), dim3(256), 0, st, a, n_items, rel, 1);
	hipLaunchKernelGGL(ext_rewalk_kernel, dim3((n_kept + 255) / 256), dim3(256), 0, st, a, n_kept);
	return hipGetLastError();
}

namespace {
// the host's e-value and bit score into the device copy of the records (two doubles per record, in record order)
__global__ __launch_bounds__(256) void ext_patch_kernel(dmnd_match* records, const double* ev_bits, uint32_t n)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	records[i].evalue = ev_bits[2 * i]; records[i].bit_score = ev_bits[2 * i + 1];
}
// block-local target ids -> database-wide ordinals while the records are gathered for a join
__global__ __launch_bounds__(256) void ext_gather_kernel(dmnd_match* dst, const dmnd_match* src, uint32_t n, uint32_t target_offset)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	dmnd_match m = src[i];
	m.target += target_offset;
	dst[i] = m;
}
}

hipError_t launch_ext_patch(dmnd_match* records, const double* ev_bits, uint32_t n, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	hipLaunchKernelGGL(ext_patch_kernel, dim3((n + 255) / 256), dim3(256), 0, st, records, ev_bits, n);
	return hipGetLastError();
}

hipError_t launch_ext_gather(dmnd_match* dst, const dmnd_match* src, uint32_t n, uint32_t target_offset, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	hipLaunchKernelGGL(ext_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dst, src, n, target_offset);
	return hipGetLastError();
}

hipError_t launch_ext_records(const ExtArgs& a, uint32_t n_kept, hipStream_t st)
{
	if (n_kept == 0) return hipSuccess;
	hipLaunchKernelGGL(ext_records_kernel, dim3(a.n_queries), dim3(64), (size_t)a.k * sizeof(SelSlot), st, a);
	return hipGetLastError();
}

hipError_t launch_ext_top_append(const ExtArgs& a, uint32_t n_items, bool kept, int64_t rel, bool last, hipStream_t st)
{
	if (n_items > 0 && (!kept || rel != 0)) hipLaunchKernelGGL(ext_rebase_kernel, dim3((n_items + 255) / 256), dim3(256), 0, st, a, n_items, rel, kept ? 1 : 0);
	hipLaunchKernelGGL(ext_top_append_kernel, dim3(a.n_queries), dim3(64), 0, st, a, last ? 1 : 0);
	// speculatively (the host only uses it when no query is left ranking): the last cut, the list the walk runs over
	hipLaunchKernelGGL(ext_top_final_kernel, dim3(a.n_queries), dim3(64), 0, st, a);
	return list_kept(a, st);
}

hipError_t launch_ext_top_records(const ExtArgs& a, uint32_t n_walked, hipStream_t st)
{
	hipError_t e = hipMemsetAsync(&a.ctr->n_records, 0, sizeof(uint32_t), st);
	if (e != hipSuccess) return e;
	if (n_walked == 0) return hipSuccess;
	if (n_walked > a.r2_cap) return hipErrorInvalidValue;
	if (filters_on(a.filt)) {
		hipLaunchKernelGGL(ext_filter_kernel, dim3((n_walked + 255) / 256), dim3(256), 0, st, a, n_walked);
		hipLaunchKernelGGL(ext_top_ffinal_kernel, dim3(a.n_queries), dim3(64), 0, st, a);
	}
	size_t need = 0;
	e = rocprim::radix_sort_pairs(nullptr, need, a.okeys, a.okeys_sorted, a.oidx, a.rperm, (size_t)n_walked, 0, 64, st);
	if (e != hipSuccess) return e;
	e = ensure_tmp(a.scan_tmp, a.scan_tmp_bytes, need);
	if (e != hipSuccess) return e;
	const unsigned blocks = (n_walked + 255) / 256;
	hipLaunchKernelGGL(ext_top_keys_kernel, dim3(blocks), dim3(256), 0, st, a, n_walked);
	e = rocprim::radix_sort_pairs(*a.scan_tmp, need, a.okeys, a.okeys_sorted, a.oidx, a.rperm, (size_t)n_walked, 0, 64, st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_top_records_kernel, dim3(blocks), dim3(256), 0, st, a, n_walked);
	return hipGetLastError();
}

// ---- transcripts (extend_kernels.h TrArgs; arithmetic: transcript_core.h) ----

namespace {

// slot widths of the first n entries of the round-2 list (entry n: 0, the scan's total). Bound: n <= r2_cap = nS, k_len holds nS + 1
__global__ __launch_bounds__(256) void ext_tr_widths_kernel(ExtArgs a, TrArgs t, uint32_t n)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k > n) return;
	int64_t w = 0;
	if (k < n) {
		const dmnd_dp_target d = a.items[a.r2_order[k]];
		w = tr_slot_bytes(d.query_len, d.target_len);
	}
	t.k_len[k] = w;
}

// The pieces of the walk, one thread: a binary search over the scan per piece (pieces are few: the limit is hundreds of MB by
// default). Bound: a piece has at least one entry, so at most n + 1 <= nS + 1 entries of `pieces` are written.
__global__ __launch_bounds__(64) void ext_tr_pieces_kernel(ExtArgs a, TrArgs t, uint32_t n, int64_t limit)
{
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	uint32_t np = 0, s = 0;
	long long raw_max = 0;
	t.pieces[0] = 0;
	while (s < n) {
		const uint32_t e = tr_piece_end(a.r2_tr, n, s, limit);
		const long long bytes = (long long)tr_raw_off(a.r2_tr[e], a.r2_tr[s]);
		raw_max = bytes > raw_max ? bytes : raw_max;
		t.pieces[++np] = e;
		s = e;
	}
	t.ctr->n_pieces = np;
	t.ctr->raw_total = (long long)a.r2_tr[n];
	t.ctr->raw_max = raw_max;
}

// kept lengths of the piece [s0, s0 + m) behind its walk (entry m: 0). Bound: m <= nS, k_len holds nS + 1
__global__ __launch_bounds__(256) void ext_tr_keep_sizes_kernel(ExtArgs a, TrArgs t, uint32_t s0, uint32_t m)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i > m) return;
	t.k_len[i] = i < m ? tr_kept_bytes(a.hsps[a.r2_order[s0 + i]].transcript_len) : 0;
}

// raw slot -> store, one wavefront per entry of the piece. Reads k_len[i] <= the slot's width bytes from the slot at
// r2_tr[s0 + i] - r2_tr[s0] (inside the piece's raw bytes); writes them at base + k_off[i] (the host sized the store to
// base + k_off[m]); one g_store entry per entry, index r2_group < n_groups.
__global__ __launch_bounds__(256) void ext_tr_keep_kernel(ExtArgs a, TrArgs t, uint32_t s0, uint32_t m, const uint8_t* raw, uint8_t* store, int64_t base)
{
	const uint32_t i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (i >= m) return;
	const int64_t src = tr_raw_off(a.r2_tr[s0 + i], a.r2_tr[s0]), dst = tr_dense_off(base, t.k_off[i]);
	const int64_t width = a.r2_tr[s0 + i + 1] - a.r2_tr[s0 + i];
	int64_t bytes = t.k_len[i];
	if (bytes > width) bytes = width;            // (never: the walk fails a transcript that does not fit its slot)
	tr_copy_lane(store + dst, raw + src, bytes, (int)lane);
	if (lane == 0) t.g_store[a.r2_group[s0 + i]] = dst;
}

// output sizes of the n records (entry n: 0). Bound: n <= nR, r_len holds nR + 1
__global__ __launch_bounds__(256) void ext_tr_gather_sizes_kernel(ExtArgs a, TrArgs t, uint32_t n)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r > n) return;
	t.r_len[r] = r < n ? tr_kept_bytes(a.records[r].hsp.transcript_len) : 0;
}

// store -> output, one wavefront per record; the record carries its group in hsp.transcript_off (a.tr_on) and leaves with its
// offset in the output. Reads r_len[r] bytes of the store at g_store[group] (what ext_tr_keep_kernel wrote for that group:
// the same length, the same transcript_len), writes them at r_off[r] (the host sized the output to r_off[n]).
__global__ __launch_bounds__(256) void ext_tr_gather_kernel(ExtArgs a, TrArgs t, uint32_t n, const uint8_t* store, uint8_t* out)
{
	const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (r >= n) return;
	const int64_t g = a.records[r].hsp.transcript_off;
	const int64_t src = g >= 0 && g < (int64_t)a.n_groups ? t.g_store[g] : -1;
	if (src < 0) {                               // (never: every record's group was walked and kept; the host fails the call)
		if (lane == 0) t.ctr->missing = 1;
		return;
	}
	const int64_t dst = tr_dense_off(0, t.r_off[r]);
	tr_copy_lane(out + dst, store + src, t.r_len[r], (int)lane);
	__builtin_amdgcn_wave_barrier();             // (every lane has read the group before lane 0 overwrites it)
	if (lane == 0) a.records[r].hsp.transcript_off = dst;
}

hipError_t scan64(const ExtArgs& a, int64_t* in, int64_t* out, size_t n, hipStream_t st)
{
	size_t need = 0;
	hipError_t e = rocprim::exclusive_scan(nullptr, need, in, out, (int64_t)0, n, rocprim::plus<int64_t>(), st);
	if (e != hipSuccess) return e;
	e = ensure_tmp(a.scan_tmp, a.scan_tmp_bytes, need);
	if (e != hipSuccess) return e;
	return rocprim::exclusive_scan(*a.scan_tmp, need, in, out, (int64_t)0, n, rocprim::plus<int64_t>(), st);
}

}  // namespace

hipError_t launch_tr_slots(const ExtArgs& a, const TrArgs& t, uint32_t n, int64_t limit, hipStream_t st)
{
	if (n > a.r2_cap) return hipErrorInvalidValue;
	hipLaunchKernelGGL(ext_tr_widths_kernel, dim3((n + 1 + 255) / 256), dim3(256), 0, st, a, t, n);
	const hipError_t e = scan64(a, t.k_len, a.r2_tr, (size_t)n + 1, st);
	if (e != hipSuccess) return e;
	hipLaunchKernelGGL(ext_tr_pieces_kernel, dim3(1), dim3(64), 0, st, a, t, n, limit);
	return hipGetLastError();
}

hipError_t launch_tr_keep_sizes(const ExtArgs& a, const TrArgs& t, uint32_t s0, uint32_t m, hipStream_t st)
{
	if ((uint64_t)s0 + m > a.r2_cap) return hipErrorInvalidValue;
	hipLaunchKernelGGL(ext_tr_keep_sizes_kernel, dim3((m + 1 + 255) / 256), dim3(256), 0, st, a, t, s0, m);
	return scan64(a, t.k_len, t.k_off, (size_t)m + 1, st);
}

hipError_t launch_tr_keep(const ExtArgs& a, const TrArgs& t, uint32_t s0, uint32_t m, const uint8_t* raw, uint8_t* store, int64_t base, hipStream_t st)
{
	if (m == 0) return hipSuccess;
	if ((uint64_t)s0 + m > a.r2_cap || base < 0) return hipErrorInvalidValue;
	hipLaunchKernelGGL(ext_tr_keep_kernel, dim3((m + 3) / 4), dim3(256), 0, st, a, t, s0, m, raw, store, base);
	return hipGetLastError();
}

hipError_t launch_tr_gather_sizes(const ExtArgs& a, const TrArgs& t, uint32_t n, hipStream_t st)
{
	if (n > a.r2_cap) return hipErrorInvalidValue;      // (r2_cap = the capacity of the records, ExtLayout::nR)
	hipLaunchKernelGGL(ext_tr_gather_sizes_kernel, dim3((n + 1 + 255) / 256), dim3(256), 0, st, a, t, n);
	return scan64(a, t.r_len, t.r_off, (size_t)n + 1, st);
}

hipError_t launch_tr_gather(const ExtArgs& a, const TrArgs& t, uint32_t n, const uint8_t* store, uint8_t* out, hipStream_t st)
{
	if (n == 0) return hipSuccess;
	if (n > a.r2_cap) return hipErrorInvalidValue;
	hipLaunchKernelGGL(ext_tr_gather_kernel, dim3((n + 3) / 4), dim3(256), 0, st, a, t, n, store, out);
	return hipGetLastError();
}

}  // namespace dmnd

// dmnd_init: the first launch of a kernel of this translation unit loads its code object onto the device
namespace { __global__ void touch_extend_kernel() {} }
extern "C" hipError_t dmnd_touch_extend(hipStream_t st) { hipLaunchKernelGGL(touch_extend_kernel, dim3(1), dim3(64), 0, st); return hipGetLastError(); }
