// cbs_kernels.hip -- composition-based matrix adjustment (--comp-based-stats 2 - 5) on the device: the kernel, its launcher and
// the C ABI around it. Replaces, per (query, target) pair, what WorkTarget::WorkTarget computes on a host thread
// (/root/reference/src/align/ungapped.cpp:44-58: Stats::adjust_matrix + Stats::TargetMatrix::TargetMatrix, src/stats/cbs.cpp:94-173;
// CompositionMatrixAdjust, src/stats/matrix_adjust.cpp:354-478; Blast_OptimizeTargetFrequencies, src/stats/blast/ncbi.cpp).
// The arithmetic, its layout over the 64 lanes and the guards are in cbs_core.h (shared with the lane emulator); the host form
// (cbs_adjust.cpp) computes the pairs the kernel hands back. Compiled with -ffp-contract=off (Makefile).
//
// Launch shape: ONE wavefront (a block of 64 threads) per pair, grid-stride over the pairs. The wavefront's workspace -- five
// 400-vectors, the packed lower triangle of the 40 x 40 factor, the 40-vectors of the triangular solves -- is 25.4 KB of LDS, so
// six wavefronts share a CU's 160 KB (occupancy 6 of the CU's 32 wavefront slots; registers do not bind, LDS does). The kernel is
// bound by the dependency chains of the factorisation and the two triangular solves (40 columns in sequence, 780 dependent
// multiply-subtracts along the longest row), not by issue slots: six independent wavefronts per CU overlap those chains, and more
// would need the 400-vectors out of LDS, where every phase reads them across lanes.
#pragma clang fp contract(off)
#include <algorithm>
#include <cstring>
#include <vector>
#include "ctx.h"
#include "cbs_model.h"

using namespace dmnd;

namespace {

__global__ __launch_bounds__(64) void cbs_adjust_kernel(const CbsDevModel* m, int64_t n, const double* comp, const int32_t* true_aa, const int32_t* qidx,
	const int64_t* toff, const int32_t* tlen, const int8_t* letters, int8_t* tables, double* scores, int32_t* rule, uint8_t* status)
{
	__shared__ CbsWave W;
	for (int64_t p = blockIdx.x; p < n; p += gridDim.x) {
		const int64_t qi = qidx ? (int64_t)qidx[p] : p;
		cbsd_pair(W, *m, comp + CBSD_N * qi, true_aa[qi], letters + toff[p], tlen[p], tables + p * (32 * 32), scores ? scores + p * (CBSD_S * CBSD_S) : nullptr,
			rule + p, status + p, nullptr);
	}
}

size_t up8(size_t x) { return (x + 7) & ~(size_t)7; }

}

// The kernel over lists that lie in HBM already (the device half of dmnd_extend lists its pairs there, extend_kernels.h): enqueued on
// w's stream between w->ev0 and w->ev1, nothing is waited for; rule_dev / status_dev stay on the device.
int dmnd_cbs_adjust_lists(dmnd_ctx* w, const CbsDevModel* model_dev, int64_t n, const double* comp_dev, const int32_t* true_aa_dev, const int32_t* qidx_dev,
	const int64_t* toff_dev, const int32_t* tlen_dev, const int8_t* letters_dev, int8_t* tables_dev, double* scores_dev, int32_t* rule_dev, uint8_t* status_dev)
{
	if (n <= 0) return DMND_OK;
	hipStream_t st = w->stream;
	static const int cus = [] { int d = 0, v = 0; return hipGetDevice(&d) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, d) == hipSuccess && v > 0 ? v : 256; }();
	const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)cus * 6);
	HIP_TRY(hipEventRecord(w->ev0, st));
	hipLaunchKernelGGL(cbs_adjust_kernel, dim3(grid), dim3(64), 0, st, model_dev, n, comp_dev, true_aa_dev, qidx_dev, toff_dev, tlen_dev, letters_dev, tables_dev, scores_dev, rule_dev, status_dev);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(w->ev1, st));
	return DMND_OK;
}

int dmnd_cbs_adjust_device(dmnd_ctx* w, const CbsModel& model, int mode, int max_its, const int8_t* letters_dev, int64_t n_q, const double* comp, const int32_t* true_aa,
	int64_t n, const int32_t* qidx, const int64_t* toff, const int32_t* tlen, int8_t* tables_dev, double* scores_dev, int32_t* rule_out, uint8_t* status_out, double* kernel_ms)
{
	if (kernel_ms) *kernel_ms = 0.0;
	if (n == 0) return DMND_OK;
	HIP_TRY(hipSetDevice(w->device));
	// one staging buffer, one copy: model | comp | toff | true_aa | qidx | tlen; behind it on the device: rule | status
	const size_t o_model = 0, o_comp = up8(sizeof(CbsDevModel)), o_toff = o_comp + (size_t)n_q * CBSD_N * sizeof(double), o_aa = o_toff + (size_t)n * sizeof(int64_t),
		o_qidx = up8(o_aa + (size_t)n_q * sizeof(int32_t)), o_tlen = up8(o_qidx + (qidx ? (size_t)n * sizeof(int32_t) : 0)), in_bytes = up8(o_tlen + (size_t)n * sizeof(int32_t)),
		o_rule = in_bytes, o_status = o_rule + (size_t)n * sizeof(int32_t), all_bytes = up8(o_status + (size_t)n);
	if (int rc = w->cbs_host.ensure(all_bytes)) return rc;
	if (int rc = w->cbs_dev.ensure(all_bytes)) return rc;
	char* hs = w->cbs_host.as<char>();
	char* ds = w->cbs_dev.as<char>();
	cbs_dev_model(*reinterpret_cast<CbsDevModel*>(hs + o_model), model, mode, max_its);
	std::memcpy(hs + o_comp, comp, (size_t)n_q * CBSD_N * sizeof(double));
	std::memcpy(hs + o_toff, toff, (size_t)n * sizeof(int64_t));
	std::memcpy(hs + o_aa, true_aa, (size_t)n_q * sizeof(int32_t));
	if (qidx) std::memcpy(hs + o_qidx, qidx, (size_t)n * sizeof(int32_t));
	std::memcpy(hs + o_tlen, tlen, (size_t)n * sizeof(int32_t));
	hipStream_t st = w->stream;
	HIP_TRY(hipMemcpyAsync(ds, hs, in_bytes, hipMemcpyHostToDevice, st));
	if (int rc = dmnd_cbs_adjust_lists(w, reinterpret_cast<const CbsDevModel*>(ds + o_model), n, reinterpret_cast<const double*>(ds + o_comp),
		reinterpret_cast<const int32_t*>(ds + o_aa), qidx ? reinterpret_cast<const int32_t*>(ds + o_qidx) : nullptr, reinterpret_cast<const int64_t*>(ds + o_toff),
		reinterpret_cast<const int32_t*>(ds + o_tlen), letters_dev, tables_dev, scores_dev, reinterpret_cast<int32_t*>(ds + o_rule), reinterpret_cast<uint8_t*>(ds + o_status))) return rc;
	HIP_TRY(hipMemcpyAsync(hs + o_rule, ds + o_rule, all_bytes - o_rule, hipMemcpyDeviceToHost, st));
	HIP_TRY(sync_stream(st));
	std::memcpy(rule_out, hs + o_rule, (size_t)n * sizeof(int32_t));
	std::memcpy(status_out, hs + o_status, (size_t)n);
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, w->ev0, w->ev1));
	if (kernel_ms) *kernel_ms = ms;
	return DMND_OK;
}

// DMND_CBS_DEVICE_MAX_ITS=n (test hook, read per call): the kernel's iteration cap; 0 = the built-in one
int dmnd_cbs_env_max_its()
{
	const char* e = std::getenv("DMND_CBS_DEVICE_MAX_ITS");
	return e ? std::max(0, std::atoi(e)) : 0;
}

// DMND_CBS_PASS_HITS=n (read per call): seed hits per pass of the host path (extend_host.hip); a pair needs a seed hit, so also
// the 1 KB matrix slots one pass -- or one call of the device half -- may ask for. Default 2 M: 2 GB of matrices
int64_t dmnd_cbs_pass_hits()
{
	const char* e = std::getenv("DMND_CBS_PASS_HITS");
	return e ? std::max<int64_t>(1, std::atoll(e)) : (int64_t)2 << 20;
}

extern "C" int dmnd_cbs_target_matrices_device(dmnd_ctx* c, int mode, int64_t n, const double* query_comp, const int32_t* query_true_aa,
	const int8_t* targets, const int64_t* target_off, int32_t* rule_out, uint8_t* status_out, int8_t* matrices_out, double* scores_out)
{
	if (!c || n < 0) return fail(DMND_E_ARG, "dmnd_cbs_target_matrices_device: bad argument");
	if (n == 0) return DMND_OK;
	if (!query_comp || !query_true_aa || !target_off || !rule_out || !status_out || !matrices_out || n > 0x7fffffff)
		return fail(DMND_E_ARG, "dmnd_cbs_target_matrices_device: bad argument");
	for (int64_t k = 0; k < n; ++k)
		if (target_off[k] < 0 || target_off[k + 1] < target_off[k] || target_off[k + 1] - target_off[k] > 0x7fffffff)
			return fail(DMND_E_ARG, "dmnd_cbs_target_matrices_device: target offsets must ascend");
	const int64_t total = target_off[n];
	if (total > 0 && !targets) return fail(DMND_E_ARG, "dmnd_cbs_target_matrices_device: bad argument");
	CbsModel model;
	cbs_model_init(model, c->params);
	if (!model.valid) return fail(DMND_E_ARG, "This value for --comp-based-stats is not supported when using a custom scoring matrix.");
	HIP_TRY(hipSetDevice(c->device));
	DevBuf tables, scores;
	struct Release { DevBuf& a; DevBuf& b; ~Release() { a.release(); b.release(); } } release{ tables, scores };
	if (int rc = c->host_t.ensure((size_t)total + 64)) return rc;
	if (int rc = tables.ensure((size_t)n * 32 * 32)) return rc;
	if (scores_out) {
		if (int rc = scores.ensure((size_t)n * CBSD_S * CBSD_S * sizeof(double))) return rc;
		HIP_TRY(hipMemsetAsync(scores.p, 0xff, (size_t)n * CBSD_S * CBSD_S * sizeof(double), c->stream));      // NaN where the kernel writes none
	}
	if (total > 0) HIP_TRY(hipMemcpyAsync(c->host_t.p, targets, (size_t)total, hipMemcpyHostToDevice, c->stream));
	HIP_TRY(sync_stream(c->stream));                     // (the letters come from pageable memory of the caller)
	std::vector<int32_t> tlen((size_t)n);
	for (int64_t k = 0; k < n; ++k) tlen[(size_t)k] = (int32_t)(target_off[k + 1] - target_off[k]);
	double ms = 0;
	if (int rc = dmnd_cbs_adjust_device(c, model, mode, dmnd_cbs_env_max_its(), c->host_t.as<int8_t>(), n, query_comp, query_true_aa, n, nullptr, target_off, tlen.data(),
		tables.as<int8_t>(), scores_out ? scores.as<double>() : nullptr, rule_out, status_out, &ms)) return rc;
	std::vector<int8_t> got((size_t)n * 32 * 32);
	if (int rc = download_bytes(c, got.data(), tables.p, got.size())) return rc;
	for (int64_t k = 0; k < n; ++k)
		if (status_out[k] == CBS_ST_DEVICE && rule_out[k] == CBSD_RULE_REL_ENTROPY) std::memcpy(matrices_out + k * 32 * 32, got.data() + k * 32 * 32, 32 * 32);
	if (scores_out) { if (int rc = download_bytes(c, scores_out, scores.p, (size_t)n * CBSD_S * CBSD_S * sizeof(double))) return rc; }
	return DMND_OK;
}

extern "C" int dmnd_cbs_device_stats(const dmnd_ctx* c, double out[6])
{
	if (!c || !out) return fail(DMND_E_ARG, "dmnd_cbs_device_stats: bad argument");
	for (int i = 0; i < 6; ++i) out[i] = c->cbs_dev_stats[i];
	for (const dmnd_ctx* a : c->aux) for (int i = 0; i < 6; ++i) out[i] += a->cbs_dev_stats[i];      // (sub-batches of the call run on auxiliary contexts)
	return DMND_OK;
}
