// filter_core.h -- the arithmetic of the HSP filters (--id, --approx-id, --query-cover, --subject-cover), HIP-free: one statement of it
// for the host path (extend_host.hip; protein and translated queries: filter_values_contexts), the filter kernel of the device half (extend_kernels.hip), the output column approx_pident
// (format_api.hip), the CLI's seed configuration and the CPU tests (tests/emu/filter_emu.cpp). The values are compared with what
// the reference prints, so every expression is spelled operation by operation: IEEE double division and one explicit fused
// multiply-add, the same on the host and on the device.
//   Stats::approx_id            src/stats/stats.cpp:113-118
//   Hsp::approx_id_percent      src/basic/hssp.cpp:380-391 (100 for identical ranges)
//   filter_hsp                  src/align/culling.cpp:147-170
//   hamming_id_cutoff           src/search/setup.cpp:70-78
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DMND_FILTER_HD __host__ __device__
#else
#define DMND_FILTER_HD
#endif

namespace dmnd {

// approximate identity of an alignment from its raw score and the longer of its two ranges
DMND_FILTER_HD inline double approx_id(int raw_score, int range1, int range2)
{
	const int m = range1 > range2 ? range1 : range2;
	if (m == 0) return 100.0;
	const double x = fma((double)raw_score / (double)m, 16.56, 11.41);
	return fmin(fmax(x, 0.0), 100.0);
}

// Hsp::approx_id as the sweeps store it: 100 where the two ranges hold the same letters (every column of the alignment an identity)
DMND_FILTER_HD inline double hsp_approx_id(int raw_score, int q_range, int s_range, int identities, int length)
{
	return (q_range == s_range && identities == length) ? 100.0 : approx_id(raw_score, q_range, s_range);
}

// the stage-1 Hamming identities an --approx-id threshold asks for (the seed stage takes the larger of this and the mode's own)
inline unsigned hamming_id_cutoff(double approx_min_id) { return approx_min_id >= 90.0 ? 30u : approx_min_id >= 50.0 ? 20u : 0u; }

struct FilterCfg {
	double min_id = 0.0, approx_id = 0.0, query_cover = 0.0, subject_cover = 0.0;      // percentages, 0 = off
};

DMND_FILTER_HD inline bool filters_on(const FilterCfg& f) { return f.min_id > 0 || f.approx_id > 0 || f.query_cover > 0 || f.subject_cover > 0; }

// the four values a filter reads of an HSP. q_range: length of the query range in the coordinates of the source sequence (3 x the
// translated range for blastx), source_len: the length it is measured against
struct FilterValues { double id, approx, qcov, scov; };

DMND_FILTER_HD inline FilterValues filter_values(int score, int identities, int length, int q_begin, int q_end, int s_begin, int s_end, int q_range_source, int source_len, int target_len)
{
	FilterValues v;
	v.id = (double)identities * 100.0 / (double)length;
	v.approx = hsp_approx_id(score, q_end - q_begin, s_end - s_begin, identities, length);
	v.qcov = (double)q_range_source * 100 / source_len;
	v.scov = (double)(s_end - s_begin) * 100 / target_len;
	return v;
}

// ... of an HSP of a query block of `contexts` contexts per query, in the coordinates of the context it lies in (context_len letters).
// One context (blastp): the query range against the query's length. Six (blastx): the query range in bases, 3 x the translated
// range, against the length of the DNA read (Hsp::query_source_range, query_cover_percent(source_query_len)); identity, approximate
// identity and subject cover from the translated coordinates as they are. read_len < 1: no read lengths are known, the cover is
// measured against 1 (what the host path did before the read lengths were set; --query-cover is refused without them).
DMND_FILTER_HD inline FilterValues filter_values_contexts(int score, int identities, int length, int q_begin, int q_end, int s_begin, int s_end, int contexts, int context_len, int read_len, int target_len)
{
	return filter_values(score, identities, length, q_begin, q_end, s_begin, s_end,
		contexts == 1 ? q_end - q_begin : 3 * (q_end - q_begin), contexts == 1 ? context_len : (read_len >= 1 ? read_len : 1), target_len);
}

// filter_hsp: true = the HSP is removed
DMND_FILTER_HD inline bool filter_fails(const FilterCfg& f, const FilterValues& v)
{
	return v.id < f.min_id || (f.approx_id > 0 && v.approx < f.approx_id) || v.qcov < f.query_cover || v.scov < f.subject_cover;
}

// a value within 1e-9 relative of a threshold that is switched on (the tolerance of the device half's e-value decisions, ext_near):
// the device half does not decide such an HSP, the host redoes its query
DMND_FILTER_HD inline bool filter_on_threshold(const FilterCfg& f, const FilterValues& v)
{
	auto near = [](double x, double t) { return t > 0 && fabs(x - t) <= 1e-9 * fmax(fabs(x), fabs(t)); };
	return near(v.id, f.min_id) || near(v.approx, f.approx_id) || near(v.qcov, f.query_cover) || near(v.scov, f.subject_cover);
}

}  // namespace dmnd
