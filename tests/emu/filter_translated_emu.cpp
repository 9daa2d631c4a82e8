// tests/emu/filter_translated_emu.cpp -- TEST INFRASTRUCTURE ONLY.
// The filter values of an HSP of a protein or a translated query as diamond_amd/csrc/filter_core.h states them for the host path and
// for the filter kernel of the device half (filter_values_contexts), for tests/test_filter_translated.py.
#include "../../diamond_amd/csrc/filter_core.h"

using namespace dmnd;

// out[4] = identity, approximate identity, query cover, subject cover
extern "C" void emu_ftr_values(int score, int identities, int length, int q_begin, int q_end, int s_begin, int s_end, int contexts, int context_len, int read_len, int target_len, double* out)
{
	const FilterValues v = filter_values_contexts(score, identities, length, q_begin, q_end, s_begin, s_end, contexts, context_len, read_len, target_len);
	out[0] = v.id; out[1] = v.approx; out[2] = v.qcov; out[3] = v.scov;
}

// the same through filter_values as a protein call reaches it (the query range against the query's length)
extern "C" void emu_ftr_values_protein(int score, int identities, int length, int q_begin, int q_end, int s_begin, int s_end, int qlen, int target_len, double* out)
{
	const FilterValues v = filter_values(score, identities, length, q_begin, q_end, s_begin, s_end, q_end - q_begin, qlen, target_len);
	out[0] = v.id; out[1] = v.approx; out[2] = v.qcov; out[3] = v.scov;
}

// 0 = passes, 1 = removed, 2 = a value on a threshold
extern "C" int emu_ftr_verdict(double min_id, double approx_min_id, double query_cover, double subject_cover, int score, int identities, int length,
	int q_begin, int q_end, int s_begin, int s_end, int contexts, int context_len, int read_len, int target_len)
{
	FilterCfg f;
	f.min_id = min_id; f.approx_id = approx_min_id; f.query_cover = query_cover; f.subject_cover = subject_cover;
	const FilterValues v = filter_values_contexts(score, identities, length, q_begin, q_end, s_begin, s_end, contexts, context_len, read_len, target_len);
	return filter_on_threshold(f, v) ? 2 : filter_fails(f, v) ? 1 : 0;
}
