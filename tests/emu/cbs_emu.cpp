// tests/emu/cbs_emu.cpp -- TEST INFRASTRUCTURE ONLY. Runs the wavefront schedule of cbs_adjust_kernel (diamond_amd/csrc/cbs_core.h:
// the kernel's phases, reduction trees and guards) lane after lane on the CPU with glibc's libm, and beside it the host
// arithmetic (cbs_adjust.cpp) with its trace, so that the guard widths can be measured and checked without a GPU.
#include "../../diamond_amd/csrc/cbs_core.h"
// the host form, compiled into this library under names of its own
#define dmnd_cbs_composition emu_host_cbs_composition
#define dmnd_cbs_rule emu_host_cbs_rule
#define dmnd_cbs_target_matrix emu_host_cbs_target_matrix
#define dmnd_cbs_ideal_lambda emu_host_cbs_ideal_lambda
#include "../../diamond_amd/csrc/cbs_adjust.cpp"
#include "../../diamond_amd/csrc/cbs_model.h"

// One pair through the kernel's code. max_its <= 0: the built-in cap. trace_out (optional, 3 + 256 doubles): angle, Newton
// steps, number of convergence tests, rnorm at each. matrix_out / scores_out are written as the kernel writes them.
extern "C" int emu_cbs_pair(const dmnd_params* params, int mode, int max_its, const double* query_comp, int query_true_aa, const int8_t* target, int target_len,
	int32_t* rule_out, uint8_t* status_out, int8_t* matrix_out, double* scores_out, double* trace_out)
{
	dmnd::CbsModel m;
	dmnd::cbs_model_init(m, *params);
	if (!m.valid) return -1;
	static thread_local dmnd::CbsDevModel dm;
	dmnd::cbs_dev_model(dm, m, mode, max_its);
	static thread_local dmnd::CbsWave W;
	dmnd::CbsEmuTrace tr;
	dmnd::cbsd_pair(W, dm, query_comp, query_true_aa, target, target_len, matrix_out, scores_out, rule_out, status_out, &tr);
	if (trace_out) {
		trace_out[0] = tr.angle; trace_out[1] = tr.its; trace_out[2] = tr.n_rnorm;
		for (int i = 0; i < tr.n_rnorm; ++i) trace_out[3 + i] = tr.rnorm[i];
	}
	return 0;
}

// The same pair through the host arithmetic: rule, table (where the rule is not NONE), and the same trace layout plus
// [3 + 256] = 1 if the optimisation converged; scores_out: the host's unrounded scores (untouched if it did not converge).
extern "C" int emu_cbs_host_pair(const dmnd_params* params, int mode, const double* query_comp, int query_true_aa, const int8_t* target, int target_len,
	int32_t* rule_out, int8_t* matrix_out, double* scores_out, double* trace_out)
{
	dmnd::CbsModel m;
	dmnd::cbs_model_init(m, *params);
	if (!m.valid) return -1;
	dmnd::CbsHostTrace tr;
	const int rule = dmnd::cbs_rule(m, mode, query_comp, query_true_aa, target, target_len, &tr);
	*rule_out = rule;
	if (rule == dmnd::CBS_RULE_REL_ENTROPY) {
		dmnd::cbs_target_matrix(m, rule, query_comp, query_true_aa, target, target_len, matrix_out, &tr);
		if (tr.converged && scores_out) for (int i = 0; i < 21 * 21; ++i) scores_out[i] = tr.scores[i];
	}
	else if (rule == dmnd::CBS_RULE_SCALE_OLD) dmnd::cbs_target_matrix(m, rule, query_comp, query_true_aa, target, target_len, matrix_out);
	if (trace_out) {
		trace_out[0] = tr.angle; trace_out[1] = tr.its; trace_out[2] = tr.n_rnorm;
		for (int i = 0; i < tr.n_rnorm; ++i) trace_out[3 + i] = tr.rnorm[i];
		trace_out[3 + 256] = tr.converged;
	}
	return 0;
}

extern "C" void emu_cbs_guards(double* out4)
{
	out4[0] = CBS_EPS_ROUND; out4[1] = CBS_EPS_NORM; out4[2] = CBS_EPS_ANGLE; out4[3] = CBS_DEVICE_MAX_ITS;
}
